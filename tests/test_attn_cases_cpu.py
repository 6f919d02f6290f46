"""What tests/test_gpu_attn_rows.py rests on, proven on the CPU: the hand-built rows (attn_cases.py) have the properties they are
named for, a faithful restatement of attn_kernel's arithmetic stays within 0.8 of the per-element budget on every case, and a
restatement with one thing wrong leaves the budget on a named case - so the GPU test can pass, and can fail.

Restatement / budget, worst element over T in {63, 300, 521} (main kernel; leftover path split / one workgroup):
                       precision 1                 precision 3
  flat                 0.53   0.46 / 0.46          0.20   0.16 / 0.16
  peaked_last          0.65   0.49 / 0.49          0.27   0.23 / 0.24
  peaked_tile_first    0.67   0.48 / 0.48          0.35   0.27 / 0.26
  peaked_tile_last     0.79   0.49 / 0.49          0.35   0.29 / 0.29
  ascending            0.42   0.30 / 0.30          0.16   0.12 / 0.12
  descending           0.30   0.22 / 0.22          0.09   0.04 / 0.06
  heavy_tail           0.49   0.49 / 0.49          0.41   0.19 / 0.19
  offset_pos           0.32   0.27 / 0.27          0.17   0.14 / 0.14
  offset_neg           0.35   0.31 / 0.31          0.18   0.14 / 0.14
  uniform              0.16   0.16 / 0.16          0.02   0.02 / 0.02
  v_range              0.54   0.44 / 0.44          0.50   0.50 / 0.50
  small_q              0.35   0.28 / 0.28          0.06   0.06 / 0.06

Mutation -> the (case, T) the test names as its killer, ratio error / budget there (precision 3):
  drop_p_lo     P's lo part dropped                        flat 300: 49          peaked_tile_last 300: 76
  no_alpha_o    O not rescaled when the maximum jumps      ascending 300: 2.9e5  heavy_tail 300: 8.9e6
  no_alpha_l    l not rescaled when the maximum jumps      ascending 300: 1.1e5  peaked_last 300: 6.2e4
  mask_gt       mask at key > T instead of key >= T        peaked_last 63: 5.7e4 peaked_last 521: 5.1e4
  out_lo_flush  output lo flushed when subnormal           flat 300: 27          small_q 300: 21
  drop_v_lo     V^T lo dropped                             v_range 300: 97       uniform 300: 16
  wave_max      leftover path: maximum of one wave's keys  flat 300: 3.5e5       ascending 521: 8.3e4
(mask_gt is harmless by construction when the extra key is no leader: peaked_tile_first 521 gives 0.65; the alpha mutations are
harmless on `descending`, where the maximum never moves: 0.09.)
"""
import functools

import numpy as np
import pytest

import attn_cases as ac

TS = (63, 300, 521)


@functools.lru_cache(maxsize=None)
def _main(name, T, precision):
    """the unmutated restatement, computed once per (case, T, precision)"""
    out = ac.restate_main(ac.case_bundle(name, T)["ops"], precision)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", ["peaked_last", "peaked_tile_first", "peaked_tile_last"])
def test_peaked_rows_have_a_few_competing_leaders_where_the_name_says(name, T):
    lead = ac.peaked_leaders(name, T)
    assert 2 <= len(lead) <= 4
    assert lead[0] == {"peaked_last": T - 1, "peaked_tile_first": 64 * ((T - 1) // 64), "peaked_tile_last": min(63, T - 1)}[name]
    for precision in (1, 3):
        ref = ac.case_bundle(name, T)["ref"][precision]
        share = ref["pt"] / ref["l"][:, None]
        assert share[:, lead].sum(axis=1).min() >= 0.9
        assert share.max() <= 0.7


@pytest.mark.parametrize("T", TS)
def test_heavy_tail_probe_channel_is_tail_mass_and_mostly_flush(T):
    b = ac.case_bundle("heavy_tail", T)
    L, d = ac.heavy_tail_leader(T), ac.HEAVY_TAIL_PROBE
    for precision in (1, 3):
        ref = b["ref"][precision]
        assert np.all(ref["pt"].argmax(axis=1) == L) and ref["v"][L, d] == 0.0 and np.all(np.delete(ref["v"][:, d], L) == 1.0)
        tail = np.delete(ref["pt"], L, axis=1)
        assert tail.max() <= 2.0 ** -16 and tail.min() >= 2.0 ** -34.5
        assert np.all((tail < 2.0 ** -28).mean(axis=1) >= 0.5)
        flush, total = ac.budget_parts(ref, precision)
        assert (flush[:, d] / total[:, d]).min() >= 0.3


@pytest.mark.parametrize("T", (300, 521))
@pytest.mark.parametrize("name", ["ascending", "descending"])
def test_running_maximum_rises_on_every_tile_or_never_after_the_first(name, T):
    s = ac.case_bundle(name, T)["ref"][3]["s"]
    tmax = np.stack([s[:, k0:k0 + 64].max(axis=1) for k0 in range(0, T, 64)], axis=1)
    if name == "ascending":
        assert np.all(np.diff(tmax, axis=1) > 0)
    else:
        assert np.all(tmax[:, 1:] <= tmax[:, :1])


@pytest.mark.parametrize("T", TS)
def test_small_q_lo_parts_are_fp16_subnormals(T):
    hi, lo = ac.case_bundle("small_q", T)["ops"]["q"]
    lo = np.abs(lo.astype(np.float64))
    assert ((lo > 0) & (lo < ac.F16_MIN_NORMAL)).mean() >= 0.5
    assert (np.abs(hi.astype(np.float64)) < 2.0 ** -3).mean() >= 0.9


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", ["offset_pos", "offset_neg", "uniform", "v_range"])
def test_offsets_uniform_and_v_range_are_what_they_say(name, T):
    b = ac.case_bundle(name, T)
    s = b["ref"][3]["s"]
    if name.startswith("offset"):
        sign = 1.0 if name == "offset_pos" else -1.0
        assert np.all(np.abs(s * sign - 160.0) < 16.0) and 0.3 < (s.max(axis=1) - s.min(axis=1)).mean() / 6.0 < 3.0
    elif name == "uniform":
        assert np.all(s == 0.0)
    else:
        v = b["ref"][3]["v"]
        assert v[:, ac.V_RANGE_SHIFTED].min() > 290.0 and np.abs(v[:, ac.V_RANGE_TINY]).max() < 1e-3


def test_numpy_split_keeps_subnormals_and_22_bits():
    x = np.array([1.0, 0.1, 2.0 ** -3 * 0.999, 3e-5, 6e-8, 1e-9, -300.123, 0.0], np.float32)
    hi, lo = ac.split_f16(x)
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    assert lo[2] != 0 and abs(float(lo[2])) < ac.F16_MIN_NORMAL          # a subnormal lo part survives
    rec = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.all(np.abs(rec - x) <= np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -25))


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_restatements_stay_within_0p8_of_the_budget(name, T):
    b = ac.case_bundle(name, T)
    for precision in (1, 3):
        ref, bud = b["ref"][precision], b["budget"][precision]
        assert np.isfinite(bud).all() and bud.min() > 0
        got = {"main": _main(name, T, precision),
               "leftover, split over the keys": ac.restate_tail(b["ops"], precision, split=True),
               "leftover, one workgroup": ac.restate_tail(b["ops"], precision, split=False, nw=4)}
        for what, out in got.items():
            r = ac.worst_ratio(out, ref["out"], bud)
            print(f"{name} T={T} p{precision} {what}: {r:.3f}")
            assert r <= 0.8, f"{name} T={T} precision {precision}, {what}: error / budget = {r:.3f}"


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_restatement_stays_within_0p8_of_the_raw_input_budget(name, T):
    """the second GPU assertion (precision 3 against the fp64 attention of the raw fp32 inputs) can pass too: worst 0.74, v_range
    (V's own 2^-22 split error has no term of its own and rides on the 2^-21 of `round`)"""
    b = ac.case_bundle(name, T)
    r = ac.worst_ratio(_main(name, T, 3), b["raw"]["out"], b["budget_raw"])
    print(f"{name} T={T} p3 main vs raw: {r:.3f}")
    assert r <= 0.8
    assert np.all(b["budget_raw"] >= 0.999 * b["budget"][3])


KILLERS = {
    "drop_p_lo": [("flat", 300), ("peaked_tile_last", 300)],
    "no_alpha_o": [("ascending", 300), ("heavy_tail", 300)],
    "no_alpha_l": [("ascending", 300), ("peaked_last", 300)],
    "mask_gt": [("peaked_last", 63), ("peaked_last", 521)],
    "out_lo_flush": [("flat", 300), ("small_q", 300)],
    "drop_v_lo": [("v_range", 300), ("uniform", 300)],
    "wave_max": [("flat", 300), ("ascending", 521)],
}


@pytest.mark.parametrize("mutation", list(KILLERS))
def test_every_mutation_of_the_restatement_leaves_the_budget(mutation):
    for name, T in KILLERS[mutation]:
        b = ac.case_bundle(name, T)
        if mutation == "wave_max":
            out = ac.restate_tail(b["ops"], 3, split=False, nw=8, mutate=mutation)
        else:
            out = ac.restate_main(b["ops"], 3, mutate=mutation)
        r = ac.worst_ratio(out, b["ref"][3]["out"], b["budget"][3])
        print(f"{mutation} on {name} T={T}: {r:.3g}")
        assert r > 1.0, f"{mutation} survives {name} T={T}: error / budget = {r:.3f}"


def test_mutations_are_harmless_where_they_must_be():
    """the restatement's switches do what their names say: no maximum jump -> alpha never matters; extra key not a leader and
    T a multiple of 64 -> the mask never matters"""
    b = ac.case_bundle("descending", 300)
    base = ac.restate_main(b["ops"], 3)
    assert np.array_equal(base, ac.restate_main(b["ops"], 3, mutate="no_alpha_o"))
    assert np.array_equal(base, ac.restate_main(b["ops"], 3, mutate="no_alpha_l"))
    b = ac.case_bundle("peaked_last", 128)
    assert np.array_equal(ac.restate_main(b["ops"], 3), ac.restate_main(b["ops"], 3, mutate="mask_gt"))


@pytest.mark.parametrize("T", (1, 17))
def test_short_rows_build_and_stay_in_budget(T):
    for name in ac.CASE_NAMES:
        b = ac.case_bundle(name, T)
        for precision in (1, 3):
            out = ac.restate_main(b["ops"], precision)
            assert np.isfinite(out).all()
            assert ac.worst_ratio(out, b["ref"][precision]["out"], b["budget"][precision]) <= 0.8
