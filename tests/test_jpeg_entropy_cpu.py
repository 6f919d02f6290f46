"""The device entropy route of the JPEG decode, on the CPU: ovm_host_jpeg_entropy_emulate runs the kernels' core routine
(csrc/jpeg_dec_core.hpp), their stages and their round schedule serially, so the algorithm is judged here without a GPU. The judge
is ovm_host_jpeg_entropy_decode, itself pinned bit for bit against Pillow by tests/test_jpeg.py. The route's contract: status 0
only with planes equal to the host decoder's; everything else is declined (by the plan, or by a non-zero status), never judged.

Round counts at 512-bit subsequences, default cap 256 (printed by test_round_counts_and_default_cap; profiles/jpeg_decode/README.md)."""
import ast
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_entropy_cases as K
from test_jpeg import _jpeg, _pil, _scene
from ovmono3d_amd import lib as _lib
from ovmono3d_amd.data import gpu_jpeg

NAMES = sorted(K.well_formed())


@pytest.mark.parametrize("name", NAMES)
def test_emulation_equals_host_decoder(name):
    want, winfo = K.host_planes(name)
    got, info, status, rounds = K.emulated(name)
    assert status == 0, f"declined a well-formed file: status {status}"
    assert rounds >= 1
    assert (info.width, info.height, info.coef_blocks) == (winfo.width, winfo.height, winfo.coef_blocks)
    bad = (got != want).any(1).nonzero().flatten()
    assert len(bad) == 0, f"{len(bad)} of {len(want)} blocks differ, first {bad[:4].tolist()}"


def test_cases_have_their_conditions():
    """Each case is there for something that can break; the something is checked on the file."""
    F = K.well_formed()
    P = {n: K.plan_of(F[n])[1] for n in F}
    sub = P["coco"].sub_bits
    # a stream shorter than one subsequence; one much longer than a workgroup's share
    assert P["420_one_pixel"].ecs_bytes * 8 < sub
    assert K.unstuffed_len(F["scene_300x400_q95"], P["scene_300x400_q95"]) * 8 > 2 * sub * P["coco"].wg_subs
    # restart segments shorter and longer than a subsequence
    assert P["444_restart_blocks"].restart_interval == 3 and P["444_restart_blocks"].segments == 20
    p = P["444_restart_every_mcu"]
    assert p.restart_interval == 1 and p.segments == p.mcus_x * p.mcus_y and p.ecs_bytes * 8 / p.segments < sub / 2
    p = P["420_restart_rows"]
    assert p.restart_interval == p.mcus_x and p.segments == p.mcus_y and (p.ecs_bytes - 2 * p.segments) * 8 / p.segments > sub
    # quality 100 noise: stuffed bytes, 16-bit codes, blocks that end at k = 64 without EOB
    ecs = F["noise_q100"][P["noise_q100"].ecs_offset:][:P["noise_q100"].ecs_bytes]
    coef = K.host_planes("noise_q100")[0].numpy()
    assert ecs.count(b"\xff\x00") >= 20
    lens = K.ac_code_lengths(F["noise_q100"], 0)
    luma_syms = [s for b in coef[:P["noise_q100"].info.bw[0] * P["noise_q100"].info.bh[0]] for s in K.ac_symbols(b)]
    assert sum(lens[s] == 16 for s in luma_syms) >= 3 and sum(lens[s] > 9 for s in luma_syms) >= 40
    assert (coef[:, 63] != 0).sum() >= 10
    # saturated primaries: DC differences of category 11 (scan order = raster order at 4:4:4)
    dc = K.host_planes("primaries_444_q100")[0].numpy()[:, 0].astype(np.int32)
    nb = P["primaries_444_q100"].info.bw[0] * P["primaries_444_q100"].info.bh[0]
    assert np.abs(np.diff(dc[:nb])).max() >= 1024
    # optimised tables: not the standard DHT
    def dht(d):
        out, i = [], d.find(b"\xff\xc4")
        while i >= 0:
            out.append(d[i:i + 2 + int.from_bytes(d[i + 2:i + 4], "big")])
            i = d.find(b"\xff\xc4", i + 4)
        return out
    assert dht(F["420_q30_optimised_tables"]) != dht(F["420_q75"]) and dht(F["420_q75"]) == dht(F["422_q75"])
    # colour layouts and table classes
    assert P["grey"].info.ncomp == 1 and P["grey"].blocks_per_mcu == 1
    assert [P[n].blocks_per_mcu for n in ("444_q90", "422_q75", "420_q75")] == [3, 4, 6]
    assert P["rgb_no_transform"].info.colorspace == 2
    # one table pair for every component: nothing in the tables tells a guessed state its block index; and the stream is longer
    # than one subsequence per step could cover within the launches
    p = P["coco_rgb_one_table_pair"]
    assert p.info.colorspace == 2 and len(set(p.sel_dc[:3])) == 1 and len(set(p.sel_ac[:3])) == 1
    assert K.unstuffed_len(F["coco_rgb_one_table_pair"], p) * 8 > p.sync_launches * p.wg_subs * sub
    # one byte under and one byte over a multiple of the subsequence size
    assert K.unstuffed_len(F["one_byte_under_multiple"], P["one_byte_under_multiple"]) % (sub // 8) == sub // 8 - 1
    assert K.unstuffed_len(F["one_byte_over_multiple"], P["one_byte_over_multiple"]) % (sub // 8) == 1


def test_round_counts_and_default_cap():
    """The cap bounds the work on a hostile file; it must not turn ordinary files over to the host. Two limits do that: max_rounds
    steps per workgroup in one launch, and sync_launches - 1 launches that decode anything (a clean one must follow). `rounds` is
    summed over the launches, so it bounds the first from above; the default leaves a factor of two on both."""
    rc, plan = K.plan_of(K.well_formed()["coco"])
    assert rc == 0
    counts = {n: K.emulated(n)[3] for n in NAMES}
    for n in NAMES:
        p = K.plan_of(K.well_formed()[n])[1]
        subs = -(-K.unstuffed_len(K.well_formed()[n], p) * 8 // p.sub_bits)
        print(f"{n:32s} subsequences {subs:5d} rounds {counts[n]:4d} productive launches {K.emulated_launches(n)}")
    print(f"subsequence {plan.sub_bits} bits, {plan.wg_subs} per workgroup, {plan.sync_launches} launches, default cap {plan.max_rounds}")
    assert plan.max_rounds >= 2 * max(counts.values()), counts
    launches = {n: K.emulated_launches(n) for n in NAMES}
    assert all(v >= 1 for v in launches.values()) and plan.sync_launches - 1 >= 2 * max(launches.values()), launches


def test_plan_declines_what_is_outside_the_scope():
    arr = _scene(40, 56, 1)
    outside = {"progressive": _jpeg(arr, quality=80, progressive=True)}
    cm = io.BytesIO()
    Image.fromarray(np.dstack([arr, arr[:, :, :1]]), mode="CMYK").save(cm, format="JPEG")
    outside["cmyk"] = cm.getvalue()
    exif = Image.Exif()
    exif[0x0112] = 6
    ex = io.BytesIO()
    Image.fromarray(arr).save(ex, format="JPEG", quality=85, exif=exif.tobytes())
    outside["exif_rotated"] = ex.getvalue()
    # per-component scans: the interleaved scan of a 4:4:4 file split into three (same tables, Ss..Se = 0..63)
    outside["per_component_scans"] = _split_scans(arr)
    for name, data in outside.items():
        rc, _ = K.plan_of(data)
        assert rc != 0, name
        with pytest.raises(gpu_jpeg.EntropyDeclined):
            gpu_jpeg.entropy_decode_emulated(data)
    # the split file is a valid JPEG that the host route reads - the plan only stepped aside
    coef, info = gpu_jpeg.entropy_decode(outside["per_component_scans"])
    from oracle import jpeg_ref
    assert np.array_equal(jpeg_ref.reconstruct(coef.numpy(), info), _pil(outside["per_component_scans"]))
    # data behind the scan other than EOI, and a missing EOI
    good = K.small_files()["baseline_420"]
    assert K.plan_of(good)[0] == 0
    assert K.plan_of(good[:-2])[0] != 0
    assert K.plan_of(good[:-2] + b"\xff\xfe\x00\x04ab\xff\xd9")[0] != 0


def _split_scans(arr):
    """Re-writes a grey-coded copy of each channel as one scan of a three-component 4:4:4 frame: a file with per-component scans."""
    planes = [_jpeg(np.ascontiguousarray(arr[:, :, c]), quality=80) for c in range(3)]
    def seg(d, marker):
        i = d.find(marker)
        return d[i:i + 2 + int.from_bytes(d[i + 2:i + 4], "big")]
    def ecs(d):
        i = d.find(b"\xff\xda")
        return d[i + 2 + int.from_bytes(d[i + 2:i + 4], "big"):-2]
    g = planes[0]
    h, w = arr.shape[:2]
    sof = b"\xff\xc0" + (8 + 9).to_bytes(2, "big") + b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + b"\x03" + \
        b"".join(bytes([c + 1, 0x11, 0]) for c in range(3))
    dht, i = b"", g.find(b"\xff\xc4")
    while i >= 0:
        dht += g[i:i + 2 + int.from_bytes(g[i + 2:i + 4], "big")]
        i = g.find(b"\xff\xc4", i + 4)
    out = b"\xff\xd8" + seg(g, b"\xff\xe0") + seg(g, b"\xff\xdb") + sof + dht
    for c in range(3):
        out += b"\xff\xda" + (6 + 2).to_bytes(2, "big") + b"\x01" + bytes([c + 1, 0x00]) + b"\x00\x3f\x00" + ecs(planes[c])
    return out + b"\xff\xd9"


def test_round_cap_declines_and_never_accepts_wrongly():
    data = K.well_formed()["scene_300x400_q95"]
    assert K.emulated("scene_300x400_q95")[3] > 6            # needs more than max_rounds = 1 allows (one step in each launch)
    coef, info, status, rounds = gpu_jpeg.entropy_decode_emulated(data, max_rounds=1)
    assert status & 4 and rounds <= 6                         # OVM_JPEG_DEC_NOSYNC
    # a cap the file fits under accepts it again
    need = K.emulated("scene_300x400_q95")[3]
    coef, info, status, rounds = gpu_jpeg.entropy_decode_emulated(data, max_rounds=need)
    assert status == 0 and torch.equal(coef, K.host_planes("scene_300x400_q95")[0])


def _emulate_or_none(data, max_rounds=None):
    try:
        coef, info, status, rounds = gpu_jpeg.entropy_decode_emulated(data, max_rounds=max_rounds)
    except gpu_jpeg.EntropyDeclined:
        return None
    return coef if status == 0 else None


@pytest.mark.parametrize("kind", sorted(K.small_files()))
def test_every_cut_is_declined_or_equal_to_the_host(kind):
    data = K.small_files()[kind]
    assert K.judge_damaged(data, _emulate_or_none(data))
    accepted = 0
    for cut in range(2, len(data)):
        part = data[:cut]
        accepted += K.judge_damaged(part, _emulate_or_none(part))
        accepted += K.judge_damaged(part + b"\xff\xd9", _emulate_or_none(part + b"\xff\xd9"))
    assert accepted <= 16, f"{accepted} cut files accepted"      # only cuts behind the last entropy-coded byte can be whole


@pytest.mark.parametrize("kind", sorted(K.small_files()))
def test_byte_flips_are_declined_or_equal_to_the_host(kind):
    data = K.small_files()[kind]
    rc, plan = K.plan_of(data)
    assert rc == 0
    g = np.random.default_rng(7)
    accepted = declined = 0
    for it in range(300):
        d = bytearray(data)
        for _ in range(int(g.integers(1, 4))):
            d[plan.ecs_offset + int(g.integers(0, plan.ecs_bytes))] = int(g.integers(0, 256)) if it % 3 else 0xFF
        ok = K.judge_damaged(bytes(d), _emulate_or_none(bytes(d), max_rounds=None if it % 5 else 2))
        accepted += ok
        declined += not ok
    assert accepted > 10 and declined > 10, (accepted, declined)    # both outcomes were exercised
    for d in K.fixed_mutations(data):                               # the list that also goes to the device
        K.judge_damaged(d, _emulate_or_none(d))


def test_capacity_and_imports():
    L = _lib.load()
    data = K.small_files()["baseline_420"]
    plan = _lib.OvmJpegDecPlan()
    tables = np.full(11008 + 16, 0x5a, dtype=np.uint8)
    assert L.ovm_host_jpeg_decode_plan(data, len(data), 0, C.byref(plan), tables.ctypes.data, 11007) == -5
    assert (tables == 0x5a).all()
    assert L.ovm_host_jpeg_decode_plan(data, len(data), 0, C.byref(plan), tables.ctypes.data, 11008) == 0
    assert plan.tables_bytes == 11008 and (tables[11008:] == 0x5a).all()
    ws = C.c_int64()
    assert L.ovm_jpeg_entropy_decode_workspace(C.byref(plan), C.byref(ws)) == 0 and ws.value > plan.ecs_bytes
    info = _lib.OvmJpegInfo()
    nb = int(plan.info.coef_blocks)
    coef = np.full((nb + 2) * 64, 0x5a5a, dtype=np.int16)
    st, rd = C.c_int32(), C.c_int32()
    assert L.ovm_host_jpeg_entropy_emulate(data, len(data), 0, coef[64:].ctypes.data, nb * 64 - 1, C.byref(info), C.byref(st), C.byref(rd), None) == -5
    assert L.ovm_host_jpeg_entropy_emulate(data, len(data), 0, coef[64:].ctypes.data, nb * 64, C.byref(info), C.byref(st), C.byref(rd), None) == 0
    assert st.value == 0 and (coef[:64] == 0x5a5a).all() and (coef[-64:] == 0x5a5a).all()
    # a record that the plan did not write is refused by the device entry points before anything is launched
    plan.blocks_per_mcu = 7
    assert L.ovm_jpeg_entropy_decode_workspace(C.byref(plan), C.byref(ws)) == -1
    # no new dependencies: the module imports what it imported before
    src = open(os.path.join(os.path.dirname(gpu_jpeg.__file__), "gpu_jpeg.py")).read()
    tops = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            tops |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            tops.add(node.module.split(".")[0])
    assert tops <= {"__future__", "ctypes", "typing", "numpy", "torch", "PIL"}, tops
