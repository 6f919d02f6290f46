"""The GroundingDINO engine's fused kernels one at a time - attn_f32_kernel, msdeform_fused_kernel / msdeform_fused4_kernel and
rowop_kernel, through ovm_g_attn_f32 / ovm_g_msdeform_fused / ovm_g_rowop (the launchers the engine itself calls) - against the
float64 restatements of tests/gdino_ops_ref.py.

Every float comparison: common.rel_err (max |a - b| / max |b|) against the float64 reference, bounded by 4 x the error PyTorch's own
fp32 evaluation of the same operation on the CPU shows against that reference from the same inputs, never below 2e-6
(gdino_ops_ref.bound; the factor is DESIGN.md's convention for SAM and Depth Pro, the floor the one test_generic_ops uses). Every
output buffer has a row stride larger than the logical width and extra rows, is pre-filled with a sentinel that is exact in fp16,
and must still hold it wherever the kernel owns nothing. Split outputs are checked bit for bit against the fp32 output:
hi == fp16(y), lo == fp16(y - hi). Each case prints `FIG <kernel> <case> err <measured> fp32 <PyTorch fp32> bound <bound>`.
"""
import ctypes as C
from functools import lru_cache

import pytest
import torch

import gdino_caption_cases as CC
import gdino_ops_ref as R
from common import rel_err

pytestmark = pytest.mark.gpu

SENT = -7.5                 # exact in fp16
OVM_ERR_INVALID, OVM_ERR_HIP, OVM_ERR_SHAPE = -1, -2, -4
F32MIN = torch.finfo(torch.float32).min


def _lib():
    from ovmono3d_amd import lib
    return lib, lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _finish(rc, what):
    """Synchronise after a launch; a HIP error means the context is lost and every later GPU test would only repeat it."""
    if rc == OVM_ERR_HIP:
        pytest.exit(f"{what}: HIP error inside the launcher, stopping the session", returncode=3)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}; stopping the session", returncode=3)


def _report(kernel, name, got, ref64, ref32):
    err, e32, tol = rel_err(got, ref64), rel_err(ref32, ref64), R.bound(ref32, ref64)
    print(f"FIG {kernel} {name} err {err:.3e} fp32 {e32:.3e} bound {tol:.2e} ratio {err / max(e32, 1e-30):.2f}")
    assert torch.isfinite(got).all(), f"{kernel} {name}: non-finite output"
    assert err <= tol, f"{kernel} {name}: error {err:.3e} against fp64 > bound {tol:.2e} (PyTorch fp32: {e32:.3e})"


def _assert_split(hi, lo, y32, what):
    """hi / lo (fp16 tensors) are the split image of the fp32 tensor y32, bit for bit"""
    whi, wlo = R.split_f16(y32)
    assert torch.equal(hi.view(torch.int16), whi.view(torch.int16)), f"{what}: hi != fp16(y)"
    assert torch.equal(lo.view(torch.int16), wlo.view(torch.int16)), f"{what}: lo != fp16(y - hi)"


def _untouched(buf, owned, what):
    """every element outside the boolean mask `owned` still holds the sentinel"""
    assert bool((buf[~owned] == SENT).all()), f"{what}: the kernel wrote outside what it owns"


# =============================================================================================================== attention
#        name  DH nb1 nb2  Tq   Tk  kind
ATTN = {
    "a": (16, 1, 1, 1, 1, "none"),
    "b": (32, 1, 2, 16, 3, "none"),
    "c": (32, 1, 2, 17, 15, "none"),
    "d": (32, 1, 2, 17, 16, "none"),
    "e": (32, 1, 2, 17, 17, "none"),
    "f": (32, 3, 4, 144, 144, "swin"),          # bias_h = relative-position table, bias_b = shift mask per window (sbb != 0)
    "g": (32, 1, 8, 150, 289, "none"),          # 4-wave route, three key chunks, the last one a single key
    "h": (16, 1, 4, 17, 145, "jump_late"),      # K rows 144.. scaled by 8: the maximum jumps in the second chunk
    "h_mirror": (16, 1, 4, 17, 145, "jump_early"),   # K rows ..143 scaled by 8
    "i": (64, 1, 12, 147, 147, "phrase"),       # scalar bias reads, one query whose first chunk is entirely masked
    "j": (64, 1, 12, 256, 256, "phrase"),       # float4 bias reads
    "k": (32, 1, 4, 256, 256, "phrase_odd"),    # ldbb = 260, bias pointer 4 bytes off: must take the scalar reads
    "l": (32, 1, 8, 30, 65, "none"),            # decoder text cross-attention, launch-per-op route
    "m": (32, 1, 8, 900, 64, "none"),
    "n": (32, 1, 2, 64, 148, "mask_tail"),      # keys 140..147 masked for every query, their V rows 1e30 and K rows 50
    "o": (64, 2, 2, 196, 196, "rel14"),         # SAM window: rel_h / rel_w on a 14 x 14 grid
    "p": (64, 2, 2, 64, 289, "rel17"),          # three chunks with the relative-position tables
}


@lru_cache(maxsize=None)
def _attn_case(name):
    """-> dict of CPU fp32 buffers and layout numbers, plus the fp64 reference and PyTorch's fp32 evaluation [nb1][nb2][Tq][DH]"""
    DH, nb1, nb2, Tq, Tk, kind = ATTN[name]
    g = torch.Generator().manual_seed(1000 + sorted(ATTN).index(name))
    E = nb2 * DH
    ldq, ldk, ldv = E + 4, E + 8, E + 4
    c = dict(DH=DH, nb1=nb1, nb2=nb2, Tq=Tq, Tk=Tk, ldq=ldq, ldk=ldk, ldv=ldv, scale=DH ** -0.5)
    q = torch.randn(nb1, Tq, ldq, generator=g)
    k = torch.randn(nb1, Tk, ldk, generator=g)
    v = torch.randn(nb1, Tk, ldv, generator=g)
    if kind == "jump_late":
        k[:, 144:] *= 8.0
    if kind == "jump_early":
        k[:, :144] *= 8.0
    bias_h = bias_b = rel_h = rel_w = None
    c["ldbh"] = c["ldbb"] = Tk
    c["bb_off"] = 0
    if kind == "swin":
        bias_h = torch.randn(nb2, Tq, Tk, generator=g)
        bias_b = torch.where(torch.rand(nb1, Tq, Tk, generator=g) < 0.4, -100.0, 0.0)
        bias_b[0] = 0.0                                           # the unshifted window
    if kind in ("phrase", "phrase_odd"):
        from pyref_gdino.bert import masks_and_position_ids
        mask = masks_and_position_ids(torch.tensor(CC.caption_ids(Tk, 0)))[0]
        assert torch.equal(mask, CC.phrase_mask(CC.caption_ids(Tk, 0)))
        assert CC.blind_rows(mask) >= 1
        bias_b = CC.additive_mask(mask)[None]
        if kind == "phrase_odd":
            c["ldbb"], c["bb_off"] = 260, 1
    if kind == "mask_tail":
        bias_b = torch.zeros(1, Tq, Tk)
        bias_b[:, :, 140:] = F32MIN
        k[:, 140:] = 50.0
        v[:, 140:] = 1e30
    if kind in ("rel14", "rel17"):
        gw = 14 if kind == "rel14" else 17
        c["rel_gw"], c["ldrel"] = gw, gw + 3
        rel_h = torch.randn(nb1, Tq, nb2, c["ldrel"], generator=g)
        rel_w = torch.randn(nb1, Tq, nb2, c["ldrel"], generator=g)
    heads = lambda t, T: t[:, :, :E].reshape(nb1, T, nb2, DH).permute(0, 2, 1, 3)          # the view the strides describe
    qv, kv, vv = heads(q, Tq), heads(k, Tk), heads(v, Tk)
    refs = []
    for dt in (torch.float64, torch.float32):
        if kind == "mask_tail":                                   # the reference never sees the masked keys
            refs.append(R.attn_ref(qv, kv[:, :, :140], vv[:, :, :140], c["scale"], dtype=dt))
        else:
            gw = c.get("rel_gw", 0)
            refs.append(R.attn_ref(qv, kv, vv, c["scale"], bias_h, bias_b, None if rel_h is None else rel_h[..., :gw],
                                   None if rel_w is None else rel_w[..., :gw], gw, dtype=dt))
    c.update(q=q, k=k, v=v, bias_h=bias_h, bias_b=bias_b, rel_h=rel_h, rel_w=rel_w, ref64=refs[0], ref32=refs[1])
    return c


def _attn_launch(c, device, want_o=True, want_split=False, mutate=None):
    """-> (rc, o buffer [nb1][Tq+2][ldo] or None, (ohi, olo) or None); buffers on the CPU"""
    lib, L = _lib()
    nb1, nb2, Tq, Tk, DH = c["nb1"], c["nb2"], c["Tq"], c["Tk"], c["DH"]
    E = nb2 * DH
    keep = {n: c[n].to(device).contiguous() for n in ("q", "k", "v")}
    d = lib.OvmAttnF32Op()
    d.q, d.k, d.v = keep["q"].data_ptr(), keep["k"].data_ptr(), keep["v"].data_ptr()
    d.ldq, d.ldk, d.ldv = c["ldq"], c["ldk"], c["ldv"]
    d.sq1, d.sq2, d.sk1, d.sk2, d.sv1, d.sv2 = Tq * c["ldq"], DH, Tk * c["ldk"], DH, Tk * c["ldv"], DH
    d.nb1, d.nb2, d.Tq, d.Tk, d.DH, d.scale = nb1, nb2, Tq, Tk, DH, c["scale"]
    ldo, ldoh, rows = E + 8, E + 12, Tq + 2
    o = ohi = olo = None
    if want_o:
        o = torch.full((nb1, rows, ldo), SENT, device=device)
        d.o, d.ldo, d.so1, d.so2 = o.data_ptr(), ldo, rows * ldo, DH
    if want_split:
        ohi = torch.full((nb1, rows, ldoh), SENT, device=device, dtype=torch.float16)
        olo = torch.full((nb1, rows, ldoh), SENT, device=device, dtype=torch.float16)
        d.ohi, d.olo, d.ldoh, d.soh1, d.soh2 = ohi.data_ptr(), olo.data_ptr(), ldoh, rows * ldoh, DH
    if c["bias_h"] is not None:
        keep["bh"] = c["bias_h"].to(device).contiguous()
        d.bias_h, d.sbh, d.ldbh = keep["bh"].data_ptr(), Tq * c["ldbh"], c["ldbh"]
    if c["bias_b"] is not None:
        nbb, ldbb, off = c["bias_b"].shape[0], c["ldbb"], c["bb_off"]
        buf = torch.zeros(nbb * Tq * ldbb + 4)
        buf[off:off + nbb * Tq * ldbb].view(nbb, Tq, ldbb)[:, :, :Tk] = c["bias_b"]
        keep["bb"] = buf.to(device)
        d.bias_b, d.sbb, d.ldbb = keep["bb"].data_ptr() + 4 * off, (Tq * ldbb if nbb > 1 else 0), ldbb
    if c["rel_h"] is not None:
        keep["rh"], keep["rw"] = c["rel_h"].to(device).contiguous(), c["rel_w"].to(device).contiguous()
        d.rel_h, d.rel_w, d.rel_gw, d.ldrel = keep["rh"].data_ptr(), keep["rw"].data_ptr(), c["rel_gw"], c["ldrel"]
    if mutate:
        mutate(d)
    rc = L.ovm_g_attn_f32(C.byref(d), _stream())
    _finish(rc, "ovm_g_attn_f32")
    return rc, (o.cpu() if o is not None else None), ((ohi.cpu(), olo.cpu()) if ohi is not None else None)


def _attn_owned(c, buf):
    owned = torch.zeros(buf.shape, dtype=torch.bool)
    owned[:, :c["Tq"], :c["nb2"] * c["DH"]] = True
    return owned


def _attn_logical(c, buf):
    """[nb1][rows][ld] buffer -> [nb1][nb2][Tq][DH]"""
    return buf[:, :c["Tq"], :c["nb2"] * c["DH"]].reshape(c["nb1"], c["Tq"], c["nb2"], c["DH"]).permute(0, 2, 1, 3)


@pytest.mark.parametrize("name", sorted(ATTN))
def test_attn_f32_matches_fp64(device, name):
    c = _attn_case(name)
    rc, o, _ = _attn_launch(c, device)
    assert rc == 0, f"attn_f32 {name}: ovm_g_attn_f32 returned {rc}"
    _untouched(o, _attn_owned(c, o), f"attn_f32 {name}")
    _report("attn_f32", name, _attn_logical(c, o), c["ref64"], c["ref32"])


@pytest.mark.parametrize("name", ["f", "j", "m"])
def test_attn_f32_split_outputs(device, name):
    c = _attn_case(name)
    rc, o_both, (hi_both, lo_both) = _attn_launch(c, device, want_o=True, want_split=True)
    assert rc == 0
    rc, _, (hi_only, lo_only) = _attn_launch(c, device, want_o=False, want_split=True)
    assert rc == 0
    _untouched(o_both, _attn_owned(c, o_both), f"attn_f32 {name} (o, both kinds)")
    for tag, hi, lo in (("both kinds", hi_both, lo_both), ("split only", hi_only, lo_only)):
        owned = _attn_owned(c, hi)
        _untouched(hi, owned, f"attn_f32 {name} ohi ({tag})")
        _untouched(lo, owned, f"attn_f32 {name} olo ({tag})")
        # the launch without the fp32 output computes the same values: its split image is that of the other launch's fp32 output
        _assert_split(hi[owned], lo[owned], o_both[_attn_owned(c, o_both)], f"attn_f32 {name} ({tag})")
    _report("attn_f32", name + "/o+split", _attn_logical(c, o_both), c["ref64"], c["ref32"])
    y = hi_only.double() + lo_only.double()
    # hi + lo carries 22 bits of the fp32 value: 2^-22 of the largest output on top of the fp32 bound
    err, tol = rel_err(_attn_logical(c, y), c["ref64"]), R.bound(c["ref32"], c["ref64"]) + 2.0 ** -22
    print(f"FIG attn_f32 {name}/split-only err {err:.3e} bound {tol:.2e}")
    assert err <= tol


def test_attn_f32_refusals_leave_the_outputs_alone(device):
    _, L = _lib()
    assert L.ovm_g_attn_f32(None, _stream()) == OVM_ERR_INVALID
    c = _attn_case("e")

    def dh48(d):
        d.DH = 48

    def ldk_odd(d):
        d.ldk = d.ldk + 2

    def o_unaligned(d):
        d.o = d.o + 4

    for what, mutate in (("DH = 48", dh48), ("ldk % 4 != 0", ldk_odd), ("unaligned o", o_unaligned)):
        rc, o, (hi, lo) = _attn_launch(c, device, want_o=True, want_split=True, mutate=mutate)
        assert rc == OVM_ERR_SHAPE, f"{what}: returned {rc}"
        assert bool((o == SENT).all()) and bool((hi == SENT).all()) and bool((lo == SENT).all()), f"{what}: outputs written"


# ========================================================================================= multi-scale deformable attention
G0 = ((7, 9), (4, 5), (2, 3), (1, 1))
#            shapes                 P   H  dh   Q  mode  kind      split
MSD = {
    "enc": (G0, 4, 4, 8, 37, 0, "random", False),
    "dec": (G0, 4, 4, 8, 37, 1, "random", False),
    "dh4": (G0, 4, 4, 4, 37, 0, "random", False),
    "dh32": (G0, 4, 4, 32, 37, 1, "random", False),
    "L2P8": (((7, 9), (4, 5)), 8, 4, 8, 37, 0, "random", False),
    "L1P16": (((7, 9),), 16, 4, 8, 37, 1, "random", False),
    "L3P3dh6": (((7, 9), (4, 5), (2, 3)), 3, 4, 6, 37, 0, "random", False),     # only the per-channel kernel runs here
    "split": (G0, 4, 4, 8, 37, 0, "random", True),
    "edges_enc": (G0, 4, 4, 8, 37, 0, "edges", False),
    "edges_dec": (G0, 4, 4, 8, 37, 1, "edges", True),
    "logits80": (G0, 4, 4, 8, 37, 0, "logits80", False),
}


def _edge_offsets(shapes, P, H, Q, mode):
    """offsets [Q][H][L][P][2] (for ref point (0, 0) / box (0, 0, 1, 1)) whose samples land exactly on pixel centres, on the outer
    edge (ix = -0.5, W - 0.5), where all taps fall out of range (ix = -1, W), 1e4 pixels outside, and inside again"""
    off = torch.zeros(Q, H, len(shapes), P, 2, dtype=torch.float64)
    for l, (hl, wl) in enumerate(shapes):
        for axis, n in ((0, wl), (1, hl)):
            places = [0.0, float(n - 1), float(min(1, n - 1)), -0.5, n - 0.5, -1.0, float(n), n + 1e4, -1e4, 0.25 * n, 0.5 * n - 0.5]
            i = torch.arange(Q * H * P).reshape(Q, H, P)
            pick = (i if axis == 0 else i // len(places) + i) % len(places)
            ix = torch.tensor(places, dtype=torch.float64)[pick]
            # mode 0: ix = off - 0.5 (loc = off / n); mode 1: loc = off * 0.5 / P, ix = loc * n - 0.5
            off[:, :, l, :, axis] = (ix + 0.5) if mode == 0 else (ix + 0.5) / n * 2.0 * P
    return off


@lru_cache(maxsize=None)
def _msd_case(name):
    shapes, P, H, dh, Q, mode, kind, split = MSD[name]
    g = torch.Generator().manual_seed(2000 + sorted(MSD).index(name))
    L, S, n = len(shapes), sum(h * w for h, w in shapes), H * len(shapes) * P
    ldv, ldow, ldref = H * dh + 4, 3 * n + 4, (2 if mode == 0 else 4)
    value = torch.randn(S, ldv, generator=g)
    ow = torch.randn(Q, ldow, generator=g)
    ref = torch.rand(Q, ldref, generator=g)
    # sampling locations spread over [-0.2, 1.2]: beyond every border of every level
    loc = torch.rand(Q, H, L, P, 2, generator=g, dtype=torch.float64) * 1.4 - 0.2
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64)[None, None, :, None, :]
    if mode == 0:
        off = (loc - ref[:, None, None, None, :2].double()) * norm
    else:
        ref[:, 2:] = 0.05 + 0.9 * ref[:, 2:]
        off = (loc - ref[:, None, None, None, :2].double()) / (ref[:, None, None, None, 2:4].double() * 0.5 / P)
    if kind == "edges":
        ref[:, :2] = 0.0
        if mode == 1:
            ref[:, 2:] = 1.0
        off = _edge_offsets(shapes, P, H, Q, mode)
        if mode == 1:                                             # boxes with w = h = 0: every point samples the centre
            ref[:5, :2] = torch.rand(5, 2, generator=g)
            ref[:5, 2:] = 0.0
    ow[:, :2 * n] = off.reshape(Q, 2 * n).float()
    if kind == "logits80":
        ow[:, 2 * n:3 * n] = torch.rand(Q, n, generator=g) * 160.0 - 80.0
    args = (value[:, :H * dh], ow[:, :3 * n], ref, mode, H, dh, L, P, shapes)
    return dict(shapes=shapes, P=P, H=H, dh=dh, Q=Q, mode=mode, L=L, S=S, ldv=ldv, ldow=ldow, ldref=ldref, split=split, value=value, ow=ow,
                ref=ref, ref64=R.msdeform_ref(*args, dtype=torch.float64), ref32=R.msdeform_ref(*args, dtype=torch.float32))


def _msd_launch(c, device, vec):
    lib, L = _lib()
    Q, E = c["Q"], c["H"] * c["dh"]
    keep = {n: c[n].to(device).contiguous() for n in ("value", "ow", "ref")}
    d = lib.OvmMsDeformOp()
    d.value, d.ow, d.ref = keep["value"].data_ptr(), keep["ow"].data_ptr(), keep["ref"].data_ptr()
    d.ldv, d.ldow, d.ldref, d.mode = c["ldv"], c["ldow"], c["ldref"], c["mode"]
    d.Q, d.H, d.dh, d.L, d.P = Q, c["H"], c["dh"], c["L"], c["P"]
    start = 0
    for l, (hl, wl) in enumerate(c["shapes"]):
        d.lh[l], d.lw[l], d.lstart[l] = hl, wl, start
        start += hl * wl
    assert start == c["S"]
    ldo, ldoh = E + 4, E + 8
    out = torch.full((Q + 2, ldo), SENT, device=device)
    d.out, d.ldo = out.data_ptr(), ldo
    hi = lo = None
    if c["split"]:
        hi = torch.full((Q + 2, ldoh), SENT, device=device, dtype=torch.float16)
        lo = torch.full((Q + 2, ldoh), SENT, device=device, dtype=torch.float16)
        d.ohi, d.olo, d.ldoh = hi.data_ptr(), lo.data_ptr(), ldoh
    try:
        assert L.ovm_tune_set(b"msdeform_vec", vec) == 0
        rc = L.ovm_g_msdeform_fused(C.byref(d), _stream())
        _finish(rc, "ovm_g_msdeform_fused")
    finally:
        L.ovm_tune_set(b"msdeform_vec", 1)
    return rc, out.cpu(), (hi.cpu() if hi is not None else None), (lo.cpu() if lo is not None else None)


@pytest.mark.parametrize("name", sorted(MSD))
def test_msdeform_fused_matches_fp64(device, name):
    c = _msd_case(name)
    Q, E = c["Q"], c["H"] * c["dh"]
    outs = {}
    for vec in (1, 0):
        rc, out, hi, lo = _msd_launch(c, device, vec)
        assert rc == 0, f"msdeform {name} vec {vec}: returned {rc}"
        owned = torch.zeros(out.shape, dtype=torch.bool)
        owned[:Q, :E] = True
        _untouched(out, owned, f"msdeform {name} vec {vec}")
        if hi is not None:
            oh = torch.zeros(hi.shape, dtype=torch.bool)
            oh[:Q, :E] = True
            _untouched(hi, oh, f"msdeform {name} vec {vec} ohi")
            _untouched(lo, oh, f"msdeform {name} vec {vec} olo")
            _assert_split(hi[:Q, :E], lo[:Q, :E], out[:Q, :E], f"msdeform {name} vec {vec}")
        _report("msdeform", f"{name}/vec{vec}", out[:Q, :E], c["ref64"], c["ref32"])
        outs[vec] = out[:Q, :E]
    if c["L"] * c["P"] == 16 and c["dh"] % 4 == 0:               # the float4 kernel ran: same operations in the same order
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"msdeform {name}: the two kernels differ"


# ============================================================================================================ row operator
#            D    ln     gather(zero_masked)  res    add    y      y2     hilo   il  hilo2
ROWOP = {
    "ln64_gather": (64, True, 0, False, False, True, False, True, 0, False),
    "ln64_gather_zm_add": (64, True, 1, False, True, True, True, False, 0, True),
    "ln70_gather_zm_res": (70, True, 1, True, False, True, False, True, 0, False),
    "ln96_res_add": (96, True, None, True, True, True, True, True, 0, True),
    "ln256_gather_il": (256, True, 0, False, False, True, False, True, 1, False),
    "ln256_gather_zm_res_add": (256, True, 1, True, True, False, True, False, 0, True),
    "ln1024_res": (1024, True, None, True, False, True, False, True, 0, False),
    "ln1028_add": (1028, True, None, False, True, True, True, False, 0, True),
    "ln4096_add": (4096, True, None, False, True, True, True, True, 0, False),
    "copy256_gather_res_il": (256, False, 0, True, False, True, False, True, 1, False),
    "copy70_add": (70, False, None, False, True, True, True, True, 0, True),
}
ROW_M = (1, 5, 130)
NSRC, ADD_ROWS, EPS = 50, 7, 1e-5


@lru_cache(maxsize=None)
def _row_case(name, M):
    D, ln, gather, res, add, *_ = ROWOP[name]
    g = torch.Generator().manual_seed(3000 + 10 * sorted(ROWOP).index(name) + ROW_M.index(M))
    c = dict(D=D, M=M)
    if gather is not None:
        seg = D // 2
        c["seg"], c["ldx"] = seg, seg + 4
        c["x"] = torch.randn(NSRC, c["ldx"], generator=g)
        idx = torch.randint(-1, NSRC, (M, 2), generator=g, dtype=torch.int32)
        idx[0, 1] = -1
        if M > 1:
            idx[1, 0], idx[2, 0], idx[2, 1] = -1, -1, -1
        c["idx"] = idx
    else:
        c["seg"], c["ldx"] = 0, D + 4
        c["x"] = torch.randn(M, c["ldx"], generator=g) + 0.5
    c["res"] = torch.randn(M, D + 4, generator=g) if res else None
    c["gamma"] = 1.0 + 0.2 * torch.randn(D, generator=g) if ln else None
    c["beta"] = 0.2 * torch.randn(D, generator=g) if ln else None
    c["add"] = torch.randn(ADD_ROWS, D + 4, generator=g) if add else None
    refs = [R.rowop_ref(c["x"], M, D, c.get("idx"), c["seg"], c["res"], c["gamma"], c["beta"], EPS, bool(gather), c["add"], ADD_ROWS, dtype=dt)
            for dt in (torch.float64, torch.float32)]
    c["ref64"], c["ref32"] = refs
    return c


def _row_launch(c, name, device, mutate=None):
    lib, L = _lib()
    D, ln, gather, res, add, want_y, want_y2, want_h, il, want_h2 = ROWOP[name]
    M = c["M"]
    keep = {n: c[n].to(device).contiguous() for n in ("x", "idx", "res", "gamma", "beta", "add") if c.get(n) is not None}
    ptr = lambda n: keep[n].data_ptr() if n in keep else None
    d = lib.OvmRowOp()
    d.x, d.idx, d.res, d.gamma, d.beta, d.add = ptr("x"), ptr("idx"), ptr("res"), ptr("gamma"), ptr("beta"), ptr("add")
    d.ldx, d.nidx, d.seg, d.ldr, d.eps = c["ldx"], (2 if gather is not None else 0), c["seg"], D + 4, EPS
    d.zero_masked, d.ld_add, d.add_rows, d.M, d.D = (1 if gather else 0), D + 4, ADD_ROWS, M, D
    out = {}
    if want_y:
        out["y"] = torch.full((M + 2, D + 8), SENT, device=device)
        d.y, d.ldy = out["y"].data_ptr(), D + 8
    if want_y2:
        out["y2"] = torch.full((M + 2, D + 12), SENT, device=device)
        d.y2, d.ldy2 = out["y2"].data_ptr(), D + 12
    if want_h:
        if il:                                                    # ONE image [row][k/32][hi 32 | lo 32]: lo starts 32 halves after hi
            out["h"] = torch.full((M + 2, 2 * D), SENT, device=device, dtype=torch.float16)
            d.hi, d.lo, d.ldh, d.il = out["h"].data_ptr(), out["h"].data_ptr() + 64, 2 * D, 1
        else:
            out["h"] = torch.full((2, M + 2, D + 24), SENT, device=device, dtype=torch.float16)
            d.hi, d.lo, d.ldh = out["h"][0].data_ptr(), out["h"][1].data_ptr(), D + 24
    if want_h2:
        out["h2"] = torch.full((2, M + 2, D + 24), SENT, device=device, dtype=torch.float16)
        d.hi2, d.lo2, d.ldh2 = out["h2"][0].data_ptr(), out["h2"][1].data_ptr(), D + 24
    if mutate:
        mutate(d)
    rc = L.ovm_g_rowop(C.byref(d), _stream())
    _finish(rc, "ovm_g_rowop")
    return rc, {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("name", sorted(ROWOP))
def test_rowop_matches_fp64(device, name):
    D, ln, gather, res, add, want_y, want_y2, want_h, il, want_h2 = ROWOP[name]
    for M in ROW_M:
        c = _row_case(name, M)
        rc, out = _row_launch(c, name, device)
        assert rc == 0, f"rowop {name} M {M}: returned {rc}"
        tag = f"{name}/M{M}"
        for key, r64, r32 in (("y", c["ref64"][0], c["ref32"][0]), ("y2", c["ref64"][1], c["ref32"][1])):
            if key in out:
                buf = out[key]
                owned = torch.zeros(buf.shape, dtype=torch.bool)
                owned[:M, :D] = True
                _untouched(buf, owned, f"rowop {tag} {key}")
                _report("rowop", f"{tag}/{key}", buf[:M, :D], r64, r32)
        if gather and "y" in out:                                 # zero_masked rows are exactly zero
            masked = c["idx"][:, 0] < 0
            assert bool((out["y"][:M, :D][masked] == 0).all())
        if want_h:
            y = out["y"][:M, :D]
            if il:
                img = out["h"]
                assert bool((img[M:] == SENT).all()), f"rowop {tag}: interleaved image, rows past M written"
                cols = torch.tensor([R.il_col(n) for n in range(D)])
                _assert_split(img[:M][:, cols], img[:M][:, cols + 32], y, f"rowop {tag} (interleaved)")
            else:
                hi, lo = out["h"][0], out["h"][1]
                assert bool((hi[M:] == SENT).all()) and bool((lo[M:] == SENT).all()), f"rowop {tag}: split rows past M written"
                _assert_split(hi[:M, :D], lo[:M, :D], y, f"rowop {tag}")
                assert bool((hi[:M, D:] == 0).all()) and bool((lo[:M, D:] == 0).all()), f"rowop {tag}: K padding of hi / lo not zero"
        if want_h2:
            hi, lo = out["h2"][0], out["h2"][1]
            assert bool((hi[M:] == SENT).all()) and bool((lo[M:] == SENT).all()), f"rowop {tag}: split rows past M written (y2)"
            _assert_split(hi[:M, :D], lo[:M, :D], out["y2"][:M, :D], f"rowop {tag} (y2)")
            assert bool((hi[:M, D:] == 0).all()) and bool((lo[:M, D:] == 0).all()), f"rowop {tag}: K padding of hi2 / lo2 not zero"


def test_rowop_refusals_leave_the_outputs_alone(device):
    _, L = _lib()
    assert L.ovm_g_rowop(None, _stream()) == OVM_ERR_INVALID
    assert L.ovm_g_msdeform_fused(None, _stream()) == OVM_ERR_INVALID

    def run(name, D, want, ldx=None, il=0):
        """the case `name` with its width declared as D (nothing is launched, so the buffers' real sizes do not matter)"""
        c = _row_case(name, 5)

        def mutate(d):
            d.D = D
            if ldx is not None:
                d.ldx = ldx
            if il:
                d.il, d.lo, d.ldh = 1, d.hi + 64, 2 * D
        rc, out = _row_launch(c, name, device, mutate)
        assert rc == want, f"D = {D}: returned {rc}, expected {want}"
        for k, v in out.items():
            assert bool((v == SENT).all()), f"D = {D}: output {k} written"

    run("ln4096_add", 4100, OVM_ERR_SHAPE)                        # float4 route, LayerNorm row too long for the registers
    run("ln1024_res", 1030, OVM_ERR_SHAPE)                        # D % 4 != 0: the scalar route holds 1024
    run("ln64_gather", 48, OVM_ERR_INVALID, il=1)                 # an interleaved image needs whole groups of 32 columns
