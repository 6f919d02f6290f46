"""swin7_qkv_attn_kernel (a Swin-T block's qkv projection + 7 x 7 window attention in one launch) through ovm_g_swin_qkv_attn, the
launcher the engine calls, against a float64 restatement on the inputs the kernel sees: activation rows and weights as the exact sums
hi + lo of their split-fp16 images, bias, relative-position bias, shift mask and softmax in float64.

Bound: 4 x the error of the same computation in plain fp32 torch on the CPU against the float64 one, on the same inputs (the
convention of test_sam_cpu.py / test_gpu_eval3d.py; common.rel_err = max |a - b| / max |b|). Every case runs with 1, 2 and 4 windows
per workgroup and the default, prints `FIG swin7 <case> wpg <n> err <measured> fp32 <torch fp32> bound <bound>`, pre-fills the
outputs with a sentinel and checks that nothing outside the context rows' C columns was written.

Measured on an MI355X (this file's seeds), 18 cases x 4 workgroup shapes: err 4.6e-07 .. 1.1e-06 with torch fp32 at 4.9e-07 .. 1.2e-06,
err / fp32 between 0.52 and 1.40 of the allowed 4; the workgroup shapes of a case give the same error. The ws = 12 case: err 9.1e-07,
fp32 8.6e-07 (ratio 1.06)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from common import rel_err

pytestmark = pytest.mark.gpu

SENT = -7.5                 # exact in fp16
OVM_ERR_INVALID, OVM_ERR_HIP, OVM_ERR_SHAPE = -1, -2, -4


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


def _split(x32):
    hi = x32.half()
    lo = (x32 - hi.float()).half()
    return hi, lo


def _frag(w32, Kpad):
    """[3 C][C] fp32 -> (fragment-ordered split image as int16 numpy, the exact weights hi + lo as float64 [3 C][C])"""
    _, L = _lib()
    N, K = w32.shape
    Npad, KS = (N + 127) // 128 * 128, Kpad // 32
    w = np.ascontiguousarray(w32.numpy(), dtype=np.float32)
    img = np.zeros(Npad * Kpad * 2, dtype=np.uint16)
    assert L.ovm_host_pack_weight(w.ctypes.data, N, K, Kpad, 3, img.ctypes.data) == 0
    img = img.reshape(Npad, KS, 2, 32)
    halves = torch.from_numpy(img.view(np.int16).copy()).view(torch.float16).double()
    exact = (halves[:, :, 0, :] + halves[:, :, 1, :]).reshape(Npad, Kpad)[:N, :K].contiguous()
    # [tile][row r][ks][part][quarter q][8] -> [tile][ks][part][lane = 16 q + r][8]
    frag = img.reshape(Npad // 16, 16, KS, 2, 4, 8).transpose(0, 2, 3, 4, 1, 5)
    return np.ascontiguousarray(frag).view(np.int16).reshape(-1), exact


def _inputs(C_, nh, nW, ws, masked, zero_rows, seed):
    g = torch.Generator().manual_seed(seed)
    T = ws * ws
    x = torch.randn(nW * T, C_, generator=g)
    if zero_rows:                                               # a padded window: its last rows are zero after the norm
        x[(nW // 2) * T + T - zero_rows:(nW // 2 + 1) * T] = 0.0
    xhi, xlo = _split(x)
    w = torch.randn(3 * C_, C_, generator=g) * (1.5 / math.sqrt(C_))
    bias = torch.randn(3 * C_, generator=g) * 0.1
    relbias = torch.randn(nh, T, T, generator=g) * 0.5
    mask = None
    if masked:                                                  # the shift mask's values: 0 / -100 between regions of a window
        region = torch.randint(0, 3, (nW, T), generator=g)
        mask = torch.where(region[:, :, None] != region[:, None, :], torch.tensor(-100.0), torch.tensor(0.0)).contiguous()
        mask[0] = 0.0
    return xhi, xlo, w, bias, relbias, mask


def _reference(xhi, xlo, w_exact, bias, relbias, mask, C_, nh, nW, ws, dtype):
    T = ws * ws
    x = (xhi.double() + xlo.double()).to(dtype)
    qkv = x @ w_exact.to(dtype).t() + bias.to(dtype)
    q, k, v = (qkv[:, i * C_:(i + 1) * C_].reshape(nW, T, nh, 32).permute(0, 2, 1, 3) for i in range(3))
    s = (q @ k.transpose(-1, -2)) * (1.0 / math.sqrt(32.0)) + relbias.to(dtype)[None]
    if mask is not None:
        s = s + mask.to(dtype)[:, None]
    o = torch.softmax(s, -1) @ v
    return o.permute(0, 2, 1, 3).reshape(nW * T, C_)


def _run(device, C_, nh, nW, ws, masked, zero_rows, wide, seed, wpgs):
    lib, L = _lib()
    T = ws * ws
    KS = (C_ + 63) // 64 * 2 + (2 if wide else 0)               # Kpad = roundup(C, 64), as the engine packs; wide: one pad k-step pair more
    Kpad = 32 * KS
    ldx, ldo = (Kpad + 8, C_ + 12) if wide else (Kpad, C_)
    xhi, xlo, w, bias, relbias, mask = _inputs(C_, nh, nW, ws, masked, zero_rows, seed)
    frag, w_exact = _frag(w, Kpad)
    ref64 = _reference(xhi, xlo, w_exact, bias, relbias, mask, C_, nh, nW, ws, torch.float64)
    ref32 = _reference(xhi, xlo, w_exact, bias, relbias, mask, C_, nh, nW, ws, torch.float32)
    e32 = rel_err(ref32, ref64)
    bound = 4.0 * e32
    M = nW * T
    dxh = torch.zeros(M, ldx, dtype=torch.float16); dxh[:, :C_] = xhi
    dxl = torch.zeros(M, ldx, dtype=torch.float16); dxl[:, :C_] = xlo
    dxh, dxl = dxh.to(device), dxl.to(device)
    dfrag = torch.from_numpy(frag).to(device)
    dbias, drel = bias.to(device), relbias.contiguous().to(device)
    dmask = mask.to(device) if mask is not None else None
    owned = torch.zeros(M + 3, ldo, dtype=torch.bool)
    owned[:M, :C_] = True
    errs = {}
    for wpg in wpgs:
        ohi = torch.full((M + 3, ldo), SENT, dtype=torch.float16, device=device)
        olo = torch.full((M + 3, ldo), SENT, dtype=torch.float16, device=device)
        op = lib.OvmSwinQkvAttnOp()
        op.xhi, op.xlo, op.wfrag, op.bias, op.relbias = dxh.data_ptr(), dxl.data_ptr(), dfrag.data_ptr(), dbias.data_ptr(), drel.data_ptr()
        op.mask = dmask.data_ptr() if dmask is not None else None
        op.ohi, op.olo = ohi.data_ptr(), olo.data_ptr()
        op.ldx, op.KS, op.C, op.nh, op.nW, op.ldo, op.scale, op.ws, op.wpg = ldx, KS, C_, nh, nW, ldo, 1.0 / math.sqrt(32.0), ws, wpg
        rc = L.ovm_g_swin_qkv_attn(C.byref(op), _stream())
        _finish(rc, f"ovm_g_swin_qkv_attn C {C_} nW {nW} wpg {wpg}")
        assert rc == 0, rc
        ohi, olo = ohi.cpu(), olo.cpu()
        for buf in (ohi, olo):
            assert bool((buf[~owned] == SENT).all()), "the kernel wrote outside the context rows"
        got = ohi[:M, :C_].double() + olo[:M, :C_].double()
        err = rel_err(got, ref64)
        errs[wpg] = err
        print(f"FIG swin7 ws {ws} C {C_} nh {nh} nW {nW} mask {int(masked)} zero {zero_rows} wide {int(wide)} wpg {wpg} "
              f"err {err:.3e} fp32 {e32:.3e} bound {bound:.3e} ratio {err / max(e32, 1e-30):.2f}")
        assert torch.isfinite(got).all()
    for wpg, err in errs.items():
        assert err <= bound, f"wpg {wpg}: error {err:.3e} against fp64 > 4 x torch fp32 ({e32:.3e})"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nW", [1, 5, 12])
@pytest.mark.parametrize("C_,nh", [(96, 3), (192, 6), (384, 12)])
def test_swin7_qkv_attn_matches_fp64(device, C_, nh, nW, masked):
    """nW = 5: one window with its last 14 rows zero (as the partition pads), row strides larger than C and pad k-steps beyond
    roundup(C, 64); nW = 1 / 12: tight strides. 5 is no multiple of 2 or 4: the last workgroup of a head has windows missing."""
    odd = nW == 5
    _run(device, C_, nh, nW, 7, masked, 14 if odd else 0, odd, 100 * nh + 10 * nW + int(masked), (0, 1, 2, 4))


def test_swin12_through_the_same_entry_point_matches_fp64(device):
    """The descriptor carries the window side: a Swin-B-shaped call (ws = 12, C = 128) reaches swin_qkv_attn_kernel. Same reference,
    same bound as the 7 x 7 cases; the bits are held by the A/B below."""
    _run(device, 128, 4, 3, 12, True, 0, False, 7, (0,))


@pytest.mark.parametrize("ws", [12, 7])
def test_entry_point_equals_the_engines_fused_path_bit_for_bit(device, ws):
    """A/B on bits: the engine runs a Swin-B-shaped (ws = 12, C = 128) or Swin-T-shaped (ws = 7, C = 96) network with
    ovm_tune_set gdino_swin_tap = 2, which keeps its second Swin block's (stage 0, shifted: with the mask) window rows and context rows;
    ovm_g_swin_qkv_attn on those rows, that block's fragment image, bias, relative-position bias and mask must give the engine's
    context rows in every bit. 100 x 130 pixels: a 25 x 33 token map, padded windows on both axes."""
    from ovmono3d_amd.gdino.config import GDinoConfig
    from ovmono3d_amd.gdino.engine import GdinoEngine
    from ovmono3d_amd.util.synth_gdino_weights import synth_gdino_state_dict
    lib, L = _lib()
    C_, heads = (128, (4, 8, 16, 32)) if ws == 12 else (96, (3, 6, 12, 24))
    cfg = GDinoConfig(d_model=64, enc_layers=1, dec_layers=1, heads=4, ffn_dim=128, num_queries=30, bert_heads=2, swin_embed=C_,
                      swin_depths=(2, 2, 2, 2), swin_heads=heads, swin_window=ws)
    sd = synth_gdino_state_dict(11, cfg, bert_hidden=64, bert_layers=1, bert_ffn=128, vocab=2000)
    H, W = 100, 130
    img = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(device)
    try:
        assert L.ovm_tune_set(b"gdino_swin_tap", 2) == 0
        eng = GdinoEngine(device, sd, cfg, use_graphs=False)
        eng.forward(img, [101, 500, 1012, 600, 601, 1012, 102])       # the plan is built here, under the knob
    finally:
        L.ovm_tune_set(b"gdino_swin_tap", 0)
    T, nh = ws * ws, heads[0]
    nW = -(-((H + 3) // 4) // ws) * -(-((W + 3) // 4) // ws)
    M, ld, Npad = nW * T, (C_ + 63) // 64 * 64, (3 * C_ + 127) // 128 * 128
    halves = lambda name: eng.debug(name, (M, ld // 2), torch.int32).view(torch.int16)     # [M][ld] halves
    xhi, xlo, ohi, olo = (halves("swin_tap_" + n) for n in ("xhi", "xlo", "ohi", "olo"))
    wfrag = eng.debug("swin_tap_wfrag", (Npad * ld,), torch.int32)
    bias, rel, mask = eng.debug("swin_tap_bias", (3 * C_,)), eng.debug("swin_tap_relbias", (nh, T, T)), eng.debug("swin_tap_mask", (nW, T, T))
    assert bool((mask != 0).any()) and bool((xhi[:, :C_] != 0).any()) and bool((ohi[:, :C_] != 0).any())
    mine_hi, mine_lo = torch.zeros_like(ohi), torch.zeros_like(olo)
    op = lib.OvmSwinQkvAttnOp()
    op.xhi, op.xlo, op.wfrag, op.bias, op.relbias, op.mask = (t.data_ptr() for t in (xhi, xlo, wfrag, bias, rel, mask))
    op.ohi, op.olo = mine_hi.data_ptr(), mine_lo.data_ptr()
    op.ldx, op.KS, op.C, op.nh, op.nW, op.ldo, op.scale, op.ws, op.wpg = ld, ld // 32, C_, nh, nW, ld, 1.0 / math.sqrt(32.0), ws, 0
    rc = L.ovm_g_swin_qkv_attn(C.byref(op), _stream())
    _finish(rc, f"ovm_g_swin_qkv_attn on the engine's rows, ws {ws}")
    assert rc == 0, rc
    assert torch.equal(mine_hi[:, :C_], ohi[:, :C_]) and torch.equal(mine_lo[:, :C_], olo[:, :C_])


def test_unsupported_geometry_is_refused_and_nothing_is_written(device):
    lib, L = _lib()
    assert L.ovm_g_swin_qkv_attn(None, _stream()) == OVM_ERR_INVALID
    ws, C_, nW = 5, 80, 2
    z16 = lambda *s: torch.zeros(*s, dtype=torch.float16, device=device)
    # every buffer is large enough for the largest geometry named below: a call that is not refused still stays inside them
    xh, xl, fr = z16(2 * 144, 128), z16(2 * 144, 128), z16(512 * 128 * 2)
    bias, rel = torch.zeros(3 * 128, device=device), torch.zeros(5, 144, 144, device=device)
    ohi = torch.full((2 * 144 + 1, 128), SENT, dtype=torch.float16, device=device)
    olo = torch.full((2 * 144 + 1, 128), SENT, dtype=torch.float16, device=device)

    def call(**kw):
        op = lib.OvmSwinQkvAttnOp()
        op.xhi, op.xlo, op.wfrag, op.bias, op.relbias, op.mask = xh.data_ptr(), xl.data_ptr(), fr.data_ptr(), bias.data_ptr(), rel.data_ptr(), None
        op.ohi, op.olo = ohi.data_ptr(), olo.data_ptr()
        vals = dict(ldx=96, KS=3, C=C_, nh=C_ // 32, nW=nW, ldo=C_, scale=0.17, ws=ws, wpg=0)
        vals.update(kw)
        for k, v in vals.items():
            setattr(op, k, v)
        rc = L.ovm_g_swin_qkv_attn(C.byref(op), _stream())
        _finish(rc, "ovm_g_swin_qkv_attn refusal")
        return rc
    assert call() == OVM_ERR_SHAPE                                  # ws = 5, C = 80
    assert call(ws=7) == OVM_ERR_SHAPE                              # C = 80 is not 32 nh
    assert call(ws=7, C=64, nh=2, wpg=3) == OVM_ERR_SHAPE           # 3 windows per workgroup is not built
    assert call(ws=12, C=64, nh=2, KS=2) == OVM_ERR_SHAPE           # the 144-row kernel wants C % 128 == 0
    for w_, kw in ((7, dict(C=64, nh=2)), (12, dict(C=128, nh=4, KS=4, ldx=128))):      # context rows are stored 8 bytes at a time
        op_ok = dict(ws=w_, ldo=128, **kw)
        assert call(**op_ok, ohi=ohi.data_ptr() + 2) == OVM_ERR_SHAPE and call(**op_ok, olo=olo.data_ptr() + 4) == OVM_ERR_SHAPE
    assert bool((ohi == SENT).all()) and bool((olo == SENT).all())
