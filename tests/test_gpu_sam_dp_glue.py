"""The glue kernels of the SAM and Depth Pro engines (csrc/sam.hip, csrc/depthpro.hip), each through its own ovm_op_sam_* / ovm_op_dp_*
entry point, and the generic ops under SAM's token attention with the engine's own strides, against the fp64 restatement of
tests/sam_dp_glue_ref.py (itself checked on the CPU by tests/test_sam_dp_glue_ref_cpu.py, torch in float64 and mutations included).

Rules (none chosen here): plain fp32 kernels meet roi_glue_ref.bound, max |got - fp64| <= 4 * E32 + one fp32 ulp of the largest |fp64|,
E32 = the fp32 run of the restatement against fp64, per case and never from the kernel's output; split outputs after render, hi alone
with bound_hi_only. The head tail (matrix cores) meets gemm_epi_ref.tolerance with K = 9 C on the operands the kernel sees. Masks
follow tests/test_gpu_sam.py: exact outside the band (= the bound of the resampled logit), at most 1 % of a mask inside. Re-layouts,
copies and refusals are bit for bit. Every destination is pre-filled with a sentinel and must keep it outside the kernel's range; after
a refusal it holds nothing else. Each test prints E32 and the measured error per case; the worst of a run on an MI355X stands next
to each test (E32 / measured error).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import roi_glue_ref as R
import sam_dp_glue_ref as S
from sam_dp_glue_ref import F32, F64, SENTINEL

pytestmark = pytest.mark.gpu
OVM_ERR_INVALID, OVM_ERR_SHAPE = -1, -4
S16 = int(np.float16(SENTINEL).view(np.uint16))
BYTE = 0x5A


def _lib():
    from ovmono3d_amd import lib
    return lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _f32(shape, device):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), SENTINEL, dtype=torch.float32, device=device)


def _h16(shape, device):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), SENTINEL, dtype=torch.float16, device=device)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _untouched(a, what):
    a = np.asarray(a)
    if a.dtype == np.uint8:
        ok = np.all(a == BYTE)
    elif a.dtype == np.float16:
        ok = np.all(R.bits(a) == S16)
    else:
        ok = np.all(a == F32(SENTINEL))
    assert ok, f"{what}: the sentinel was overwritten"


def _strided(a, ld, device):
    """rows [M][w] -> device buffer [M][ld] with the sentinel behind every row; returns the buffer"""
    M, w = a.shape
    buf = np.full((M, ld), SENTINEL, dtype=a.dtype)
    buf[:, :w] = a
    return _dev(buf, device)


class Worst:
    def __init__(self, kernel):
        self.kernel, self.w = kernel, {}

    def add(self, case, figures):
        for name, (e32, err) in figures.items():
            print(f"\n{self.kernel} {S.case_id(case)} {name}: E32 {e32:.3e} err {err:.3e}", end="")
            a = self.w.setdefault(name, [0.0, 0.0])
            a[0], a[1] = max(a[0], e32), max(a[1], err)

    def done(self):
        print(f"\n{self.kernel} worst: " + ", ".join(f"{k} {v[0]:.2e} / {v[1]:.2e}" for k, v in self.w.items()))


def _refs(kernel, case):
    inp = S.inputs(kernel, case)
    return inp, S.run(kernel, case, inp, F64), S.run(kernel, case, inp, F32)


# ================================================================================================ SAM
# MI355X, worst over the cases (E32 / error): pe 1.49e-06 / 1.49e-06
def test_dense_pe(device):
    """G in {2, 5}, F in {32, 128}"""
    w = Worst("dense_pe")
    for case in S.CASES["dense_pe"]:
        inp, r64, r32 = _refs("dense_pe", case)
        G, F = case["G"], case["F"]
        pe = _f32((G * G + 1, 2 * F), device)
        g = _dev(inp["gauss"], device)
        assert _lib().ovm_op_sam_dense_pe(g.data_ptr(), G, F, pe.data_ptr(), _stream()) == 0
        pe = _np(pe)
        _untouched(pe[-1], "dense_pe")
        w.add(case, S.compare("dense_pe", case, dict(pe=pe[:-1]), r64, r32))
    w.done()


# MI355X, worst over the cases (E32 / error): corners 2.42e-06 / 2.42e-06; the token rows and `sparse` bit-equal
def test_box_tokens(device):
    """nb in {1, 3}, C in {64, 256}, nout = 5; negative, fractional and beyond-the-image corners; 70 x 100 and 99 x 71 in a 128 frame."""
    w = Worst("box_tokens")
    for case in S.CASES["box_tokens"]:
        inp, r64, r32 = _refs("box_tokens", case)
        nb, Cc, (H, W, Sz) = case["nb"], case["C"], case["frame"]
        nh, nw = S.preprocess_shape(H, W, Sz)
        tok, sparse = _f32((nb + 1, 7, Cc), device), _f32((nb + 1, 2, Cc), device)
        d = {k: _dev(inp[k], device) for k in ("boxes", "out_tokens", "gauss", "corner")}
        rc = _lib().ovm_op_sam_box_tokens(d["boxes"].data_ptr(), nb, 5, Cc, d["out_tokens"].data_ptr(), d["gauss"].data_ptr(), d["corner"].data_ptr(),
                                          H, W, nh, nw, Sz, tok.data_ptr(), sparse.data_ptr(), _stream())
        assert rc == 0
        tok, sparse = _np(tok), _np(sparse)
        _untouched(tok[-1], "tok")
        _untouched(sparse[-1], "sparse")
        assert S.same_bits(tok[:nb, 5:], sparse[:nb]), "sparse is not the two corner rows of tok"
        w.add(case, S.compare("box_tokens", case, dict(corners=sparse[:nb], head=tok[:nb, :5]), r64, r32))
    w.done()
    tok, sparse = _f32((2, 7, 64), device), _f32((2, 2, 64), device)
    rc = _lib().ovm_op_sam_box_tokens(d["boxes"].data_ptr(), 1, 5, 63, d["out_tokens"].data_ptr(), d["gauss"].data_ptr(), d["corner"].data_ptr(),
                                      70, 100, 90, 128, 128, tok.data_ptr(), sparse.data_ptr(), _stream())
    assert rc == OVM_ERR_SHAPE                                            # an odd C has no [sin | cos] halves
    _untouched(_np(tok), "box_tokens refusal")
    _untouched(_np(sparse), "box_tokens refusal")


# MI355X, worst over the cases (E32 / error): y 8.31e-07 / 6.97e-07
def test_ln_gelu(device):
    """M in {1, 5, 64} (a partial workgroup, two, sixteen), D in {16, 48, 64, 256}; D = 260 is refused."""
    w = Worst("ln_gelu")
    for case in S.CASES["ln_gelu"]:
        inp, r64, r32 = _refs("ln_gelu", case)
        M, D = case["M"], case["D"]
        x = _dev(np.concatenate([inp["x"], np.full((1, D), SENTINEL, dtype=F32)]), device)
        g, b = _dev(inp["gamma"], device), _dev(inp["beta"], device)
        assert _lib().ovm_op_sam_ln_gelu(x.data_ptr(), M, D, g.data_ptr(), b.data_ptr(), 1e-6, _stream()) == 0
        x = _np(x)
        _untouched(x[-1], "ln_gelu")
        w.add(case, S.compare("ln_gelu", case, dict(y=x[:-1]), r64, r32))
    w.done()
    x = _f32((2, 260), device)
    g = _dev(np.ones(260, dtype=F32), device)
    assert _lib().ovm_op_sam_ln_gelu(x.data_ptr(), 2, 260, g.data_ptr(), g.data_ptr(), 1e-6, _stream()) == OVM_ERR_SHAPE
    _untouched(_np(x), "ln_gelu refusal")


def _i2t_call(device, q, k, v, nt, heads, G2, nb, pad=(8, 4, 12)):
    wd = heads * 16
    dq, dk, dv = _strided(q, wd + pad[0], device), _strided(k, wd + pad[1], device), _strided(v, wd + pad[1], device)
    o = _f32((nb * G2 + 1, wd + pad[2]), device)
    rc = _lib().ovm_op_sam_i2t_attn(dq.data_ptr(), wd + pad[0], dk.data_ptr(), dv.data_ptr(), wd + pad[1], nt, heads, G2, nb, 0.25, o.data_ptr(),
                                    wd + pad[2], _stream())
    return rc, _np(o)


# MI355X, worst over the cases (E32 / error): o 3.25e-06 / 3.25e-06 (the case with scores over +-30)
def test_i2t_attn(device):
    """(heads, G2) in {(8, 64), (2, 128), (1, 256)}, nt in {1, 7, 8}, nb in {1, 3}, every row stride larger than heads * 16; one case
    with scores over +-30. Every box has its own tokens. nt = 9 and G2 = 48 with 8 heads are refused."""
    w = Worst("i2t_attn")
    for case in S.CASES["i2t_attn"]:
        inp, r64, r32 = _refs("i2t_attn", case)
        (heads, G2), nt, nb = case["hg"], case["nt"], case["nb"]
        rc, o = _i2t_call(device, inp["q"], inp["k"], inp["v"], nt, heads, G2, nb)
        assert rc == 0
        _untouched(o[-1], "i2t o")
        _untouched(o[:, heads * 16:], "i2t o behind the rows")
        w.add(case, S.compare("i2t_attn", case, dict(o=o[:-1, :heads * 16]), r64, r32))
    w.done()
    for nt, heads, G2 in ((9, 8, 64), (7, 8, 48), (7, 3, 256)):
        rc, o = _i2t_call(device, np.zeros((G2, heads * 16), F32), np.zeros((nt, heads * 16), F32), np.zeros((nt, heads * 16), F32), nt, heads, G2, 1)
        assert rc == OVM_ERR_SHAPE, (nt, heads, G2)
        _untouched(o, "i2t refusal")


# MI355X, worst over the cases (E32 / error): masks 2.12e-06 / 4.32e-06
def test_mask_prod(device):
    """G in {2, 3}, C8 in {8, 32}, nb in {1, 2}, (t0, ntk, out_box_stride) in {(1, 3, 3 L^2), (2, 1, L^2)}"""
    w = Worst("mask_prod")
    for case in S.CASES["mask_prod"]:
        inp, r64, r32 = _refs("mask_prod", case)
        G, C8, nb, (t0, ntk, sk) = case["G"], case["C8"], case["nb"], case["tk"]
        LL = 16 * G * G
        out = _f32(nb * sk * LL + LL, device)
        up, hy = _dev(inp["up"], device), _dev(inp["hyper"], device)
        rc = _lib().ovm_op_sam_mask_prod(up.data_ptr(), hy.data_ptr(), 4 * C8, t0, ntk, C8, G, nb, out.data_ptr(), sk * LL, _stream())
        assert rc == 0
        out = _np(out)
        _untouched(out[nb * sk * LL:], "mask_prod")
        got = out[:nb * sk * LL].reshape(nb, sk, 4 * G, 4 * G)[:, :ntk]
        w.add(case, S.compare("mask_prod", case, dict(masks=got), r64, r32))
    w.done()
    out = _f32(nb * 3 * LL, device)                                        # tokens 2 .. 4 of a hypernetwork output that has four
    assert _lib().ovm_op_sam_mask_prod(up.data_ptr(), hy.data_ptr(), 4 * C8, 2, 3, C8, G, nb, out.data_ptr(), 3 * LL, _stream()) == OVM_ERR_SHAPE
    _untouched(_np(out), "mask_prod refusal")


# MI355X, worst over the cases: E32 of the resampled logit 1.07e-05 (band = 4 x that + one ulp, against logits of standard deviation 10); no pixel outside
# the band disagrees, at most 0.017 % of a mask inside it; the four byte offsets give the same masks
def test_mask_out(device):
    """L = 8, S = 32; portrait, landscape, square, tiny and larger-than-S images, nb in {1, 3} (nb H W is and is not a multiple of 4), the
    destination offset by 0 .. 3 bytes, and a plane offset with box_stride = 3 L^2."""
    w = Worst("mask_out")
    for case in S.CASES["mask_out"]:
        inp, r64, r32 = _refs("mask_out", case)
        (H, W), nb = case["hw"], case["nb"]
        nh, nw = S.preprocess_shape(H, W, 32)
        lg = _dev(inp["logits"], device)                                     # [nb][planes][8][8]
        planes = inp["logits"].shape[1]
        total = nb * H * W
        first = None
        for off in range(4):
            out = torch.full((total + 24,), BYTE, dtype=torch.uint8, device=device)
            rc = _lib().ovm_op_sam_mask_out(lg.data_ptr() + (4 * 64 if case["plane"] else 0), planes * 64, 8, 32, nh, nw, H, W, nb,
                                            out.data_ptr() + 8 + off, _stream())
            assert rc == 0
            out = _np(out)
            _untouched(out[:8 + off], f"mask_out off {off}: before the masks")
            _untouched(out[8 + off + total:], f"mask_out off {off}: behind the masks")
            got = out[8 + off:8 + off + total].reshape(nb, H, W)
            fig = S.compare("mask_out", case, dict(mask=got), r64, r32)
            if first is None:
                first = got
                w.add(case, fig)
            assert np.array_equal(got, first), f"offset {off} changes the masks"
    w.done()
    out = torch.full((64,), BYTE, dtype=torch.uint8, device=device)
    assert _lib().ovm_op_sam_mask_out(lg.data_ptr(), 64, 8, 32, 33, 20, 5, 3, 1, out.data_ptr(), _stream()) == OVM_ERR_SHAPE
    _untouched(_np(out), "mask_out refusal")


def test_unpatch_iou_slice_add_bcast_exact(device):
    """Bit for bit: G = 2 with P = 16 (row stride 832), with and without lo; n in {1, 5} with ldh = 128; bmod < n, bmod = n, b = NULL, and a
    length that is no multiple of the workgroup; n = 6 (and bmod = 6) refused."""
    L = _lib()
    for case in S.CASES["unpatch"]:
        inp, r64, _ = _refs("unpatch", case)
        hi, lo = _dev(inp["hi"], device), (_dev(inp["lo"], device) if case["lo"] else None)
        out = _f32(3 * 32 * 32 + 16, device)
        assert L.ovm_op_sam_unpatch(hi.data_ptr(), _ptr(lo), 832, 2, 16, out.data_ptr(), _stream()) == 0
        out = _np(out)
        _untouched(out[3 * 32 * 32:], "unpatch")
        S.compare("unpatch", case, dict(out=out[:3 * 32 * 32].reshape(3, 32, 32)), r64, r64)
    out = _f32(8, device)
    assert L.ovm_op_sam_unpatch(hi.data_ptr(), None, 767, 2, 16, out.data_ptr(), _stream()) == OVM_ERR_SHAPE
    _untouched(_np(out), "unpatch refusal")
    for case in S.CASES["iou_slice"]:
        inp, r64, _ = _refs("iou_slice", case)
        n = case["n"]
        head, iou = _dev(inp["head"], device), _f32(3 * n + 3, device)
        assert L.ovm_op_sam_iou_slice(head.data_ptr(), 128, n, iou.data_ptr(), _stream()) == 0
        iou = _np(iou)
        _untouched(iou[3 * n:], "iou_slice")
        S.compare("iou_slice", case, dict(iou=iou[:3 * n].reshape(n, 3)), r64, r64)
    for case in S.CASES["add_bcast"]:
        inp, r64, _ = _refs("add_bcast", case)
        n = case["n"]
        a, b, out = _dev(inp["a"], device), (_dev(inp["b"], device) if case["b"] else None), _f32(n + 4, device)
        assert L.ovm_op_sam_add_bcast(a.data_ptr(), _ptr(b), out.data_ptr(), n, case["bmod"], _stream()) == 0
        out = _np(out)
        _untouched(out[n:], "add_bcast")
        S.compare("add_bcast", case, dict(out=out[:n]), r64, r64)
    a, out = _dev(np.ones(16, dtype=F32), device), _f32(16, device)
    for n, bmod, b in ((6, 4, a), (6, 4, None), (8, 6, a), (8, 6, None)):
        assert L.ovm_op_sam_add_bcast(a.data_ptr(), _ptr(b), out.data_ptr(), n, bmod, _stream()) == OVM_ERR_SHAPE, (n, bmod)
        _untouched(_np(out), "add_bcast refusal")


# ================================================================================================ Depth Pro
# MI355X, worst over the cases (E32 / error): P0 1.21e-07 / 1.10e-07, P1 1.20e-07 / 1.08e-07, P2 9.07e-08 / 9.07e-08
def test_pyramid(device):
    """S in {16, 64}; images smaller than, equal to and larger than the canvas, both ways round; [H][W][3] and [3][H][W] strides, flip 0 / 1."""
    w = Worst("pyramid")
    for case in S.CASES["pyramid"]:
        inp, r64, r32 = _refs("pyramid", case)
        Sz, (H, W) = case["S"], case["hw"]
        if case["chw"]:
            img, st = _dev(inp["img"].transpose(2, 0, 1), device), (W, 1, H * W)
        else:
            img, st = _dev(inp["img"], device), (3 * W, 3, 1)
        P = [_f32((Sz >> l) ** 2 * 3 + 8, device) for l in range(3)]
        rc = _lib().ovm_op_dp_pyramid(img.data_ptr(), H, W, st[0], st[1], st[2], case["flip"], Sz, P[0].data_ptr(), P[1].data_ptr(), P[2].data_ptr(), _stream())
        assert rc == 0
        got = {}
        for l in range(3):
            a, s = _np(P[l]), Sz >> l
            _untouched(a[s * s * 3:], f"pyramid level {l}")
            got[f"P{l}"] = a[:s * s * 3].reshape(s, s, 3)
        w.add(case, S.compare("pyramid", case, got, r64, r32))
    w.done()
    P = [_f32(64, device) for _ in range(3)]
    assert _lib().ovm_op_dp_pyramid(img.data_ptr(), H, W, st[0], st[1], st[2], 0, 18, P[0].data_ptr(), P[1].data_ptr(), P[2].data_ptr(), _stream()) == OVM_ERR_SHAPE
    for p in P:
        _untouched(_np(p), "pyramid refusal")


# MI355X, worst over the cases (E32 / error): map 5.66e-07 / 5.37e-07 with lo; hi alone 1.77e-03 (within half an fp16 step)
def test_merge(device):
    """(g, n, pad) in {(4, 1, 0), (4, 3, 1), (8, 5, 2), (8, 3, 0), (8, 5, 1)}, D in {4, 128}, out = Ms and out in {g, 2g, 4g}, crop0 in {0, 2},
    with and without lo; the class-token rows hold the sentinel."""
    w = Worst("merge")
    for case in S.CASES["merge"]:
        inp, r64, r32 = _refs("merge", case)
        g, n, pad, D, out = case["g"], case["n"], case["pad"], case["D"], case["out"]
        tok = _dev(inp["tok"], device)
        hi, lo = _h16((out * out + 1, D), device), (_h16((out * out + 1, D), device) if case["lo"] else None)
        rc = _lib().ovm_op_dp_merge(tok.data_ptr(), 1 + g * g, D, case["crop0"], n, g, pad, case["Ms"], out, hi.data_ptr(), _ptr(lo), _stream())
        assert rc == 0
        hi = _np(hi)
        _untouched(hi[-1], "merge hi")
        if lo is not None:
            lo = _np(lo)
            _untouched(lo[-1], "merge lo")
        got = S.join(hi[:-1], None if lo is None else lo[:-1]).reshape(out, out, D)
        w.add(case, S.compare("merge", case, dict(map=got), r64, r32))
    w.done()
    hi = _h16((17, 6), device)
    for D, Ms in ((6, 8), (4, 9)):
        assert _lib().ovm_op_dp_merge(tok.data_ptr(), 17, D, 0, 3, 4, 1, Ms, 4, hi.data_ptr(), None, _stream()) == OVM_ERR_SHAPE
        _untouched(_np(hi), "merge refusal")


def test_unsplit_exact(device):
    """side in {2, 5}, C in {4, 64}, pixel stride C + 4, plain and zero-bordered sources, the three output combinations; the frame of the
    bordered destination keeps the sentinel. C = 6 is refused."""
    for case in S.CASES["unsplit"]:
        inp, r64, _ = _refs("unsplit", case)
        side, Cc = case["side"], case["C"]
        hi, lo = _dev(inp["hi"], device), _dev(inp["lo"], device)
        want_f, want_s = case["outs"] in ("f32", "both"), case["outs"] in ("split", "both")
        out = _f32((side * side + 1, Cc), device) if want_f else None
        ph, pl = (_h16((side + 2, side + 2, Cc), device), _h16((side + 2, side + 2, Cc), device)) if want_s else (None, None)
        rc = _lib().ovm_op_dp_unsplit(hi.data_ptr(), lo.data_ptr(), side, Cc, Cc + 4, case["pad_in"], _ptr(out), _ptr(ph), _ptr(pl), _stream())
        assert rc == 0
        got = {}
        if want_f:
            out = _np(out)
            _untouched(out[-1], "unsplit out")
            got["out"] = out[:-1].reshape(side, side, Cc)
        if want_s:
            for name, buf in (("p_hi", _np(ph)), ("p_lo", _np(pl))):
                frame = buf.copy()
                frame[1:-1, 1:-1] = np.float16(SENTINEL)
                _untouched(frame, f"unsplit {name} frame")
                got[name] = buf[1:-1, 1:-1]
        S.compare("unsplit", case, got, r64, r64)
    out = _f32((5, 6), device)
    assert _lib().ovm_op_dp_unsplit(hi.data_ptr(), lo.data_ptr(), 2, 6, 8, 0, out.data_ptr(), None, None, _stream()) == OVM_ERR_SHAPE
    _untouched(_np(out), "unsplit refusal")


# MI355X, worst over the cases (E32 / error): conv_s2 1.72e-06 / 6.92e-06 (not the same case); dot 2.83e-06 / 9.90e-07
def test_conv_s2_and_dot(device):
    """Si in {5, 8} (an odd side: the last output reads one row and column of padding less), Cin in {4, 32}, Cout in {1, 8}, without add
    and with ld_add = Cout + 3; the dot product at n in {1, 255, 256, 1000}. Cin = 6 is refused."""
    w = Worst("conv_s2")
    for case in S.CASES["conv_s2"]:
        inp, r64, r32 = _refs("conv_s2", case)
        Si, Cin, Cout = case["Si"], case["Cin"], case["Cout"]
        So = (Si - 1) // 2 + 1
        d = {k: _dev(inp[k], device) for k in ("x", "w", "bias")}
        add = _dev(inp["add"], device) if case["add"] else None
        out = _f32(So * So * Cout + 4, device)
        rc = _lib().ovm_op_dp_conv_s2(d["x"].data_ptr(), Si, Cin, d["w"].data_ptr(), d["bias"].data_ptr(), Cout, _ptr(add), Cout + 3 if case["add"] else 0,
                                      out.data_ptr(), _stream())
        assert rc == 0
        out = _np(out)
        _untouched(out[So * So * Cout:], "conv_s2")
        w.add(case, S.compare("conv_s2", case, dict(out=out[:So * So * Cout].reshape(So, So, Cout)), r64, r32))
    w.done()
    out = _f32(16, device)
    assert _lib().ovm_op_dp_conv_s2(d["x"].data_ptr(), 4, 6, d["w"].data_ptr(), d["bias"].data_ptr(), 1, None, 0, out.data_ptr(), _stream()) == OVM_ERR_SHAPE
    _untouched(_np(out), "conv_s2 refusal")
    w = Worst("dot")
    for case in S.CASES["dot"]:
        inp, r64, r32 = _refs("dot", case)
        d = {k: _dev(inp[k], device) for k in ("x", "w", "bias")}
        out = _f32(2, device)
        assert _lib().ovm_op_dp_dot(d["x"].data_ptr(), d["w"].data_ptr(), d["bias"].data_ptr(), case["n"], out.data_ptr(), _stream()) == 0
        out = _np(out)
        _untouched(out[1:], "dot")
        w.add(case, S.compare("dot", case, dict(out=out[:1]), r64, r32))
    w.done()


def _tail_call(device, x, wt, b1, w2, b2, Sz, Cc, precision):
    xp = np.zeros((Sz + 2, Sz + 2, Cc), dtype=F32)
    xp[1:-1, 1:-1] = x
    xh, xl = S.split(xp)
    wh, wl = S.split(wt.reshape(32, 9 * Cc))
    d = [_dev(a, device) for a in (xh, xl, wh, wl, b1, w2, b2)]
    out = _f32(Sz * Sz + Sz, device)
    p3 = precision == 3
    rc = _lib().ovm_op_dp_head_tail(d[0].data_ptr(), d[1].data_ptr() if p3 else None, Sz, Cc, d[2].data_ptr(), d[3].data_ptr() if p3 else None,
                                    d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), precision, out.data_ptr(), _stream())
    return rc, _np(out)


# MI355X, worst scale-relative error over the cases: precision 3 2.4e-07 (bound 2.0e-06), precision 1 1.9e-07 (bound 3e-03; the
# reference takes the operands as fp16, so what is left is the accumulation order)
def test_head_tail(device):
    """S in {16, 48} (one workgroup, nine), C in {32, 64} (one k-step per tap, two), precision 1 and 3; S = 24 and C = 48 are refused."""
    for case in S.CASES["head_tail"]:
        inp, r64, r32 = _refs("head_tail", case)
        Sz, Cc = case["S"], case["C"]
        rc, out = _tail_call(device, inp["x"], inp["w"], inp["b1"], inp["w2"], inp["b2"], Sz, Cc, case["precision"])
        assert rc == 0
        _untouched(out[Sz * Sz:], "head_tail")
        fig = S.compare("head_tail", case, dict(out=out[:Sz * Sz].reshape(Sz, Sz)), r64, r32)
        print(f"\nhead_tail {S.case_id(case)}: scale-relative error {fig['out'][1]:.3e} (bound {S.tail_tolerance(case):.1e})", end="")
    for Sz, Cc in ((24, 32), (16, 48)):
        rc, out = _tail_call(device, np.zeros((Sz, Sz, Cc), F32), np.zeros((32, 3, 3, Cc), F32), inp["b1"], inp["w2"], inp["b2"], Sz, Cc, 3)
        assert rc == OVM_ERR_SHAPE
        _untouched(out, "head_tail refusal")


def test_clear_borders_exact(device):
    """Two images in one call, (side, C) = (1, 8) with lo and (4, 32) without: the frame zero, the interior (and the second image's absent
    lo) untouched. C = 12 is refused."""
    case = S.CASES["clear_borders"][0]
    _, r64, _ = _refs("clear_borders", case)
    his = [_h16((s + 2) * (s + 2) * c + 16, device) for s, c, _ in case["images"]]
    los = [(_h16((s + 2) * (s + 2) * c + 16, device) if wl else None) for s, c, wl in case["images"]]
    n = len(his)
    hp, lp = (C.c_void_p * n)(*[t.data_ptr() for t in his]), (C.c_void_p * n)(*[_ptr(t) for t in los])
    sides, cs = (C.c_int32 * n)(*[s for s, _, _ in case["images"]]), (C.c_int32 * n)(*[c for _, c, _ in case["images"]])
    assert _lib().ovm_op_dp_clear_borders(hp, lp, sides, cs, n, _stream()) == 0
    got = {}
    for i, (s, c, wl) in enumerate(case["images"]):
        for name, t in (("hi", his[i]), ("lo", los[i])):
            if t is None:
                continue
            a = _np(t)
            _untouched(a[(s + 2) * (s + 2) * c:], f"clear_borders image {i} {name}")
            img = a[:(s + 2) * (s + 2) * c].reshape(s + 2, s + 2, c).astype(F32)
            if name == "hi":
                got[f"img{i}"] = img
            else:
                assert S.same_bits(img, r64[f"img{i}"]), "lo frame"
    S.compare("clear_borders", case, got, r64, r64)
    bad = _h16(3 * 3 * 12, device)
    hp, sides, cs = (C.c_void_p * 1)(bad.data_ptr()), (C.c_int32 * 1)(1), (C.c_int32 * 1)(12)
    assert _lib().ovm_op_dp_clear_borders(hp, None, sides, cs, 1, _stream()) == OVM_ERR_SHAPE
    _untouched(_np(bad), "clear_borders refusal")


# MI355X, worst over the cases (E32 / error): depth 4.89e-03 / 4.89e-03 (at depth 1e4: the fp32 clamp bound 1e-4f), f 1.24e-05 / 2.82e-06
def test_depth_out(device):
    """S = 16 to portrait, landscape, square and larger images; a given focal length and the field-of-view route at 30 and 90 degrees;
    canon reaches both clamps (inverse depth 0 and 5e4); fov_out / f_out given and NULL."""
    w = Worst("depth_out")
    for case in S.CASES["depth_out"]:
        inp, r64, r32 = _refs("depth_out", case)
        (H, W), (kind, val) = case["hw"], case["focal"]
        canon = _dev(inp["canon"], device)
        fov = _dev(np.array([val], dtype=F32), device) if kind == "fov" else None
        depth = _f32(H * W + 4, device)
        fo, fx = (_f32(2, device), _f32(2, device)) if case["outs"] else (None, None)
        rc = _lib().ovm_op_dp_depth_out(canon.data_ptr(), 16, H, W, val if kind == "f" else 0.0, _ptr(fov), depth.data_ptr(), _ptr(fo), _ptr(fx), _stream())
        assert rc == 0
        depth = _np(depth)
        _untouched(depth[H * W:], "depth_out")
        got = dict(depth=depth[:H * W].reshape(H, W))
        if case["outs"]:
            fo, fx = _np(fo), _np(fx)
            _untouched(fo[1:], "fov_out")
            _untouched(fx[1:], "f_out")
            assert fo[0] == (F32(val) if kind == "fov" else F32(0))
            got["f"] = fx[:1]
        else:
            r64, r32 = ({k: v for k, v in r.items() if k != "f"} for r in (r64, r32))
        w.add(case, S.compare("depth_out", case, got, r64, r32))
    w.done()
    depth = _f32(8, device)
    assert _lib().ovm_op_dp_depth_out(canon.data_ptr(), 16, 2, 2, 0.0, None, depth.data_ptr(), None, None, _stream()) == OVM_ERR_INVALID
    _untouched(_np(depth), "depth_out refusal")


# ================================================================================================ generic ops as SAM's token attention calls them
def _bound_check(name, got, r64, r32, w):
    e32, tol = S.bound(r64, r32)
    err = float(np.max(np.abs(np.asarray(got, F64) - r64)))
    print(f"\n{name}: E32 {e32:.3e} err {err:.3e}", end="")
    w[0], w[1] = max(w[0], e32), max(w[1], err)
    assert err <= tol, f"{name}: |got - fp64| = {err:.3e} > 4 * E32 + ulp = {tol:.3e} (E32 {e32:.3e})"


# MI355X, worst over the cases (E32 / error): scores 5.72e-07 / 9.54e-07, context 4.02e-07 / 3.42e-07
def test_bmm2_with_token_attention_strides(device):
    """ovm_g_bmm2 exactly as token_attention calls it: two batch levels (nb in {1, 3} x heads in {2, 8}), nt = 7, dh = 16,
    Tk in {7, 64, 1024, 1040}; transB = 1 for the scores, transB = 0 for the context, where Tk >= 1024 takes the split-K route with nb2 > 1."""
    g = np.random.default_rng(77)
    nt, dh = 7, 16
    ws, wc = [0.0, 0.0], [0.0, 0.0]
    for nb in (1, 3):
        for hd in (2, 8):
            for Tk in (7, 64, 1024, 1040):
                I = hd * dh
                Q, K, V = (g.standard_normal((nb * t, I)).astype(F32) for t in (nt, Tk, Tk))
                alpha = 1.0 / np.sqrt(F32(dh))
                s64, s32 = (S.token_scores(Q, K, nb, hd, nt, Tk, dh, alpha, d) for d in (F64, F32))
                dQ, dK, dV = _dev(Q, device), _dev(K, device), _dev(V, device)
                sc = _f32(nb * hd * nt * Tk + 8, device)
                rc = _lib().ovm_g_bmm2(dQ.data_ptr(), dK.data_ptr(), sc.data_ptr(), nb, hd, nt, Tk, dh, I, I, Tk, nt * I, Tk * I, hd * nt * Tk, dh, dh,
                                       nt * Tk, 1, float(alpha), _stream())
                assert rc == 0
                a = _np(sc)
                _untouched(a[nb * hd * nt * Tk:], "scores")
                _bound_check(f"scores nb{nb} hd{hd} Tk{Tk}", a[:-8].reshape(nb, hd, nt, Tk), s64, s32, ws)
                P = S.softmax(s32.astype(F64), F64).astype(F32)                   # the probabilities are an input of the second product
                c64, c32 = (S.token_context(P, V, nb, hd, nt, Tk, dh, d) for d in (F64, F32))
                dP, ctx = _dev(P, device), _f32((nb * nt + 1, I), device)
                rc = _lib().ovm_g_bmm2(dP.data_ptr(), dV.data_ptr(), ctx.data_ptr(), nb, hd, nt, dh, Tk, Tk, I, I, hd * nt * Tk, Tk * I, nt * I, nt * Tk,
                                       dh, dh, 0, 1.0, _stream())
                assert rc == 0
                c = _np(ctx)
                _untouched(c[-1], "context")
                _bound_check(f"context nb{nb} hd{hd} Tk{Tk}", c[:-1], c64, c32, wc)
    print(f"\nbmm2 worst: scores {ws[0]:.2e} / {ws[1]:.2e}, context {wc[0]:.2e} / {wc[1]:.2e}")


# MI355X, worst over the cases (E32 / error): softmax 1.69e-07 / 9.96e-08, layernorm 6.35e-07 / 7.79e-07
def test_softmax_rows_and_layernorm(device):
    """ovm_g_softmax on rows of 7, 64, 512, 513 (the looping path) and 1040 columns, ld = cols and ld > cols with the sentinel behind the
    row; ovm_g_layernorm with M in {1, 7}, D in {64, 256}, with and without the residual."""
    g = np.random.default_rng(78)
    w = [0.0, 0.0]
    for cols in (7, 64, 512, 513, 1040):
        for ld in (cols, cols + 5):
            x = (g.standard_normal((9, cols)) * 3).astype(F32)
            r64, r32 = S.softmax(x.astype(F64), F64), S.softmax(x, F32)
            d = _strided(np.concatenate([x, np.full((1, cols), SENTINEL, F32)]), ld, device)
            assert _lib().ovm_g_softmax(d.data_ptr(), 9, cols, ld, None, 0, 0, 0, _stream()) == 0
            a = _np(d)
            _untouched(a[-1], "softmax")
            _untouched(a[:, cols:], "softmax behind the rows")
            _bound_check(f"softmax cols{cols} ld{ld}", a[:-1, :cols], r64, r32, w)
    print(f"\nsoftmax worst: {w[0]:.2e} / {w[1]:.2e}")
    w = [0.0, 0.0]
    for M in (1, 7):
        for D in (64, 256):
            for with_res in (False, True):
                x, res = (g.standard_normal((M, D)) * 2 + 0.5).astype(F32), g.standard_normal((M, D)).astype(F32)
                gam, bet = (g.random(D) + 0.5).astype(F32), g.standard_normal(D).astype(F32)
                r64, r32 = (R.layer_norm(x.astype(d) + res.astype(d) if with_res else x, gam, bet, 1e-5, d) for d in (F64, F32))
                dx, dr, dg, db = (_dev(a, device) for a in (x, res, gam, bet))
                y = _f32((M + 1, D), device)
                rc = _lib().ovm_g_layernorm(dx.data_ptr(), dr.data_ptr() if with_res else None, M, D, dg.data_ptr(), db.data_ptr(), 1e-5, y.data_ptr(), _stream())
                assert rc == 0
                a = _np(y)
                _untouched(a[-1], "layernorm")
                _bound_check(f"layernorm M{M} D{D} res{int(with_res)}", a[:-1], r64, r32, w)
    print(f"\nlayernorm worst: {w[0]:.2e} / {w[1]:.2e}")
