"""The prompt kernels of csrc/sam.hip one at a time, through ovm_op_sam_point_tokens / ovm_op_sam_mask_embed / ovm_op_sam_i2t_attn16 and
ovm_sam_mask_boxes, against the fp64 restatements of tests/sam_prompt_oracle.py and tests/sam_dp_glue_ref.py (themselves checked
against Hugging Face's prompt encoder on the CPU, tests/test_sam_prompts_cpu.py).

Rule (tests/roi_glue_ref.bound, none chosen here): max |got - fp64| <= 4 * E32 + one fp32 ulp of the largest |fp64|, E32 = the fp32
run of the restatement against fp64 on the same inputs. Copies, the 16-token attention at nt <= 8 against the 8-token one, the mask
boxes and refusals are bit for bit. Every destination is pre-filled with a sentinel that must survive outside the kernel's range.

MI355X, worst over the cases (E32 / error): point tokens 4.60e-06 / 4.60e-06 (the box corners far outside the image), mask embedding
8.87e-07 / 8.22e-07, 16-token attention 3.15e-06 / 3.15e-06 (the case with scores over +-30).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import roi_glue_ref as R
import sam_dp_glue_ref as S
import sam_prompt_oracle as po
from roi_glue_ref import F32, F64, SENTINEL

pytestmark = pytest.mark.gpu
OVM_ERR_INVALID, OVM_ERR_SHAPE = -1, -4


def _lib():
    from ovmono3d_amd import lib
    return lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _f32(shape, device):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=device)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _untouched(a, what):
    assert np.all(np.asarray(a) == F32(SENTINEL)), f"{what}: the sentinel was overwritten"


def _within(name, got, r64, r32):
    e32, tol = R.bound(r64, r32)
    err = float(np.max(np.abs(got.astype(F64) - r64)))
    print(f"\n{name}: E32 {e32:.3e} err {err:.3e} bound {tol:.3e}", end="")
    assert err <= tol, f"{name}: error {err:.3e} over the bound {tol:.3e} (E32 {e32:.3e})"


# ---- point tokens ------------------------------------------------------------------------------------------------------------------
POINT_CASES = [  # (nb, P, box, C, (H, W, S))
    (1, 1, False, 256, (70, 100, 128)), (3, 3, False, 64, (99, 71, 128)), (2, 2, True, 256, (70, 100, 128)), (3, 8, True, 64, (99, 71, 128)),
    (2, 8, False, 256, (70, 100, 128)), (3, 0, True, 64, (70, 100, 128))]


def _point_inputs(nb, P, box, Cc, frame, seed):
    g = np.random.RandomState(seed)
    H, W, _ = frame
    pts = (g.uniform(-0.1, 1.1, (nb, P, 2)) * np.array([W, H])).astype(F32) if P else None      # some clicks beyond the image, fractional
    if P:
        pts[0, 0] = (W - 1, H - 1)                                                                # the last pixel
    lab = g.choice(np.array([1, 0, -1], np.int32), size=(nb, P)).astype(np.int32) if P else None
    if P >= 3:
        lab[0, :3] = (1, 0, -1)
    boxes = None
    if box:
        boxes = np.concatenate([g.uniform(-10, 40, (nb, 2)), g.uniform(41, 120, (nb, 2))], 1).astype(F32)
    w = dict(out_tokens=g.normal(0, 0.5, (5, Cc)).astype(F32), gauss=g.normal(0, 1, (2, Cc // 2)).astype(F32), point_emb=g.normal(0, 0.5, (2, Cc)).astype(F32),
             not_a_point=g.normal(0, 0.5, Cc).astype(F32), corner=g.normal(0, 0.5, (2, Cc)).astype(F32))
    return pts, lab, boxes, w


def _point_call(device, pts, lab, boxes, w, nb, P, Cc, frame, ns):
    H, W, Sz = frame
    nh, nw = S.preprocess_shape(H, W, Sz)
    tok, sparse = _f32((nb + 1, 5 + ns, Cc), device), _f32((nb + 1, ns, Cc), device)
    d = {k: _dev(v, device) for k, v in w.items()}
    dp, dl, db = _dev(pts, device), _dev(lab, device), _dev(boxes, device)
    rc = _lib().ovm_op_sam_point_tokens(_ptr(dp), _ptr(dl), _ptr(db), nb, P, 5, Cc, d["out_tokens"].data_ptr(), d["gauss"].data_ptr(), d["point_emb"].data_ptr(),
                                        d["not_a_point"].data_ptr(), d["corner"].data_ptr(), H, W, nh, nw, Sz, tok.data_ptr(), sparse.data_ptr(), _stream())
    return rc, _np(tok), _np(sparse), (nh, nw)


@pytest.mark.parametrize("nb,P,box,Cc,frame", POINT_CASES)
def test_point_tokens(device, nb, P, box, Cc, frame):
    """P in {0, 1, 2, 3, 8}, with and without a box, labels 1 / 0 / -1, clicks on the last pixel and beyond the image, C in {64, 256},
    70 x 100 and 99 x 71 in a 128 frame, more than one workgroup. Padding and -1 rows are not_a_point bit for bit; P = 0 with a box is
    ovm_op_sam_box_tokens bit for bit."""
    pts, lab, boxes, w = _point_inputs(nb, P, box, Cc, frame, seed=100 + 10 * P + nb)
    ns = P + (2 if box else 1)
    rc, tok, sparse, (nh, nw) = _point_call(device, pts, lab, boxes, w, nb, P, Cc, frame, ns)
    assert rc == 0
    _untouched(tok[-1], "tok")
    _untouched(sparse[-1], "sparse")
    assert S.same_bits(tok[:nb, 5:], sparse[:nb]), "sparse is not the prompt rows of tok"
    assert S.same_bits(tok[:nb, :5], np.broadcast_to(w["out_tokens"], (nb, 5, Cc))), "the output tokens are copies"
    H, W, Sz = frame
    r64 = po.point_tokens(pts, lab, boxes, H=H, W=W, newh=nh, neww=nw, S=Sz, dtype=F64, **w)[1]
    r32 = po.point_tokens(pts, lab, boxes, H=H, W=W, newh=nh, neww=nw, S=Sz, dtype=F32, **w)[1]
    _within(f"point_tokens nb{nb} P{P} box{int(box)} C{Cc}", sparse[:nb], r64, r32)
    for b in range(nb):
        for p in range(P):
            if lab[b, p] == -1:
                assert S.same_bits(sparse[b, p], w["not_a_point"])
    if not box:
        assert S.same_bits(sparse[:nb, -1], np.broadcast_to(w["not_a_point"], (nb, Cc)))
    if P == 0:
        tok2, sp2 = _f32((nb, 7, Cc), device), _f32((nb, 2, Cc), device)
        d = {k: _dev(w[k], device) for k in ("out_tokens", "gauss", "corner")}
        assert _lib().ovm_op_sam_box_tokens(_dev(boxes, device).data_ptr(), nb, 5, Cc, d["out_tokens"].data_ptr(), d["gauss"].data_ptr(), d["corner"].data_ptr(),
                                            H, W, nh, nw, Sz, tok2.data_ptr(), sp2.data_ptr(), _stream()) == 0
        assert S.same_bits(_np(tok2), tok[:nb]) and S.same_bits(_np(sp2), sparse[:nb])


def test_point_tokens_refusals(device):
    frame = (70, 100, 128)
    pts, lab, boxes, w = _point_inputs(1, 9, True, 64, frame, seed=7)
    rc, tok, sparse, _ = _point_call(device, pts, lab, boxes, w, 1, 9, 64, frame, 11)
    assert rc == OVM_ERR_SHAPE                                              # nine points
    _untouched(tok, "nine points")
    rc, tok, sparse, _ = _point_call(device, None, None, None, w, 1, 0, 64, frame, 1)
    assert rc == OVM_ERR_INVALID                                            # neither points nor box
    _untouched(tok, "no prompt")
    rc, tok, sparse, _ = _point_call(device, pts[:, :1], lab[:, :1], None, w, 1, 1, 63, frame, 2)
    assert rc == OVM_ERR_SHAPE                                              # an odd C has no [sin | cos] halves
    _untouched(sparse, "odd C")


# ---- mask embedding ----------------------------------------------------------------------------------------------------------------
def _mask_weights(Cc, seed):
    g = np.random.RandomState(seed)
    n = lambda *s, std=1.0: (g.normal(0, std, s)).astype(F32)                                     # noqa: E731
    return {"0.weight": n(4, 1, 2, 2, std=0.5), "0.bias": n(4, std=0.02), "1.weight": (0.5 + g.uniform(size=4)).astype(F32), "1.bias": n(4, std=0.05),
            "3.weight": n(16, 4, 2, 2, std=0.25), "3.bias": n(16, std=0.02), "4.weight": (0.5 + g.uniform(size=16)).astype(F32), "4.bias": n(16, std=0.05),
            "6.weight": n(Cc, 16, 1, 1, std=0.25), "6.bias": n(Cc, std=0.02)}


def _mask_call(device, mask, w, n, G, Cc):
    out = _f32((n + 1, G * G, Cc), device)
    d = [_dev(w[k], device) for k in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias", "6.weight", "6.bias")]
    rc = _lib().ovm_op_sam_mask_embed(_dev(mask, device).data_ptr(), n, G, Cc, *[t.data_ptr() for t in d], out.data_ptr(), _stream())
    return rc, _np(out)


@pytest.mark.parametrize("n,G,Cc,kind", [(1, 2, 64, "noise"), (3, 5, 256, "noise"), (2, 8, 256, "logits"), (2, 5, 192, "constant")])
def test_mask_embed(device, n, G, Cc, kind):
    """Noise, logit-sized noise (std 30, what a previous pass hands back) and a constant plane (every cell the same row); G odd and
    even, C in {64, 192, 256} (C < the workgroup), more than one prompt."""
    g = np.random.RandomState(5 + G)
    L = 4 * G
    mask = {"noise": g.normal(0, 1, (n, L, L)), "logits": g.normal(0, 30, (n, L, L)), "constant": np.full((n, L, L), -7.25)}[kind].astype(F32)
    w = _mask_weights(Cc, seed=G)
    rc, out = _mask_call(device, mask, w, n, G, Cc)
    assert rc == 0
    _untouched(out[-1], "mask_embed")
    _within(f"mask_embed {kind} n{n} G{G} C{Cc}", out[:n], po.mask_embed(mask, w, F64), po.mask_embed(mask, w, F32))
    if kind == "constant":
        assert S.same_bits(out[:n], np.broadcast_to(out[0, 0], (n, G * G, Cc)))
    rc, out = _mask_call(device, mask, _mask_weights(260, seed=1), n, G, 260)
    assert rc == OVM_ERR_SHAPE
    _untouched(out, "mask_embed refusal")


# ---- image -> token attention, 16 tokens -------------------------------------------------------------------------------------------
def _i2t_call(fn, device, q, k, v, nt, heads, G2, nb, pad=(8, 4, 12)):
    wd = heads * 16

    def strided(a, ld):
        buf = np.full((a.shape[0], ld), SENTINEL, dtype=F32)
        buf[:, :wd] = a
        return _dev(buf, device)

    dq, dk, dv = strided(q, wd + pad[0]), strided(k, wd + pad[1]), strided(v, wd + pad[1])
    o = _f32((nb * G2 + 1, wd + pad[2]), device)
    rc = fn(dq.data_ptr(), wd + pad[0], dk.data_ptr(), dv.data_ptr(), wd + pad[1], nt, heads, G2, nb, 0.25, o.data_ptr(), wd + pad[2], _stream())
    return rc, _np(o)


def _i2t_inputs(nt, heads, G2, nb, seed, spread=1.0):
    g = np.random.RandomState(seed)
    wd = heads * 16
    return (g.normal(0, spread, (nb * G2, wd)).astype(F32), g.normal(0, spread, (nb * nt, wd)).astype(F32), g.normal(0, 1, (nb * nt, wd)).astype(F32))


@pytest.mark.parametrize("nt,heads,G2,nb,spread", [(9, 8, 64, 3, 1.0), (15, 8, 64, 2, 1.0), (16, 2, 128, 1, 1.0), (15, 1, 256, 2, 3.0), (1, 8, 64, 1, 1.0)])
def test_i2t_attn16_against_fp64(device, nt, heads, G2, nb, spread):
    """nt in {1, 9, 15, 16}, (heads, G2) in {(8, 64), (2, 128), (1, 256)}, several prompts with their own tokens, one case with scores
    over +-30; every row stride larger than heads * 16."""
    q, k, v = _i2t_inputs(nt, heads, G2, nb, seed=nt * 7 + heads, spread=spread)
    rc, o = _i2t_call(_lib().ovm_op_sam_i2t_attn16, device, q, k, v, nt, heads, G2, nb)
    assert rc == 0
    _untouched(o[-1], "i2t16 o")
    _untouched(o[:, heads * 16:], "i2t16 o behind the rows")
    r64, r32 = S.i2t_attn(q, k, v, nt, heads, G2, nb, 0.25, F64), S.i2t_attn(q, k, v, nt, heads, G2, nb, 0.25, F32)
    _within(f"i2t_attn16 nt{nt} heads{heads} G2 {G2} nb{nb}", o[:-1, :heads * 16], r64, r32)


@pytest.mark.parametrize("nt", [7, 8])
def test_i2t_attn16_is_the_8_token_kernel_bit_for_bit(device, nt):
    q, k, v = _i2t_inputs(nt, 8, 64, 3, seed=nt)
    rc8, o8 = _i2t_call(_lib().ovm_op_sam_i2t_attn, device, q, k, v, nt, 8, 64, 3)
    rc16, o16 = _i2t_call(_lib().ovm_op_sam_i2t_attn16, device, q, k, v, nt, 8, 64, 3)
    assert rc8 == 0 and rc16 == 0 and S.same_bits(o8, o16)


def test_i2t_attn16_refusals(device):
    for nt, heads, G2 in ((17, 8, 64), (0, 8, 64), (9, 8, 48), (9, 3, 256)):
        z = np.zeros((max(nt, 1), heads * 16), F32)
        rc, o = _i2t_call(_lib().ovm_op_sam_i2t_attn16, device, np.zeros((G2, heads * 16), F32), z, z, nt, heads, G2, 1)
        assert rc == OVM_ERR_SHAPE, (nt, heads, G2)
        _untouched(o, "i2t16 refusal")


# ---- mask boxes --------------------------------------------------------------------------------------------------------------------
def test_mask_boxes_exact(device):
    """Empty, one pixel, full and L-shaped masks at width 13 (no multiple of 4), values other than 1 count as inside; then planes of
    70 x 101 pixels (several workgroups per plane: the atomics) with a far corner pixel, a full one and an empty one."""
    H, W = 9, 13
    m = np.zeros((5, H, W), np.uint8)
    m[1, 4, 7] = 1
    m[2] = 1
    m[3, 1:8, 2] = 1
    m[3, 7, 2:12] = 255
    m[4, H - 1, W - 1] = 1
    big = np.zeros((4, 70, 101), np.uint8)
    big[0, 3, 5] = big[0, 69, 100] = 1
    big[1] = 1
    big[3, 10:60, 17:90] = (np.random.RandomState(0).uniform(size=(50, 73)) < 0.3)
    for masks in (m, big):
        n, h, w = masks.shape
        boxes, counts = _f32((n + 1, 4), device), torch.full((n + 1,), -77, dtype=torch.int32, device=device)
        rc = _lib().ovm_sam_mask_boxes(_dev(masks, device).data_ptr(), n, h, w, boxes.data_ptr(), counts.data_ptr(), _stream())
        assert rc == 0
        boxes, counts = _np(boxes), _np(counts)
        rb, rc_ = po.mask_boxes(masks)
        _untouched(boxes[-1], "mask boxes")
        assert counts[-1] == -77
        assert np.array_equal(boxes[:n], rb) and np.array_equal(counts[:n], rc_), (boxes[:n], rb, counts[:n], rc_)
    keep = _f32((5, 4), device)
    assert _lib().ovm_sam_mask_boxes(_dev(m, device).data_ptr(), 5, 0, W, keep.data_ptr(), None, _stream()) == OVM_ERR_INVALID      # H = 0, no counts
    _untouched(_np(keep), "mask boxes refusal")
