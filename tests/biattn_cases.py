"""Inputs and the float64 reference of the fusion layer's bi-attention, shared by test_biattn_math_cpu.py and test_gpu_biattn.py.

With A = scale * Q K_text^T per head: image context = softmax over T of A, times V_text; text context = softmax over S of A^T,
times V_img (GroundingDINO BiMultiHeadAttention.forward after its projections)."""
import numpy as np


def make_inputs(S, T, H=4, dh=256, seed=0, peaked_chunk=0):
    """fp32 q, v_img [S, H*dh] and k_text, v_text [T, H*dh]; unit normal, so that scale * q.k is about unit normal too.

    peaked_chunk > 0 (the chunk length of the kernel under test) builds the peaked case: a common direction e (|e| = 1 per head) is
    added to every query (16 e) and, 30-fold, to text token 3's key, so that token's scores lie about 30 above the others
    (scale * 16 * 30 = 30, the cross terms are +-2); the queries of the second chunk are multiplied by -1/3, which puts that chunk's
    maximum of the peaked column at about -10, 40 below its neighbours'."""
    rng = np.random.default_rng(seed)
    E = H * dh
    q = rng.standard_normal((S, E)).astype(np.float32)
    k = rng.standard_normal((T, E)).astype(np.float32)
    vi = rng.standard_normal((S, E)).astype(np.float32)
    vt = rng.standard_normal((T, E)).astype(np.float32)
    if peaked_chunk:
        assert T > 3 and S >= 2 * peaked_chunk
        e = np.float32(1.0 / np.sqrt(dh))
        q += np.float32(16.0) * e
        k[3] += np.float32(30.0) * e
        q[peaked_chunk:2 * peaked_chunk] *= np.float32(-1.0 / 3.0)
    return q, k, vi, vt


def reference(q, k, vi, vt, H, scale):
    """float64 image context [S, E] and text context [T, E]"""
    S, E = q.shape
    T, dh = k.shape[0], E // H
    q, k, vi, vt = (x.astype(np.float64) for x in (q, k, vi, vt))
    ci, ct = np.empty((S, E)), np.empty((T, E))
    for h in range(H):
        sl = slice(h * dh, (h + 1) * dh)
        a = scale * (q[:, sl] @ k[:, sl].T)                     # [S, T]
        p = np.exp(a - a.max(axis=1, keepdims=True))
        ci[:, sl] = (p / p.sum(axis=1, keepdims=True)) @ vt[:, sl]
        p = np.exp(a - a.max(axis=0, keepdims=True))
        ct[:, sl] = (p / p.sum(axis=0, keepdims=True)).T @ vi[:, sl]
    return ci, ct


def rel_err(a, b):
    """max |a - b| / max |b|"""
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())
