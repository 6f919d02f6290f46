"""The chunked one-pass bi-attention (biattn_mfma_kernel + biattn_mfma_combine_kernel) restated in float32 numpy against the float64
formula: per-chunk column maximum, sum and partial context, text blocks of 32 with the image side's online rescale, rows past S and
text tokens past T masked, chunks combined in increasing order. No GPU."""
import numpy as np
import pytest

from biattn_cases import make_inputs, reference, rel_err

CHUNK, TB = 64, 32
f32 = np.float32


def chunked_f32(q, k, vi, vt, H, scale):
    S, E = q.shape
    T, dh = k.shape[0], E // H
    nchunk = (S + CHUNK - 1) // CHUNK
    ci = np.zeros((S, E), f32)
    part = np.zeros((nchunk, T, E), f32)
    m = np.full((nchunk, H, T), -np.inf, f32)
    l = np.zeros((nchunk, H, T), f32)
    for c in range(nchunk):
        rows = np.arange(c * CHUNK, (c + 1) * CHUNK)
        valid = rows < S
        rc = np.minimum(rows, S - 1)                           # rows past S: the last row, masked below
        for h in range(H):
            sl = slice(h * dh, (h + 1) * dh)
            o = np.zeros((CHUNK, dh), f32)
            mi = np.full(CHUNK, -np.inf, f32)
            li = np.zeros(CHUNK, f32)
            for t0 in range(0, T, TB):
                nt = min(TB, T - t0)
                kb, vb = np.zeros((TB, dh), f32), np.zeros((TB, dh), f32)
                kb[:nt], vb[:nt] = k[t0:t0 + nt, sl], vt[t0:t0 + nt, sl]
                sc = (q[rc][:, sl] @ kb.T).astype(f32) * f32(scale)                     # [CHUNK, TB]
                # image side
                x = np.where(np.arange(TB)[None, :] < nt, sc, f32(-np.inf))
                mn = np.maximum(mi, x.max(axis=1))
                alpha = np.exp(mi - mn).astype(f32)
                p = np.exp(x - mn[:, None]).astype(f32)
                li = li * alpha + p.sum(axis=1, dtype=f32)
                o = o * alpha[:, None] + (p @ vb).astype(f32)
                mi = mn
                # text side
                cm = np.where(valid[:, None], sc, f32(-np.inf)).max(axis=0)             # [TB]
                pp = np.where(valid[:, None], np.exp(sc - cm[None, :]), 0).astype(f32)
                m[c, h, t0:t0 + nt] = cm[:nt]
                l[c, h, t0:t0 + nt] = pp.sum(axis=0, dtype=f32)[:nt]
                part[c, t0:t0 + nt, sl] = (pp.T @ vi[rc][:, sl]).astype(f32)[:nt]
            ci[rows[valid], sl] = (o / li[:, None])[valid]
    ct = np.zeros((T, E), f32)
    for h in range(H):
        sl = slice(h * dh, (h + 1) * dh)
        M = m[:, h].max(axis=0)                                # [T]
        num, den = np.zeros((T, dh), f32), np.zeros(T, f32)
        for c in range(nchunk):
            w = np.exp(m[c, h] - M).astype(f32)
            num += part[c][:, sl] * w[:, None]
            den += l[c, h] * w
        ct[:, sl] = num / den[:, None]
    return ci, ct, m


CASES = {
    "last_chunk_of_two_rows": dict(S=CHUNK + 2, T=20),
    "second_text_block_of_one": dict(S=3 * CHUNK, T=33),
    "text_limit": dict(S=2 * CHUNK + 1, T=256),
    "peaked": dict(S=3 * CHUNK, T=20, peaked_chunk=CHUNK),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_chunked_algorithm_matches_float64_formula(name):
    """Bound: a score is a sum of dh fp32 products, so its rounding error is about sqrt(dh) * 2^-24 * max |score|, and the exponential
    turns an absolute error of a score into a relative error of a probability. Four times that (3.8e-6 * max(1, max |score|): about 2e-5
    for unit-normal scores of up to 5, 1.4e-4 for the peaked case's scores of 35 - 40) covers the sums that follow; a masking or rescaling mistake
    is an error of 1e-2 and more."""
    H, dh = 4, 256
    q, k, vi, vt = make_inputs(H=H, dh=dh, seed=3, **CASES[name])
    scale = 1.0 / np.sqrt(dh)
    ri, rt = reference(q, k, vi, vt, H, scale)
    assert np.isfinite(ri).all() and np.isfinite(rt).all()
    assert np.abs(ri).max() > 0.1 and np.abs(rt).max() > 0.1 and ri.std() > 1e-2 and rt.std() > 1e-2      # non-degenerate
    ci, ct, m = chunked_f32(q, k, vi, vt, H, scale)
    assert np.isfinite(ci).all() and np.isfinite(ct).all()
    ei, et = rel_err(ci, ri), rel_err(ct, rt)
    print(f"{name}: image {ei:.3e} text {et:.3e}")
    amax = max(np.abs(scale * (q[:, h * dh:(h + 1) * dh].astype(np.float64) @ k[:, h * dh:(h + 1) * dh].astype(np.float64).T)).max()
               for h in range(H))
    tol = 4 * np.sqrt(dh) * 2.0 ** -24 * max(1.0, amax)
    assert ei < tol and et < tol, (ei, et, tol)
    if name == "peaked":
        # the construction holds: the peaked column leads its rows by about 30 and the second chunk's maximum lies about 40 lower
        a = scale * (q[:, :dh].astype(np.float64) @ k[:, :dh].astype(np.float64).T)
        lead = a[:CHUNK, 3] - np.delete(a[:CHUNK], 3, axis=1).max(axis=1)
        assert 20 < lead.mean() < 40
        assert 30 < m[0, 0, 3] - m[1, 0, 3] < 50
