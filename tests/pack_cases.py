"""Inputs and the numpy reference of the packed fp16 weight image (csrc/gemm.hpp), shared by the host test of
ovm_host_pack_weight and the GPU test that pins it to ovm_g_pack_weight."""
import numpy as np

# (N, K, Kpad): two row blocks, the second mostly padding, K ending inside a 32-group, a pad wider than ceil64(K); one element; no padding at all
SHAPES = [(130, 70, 128), (1, 1, 64), (128, 64, 64)]


def values():
    """fp32 pool: every fp16 edge first, then seeded normals at four scales."""
    ties = [(m + 0.5) * 2.0 ** (e - 10) for e in (-14, -3, 0, 5, 15) for m in range(1024, 1040)]     # halfway between two fp16 normals
    ties += [(j + 0.5) * 2.0 ** -24 for j in range(8)]                                                  # ... between two subnormals
    edge = ties + [-t for t in ties] + [0.0, -0.0, 65504.0, 65520.0, 6e-8, 2.98e-8, -65504.0, -65520.0, -6e-8, -2.98e-8]
    rng = np.random.default_rng(20240607)
    normals = [rng.standard_normal(2048) * s for s in (1.0, 1e-3, 1e-5, 1e-7)]
    return np.concatenate([np.asarray(edge)] + normals).astype(np.float32)


def matrix(N, K):
    """[N][K] fp32 that cycles through values(); the single-element shape gets a rounding tie."""
    v = values()
    return np.resize(v, N * K).reshape(N, K).copy()


def reference_image(w, Kpad, precision):
    """uint16 bits of the image: hi = fp16(x), lo = fp16(x - hi); rows padded to 128; split mode [Npad][Kpad/32][hi 32 | lo 32]."""
    N, K = w.shape
    Npad = (N + 127) // 128 * 128
    with np.errstate(over="ignore"):
        hi = w.astype(np.float16)
        lo = (w - hi.astype(np.float32)).astype(np.float16)
    H = np.zeros((Npad, Kpad), np.float16); H[:N, :K] = hi
    if precision == 1:
        return H.view(np.uint16).reshape(-1)
    Lo = np.zeros((Npad, Kpad), np.float16); Lo[:N, :K] = lo
    img = np.stack([H.reshape(Npad, Kpad // 32, 32), Lo.reshape(Npad, Kpad // 32, 32)], axis=2)
    return np.ascontiguousarray(img).view(np.uint16).reshape(-1)


def host_image(L, w, Kpad, precision, fill=0xABCD):
    """ovm_host_pack_weight's image of w (uint16 bits) and its return code; the buffer starts as `fill`."""
    N, K = w.shape
    Npad = (max(N, 1) + 127) // 128 * 128
    out = np.full(Npad * Kpad * (2 if precision == 3 else 1), fill, np.uint16)
    w = np.ascontiguousarray(w, np.float32)
    rc = L.ovm_host_pack_weight(w.ctypes.data, N, K, Kpad, precision, out.ctypes.data)
    return rc, out
