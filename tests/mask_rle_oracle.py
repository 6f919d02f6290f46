"""numpy restatement of COCO's run-length encoding of binary masks (pycocotools' maskApi.c: rleEncode, rleToString, rleFrString), the
reference of ovm_mask_rle_encode / ovm_mask_rle_decode. Written from the rules in include/ovm3d.h, independently of
ovmono3d_amd.masks. pycocotools is not installed here: string parity with it is unpinned (tests/test_mask_rle_cpu.py says how it is
held instead); the counts are pinned against transformers' _mask_to_rle there."""
from typing import List

import numpy as np


def counts(plane: np.ndarray) -> List[int]:
    """uint8 / bool [H, W], nonzero = inside -> run lengths along the column-major scan, the first a run of zeros."""
    v = (np.asarray(plane) != 0).T.reshape(-1).astype(np.int8)            # column-major: p = x * H + y
    change = np.flatnonzero(np.diff(np.concatenate([[0], v])) != 0)       # positions whose value differs from the one in front
    edges = np.concatenate([[0], change, [v.size]])
    return [int(c) for c in np.diff(edges)]


def to_string(cnts: List[int]) -> str:
    out = []
    for i, c in enumerate(cnts):
        x = int(c)
        if i > 2:
            x -= int(cnts[i - 2])
        more = True
        while more:
            c5 = x & 0x1f
            x >>= 5                                                       # Python's >> on int is arithmetic
            more = (x != -1) if (c5 & 0x10) else (x != 0)
            if more:
                c5 |= 0x20
            out.append(chr(c5 + 48))
    return "".join(out)


def from_string(s: str) -> List[int]:
    cnts: List[int] = []
    p = 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def decode(cnts: List[int], H: int, W: int) -> np.ndarray:
    """counts -> uint8 [H, W] of 0 / 1 (the value of run k is k & 1)."""
    assert sum(cnts) == H * W
    v = np.repeat(np.arange(len(cnts)) & 1, cnts).astype(np.uint8)
    return np.ascontiguousarray(v.reshape(W, H).T)


def encode(plane: np.ndarray, compressed: bool = True) -> dict:
    c = counts(plane)
    return {"size": [int(plane.shape[0]), int(plane.shape[1])], "counts": to_string(c) if compressed else c}


# ---- the planes both test files use --------------------------------------------------------------------------------------------
SHAPES = [(1, 7), (7, 1), (17, 9), (37, 53), (64, 64), (65, 129), (250, 333)]


def blobs(H: int, W: int, seed: int, k: int = 4) -> np.ndarray:
    """A few seeded discs and a bar: runs of many lengths, some through column boundaries."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(k):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1, max(2.0, min(H, W) / 2.5))
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    m[:, rng.randint(0, W)] = True
    return m.astype(np.uint8)


def edge_planes(H: int, W: int) -> dict:
    """name -> uint8 [H, W]: the contents the issue lists."""
    first = np.zeros((H, W), np.uint8); first[0, 0] = 1
    last = np.zeros((H, W), np.uint8); last[H - 1, W - 1] = 1
    rows = np.zeros((H, W), np.uint8); rows[::2, :] = 1; rows[H - 1, :] = 1      # full rows: with the last row set a run crosses every column boundary
    p = np.arange(W)[None, :] * H + np.arange(H)[:, None]
    checker = (p % 2 == 0).astype(np.uint8)                                      # alternates along p, first pixel set: H * W + 1 counts
    b = blobs(H, W, seed=H * 1000 + W)
    return {"zeros": np.zeros((H, W), np.uint8), "ones": np.ones((H, W), np.uint8), "first": first, "last": last, "rows": rows,
            "checker": checker, "blobs": b, "values_2_255": np.where(b != 0, 2, 0).astype(np.uint8) | np.where(blobs(H, W, seed=7) != 0, 255, 0).astype(np.uint8),
            "noise": (np.random.RandomState(H + W).rand(H, W) < 0.3).astype(np.uint8)}
