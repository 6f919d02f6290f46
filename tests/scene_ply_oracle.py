"""Numpy restatement of <name>_scene.ply (include/ovm3d.h, "Scene as a PLY file"): fp64 arithmetic, one rounding to float32,
struct-packed little-endian bytes - and a minimal reader of the files it describes. Written from the rules, not from the package's
code: the tables below are typed here again."""
import struct

import numpy as np

QUADS = ((0, 1, 2, 3), (1, 5, 6, 2), (4, 0, 3, 7), (5, 4, 7, 6), (4, 5, 1, 0), (3, 2, 6, 7))
TRIS = tuple(t for a, b, c, d in QUADS for t in ((a, b, c), (c, d, a)))
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (1, 5), (5, 6), (6, 2), (4, 5), (4, 7), (6, 7), (0, 4), (3, 7))
TILE = 2048


def header(n_points, n_boxes, frame):
    lines = ["ply", "format binary_little_endian 1.0", f"comment ovmono3d_amd scene, frame {frame}, metres",
             f"element vertex {n_points + 8 * n_boxes}", "property float x", "property float y", "property float z",
             "property uchar red", "property uchar green", "property uchar blue",
             f"element face {12 * n_boxes}", "property list uchar int vertex_indices",
             f"element edge {12 * n_boxes}", "property int vertex1", "property int vertex2", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def edge_u8(colors):
    """min(255, c * 255 * 1.25) of the float32 colour, rounded half to even: uint8 [n, 3] in the image's channel order."""
    c = np.asarray(colors, np.float32).reshape(-1, 3).astype(np.float64)
    return np.rint(np.minimum(255.0, c * 255 * 1.25)).astype(np.uint8)


def valid_mask(depth, stride=1, max_depth=None):
    d = np.asarray(depth, np.float32)
    keep = np.zeros(d.shape, bool)
    keep[::stride, ::stride] = True
    with np.errstate(invalid="ignore"):
        keep &= np.isfinite(d) & (d > 0)
        if max_depth is not None:
            keep &= d <= np.float32(max_depth)
    return keep


def point_records(im, K, depth, labels=None, tint=None, stride=1, max_depth=None, frame="camera"):
    """(xyz float32 [P, 3], rgb uint8 [P, 3]) in row-major pixel order. tint: uint8 [n, 3] edge colours (BGR)."""
    K = np.asarray(K, np.float64).reshape(9)
    keep = valid_mask(depth, stride, max_depth)
    i, j = np.nonzero(keep)                                                # row-major
    d = np.asarray(depth, np.float32)[i, j].astype(np.float64)
    X = ((j + 0.5) - K[2]) / K[0] * d
    Y = ((i + 0.5) - K[5]) / K[4] * d
    xyz = np.stack([X, Y, d], 1).astype(np.float32)
    if frame == "opengl":
        xyz[:, 1:] = -xyz[:, 1:]
    c = np.asarray(im, np.uint8)[i, j].astype(np.int64)                    # B, G, R
    n = 0 if tint is None else len(tint)
    if labels is not None and n:
        b = np.asarray(labels, np.int64)[i, j]
        t = (b >= 0) & (b < n)
        c[t] = (c[t] + np.asarray(tint, np.int64).reshape(n, -1)[b[t], :3] + 1) >> 1
    return xyz, c[:, ::-1].astype(np.uint8)


def pack_vertices(xyz, rgb):
    return b"".join(struct.pack("<fffBBB", *(float(v) for v in p), *(int(v) for v in c)) for p, c in zip(xyz, rgb))


def box_part(corners, tint, n_points, frame="camera"):
    corners = np.asarray(corners, np.float64).reshape(-1, 8, 3)
    out = []
    for b, box in enumerate(corners):
        p = box.astype(np.float32)
        if frame == "opengl":
            p[:, 1:] = -p[:, 1:]
        out.append(pack_vertices(p, np.repeat(np.asarray(tint[b], np.uint8)[None, 2::-1], 8, 0)))
    for b in range(len(corners)):
        out += [struct.pack("<Biii", 3, *(n_points + 8 * b + v for v in t)) for t in TRIS]
    for b in range(len(corners)):
        out += [struct.pack("<ii", *(n_points + 8 * b + v for v in e)) for e in EDGES]
    return b"".join(out)


def scene_ply(im, K, depth=None, corners=None, colors=None, point_labels=None, stride=1, max_depth=None, frame="camera"):
    """(file bytes, P)."""
    corners = np.zeros((0, 8, 3)) if corners is None else np.asarray(corners, np.float64).reshape(-1, 8, 3)
    tint = edge_u8(colors) if len(corners) else np.zeros((0, 3), np.uint8)
    pts, P = b"", 0
    if depth is not None:
        xyz, rgb = point_records(im, K, depth, point_labels, tint, stride, max_depth, frame)
        P = len(xyz)
        rec = np.zeros(P, np.dtype({"names": ["p", "c"], "formats": [("<f4", 3), ("u1", 3)], "offsets": [0, 12], "itemsize": 15}))
        rec["p"], rec["c"] = xyz, rgb
        pts = rec.tobytes()                                                # the same bytes as pack_vertices (tests/test_scene_ply_cpu.py)
    return header(P, len(corners), frame) + pts + box_part(corners, tint, P, frame), P


def read_ply(data):
    """Minimal reader of the files above: {frame, xyz float32 [V, 3], rgb uint8 [V, 3], faces int32 [F, 3], edges int32 [E, 2]}."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"], lines[:2]
    assert lines[2].startswith("comment ovmono3d_amd scene, frame ") and lines[2].endswith(", metres")
    frame = lines[2][len("comment ovmono3d_amd scene, frame "):-len(", metres")]
    counts, props = {}, {}
    for ln in lines[3:]:
        w = ln.split()
        if w[:1] == ["element"]:
            cur = w[1]
            counts[cur], props[cur] = int(w[2]), []
        elif w[:1] == ["property"]:
            props[cur].append(tuple(w[1:]))
    assert list(counts) == ["vertex", "face", "edge"]
    assert props["vertex"] == [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    assert props["face"] == [("list", "uchar", "int", "vertex_indices")] and props["edge"] == [("int", "vertex1"), ("int", "vertex2")]
    V, F, E = counts["vertex"], counts["face"], counts["edge"]
    assert len(data) == end + 15 * V + 13 * F + 8 * E, (len(data), end, V, F, E)
    v = np.frombuffer(data, np.dtype({"names": ["p", "c"], "formats": [("<f4", 3), ("u1", 3)], "offsets": [0, 12], "itemsize": 15}), V, end)
    f = np.frombuffer(data, np.dtype({"names": ["n", "v"], "formats": ["u1", ("<i4", 3)], "offsets": [0, 1], "itemsize": 13}), F, end + 15 * V)
    assert (f["n"] == 3).all()
    e = np.frombuffer(data, "<i4", 2 * E, end + 15 * V + 13 * F).reshape(E, 2)
    return {"frame": frame, "xyz": v["p"].copy(), "rgb": v["c"].copy(), "faces": f["v"].copy(), "edges": e.copy()}


# ---- seeded inputs shared by the tests ----

def scene(H, W, seed, bad=0.0, n=0, wide=0):
    """Seeded image, depth, labels, K, corners and colours of one case. bad: the share of depth pixels set to NaN, +-inf, 0 or a
    negative value; wide: extra columns of the buffers the [H, W] maps are column slices of."""
    rng = np.random.RandomState(seed)
    Wb = W + wide
    im = rng.randint(0, 256, (H, Wb, 3)).astype(np.uint8)
    depth = rng.uniform(0.5, 9.0, (H, Wb)).astype(np.float32)
    if bad > 0:
        kind = rng.randint(0, 5, (H, Wb))
        hit = rng.uniform(size=(H, Wb)) < bad
        for k, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -1.5)):
            depth[hit & (kind == k)] = v
    labels = rng.randint(-1, n + 2, (H, Wb)).astype(np.int32)              # -1, valid indices, and values >= n
    f = 2.0 * max(H, W) + 0.25
    K = np.array([[f, 0.0, W / 2 + 0.3], [0.0, f * 1.01, H / 2 - 0.7], [0.0, 0.0, 1.0]])
    corners = rng.uniform(-3.0, 8.0, (n, 8, 3))
    colors = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    return {"im": im, "depth": depth, "labels": labels, "K": K, "corners": corners, "colors": colors, "wide": wide}
