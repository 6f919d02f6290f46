"""GPU: ovm_render_scene_points (ovmono3d_amd/csrc/render.hip) against the numpy restatement tests/scene_points_oracle.py.

The key buffer of the splat equals the oracle's bit for bit (both sides are the same IEEE fp64 operations and a minimum, which no
execution order changes); the composition is checked against the render without points of the same layout; with depth=None
draw_scene_view gives the bytes of ovm_render_scene called directly."""
import ctypes as C

import numpy as np
import pytest
import torch

import scene_oracle as so
import scene_points_oracle as po

pytestmark = pytest.mark.gpu

H, W, S = 48, 64, 96
K = np.array([[96.0, 0.0, W / 2], [0.0, 96.0, H / 2], [0.0, 0.0, 1.0]])
COLORS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)    # saturated: no shaded face, edge or label comes out grey
ROT = {"default": None, "tilt": so.euler2mat([2.2, 0.3, 0.1]), "side": so.euler2mat([0.2, 1.2, 0.0])}


def _boxes(n):
    cs = [((-0.6, 0.3, 4.5), (0.8, 0.7, 0.9), 0.3), ((0.7, 0.2, 5.5), (0.9, 0.9, 0.7), -0.5), ((0.0, 0.45, 3.6), (0.5, 0.4, 0.5), 1.0)][:n]
    return np.stack([so.cuboid(*c) for c in cs]) if n else np.zeros((0, 8, 3))


def _depth(kind, h=H, w=W, seed=5):
    rng = np.random.default_rng(seed)
    ii, jj = np.mgrid[0:h, 0:w]
    if kind == "plane":                                            # a tilted plane through the boxes
        return (4.5 + 0.03 * (jj - w / 2) * (64 / w) + 0.04 * (ii - h / 2) * (48 / h)).astype(np.float32)
    if kind == "noise":                                            # 0.5 .. 8 m salted with the values the depth rule removes
        d = rng.uniform(0.5, 8.0, (h, w)).astype(np.float32)
        salt = rng.integers(0, 40, (h, w))
        for v, k in ((np.nan, 0), (np.inf, 1), (0.0, 2), (-1.5, 3), (-np.inf, 4)):
            d[salt == k] = v
        return d
    if kind == "far":                                              # most points project off the canvas
        return (3.0 + 40.0 * rng.random((h, w)) ** 3).astype(np.float32)
    assert kind == "slab"                                          # the upper half right in front of the camera: behind zplane in the novel view
    return np.where(ii < h // 2, 0.2 + 0.01 * jj, 5.0).astype(np.float32)


def _novel(lay, R):
    return dict(Kn=np.array(list(lay.view[1].K)).reshape(3, 3), R=so.euler2mat([np.pi / 3, 0, 0]) if R is None else R,
                center=list(lay.center), shift=lay.zoom_bias * lay.zoom_factor, zplane=lay.zplane)


def _direct(lay, grid, img_t):
    """ovm_render_scene called directly: (front, novel) uint8 numpy."""
    from ovmono3d_amd import lib
    L = lib.load()
    h, w, s = lay.view[0].height, lay.view[0].width, lay.view[1].height
    nbytes = C.c_int64()
    lib.check(L.ovm_render_scene_workspace(C.byref(lay), 0, C.byref(nbytes)), what="ovm_render_scene_workspace")
    ws = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=img_t.device)
    front = torch.empty((h, w, 3), dtype=torch.uint8, device=img_t.device)
    novel = torch.empty((s, s, 3), dtype=torch.uint8, device=img_t.device)
    lib.check(L.ovm_render_scene(C.byref(lay), grid.ctypes.data if len(grid) else None, None, 0, img_t.data_ptr(), img_t.stride(0), front.data_ptr(),
                                 3 * w, novel.data_ptr(), 3 * s, ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              what="ovm_render_scene")
    torch.cuda.synchronize()
    return front.cpu().numpy(), novel.cpu().numpy()


def _pitched(a, device, pad=5):
    """The map as a column slice of a wider device buffer: rows pitched, columns dense."""
    t = torch.from_numpy(a).to(device)
    buf = torch.full((a.shape[0], a.shape[1] + pad), 77, dtype=t.dtype, device=device)
    buf[:, :a.shape[1]] = t
    return buf[:, :a.shape[1]]


def _drawn_mask(lay, n):
    """Novel-view pixels a label rectangle or a box edge of the layout covers."""
    V = lay.view[1]
    yy, xx = np.mgrid[0:V.height, 0:V.width].astype(np.float64)
    m = np.zeros((V.height, V.width), bool)
    r2 = (V.thickness / 2.0) ** 2
    for b in range(n):
        B = V.box[b]
        m[B.rect[1]:B.rect[3], B.rect[0]:B.rect[2]] = True
        for e in range(12):
            if not B.edge_drawn[e]:
                continue
            x0, y0, x1, y1 = (float(v) for v in B.edge[e])
            dx, dy = x1 - x0, y1 - y0
            ll = dx * dx + dy * dy
            t = np.clip(((xx - x0) * dx + (yy - y0) * dy) / ll, 0.0, 1.0) if ll > 0 else np.zeros_like(xx)
            m |= (xx - x0 - t * dx) ** 2 + (yy - y0 - t * dy) ** 2 <= r2
    return m


CASES = [  # n boxes, rotation, depth, point_size, labels, pitched rows
    (1, "default", "plane", 3, True, False),
    (1, "default", "slab", 1, False, False),
    (2, "default", "noise", 3, True, True),
    (3, "default", "plane", 9, True, False),
    (3, "tilt", "far", 1, False, True),
    (2, "side", "noise", 9, True, False),
    (0, "default", "plane", 3, True, False),                        # no boxes, no ground bounds: the early_return layout
]


@pytest.mark.parametrize("n,rot,kind,ps,with_labels,pitched", CASES)
def test_points_match_oracle_and_compose_under_the_boxes(device, n, rot, kind, ps, with_labels, pitched):
    from ovmono3d_amd import vis
    rng = np.random.default_rng(100 * n + ps)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[(img == 225).all(-1) | (img == 175).all(-1)] = 0
    depth = _depth(kind)
    labels = rng.integers(-1, max(n, 1), (H, W)).astype(np.int32) if with_labels else None
    corners, colors, R = _boxes(n), COLORS[:n], ROT[rot]
    lay, grid = vis.scene_layout(K, H, W, corners, colors, None, S, R=R)
    assert lay.early_return == (1 if n == 0 else 0)
    nv = _novel(lay, R)
    img_t = torch.from_numpy(img).to(device)
    p0_front, p0_novel = _direct(lay, grid, img_t)

    up = (lambda a: _pitched(a, device)) if pitched else (lambda a: torch.from_numpy(a).to(device))
    zb = torch.zeros((S, S), dtype=torch.int64, device=device)
    front, novel = vis.draw_scene_view(img_t, K, corners, colors, scale=S, R=R, depth=up(depth), point_size=ps,
                                       point_labels=up(labels) if with_labels else None, zbuf_out=zb)
    torch.cuda.synchronize()
    zdev = zb.cpu().numpy().view(np.uint64)
    front, novel = front.cpu().numpy(), novel.cpu().numpy()

    # 1. the key buffer, bit for bit
    if n == 0:
        zref = np.full((S, S), po.EMPTY, np.uint64)               # early_return: nothing is splatted
    else:
        zref, stats = po.splat(depth, K, nv["Kn"], nv["R"], nv["center"], nv["shift"], nv["zplane"], S, ps)
        assert stats["splatted"] > 100 and stats["off_canvas"] > 100, stats      # the case reaches the paths it is here for
        if kind in ("noise",):
            assert stats["bad_depth"] > 300, stats
        if kind == "slab" or rot == "tilt":
            assert stats["behind"] > 1000, stats
    bad = np.argwhere(zdev != zref)
    assert len(bad) == 0, f"{len(bad)} keys differ, first at {bad[:3].tolist()}: {[(hex(zdev[y, x]), hex(zref[y, x])) for y, x in bad[:3]]}"

    # 3. composition against the render without points
    assert np.array_equal(front, p0_front)
    edge_u8 = np.ctypeslib.as_array(lay.edge_u8)[:n]
    hit, col = po.compose(zref, img, labels, edge_u8)
    grey = (p0_novel == 225).all(-1) | (p0_novel == 175).all(-1)
    assert not (grey & _drawn_mask(lay, n)).any()                  # no face, edge or label of these scenes is one of the two greys
    same = (novel == p0_novel).all(-1)
    point = hit & (novel == col).all(-1)
    assert (same | point).all(), f"{int((~(same | point)).sum())} novel pixels are neither the plain render nor the point colour"
    assert point[hit & grey].all(), f"{int((~point[hit & grey]).sum())} points are missing on the canvas"
    if n == 0:
        assert (novel == 255).all()
    else:
        assert (hit & grey).sum() > 100
    if (n, kind) == (3, "plane"):                                  # box faces cover part of the cloud and stay on top
        covered = hit & ~grey & ~_drawn_mask(lay, n)
        assert covered.sum() > 50 and same[covered].all()
        assert (col[covered] != p0_novel[covered]).any()


def test_early_return_with_boxes_draws_the_bare_render(device):
    from ovmono3d_amd import vis
    corners, colors, K2, kw = so.make_scene(21, 2, "early", H, W)
    img = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    lay, grid = vis.scene_layout(K2, H, W, corners, colors, None, S, **kw)
    assert lay.early_return == 1
    img_t = torch.from_numpy(img).to(device)
    p0_front, p0_novel = _direct(lay, grid, img_t)
    zb = torch.zeros((S, S), dtype=torch.int64, device=device)
    front, novel = vis.draw_scene_view(img_t, K2, corners, colors, scale=S, depth=_depth("plane"), zbuf_out=zb, **kw)
    assert np.array_equal(front.cpu().numpy(), p0_front) and np.array_equal(novel.cpu().numpy(), p0_novel)
    assert (zb.cpu().numpy().view(np.uint64) == po.EMPTY).all()


@pytest.mark.parametrize("n,scale", ((3, S), (2, H), (0, S)))
def test_without_depth_the_bytes_are_ovm_render_scenes(device, n, scale):
    from ovmono3d_amd import vis
    img = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)
    corners, colors = _boxes(n), COLORS[:n]
    lay, grid = vis.scene_layout(K, H, W, corners, colors, None, scale)
    img_t = torch.from_numpy(img).to(device)
    p0_front, p0_novel = _direct(lay, grid, img_t)
    front, novel = vis.draw_scene_view(img_t, K, corners, colors, scale=scale, depth=None)
    assert np.array_equal(front.cpu().numpy(), p0_front) and np.array_equal(novel.cpu().numpy(), p0_novel)


def test_labels_from_masks_lowest_index_wins(device):
    from ovmono3d_amd import vis
    rng = np.random.default_rng(3)
    m = (rng.random((4, H, W)) > 0.7).astype(np.uint8) * rng.integers(1, 255, (4, H, W)).astype(np.uint8)
    got = vis.labels_from_masks(torch.from_numpy(m).to(device))
    assert got.is_cuda and got.dtype == torch.int32
    want = np.where((m != 0).any(0), (m != 0).argmax(0), -1)
    assert np.array_equal(got.cpu().numpy(), want)


def test_full_hd_key_buffer(device):
    """1080 x 1920 into a 1080 x 1080 canvas at point_size 3: about 19 M atomics; the buffer is the oracle's."""
    from ovmono3d_amd import vis
    h, w, s = 1080, 1920, 1080
    K2 = np.array([[2160.0, 0.0, w / 2], [0.0, 2160.0, h / 2], [0.0, 0.0, 1.0]])
    depth = _depth("plane", h, w)
    noise = _depth("noise", h, w)
    depth[::3] = noise[::3]
    img_t = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (h, w, 3), dtype=np.uint8)).to(device)
    corners, colors = _boxes(3), COLORS
    lay, _ = vis.scene_layout(K2, h, w, corners, colors, None, s)
    nv = _novel(lay, None)
    zb = torch.zeros((s, s), dtype=torch.int64, device=device)
    vis.draw_scene_view(img_t, K2, corners, colors, scale=s, depth=torch.from_numpy(depth).to(device), point_size=3, zbuf_out=zb)
    zref, stats = po.splat(depth, K2, nv["Kn"], nv["R"], nv["center"], nv["shift"], nv["zplane"], s, 3)
    assert stats["splatted"] > 500_000, stats
    assert np.array_equal(zb.cpu().numpy().view(np.uint64), zref)
