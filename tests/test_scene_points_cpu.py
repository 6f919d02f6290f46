"""CPU: the numpy restatement of the point cloud (tests/scene_points_oracle.py) on closed cases, its agreement with the host
layout's own box corners, and the refusals of ovm_render_scene_points and draw_scene_view - all before any device work."""
import ctypes as C

import numpy as np
import pytest
import torch

import scene_oracle as so
import scene_points_oracle as po

EMPTY = int(po.EMPTY)
I3 = np.eye(3)


def _key(z, idx):
    return (int(np.float32(z).view(np.uint32)) << 32) | idx


def _layout(n=2, seed=3, H=48, W=64, S=96, **kw):
    from ovmono3d_amd import vis
    corners, colors, K, kw2 = so.make_scene(seed, n, "plain", H, W)
    kw2.update(kw)
    lay, grid = vis.scene_layout(K, H, W, corners, colors, None, S, **kw2)
    return lay, grid, corners, K


def _novel(lay):
    return dict(Kn=np.array(list(lay.view[1].K)).reshape(3, 3), center=list(lay.center), shift=lay.zoom_bias * lay.zoom_factor, zplane=lay.zplane)


def test_plane_corners_land_where_project_puts_them():
    H, W, S = 48, 64, 96
    lay, _, _, K = _layout()
    nv = _novel(lay)
    R = so.euler2mat([np.pi / 3, 0, 0])
    depth = np.full((H, W), 5.0, np.float32)                       # fronto-parallel plane
    valid, front, x, y, key = po.targets(depth, K, nv["Kn"], R, nv["center"], nv["shift"], nv["zplane"])
    zbuf, stats = po.splat(depth, K, nv["Kn"], R, nv["center"], nv["shift"], nv["zplane"], S, 1)
    assert stats["bad_depth"] == 0 and stats["behind"] == 0
    for i, j in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        p = (((j + 0.5) - K[0, 2]) / K[0, 0] * 5.0, ((i + 0.5) - K[1, 2]) / K[1, 1] * 5.0, 5.0)
        r0, r1, r2 = so._rot(R, nv["center"], *p)
        r2 = r2 + nv["shift"]
        u, v = so._proj(nv["Kn"], r0, r1, r2, r2)
        assert (x[i, j], y[i, j]) == (np.floor(u), np.floor(v))
        assert key[i, j] == _key(r2, i * W + j)
        if 0 <= u < S and 0 <= v < S:
            assert int(zbuf[int(np.floor(v)), int(np.floor(u))]) <= int(key[i, j])   # that pixel holds this point or a nearer one


def _two_pixels(d0, d1, point_size=1, S=8, cx=4.0, cy=4.0):
    """A 1 x 2 image under a long focal length seen by a novel camera of focal length 1: both pixels land on one target."""
    K = np.array([[100.0, 0, 2.0], [0, 100.0, 0.5], [0, 0, 1]])    # X / Z = -0.015 and -0.005, Y = 0
    Kn = np.array([[1.0, 0, cx], [0, 1.0, cy], [0, 0, 1]])
    return po.splat(np.array([[d0, d1]], np.float32), K, Kn, I3, [0, 0, 0], 0.0, 0.05, S, point_size)


def test_nearer_point_wins_and_lower_index_wins_a_tie():
    zbuf, stats = _two_pixels(2.0, 1.0)
    assert stats["splatted"] == 2 and (zbuf != po.EMPTY).sum() == 1
    assert int(zbuf[4, 3]) == _key(1.0, 1)                         # u = 4 - 0.015 and 4 - 0.005 -> floor 3; v = 4 + 0 -> 4
    zbuf, _ = _two_pixels(1.0, 2.0)
    assert int(zbuf[4, 3]) == _key(1.0, 0)
    zbuf, _ = _two_pixels(1.5, 1.5)
    assert int(zbuf[4, 3]) == _key(1.5, 0)                         # equal depth: the lower source index


def test_depth_rules_and_zplane():
    for bad in (np.nan, np.inf, -np.inf, 0.0, -1.0):
        zbuf, stats = _two_pixels(bad, 1.0)
        assert stats["bad_depth"] == 1 and int(zbuf[4, 3]) == _key(1.0, 1)
    zbuf, stats = _two_pixels(0.04, 0.05)                          # zplane 0.05: >= keeps the point on the plane
    assert stats["behind"] == 1 and int(zbuf[4, 3]) == _key(np.float32(0.05), 1)


def test_footprint_is_clipped_at_the_canvas_edge():
    zbuf, _ = _two_pixels(1.0, np.nan, point_size=5, cx=0.5, cy=0.0)   # target (0, 0)
    hit = zbuf != po.EMPTY
    assert hit[:3, :3].all() and hit.sum() == 9
    zbuf, stats = _two_pixels(1.0, np.nan, point_size=5, cx=-0.5, cy=0.0)   # target (-1, 0): two columns of the square are left
    assert stats["splatted"] == 1 and (zbuf != po.EMPTY)[:3, :2].all() and (zbuf != po.EMPTY).sum() == 6
    zbuf, stats = _two_pixels(1.0, np.nan, point_size=5, cx=-2.5, cy=0.0)   # target (-3, 0): nothing reaches the canvas
    assert stats["off_canvas"] == 1 and (zbuf == po.EMPTY).all()
    zbuf, _ = _two_pixels(1.0, np.nan, point_size=9, S=8, cx=7.5, cy=7.5)   # target (7, 7), bottom right
    assert (zbuf != po.EMPTY)[3:, 3:].all() and (zbuf != po.EMPTY).sum() == 25


@pytest.mark.parametrize("pix", ((10, 20), (30, 41), (5, 60)))
def test_point_on_a_box_corner_lands_on_the_layouts_edge_endpoint(pix):
    """Corner 0 of a box is the camera point of a source pixel: the pixel's target is the endpoint ovm_host_scene_layout gives the edges
    that start (0-1, 0-4) or end (3-0) at that corner."""
    from ovmono3d_amd import vis
    H, W, S = 48, 64, 96
    i, j = pix
    corners, colors, K, _ = so.make_scene(11, 2, "plain", H, W)
    d = np.float32(6.25)
    corners[0, 0] = (((j + 0.5) - K[0, 2]) / K[0, 0] * float(d), ((i + 0.5) - K[1, 2]) / K[1, 1] * float(d), float(d))
    lay, _ = vis.scene_layout(K, H, W, corners, colors, None, S)
    nv = _novel(lay)
    depth = np.full((H, W), np.nan, np.float32)
    depth[i, j] = d
    valid, front, x, y, _ = po.targets(depth, K, nv["Kn"], so.euler2mat([np.pi / 3, 0, 0]), nv["center"], nv["shift"], nv["zplane"])
    assert valid[i, j] and front[i, j] and x[i, j] >= 0 and y[i, j] >= 0
    B = lay.view[1].box[0]
    assert B.edge_drawn[0] and B.edge_drawn[1] and B.edge_drawn[5]
    assert list(B.edge[0])[:2] == list(B.edge[1])[:2] == list(B.edge[5])[2:] == [int(x[i, j]), int(y[i, j])]


def test_compose_rule():
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 10
    zbuf = np.full((2, 2), po.EMPTY, np.uint64)
    zbuf[0, 1] = _key(1.0, 4)                                      # source pixel (1, 1)
    zbuf[1, 0] = _key(2.0, 2)                                      # source pixel (0, 2)
    labels = np.array([[-1, -1, 0], [-1, -1, -1]], np.int32)
    hit, col = po.compose(zbuf, img, labels, np.array([[255, 0, 7, 0]], np.uint8))
    assert hit.tolist() == [[False, True], [True, False]]
    assert col[0, 1].tolist() == img[1, 1].tolist()
    assert col[1, 0].tolist() == [(60 + 255 + 1) >> 1, (70 + 0 + 1) >> 1, (80 + 7 + 1) >> 1]
    _, plain = po.compose(zbuf, img)
    assert plain[1, 0].tolist() == img[0, 2].tolist()


# ------------------------------------------------------------------------------------------------------------------ refusals

def _call(lay, grid, **over):
    """ovm_render_scene_points with pointers that are never followed: every case here is refused before any device work."""
    from ovmono3d_amd import lib
    L = lib.load()
    H, W, S = lay.view[0].height, lay.view[0].width, lay.view[1].height
    fake = 1 << 20
    a = dict(image=fake, image_pitch=3 * W, front=fake, front_pitch=3 * W, novel=fake, novel_pitch=3 * S, depth=fake, depth_pitch=4 * W,
             labels=None, labels_pitch=0, R=(C.c_double * 9)(*so.euler2mat([np.pi / 3, 0, 0]).reshape(-1).tolist()), point_size=3)
    a.update(over)
    return L.ovm_render_scene_points(C.byref(lay), grid.ctypes.data if len(grid) else None, None, 0, a["image"], a["image_pitch"], a["front"],
                                     a["front_pitch"], a["novel"], a["novel_pitch"], a["depth"], a["depth_pitch"], a["labels"], a["labels_pitch"],
                                     C.byref(a["R"]) if a["R"] is not None else None, a["point_size"], None, fake, 1 << 40, None)


def test_library_refuses_bad_point_arguments():
    from ovmono3d_amd import lib, vis
    lay, grid, corners, K = _layout()
    W = lay.view[0].width
    assert _call(lay, grid, depth=None) == -1
    assert _call(lay, grid, depth_pitch=4 * W - 4) == -1
    assert _call(lay, grid, depth_pitch=4 * W + 2) == -1
    assert _call(lay, grid, labels=1 << 20, labels_pitch=4 * W - 4) == -1
    assert _call(lay, grid, R=None) == -1
    for ps in (0, 2, 4, 8, 10, 11, -1):
        assert _call(lay, grid, point_size=ps) == -1, ps
    ws = C.c_int64()
    for mode in ("front", "novel"):
        one, g1 = vis.scene_layout(K, 48, 64, corners, so.make_scene(3, 2, "plain", 48, 64)[1], None, 96, mode=mode)
        assert _call(one, g1) == -1, mode
        assert lib.load().ovm_render_scene_points_workspace(C.byref(one), 0, C.byref(ws)) == -1
    base = C.c_int64()
    L = lib.load()
    assert L.ovm_render_scene_points_workspace(C.byref(lay), 0, C.byref(ws)) == 0 and L.ovm_render_scene_workspace(C.byref(lay), 0, C.byref(base)) == 0
    assert ws.value >= base.value + 8 * 96 * 96                    # the key buffer on top of ovm_render_scene's workspace


def test_draw_scene_view_refuses_bad_point_arguments():
    from ovmono3d_amd import vis
    H, W = 48, 64
    corners, colors, K, _ = so.make_scene(3, 2, "plain", H, W)
    im = np.zeros((H, W, 3), np.uint8)
    good = np.ones((H, W), np.float32)

    def bad(**kw):
        kw.setdefault("depth", good)
        with pytest.raises(ValueError):
            vis.draw_scene_view(im, K, corners, colors, scale=96, **kw)

    bad(depth=good.astype(np.float64))                             # dtype
    bad(depth=np.ones((H, W + 1), np.float32))                     # shape
    bad(depth=np.ones((1, H, W), np.float32))
    bad(depth=torch.ones(H, W))                                    # a CPU tensor
    bad(depth=good.tolist())
    bad(point_labels=np.zeros((H, W), np.int64))
    bad(point_labels=np.zeros((H + 1, W), np.int32))
    bad(point_labels=torch.zeros(H, W, dtype=torch.int32))
    for ps in (0, 2, 10, 11, 3.0, True):
        bad(point_size=ps)
    bad(mode="novel")
    bad(mode="front")
    bad(depth=None, point_labels=np.zeros((H, W), np.int32))       # labels without a depth


def test_labels_from_masks_rule_on_the_host():
    from ovmono3d_amd import vis
    m = torch.zeros(3, 2, 3, dtype=torch.uint8)
    m[2, 0, :] = 1
    m[1, 0, 1:] = 7
    m[0, 1, 2] = 1
    assert vis.labels_from_masks(m).tolist() == [[2, 1, 1], [-1, -1, 0]]
    assert vis.labels_from_masks(m).dtype == torch.int32
    assert vis.labels_from_masks(m[:0]).tolist() == [[-1] * 3] * 2
    with pytest.raises(ValueError):
        vis.labels_from_masks(m.float())
