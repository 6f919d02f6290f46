"""CPU: the host scene layout of the visualisation (ovm_host_scene_layout, include/ovm3d.h) equals the numpy restatement
tests/scene_oracle.py exactly - zoom, ground bounds, grid segment set, depth order, clipped edge endpoints, label rectangles -
and bad arguments are refused before any device work."""
import ctypes as C

import numpy as np
import pytest

import scene_oracle as so

N_BOXES = (1, 7, 100)


def _cases():
    cases, seed = [], 0
    for kind in so.KINDS:
        for n in N_BOXES:
            reps = 4 if n == 100 else 15
            for _ in range(reps):
                cases.append((seed, n, kind))
                seed += 1
    return cases


CASES = _cases()
assert len(CASES) >= 200


def _labels(rng, n):
    return rng.integers(0, 60, (2, n, 2)).astype(np.int32) * (rng.random((2, n, 1)) > 0.1)


def _compare(lay, grid, o, n):
    from ovmono3d_amd import lib
    assert lay.early_return == o["early_return"]
    assert lay.zoom_factor == o["zoom_factor"] and lay.zoom_bias == o["zoom_bias"]
    assert list(lay.center) == list(o["center"])
    assert list(lay.ground) == list(o["ground"])
    assert lay.grid_thickness == o["grid_thickness"]
    assert sorted(map(tuple, grid.tolist())) == o["grid"]
    assert np.array_equal(np.ctypeslib.as_array(lay.edge_color)[:n], o["edge_color"])
    assert np.array_equal(np.ctypeslib.as_array(lay.edge_u8)[:n, :3], o["edge_u8"])
    assert np.array_equal(np.ctypeslib.as_array(lay.edge_u8)[:n, 3], o["text_u8"])
    for v in range(2):
        ov = o["views"][v]
        V = lay.view[v]
        assert V.drawn == (ov is not None)
        if ov is None:
            continue
        assert (V.height, V.width, V.thickness) == (ov["H"], ov["W"], ov["thickness"])
        assert list(V.K) == ov["K"].reshape(-1).tolist()
        assert list(V.order)[:n] == ov["order"]
        for b in range(n):
            B, ob = V.box[b], ov["boxes"][b]
            assert np.array_equal(np.ctypeslib.as_array(B.verts), ob["verts"])
            assert np.array_equal(np.ctypeslib.as_array(B.edge_drawn), ob["edge_drawn"])
            assert np.array_equal(np.ctypeslib.as_array(B.edge), ob["edge"]), (v, b)
            assert (B.label_w, B.label_h) == ob["label"]
            assert tuple(B.rect) == ob["rect"] and tuple(B.text_org) == ob["text_org"], (v, b)
    assert lay.n_boxes == n and lib.OVM_SCENE_MAX_BOXES == 1024


@pytest.mark.parametrize("seed,n,kind", CASES)
def test_layout_matches_oracle(seed, n, kind):
    from ovmono3d_amd import vis
    corners, colors, K, kw = so.make_scene(seed, n, kind)
    rng = np.random.default_rng(1000 + seed)
    sizes = _labels(rng, n)
    masks = [[np.zeros((sizes[v, b, 1], sizes[v, b, 0]), np.uint8) for b in range(n)] for v in range(2)]
    H, W = 120, 160
    scale = int(rng.choice([H, 97, 200]))
    lay, grid = vis.scene_layout(K, H, W, corners, colors, masks, scale, blend_weight=0.5, blend_weight_overlay=0.85, **kw)
    o = so.layout(corners, colors, K, H, W, scale, label_size=sizes, blend_weight=0.5, blend_weight_overlay=0.85, **kw)
    _compare(lay, grid, o, n)
    if kind == "early":
        assert lay.early_return == 1
    if kind == "explicit":
        assert lay.early_return == 0 and lay.zoom_factor == 1.0 and lay.n_grid > 0


def test_modes_and_default_rotation():
    from ovmono3d_amd import vis
    corners, colors, K, _ = so.make_scene(7, 7, "plain")
    for mode, bits in (("front", so.FRONT), ("novel", so.NOVEL)):
        lay, grid = vis.scene_layout(K, 120, 160, corners, colors, None, 120, mode=mode)
        o = so.layout(corners, colors, K, 120, 160, 120, mode=bits)
        _compare(lay, grid, o, 7)
    assert np.array_equal(vis.euler2mat([np.pi / 3, 0, 0]), so.euler2mat([np.pi / 3, 0, 0]))


def test_face_winding_is_inward():
    """The front face's (v1 - v0) x (v2 - v0) points +z (into the box); every triangle's normal points to the box centre."""
    v = so.cuboid([0, 0, 5], [2, 1, 3], 0.0)
    assert np.cross(v[1] - v[0], v[2] - v[0])[2] > 0
    c = v.mean(0)
    for a, b, d in so.TRIS:
        n = np.cross(v[b] - v[a], v[d] - v[a])
        assert np.dot(n, c - (v[a] + v[b] + v[d]) / 3) > 0


def test_capacity_is_reported():
    from ovmono3d_amd import lib, vis
    L = lib.load()
    corners, colors, K, _ = so.make_scene(3, 7, "plain")
    lay_full, grid_full = vis.scene_layout(K, 120, 160, corners, colors, None, 120)
    inp = lib.OvmSceneInput()
    inp.n_boxes, inp.mode, inp.height, inp.width, inp.scale = 7, 3, 120, 160, 120
    inp.K[:] = K.reshape(-1).tolist()
    inp.R[:] = vis.euler2mat([np.pi / 3, 0, 0]).reshape(-1).tolist()
    inp.blend_weight, inp.blend_weight_overlay, inp.zplane = 0.8, 1.0, 0.05
    c64, c32 = np.ascontiguousarray(corners), np.ascontiguousarray(colors)
    inp.corners, inp.colors = c64.ctypes.data, c32.ctypes.data
    lay = lib.OvmSceneLayout()
    small = np.zeros((4, 4), np.int64)
    assert L.ovm_host_scene_layout(C.byref(inp), C.byref(lay), small.ctypes.data, 4) == -5
    assert lay.n_grid == lay_full.n_grid == len(grid_full) > 4


def test_bad_arguments_are_refused_without_device_work():
    """Every refusal happens in argument checking: none of these calls reaches the HIP runtime (there is no GPU here)."""
    from ovmono3d_amd import lib, vis
    L = lib.load()
    corners, colors, K, _ = so.make_scene(5, 7, "plain")
    lay, grid = vis.scene_layout(K, 120, 160, corners, colors, None, 120)
    g = np.zeros((16, 4), np.int64)

    def inp_with(**over):
        i = lib.OvmSceneInput()
        i.n_boxes, i.mode, i.height, i.width, i.scale = 7, 3, 120, 160, 120
        i.K[:] = K.reshape(-1).tolist()
        i.R[:] = np.eye(3).reshape(-1).tolist()
        i.zplane = 0.05
        c64, c32 = np.ascontiguousarray(over.pop("corners", corners)), np.ascontiguousarray(over.pop("colors", colors))
        i.corners, i.colors = c64.ctypes.data, c32.ctypes.data
        for k, v in over.items():
            setattr(i, k, v)
        return i, (c64, c32)

    out = lib.OvmSceneLayout()
    assert L.ovm_host_scene_layout(None, C.byref(out), g.ctypes.data, 16) == -1
    for over in ({"n_boxes": 1025}, {"n_boxes": -1}, {"mode": 0}, {"mode": 4}, {"height": 0}, {"width": -3}, {"scale": 0},
                 {"corners": np.where(np.arange(168).reshape(7, 8, 3) == 5, np.nan, corners)},
                 {"colors": colors + 1.5}, {"has_labels": 1}, {"zplane": float("inf")}):
        i, keep = inp_with(**over)
        assert L.ovm_host_scene_layout(C.byref(i), C.byref(out), g.ctypes.data, 16) == -1, over
    i, keep = inp_with()
    i.corners = None
    assert L.ovm_host_scene_layout(C.byref(i), C.byref(out), g.ctypes.data, 16) == -1

    # the device call: null / inconsistent arguments -> OVM_ERR_INVALID, a short workspace -> OVM_ERR_CAPACITY
    ws = C.c_int64()
    assert L.ovm_render_scene_workspace(C.byref(lay), 0, C.byref(ws)) == 0 and ws.value > 0
    assert L.ovm_render_scene_workspace(None, 0, C.byref(ws)) == -1
    assert L.ovm_render_scene_workspace(C.byref(lay), -1, C.byref(ws)) == -1
    fake = C.c_void_p(0x1000)                       # never dereferenced: every call below is refused first
    gp = grid.ctypes.data

    def render(lay_=lay, glyphs=None, nglyph=0, image=fake, pitch=480, front=fake, novel=fake, wsb=None, grid_p=gp):
        return L.ovm_render_scene(C.byref(lay_) if lay_ is not None else None, grid_p, glyphs, nglyph, image, pitch, front, 3 * 160,
                                  novel, 3 * 120, fake, ws.value if wsb is None else wsb, None)

    assert render(lay_=None) == -1
    assert render(nglyph=5) == -1                   # glyph bytes must match the layout's label sizes
    assert render(image=None) == -1
    assert render(pitch=100) == -1                  # row pitch shorter than a row
    assert render(novel=None) == -1
    assert render(grid_p=None) == -1
    assert render(wsb=ws.value - 1) == -5
    bad = lib.OvmSceneLayout.from_buffer_copy(lay)
    bad.view[0].order[0] = 99
    assert render(lay_=bad) == -1
    bad = lib.OvmSceneLayout.from_buffer_copy(lay)
    bad.mode = 1                                    # mode disagrees with the views drawn
    assert render(lay_=bad) == -1


def test_palette_and_glyphs():
    from ovmono3d_amd import vis
    cols = [vis.get_color(i) for i in range(64)]
    assert cols == [vis.get_color(i) for i in range(64)]
    assert all(0 <= c <= 255 for col in cols for c in col) and len(set(map(tuple, cols))) == 64
    m = vis.text_mask("chair 0.90", 0.5 * 480 / 500)
    assert m.dtype == np.uint8 and m.ndim == 2 and m.shape[1] > m.shape[0] > 4 and 0 < m.sum() < m.size
    assert vis.text_mask("", 1.0).shape == (0, 0)
    with pytest.raises(ValueError):
        vis.scene_layout(np.eye(3), 10, 10, np.zeros((1, 8, 3)), np.zeros((1, 3)), mode="2D_only")
