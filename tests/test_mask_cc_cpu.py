"""Connected components and the small-region clean-up without a device: the oracle's closed cases (tests/mask_cc_oracle.py), the
refusals of the two C calls, their workspace statements, and the keyword / flag on the Python surface."""
import ctypes as C
import importlib.util
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import mask_cc_oracle as O  # noqa: E402

from ovmono3d_amd import lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plane(rows):
    return np.array([[int(c == "#") for c in r] for r in rows], np.uint8)


# ------------------------------------------------------------------------------------------------ the oracle's closed cases
def test_two_diagonal_pixels_are_one_component_under_8_and_two_under_4():
    p = _plane(["#.",
                ".#"])
    lab8, n8 = O.label(p, 8)
    lab4, n4 = O.label(p, 4)
    assert n8 == 1 and lab8.tolist() == [[1, 0], [0, 1]]
    assert n4 == 2 and lab4.tolist() == [[1, 0], [0, 2]]                 # numbered in row-major order of the first pixel


def test_labels_are_numbered_by_first_pixel_in_row_major_order():
    p = _plane(["..#.#",
                "#.#.#",
                "#...#"])
    lab, n = O.label(p, 4)
    assert n == 3 and lab.tolist() == [[0, 0, 1, 0, 2], [3, 0, 1, 0, 2], [3, 0, 0, 0, 2]]
    for name, plane in O.edge_planes(9, 70).items():
        for conn in (4, 8):
            lab, n = O.label(plane, conn)
            firsts = [int(np.flatnonzero(lab.ravel() == k)[0]) for k in range(1, n + 1)]
            assert firsts == sorted(firsts), (name, conn)


def test_the_edge_planes_are_what_their_names_say():
    H, W = 12, 70
    e = O.edge_planes(H, W)
    assert O.label(e["checkerboard"], 8)[1] == 1 and O.label(e["checkerboard"], 4)[1] == H * W // 2
    assert O.label(e["serpentine"], 4)[1] == 1 and O.label(e["serpentine"], 8)[1] == 1
    assert e["serpentine"][1].sum() == 1 and e["serpentine"][3].sum() == 1 and e["serpentine"][1, W - 1] and e["serpentine"][3, 0]
    assert O.label(e["comb"], 4)[1] == 1 and O.label(e["comb"][:-1], 4)[1] == W // 2
    assert O.label(e["u"], 8)[1] == 1 and O.label(e["u"][:-1], 8)[1] == 2
    assert O.label(e["rings"], 8)[1] == 3 and O.label(e["rings"], 8, invert=True)[1] == 3
    assert O.label(e["empty"], 8)[1] == 0 and O.label(e["empty"], 8, invert=True)[1] == 1 and O.label(e["full"], 4)[1] == 1
    assert O.SHAPES[0] == (1, 1) and O.SHAPES[-1] == (1080, 1920)


def test_a_ring_has_one_hole():
    ring = _plane([".....",
                   ".###.",
                   ".#.#.",
                   ".###.",
                   "....."])
    assert O.label(ring, 8, invert=True)[1] == 2                         # the outer background and the hole
    out, changed = O.remove_small_regions(ring, 2, "holes")
    assert changed and out.sum() == 9 and out[2, 2] == 1 and out[0].sum() == 0
    out, changed = O.remove_small_regions(ring, 1, "holes")
    assert not changed and (out == ring).all()


def test_a_small_outer_background_is_filled_in_holes_mode():
    p = np.ones((4, 5), np.uint8)
    p[0, 0] = 0                                                          # the "outer background" is one pixel: a region like any other
    out, changed = O.remove_small_regions(p, 2, "holes")
    assert changed and out.all()


def test_area_equal_to_the_threshold_is_not_small():
    p = _plane(["##...",
                "##...",
                "....#"])
    out, changed = O.remove_small_regions(p, 4, "islands")               # areas 4 and 1: only the speck is below 4
    assert changed and out.tolist() == _plane(["##...", "##...", "....."]).tolist()
    out, changed = O.remove_small_regions(p[:2], 4, "islands")
    assert not changed and (out == p[:2]).all()
    out, changed = O.remove_small_regions(p[:2], 5, "islands")           # now small, and the only one: kept, but reported
    assert changed and (out == p[:2]).all()


def test_all_small_keeps_the_largest_and_a_tie_keeps_the_first():
    p = _plane(["#..##",
                ".....",
                "##..."])
    out, changed = O.remove_small_regions(p, 100, "islands")
    assert changed and out.tolist() == _plane(["...##", ".....", "....."]).tolist()       # areas 1, 2, 2: the first of the two
    p[2, 2] = 1
    out, changed = O.remove_small_regions(p, p.size + 1, "islands")      # "keep the largest component"
    assert changed and out.tolist() == _plane([".....", ".....", "###.."]).tolist()


def test_mode_both_when_only_the_island_step_changes_the_plane():
    p = _plane(["###....",
                "###....",
                "###...#"])
    holes, ch_h = O.remove_small_regions(p, 2, "holes")
    assert not ch_h and (holes == p).all()                               # the complement is one region of 11 pixels
    both, ch = O.remove_small_regions(p, 2, "both")
    isl, ch_i = O.remove_small_regions(p, 2, "islands")
    assert ch and ch_i and (both == isl).all() and both.sum() == 9 and both[2, 6] == 0
    # and when hole filling merges islands: the speck next to the ring's hole survives only through the filled hole
    q = _plane(["###....",
                "#.#....",
                "###...."])
    both, ch = O.remove_small_regions(q, 9, "both")
    assert ch and both.sum() == 9                                        # 8 pixels + the filled hole = 9: not small any more
    isl, _ = O.remove_small_regions(q, 9, "islands")
    assert isl.sum() == 8                                                # alone it is all-small: kept as the largest


def test_postprocess_drops_a_changed_duplicate_and_keeps_unchanged_first():
    H, W = 12, 16
    a = np.zeros((H, W), np.uint8)
    a[2:8, 3:10] = 1
    b = a.copy()
    b[10, 14] = 1                                                        # the same mask with a speck
    c = np.zeros((H, W), np.uint8)
    c[9:12, 0:3] = 1
    masks = np.stack([b, a, c])
    boxes, areas = zip(*(O.tight_box(m) for m in masks))
    out = dict(masks=masks, boxes=np.stack(boxes), areas=np.asarray(areas, np.int32), scores=np.array([0.99, 0.9, 0.95], np.float32),
               stability=np.array([0.97, 0.96, 0.98], np.float32), points=np.zeros((3, 2), np.float32), index=np.array([0, 4, 8]))
    res = O.postprocess_small_regions(out, 2, 0.7)
    assert res["index"].tolist() == [4, 8] and not res["changed"].any()  # b became box-equal to a: dropped, the score of a is lower or not
    assert (res["masks"][0] == a).all() and res["scores"].tolist() == [np.float32(0.9), np.float32(0.95)]
    res = O.postprocess_small_regions(dict(out, masks=masks[[0, 2]], boxes=out["boxes"][[0, 2]], areas=out["areas"][[0, 2]], scores=out["scores"][[0, 2]],
                                           stability=out["stability"][[0, 2]], points=out["points"][[0, 2]], index=out["index"][[0, 2]]), 2, 0.7)
    assert res["index"].tolist() == [8, 0] and res["changed"].tolist() == [False, True]           # unchanged masks first
    assert (res["masks"][1] == a).all() and res["boxes"][1].tolist() == [3, 2, 10, 8] and res["areas"][1] == 42


# ------------------------------------------------------------------------------------------------ the C calls without a device
def test_library_refusals_without_a_device():
    L = lib.load()
    INV, CAP = lib.OVM_ERR_INVALID, lib.OVM_ERR_CAPACITY
    for ws_fn in (L.ovm_mask_cc_label_workspace, L.ovm_mask_remove_small_regions_workspace):
        n = C.c_int64(-7)
        for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 65536, 32768), (-1, 4, 4)):
            assert ws_fn(*bad, C.byref(n)) == INV and n.value == -7, bad
        assert ws_fn(1, 4, 4, None) == INV
        assert ws_fn(1, 46340, 46340, C.byref(n)) == 0                   # H * W just below 2^31
        assert ws_fn(2 ** 26, 4, 4, C.byref(n)) == CAP                   # more workgroups than a launch takes
        prev = 0
        for k in (1, 2, 3, 7, 64, 65):                                   # monotone in n
            assert ws_fn(k, 1080, 1920, C.byref(n)) == 0 and n.value > prev and n.value % 16 == 0
            prev = n.value
    assert L.ovm_mask_cc_label_workspace(1, 1080, 1920, C.byref(n)) == 0 and 4 * 1080 * 1920 <= n.value < 20 * 2 ** 20
    assert L.ovm_mask_remove_small_regions_workspace(1, 1080, 1920, C.byref(n)) == 0 and 8 * 1080 * 1920 <= n.value < 20 * 2 ** 20

    buf = (C.c_uint8 * 8192)(*([0xA5] * 8192))
    p = C.addressof(buf)
    p += -p % 16
    q = p + 4096                                                         # a second region: the output must not overlap the input
    ok = dict(masks=p, ps=16, pitch=4, n=1, H=4, W=4, conn=8, invert=0, labels=q, lps=16, lp=4, counts=q, status=q, ws=q, ws_bytes=4096)

    def label(**kw):
        a = dict(ok, **kw)
        return L.ovm_mask_cc_label(a["masks"], a["ps"], a["pitch"], a["n"], a["H"], a["W"], a["conn"], a["invert"], a["labels"], a["lps"], a["lp"],
                                   a["counts"], a["status"], a["ws"], a["ws_bytes"], None)
    for kw in (dict(masks=None), dict(labels=None), dict(counts=None), dict(status=None), dict(ws=None), dict(n=0), dict(H=0), dict(W=0),
               dict(H=65536, W=32768, pitch=32768, lp=32768), dict(pitch=3), dict(lp=3), dict(conn=6), dict(conn=0), dict(ws=q + 4)):
        assert label(**kw) == INV, kw
    assert label(ws_bytes=64) == CAP and label(n=2 ** 26) == CAP

    okr = dict(masks=p, ps=16, pitch=4, n=1, H=4, W=4, min_area=2, mode=3, out=q, ops=16, opitch=4, changed=q + 1024, status=q + 2048, ws=q + 3072,
               ws_bytes=1024)

    def clean(**kw):
        a = dict(okr, **kw)
        return L.ovm_mask_remove_small_regions(a["masks"], a["ps"], a["pitch"], a["n"], a["H"], a["W"], a["min_area"], a["mode"], a["out"], a["ops"],
                                               a["opitch"], a["changed"], a["status"], a["ws"], a["ws_bytes"], None)
    for kw in (dict(masks=None), dict(out=None), dict(changed=None), dict(status=None), dict(ws=None), dict(n=0), dict(H=0), dict(W=0),
               dict(H=65536, W=32768, pitch=32768, opitch=32768), dict(pitch=3), dict(opitch=3), dict(min_area=0), dict(min_area=-5), dict(mode=0),
               dict(mode=4), dict(ws=q + 3072 + 8), dict(out=p), dict(out=p + 15), dict(masks=p + 4096 + 12), dict(n=2, out=p + 16)):
        assert clean(**kw) == INV, kw
    assert clean(ws_bytes=64) == CAP and clean(n=2 ** 26, ps=0) == CAP
    # output planes that overlap each other: every one of them is written, and mode 3 reads them back
    for kw in (dict(n=2, ps=0, ops=0), dict(n=2, ps=0, ops=15), dict(n=2, ps=0, ops=-15), dict(n=3, ps=0, opitch=6, ops=21), dict(n=2 ** 26, ps=0, ops=0)):
        assert clean(**kw) == INV, kw
    assert clean(n=2, ps=0, ops=16, ws_bytes=64) == CAP and clean(n=1, ops=0, ws_bytes=64) == CAP          # side by side; one plane has no stride
    assert bytes(buf) == b"\xA5" * 8192                                  # nothing was written


def test_python_layer_refuses_host_tensors_and_bad_arguments():
    from ovmono3d_amd import masks as M
    assert M.MAX_CC_WORKSPACE == 1 << 30
    with pytest.raises(RuntimeError, match="HIP device only"):
        M.connected_components(torch.zeros((1, 4, 4), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device only"):
        M.remove_small_regions(torch.zeros((1, 4, 4), dtype=torch.uint8), 2, "both")
    assert "keep the largest" in M.remove_small_regions.__doc__
    assert inspect.signature(M.connected_components).parameters["connectivity"].default == 8
    assert inspect.signature(M.connected_components).parameters["invert"].default is False


# ------------------------------------------------------------------------------------------------ the Python surface
def test_generate_signatures_carry_the_keyword_and_the_constructor_keeps_refusing():
    from ovmono3d_amd.sam import SamAutomaticMaskGenerator as G
    for name in ("generate_device", "generate", "generate_rle"):
        par = inspect.signature(getattr(G, name)).parameters
        assert "min_mask_region_area" in par and par["min_mask_region_area"].default == 0, name
    assert list(inspect.signature(G.postprocess_small_regions).parameters) == ["out", "min_area", "nms_thresh"]
    assert isinstance(inspect.getattr_static(G, "postprocess_small_regions"), staticmethod)
    with pytest.raises(ValueError, match="min_mask_region_area"):
        G(object(), min_mask_region_area=10)


def _tool(folder, name):
    spec = importlib.util.spec_from_file_location("cc_tool_" + name, os.path.join(ROOT, folder, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_both_argument_parsers_know_the_flag():
    demo = _tool("demo", "demo_geo").argument_parser()
    a = demo.parse_args(["--input-folder", "x"])
    assert a.min_mask_region_area == 0
    assert demo.parse_args(["--input-folder", "x", "--min-mask-region-area", "25"]).min_mask_region_area == 25
    geo = _tool("tools", "ovmono3d_geo")
    base = ["--oracle2d", "o", "--dataset", "d", "--output", "out.json", "--depth-dir", "z"]
    assert geo.argument_parser().parse_args(base).min_mask_region_area == 0
    a = geo.argument_parser().parse_args(base + ["--min-mask-region-area", "9", "--mask", "box"])           # accepted with --mask box
    assert a.min_mask_region_area == 9 and geo.check_args(a) is a
    with pytest.raises(SystemExit):
        geo.check_args(geo.argument_parser().parse_args(base + ["--min-mask-region-area", "-1"]))
    from ovmono3d_amd.geo.sources import clean_planes
    assert clean_planes(None, 5) is None and clean_planes([], 5) == []
    planes = [np.zeros((2, 2), np.uint8)]
    assert clean_planes(planes, 0) is planes                         # off: what was given, untouched, no device
