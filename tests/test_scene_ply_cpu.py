"""CPU: the rules of <name>_scene.ply without a device. The numpy restatement (tests/scene_ply_oracle.py) round-trips through its
own reader, one 2 x 2 case is worked by hand to literal bytes, the opengl frame is the camera frame with y and z negated and
nothing else changed, and the boxes-only file of ``ovmono3d_amd.vis.scene_ply`` - host work, no device - equals the restatement's.
Also: the library's refusals before any device work (a poisoned buffer stays untouched), the Python layer's argument checks before
the library is touched, the two command lines' new flags, and the package's imports staying clean."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_ply_oracle as po
from common import ROOT
from ovmono3d_amd import lib
from ovmono3d_amd import vis

F0, F1, F4, F5 = b"\x00\x00\x00\x00", b"\x00\x00\x80\x3f", b"\x00\x00\x80\x40", b"\x00\x00\xa0\x40"


def _i32(*v):
    return b"".join(bytes([x, 0, 0, 0]) for x in v)


def _hand_case():
    im = np.zeros((2, 2, 3), np.uint8)
    im[1, 1] = (10, 20, 30)                                               # B, G, R
    depth = np.array([[0.0, np.nan], [-2.0, 4.0]], np.float32)
    labels = np.array([[0, 0], [0, 0]], np.int32)
    K = np.array([[2.0, 0.0, 1.0], [0.0, 2.0, 1.0], [0.0, 0.0, 1.0]])
    corners = np.array([[[0, 0, 4], [1, 0, 4], [1, 1, 4], [0, 1, 4], [0, 0, 5], [1, 0, 5], [1, 1, 5], [0, 1, 5]]], np.float64)
    colors = np.array([[0.2, 0.4, 0.8]], np.float32)
    return im, K, depth, corners, colors, labels


def test_hand_worked_point_and_box():
    """Pixel (1, 1) is the only valid one: X = ((1 + 0.5) - 1) / 2 * 4 = 1, Y the same, Z = 4. The box colour (0.2, 0.4, 0.8) as float32
    is a little above each decimal, so c * 255 * 1.25 = 63.750000950, 127.500001900 and 255.0000038 -> min 255: edge colour B, G, R =
    (64, 128, 255). The pixel's B, G, R = (10, 20, 30) has label 0 and is tinted (10 + 64 + 1) >> 1 = 37, (20 + 128 + 1) >> 1 = 74,
    (30 + 255 + 1) >> 1 = 143; the record is x, y, z, then red, green, blue = 143, 74, 37. The box follows with P = 1 in front of it."""
    im, K, depth, corners, colors, labels = _hand_case()
    data, P = po.scene_ply(im, K, depth, corners, colors, labels)
    head = (b"ply\nformat binary_little_endian 1.0\ncomment ovmono3d_amd scene, frame camera, metres\nelement vertex 9\n"
            b"property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            b"element face 12\nproperty list uchar int vertex_indices\nelement edge 12\nproperty int vertex1\nproperty int vertex2\nend_header\n")
    point = F1 + F1 + F4 + bytes([143, 74, 37])
    rgb = bytes([255, 128, 64])
    verts = b"".join(x + y + z + rgb for x, y, z in ((F0, F0, F4), (F1, F0, F4), (F1, F1, F4), (F0, F1, F4),
                                                     (F0, F0, F5), (F1, F0, F5), (F1, F1, F5), (F0, F1, F5)))
    faces = b"".join(b"\x03" + _i32(*t) for t in ((1, 2, 3), (3, 4, 1), (2, 6, 7), (7, 3, 2), (5, 1, 4), (4, 8, 5), (6, 5, 8), (8, 7, 6),
                                                  (5, 6, 2), (2, 1, 5), (4, 3, 7), (7, 8, 4)))
    edges = b"".join(_i32(*e) for e in ((1, 2), (2, 3), (3, 4), (4, 1), (2, 6), (6, 7), (7, 3), (5, 6), (5, 8), (7, 8), (1, 5), (4, 8)))
    assert P == 1 and data == head + point + verts + faces + edges
    assert len(point) == 15 and len(verts) == 120 and len(faces) == 156 and len(edges) == 96
    # without the label map the point keeps the image's colour
    plain, _ = po.scene_ply(im, K, depth, corners, colors)
    assert plain[len(head):len(head) + 15] == F1 + F1 + F4 + bytes([30, 20, 10]) and plain[len(head) + 15:] == data[len(head) + 15:]


@pytest.mark.parametrize("H,W,n,stride", [(3, 5, 0, 1), (7, 4, 1, 1), (45, 91, 3, 2), (64, 65, 2, 3)])
def test_the_oracles_file_round_trips_through_its_reader(H, W, n, stride):
    s = po.scene(H, W, seed=H + n, bad=0.3, n=n)
    data, P = po.scene_ply(s["im"], s["K"], s["depth"], s["corners"], s["colors"], s["labels"], stride=stride, max_depth=7.0)
    keep = po.valid_mask(s["depth"], stride, 7.0)
    off_grid = keep.copy()
    off_grid[::stride, ::stride] = False
    assert P == int(keep.sum()) and 0 < P < keep.size and not off_grid.any()
    r = po.read_ply(data)
    xyz, rgb = po.point_records(s["im"], s["K"], s["depth"], s["labels"], po.edge_u8(s["colors"]), stride, 7.0)
    assert r["frame"] == "camera" and len(r["xyz"]) == P + 8 * n and len(r["faces"]) == 12 * n and len(r["edges"]) == 12 * n
    assert np.array_equal(r["xyz"][:P], xyz) and np.array_equal(r["rgb"][:P], rgb)
    assert np.array_equal(r["xyz"][P:], s["corners"].reshape(-1, 3).astype(np.float32))
    assert np.array_equal(r["rgb"][P:], np.repeat(po.edge_u8(s["colors"])[:, ::-1], 8, 0))
    for b in range(n):
        assert np.array_equal(r["faces"][12 * b:12 * b + 12] - (P + 8 * b), np.asarray(po.TRIS))
        assert np.array_equal(r["edges"][12 * b:12 * b + 12] - (P + 8 * b), np.asarray(po.EDGES))
    # the bulk packing of the points is the struct packing
    assert data[len(po.header(P, n, "camera")):][:15 * P] == po.pack_vertices(xyz, rgb)
    # every pixel the rules drop is dropped: non-finite, zero, negative, beyond max_depth (<= keeps the bound itself)
    d = s["depth"]
    with np.errstate(invalid="ignore"):
        assert not keep[~np.isfinite(d) | (d <= 0) | (d > np.float32(7.0))].any()
    some = float(d[np.isfinite(d) & (d > 0)][0])
    assert po.valid_mask(d, 1, some)[d == np.float32(some)].all()


def test_opengl_is_camera_with_y_and_z_negated_and_nothing_else():
    s = po.scene(9, 14, seed=4, bad=0.2, n=2)
    cam = po.read_ply(po.scene_ply(s["im"], s["K"], s["depth"], s["corners"], s["colors"], s["labels"])[0])
    gl = po.read_ply(po.scene_ply(s["im"], s["K"], s["depth"], s["corners"], s["colors"], s["labels"], frame="opengl")[0])
    assert (cam["frame"], gl["frame"]) == ("camera", "opengl")
    assert np.array_equal(gl["xyz"].view(np.uint32), (cam["xyz"] * np.float32([1, -1, -1])).view(np.uint32))
    assert np.array_equal(gl["xyz"][:, 0].view(np.uint32), cam["xyz"][:, 0].view(np.uint32)) and (gl["xyz"][:, 2] < 0).any()
    for k in ("rgb", "faces", "edges"):
        assert np.array_equal(gl[k], cam[k])
    assert po.header(5, 2, "camera").replace(b"frame camera", b"frame opengl") == po.header(5, 2, "opengl")


@pytest.mark.parametrize("frame", ["camera", "opengl"])
@pytest.mark.parametrize("n", [0, 1, 3])
def test_boxes_only_file_is_host_work_and_equals_the_oracle(n, frame):
    s = po.scene(6, 7, seed=11 + n, n=n)
    got = vis.scene_ply(s["im"], s["K"], corners=s["corners"], colors=s["colors"], frame=frame)
    want, P = po.scene_ply(s["im"], s["K"], None, s["corners"], s["colors"], frame=frame)
    assert P == 0 and isinstance(got, bytes) and got == want
    assert len(po.read_ply(got)["xyz"]) == 8 * n
    # the hand-worked box through the package
    im, K, depth, corners, colors, labels = _hand_case()
    assert vis.scene_ply(im, K, corners=corners, colors=colors) == po.scene_ply(im, K, None, corners, colors)[0]


def test_write_scene_ply_writes_the_bytes(tmp_path):
    s = po.scene(4, 4, seed=2, n=2)
    size = vis.write_scene_ply(tmp_path / "a_scene.ply", s["im"], s["K"], corners=s["corners"], colors=s["colors"])
    assert (tmp_path / "a_scene.ply").read_bytes() == vis.scene_ply(s["im"], s["K"], corners=s["corners"], colors=s["colors"]) and size == os.path.getsize(tmp_path / "a_scene.ply")


def test_library_refusals_without_a_device():
    L = lib.load()
    INV, CAP = lib.OVM_ERR_INVALID, lib.OVM_ERR_CAPACITY
    n = C.c_int64(-7)
    assert L.ovm_scene_ply_points_workspace(768, 1024, 1, 3, C.byref(n)) == 0 and n.value >= 384 * 4 + 385 * 8 + 12
    assert L.ovm_scene_ply_points_workspace(46340, 46340, 16, 1024, C.byref(n)) == 0                      # H * W just below 2^31
    for bad in ((0, 4, 1, 0), (4, 0, 1, 0), (4, 4, 0, 0), (4, 4, 17, 0), (4, 4, 1, -1), (4, 4, 1, lib.OVM_SCENE_MAX_BOXES + 1), (65536, 32768, 1, 0)):
        n.value = -7
        assert L.ovm_scene_ply_points_workspace(*bad, C.byref(n)) == INV and n.value == -7, bad
    assert L.ovm_scene_ply_points_workspace(4, 4, 1, 0, None) == INV
    assert L.ovm_scene_ply_points_workspace(4, 6, 1, 2, C.byref(n)) == 0
    buf = (C.c_uint8 * 8192)(*([0xA5] * 8192))
    p = C.addressof(buf)
    p += -p % 16
    K = (C.c_double * 9)(2.0, 0.0, 1.0, 0.0, 2.0, 1.0, 0.0, 0.0, 1.0)
    tint = (C.c_uint8 * 8)()
    ok = dict(image=p, ip=18, depth=p, dp=24, labels=p, lp=24, tint=C.addressof(tint), n=2, H=4, W=6, K=C.addressof(K), stride=1, md=0.0, flip=0,
              out=p, ob=4 * 6 * 15, count=p, ws=p, wb=int(n.value))

    def call(**kw):
        a = dict(ok, **kw)
        return L.ovm_scene_ply_points(a["image"], a["ip"], a["depth"], a["dp"], a["labels"], a["lp"], a["tint"], a["n"], a["H"], a["W"], a["K"],
                                      a["stride"], a["md"], a["flip"], a["out"], a["ob"], a["count"], a["ws"], a["wb"], None)
    for kw in (dict(image=None), dict(depth=None), dict(K=None), dict(out=None), dict(count=None), dict(ws=None), dict(H=0), dict(W=0),
               dict(H=65536, W=32768, ip=3 * 32768, dp=4 * 32768, lp=4 * 32768), dict(stride=0), dict(stride=17), dict(n=-1),
               dict(n=lib.OVM_SCENE_MAX_BOXES + 1), dict(ip=17), dict(dp=20), dict(dp=26), dict(lp=20), dict(lp=26), dict(tint=None),
               dict(tint=None, n=0), dict(flip=2), dict(md=float("nan")), dict(ws=p + 4), dict(count=p + 4)):
        assert call(**kw) == INV, kw
    badK = (C.c_double * 9)(0.0, 0.0, 1.0, 0.0, 2.0, 1.0, 0.0, 0.0, 1.0)
    assert call(K=C.addressof(badK)) == INV
    assert call(ob=4 * 6 * 15 - 1) == CAP and call(wb=int(n.value) - 1) == CAP
    assert call(stride=4, ob=1 * 2 * 15 - 1) == CAP                       # ceil(4 / 4) * ceil(6 / 4) records
    assert bytes(buf) == b"\xA5" * 8192                                  # nothing was written


def test_argument_checks_come_before_the_library(monkeypatch):
    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(lib, "load", touched)
    s = po.scene(4, 5, seed=1, n=1)
    im, K, d, lab = s["im"], s["K"], s["depth"], s["labels"]
    box = dict(corners=s["corners"], colors=s["colors"])
    bad = [dict(im=torch.from_numpy(im)), dict(depth=torch.from_numpy(d)), dict(depth=d, point_labels=torch.from_numpy(lab)),
           dict(im=im.astype(np.float32)), dict(im=im[:, :, :2]), dict(im=im[0]), dict(depth=d.astype(np.float64)), dict(depth=d[:3]), dict(depth=d[None]),
           dict(depth=d, point_labels=lab.astype(np.int64)), dict(depth=d, point_labels=lab[:, :4]), dict(point_labels=lab), dict(depth=[[1.0]]),
           dict(depth=d, stride=0), dict(depth=d, stride=17), dict(stride=0), dict(stride=2.0), dict(stride=True), dict(frame="world"), dict(depth=d, frame="OpenGL"),
           dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=float("nan")), dict(max_depth=float("inf")), dict(max_depth=1e-50), dict(K=np.zeros((3, 3))), dict(K=np.ones(4)),
           dict(corners=np.zeros((1, 8, 2))), dict(corners=np.full((1, 8, 3), np.nan)), dict(colors=None), dict(colors=np.zeros((2, 3))),
           dict(corners=np.zeros((lib.OVM_SCENE_MAX_BOXES + 1, 8, 3)), colors=np.zeros((lib.OVM_SCENE_MAX_BOXES + 1, 3)))]
    for kw in bad:
        a = dict(dict(im=im, K=K, **box), **kw)
        with pytest.raises(ValueError):
            vis.scene_ply(a.pop("im"), a.pop("K"), **a)
    assert vis.scene_ply(im, K, **box)                                   # boxes only: host work, the library stays untouched


def test_command_lines_know_the_new_flags():
    for script in ("demo_geo.py", "demo.py"):
        path = os.path.join(ROOT, "demo", script)
        r = subprocess.run([sys.executable, path, "--help"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and all(f in r.stdout for f in ("--scene-ply", "--no-scene-ply", "--ply-stride", "--ply-max-depth", "--ply-frame")), script
        base = [sys.executable, path, "--input-folder", "x", "--labels-file", "y", "--scene-ply"]
        for flag, value in (("--ply-frame", "x"), ("--ply-stride", "0"), ("--ply-stride", "17"), ("--ply-max-depth", "-1"), ("--ply-max-depth", "nan")):
            r = subprocess.run(base + [flag, value], capture_output=True, text=True, timeout=300)
            assert r.returncode == 2 and flag in r.stderr, (script, flag, value, r.stderr[-500:])


def test_the_package_imports_stay_clean():
    code = ("import sys; import ovmono3d_amd.vis, ovmono3d_amd.vis.ply, ovmono3d_amd.masks, ovmono3d_amd.geo; "
            "bad = [m for m in ('transformers', 'open3d', 'plyfile') if m in sys.modules]; assert not bad, bad; "
            "assert callable(ovmono3d_amd.vis.scene_ply) and callable(ovmono3d_amd.vis.write_scene_ply); print('ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
