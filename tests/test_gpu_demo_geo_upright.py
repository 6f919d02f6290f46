"""GPU: demo/demo_geo.py with MODEL.AMD.GEO_UPRIGHT. Off, the key changes nothing: the same files with the same bytes as a run that
never names it, and no new file. On, <name>_ground.json is the restatement's plane (tests/ground_oracle.py), the records are
geo.lift_boxes' in the fitted frame and carry height_above_ground; an image with no floor in view is lifted level, says so, and its
<name>_dets.json is the off run's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import ground_oracle as O
import sam_oracle as so
from common import ROOT

pytestmark = pytest.mark.gpu

CONFIG = os.path.join(ROOT, "configs", "OVMono3D_dinov2_SFP.yaml")
CASES = {"room": "demo_room", "wall": "demo_wall"}                  # both 120 x 160, one K


def _box(name):
    s = O.case(CASES[name])["scene"]
    if name == "wall":
        return [30.0, 20.0, 60.0, 50.0]
    ys, xs = np.nonzero(s["surface"] == O.CUBOID)
    return [float(xs.min()), float(ys.min()), float(xs.max() + 1 - xs.min()), float(ys.max() + 1 - ys.min())]


def _setup(tmp_path):
    inp, maps = tmp_path / "in", tmp_path / "maps"
    inp.mkdir()
    maps.mkdir()
    for k, (name, case) in enumerate(CASES.items()):
        s = O.case(case)["scene"]
        Image.fromarray(so.test_image(*s["depth"].shape, seed=40 + k)).save(inp / (name + ".jpg"), quality=92)
        np.savez(maps / (name + ".npz"), depth=s["depth"])
    (tmp_path / "labels.json").write_text(json.dumps({n: ["box"] for n in CASES}))
    (tmp_path / "boxes.json").write_text(json.dumps({n: [{"bbox": _box(n), "category_id": 0, "score": 0.9}] for n in CASES}))
    return inp, maps


def _demo(tmp_path, inp, maps, out, *opts):
    K = O.case("demo_room")["scene"]["K"]
    cmd = [sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), "--config-file", CONFIG, "--input-folder", str(inp), "--labels-file",
           str(tmp_path / "labels.json"), "--boxes-file", str(tmp_path / "boxes.json"), "--depth", "files", "--depth-dir", str(maps), "--mask", "box",
           "--focal-length", repr(float(K[0, 0])), "--principal-point", repr(float(K[0, 2])), repr(float(K[1, 2])), *opts, "OUTPUT_DIR", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return r


def test_upright_off_on_and_without_a_floor(device, tmp_path):
    from ovmono3d_amd.geo import ground_plane, lift_boxes
    inp, maps = _setup(tmp_path)
    never, off, on = tmp_path / "never", tmp_path / "off", tmp_path / "on"
    _demo(tmp_path, inp, maps, never)
    _demo(tmp_path, inp, maps, off, "MODEL.AMD.GEO_UPRIGHT", "False")
    _demo(tmp_path, inp, maps, on, "MODEL.AMD.GEO_UPRIGHT", "True")
    files = sorted(os.listdir(never))
    assert files == sorted(os.listdir(off)) == ["room_combine.jpg", "room_dets.json", "wall_combine.jpg", "wall_dets.json"]
    for f in files:
        assert (never / f).read_bytes() == (off / f).read_bytes(), f
    assert sorted(os.listdir(on)) == sorted(files + ["room_ground.json", "wall_ground.json"])

    # the room: the restatement's plane, in the camera's frame
    ref, s = O.reference("demo_room"), O.case("demo_room")["scene"]
    g = json.loads((on / "room_ground.json").read_text())
    assert set(g) == {"status", "upright", "normal", "offset", "n_points", "n_inliers", "share"}
    assert (g["status"], g["upright"], g["n_points"], g["n_inliers"]) == ("ok", True, ref["n_points"], ref["n_inliers"])
    assert np.abs(np.array(g["normal"]) - ref["normal"] * [1.0, -1.0, -1.0]).max() <= 1e-9 and abs(g["offset"] - ref["offset"]) <= 1e-9
    assert g["share"] == ref["n_inliers"] / ref["n_points"]
    assert np.degrees(np.arccos(min(1.0, float(np.array(g["normal"]) @ (s["normal"] * [1.0, -1.0, -1.0]))))) <= 0.5 and abs(g["offset"] - s["offset"]) <= 0.01
    depth = torch.from_numpy(s["depth"]).to(device)
    x, y, w, h = _box("room")
    want = lift_boxes(depth, s["K"], boxes_xyxy=np.array([[x, y, x + w, y + h]]), frame=ground_plane(depth, s["K"]))[0]
    d_on = json.loads((on / "room_dets.json").read_text())["detections"]
    d_off = json.loads((off / "room_dets.json").read_text())["detections"]
    assert len(d_on) == len(d_off) == 1 and set(d_on[0]) == set(d_off[0]) | {"height_above_ground"}
    assert d_on[0]["bbox3D"] == json.loads(json.dumps(list(want["center_cam"]) + list(want["dimensions"]))) and d_on[0]["pose"] == want["pose"]
    assert d_on[0]["corners3D"] == json.loads(json.dumps(want["bbox3D"])) and d_on[0]["height_above_ground"] == want["height_above_ground"]
    assert d_on[0]["bbox2D"] == d_off[0]["bbox2D"] and d_on[0]["pose"] != d_off[0]["pose"]
    up = np.array(g["normal"])
    assert np.linalg.norm(np.cross(np.array(d_on[0]["pose"])[:, 1], up)) <= 1e-9      # upright on: the box's vertical axis is the floor's normal
    assert np.linalg.norm(np.cross(np.array(d_off[0]["pose"])[:, 1], up)) > 0.3       # level: it leans with the camera's 20 degrees

    # the wall: no floor in view
    g = json.loads((on / "wall_ground.json").read_text())
    assert (g["status"], g["upright"], g["normal"], g["offset"], g["n_inliers"], g["share"]) == ("no plane", False, None, None, 0, 0.0)
    assert g["n_points"] == O.reference("demo_wall")["n_points"]
    assert (on / "wall_dets.json").read_bytes() == (off / "wall_dets.json").read_bytes()
    assert len(json.loads((on / "wall_dets.json").read_text())["detections"]) == 1
