"""GPU: --scene-ply of the two command lines. A GEO run writes <name>_scene.ply whose 8 n box vertices are float32 of the corners in
<name>_dets.json ("corners3D", pred_bbox3D order) in the colours of <name>_combine.jpg, and whose P points are the numpy restatement
(tests/scene_ply_oracle.py) on the run's depth map, the image as the run decoded it and the label map of the kept instances' masks;
<name>_dets.json and <name>_combine.jpg keep their bytes. demo.py --depth none --scene-ply writes a boxes-only file. Same synthetic
tiny weights and sizes as tests/test_gpu_demo_geo_masks.py and tests/test_gpu_demo_points.py."""
import json
import os

import numpy as np
import pytest
import torch

import mask_overlay_oracle as oo
import scene_ply_oracle as po
from ovmono3d_amd.vis import scene_ply  # noqa: F401  (the feature under test: without it this module does not load)
from test_gpu_demo_geo_everything import H, NAME, W, _K, _depth
from test_gpu_demo_geo_masks import _demo, generator, scene  # noqa: F401  (fixtures)
from test_gpu_demo_points import _demo as _lift_demo, _setup as _lift_setup

pytestmark = pytest.mark.gpu


def _box_colors(kept):
    from ovmono3d_amd import vis
    return np.asarray([[c / 255.0 for c in vis.get_color(i)] for i in kept], np.float32).reshape(-1, 3)


def test_geo_run_writes_points_and_boxes(device, scene, generator, tmp_path):  # noqa: F811
    from ovmono3d_amd.data.gpu_jpeg import read_image_device
    from ovmono3d_amd.geo import lift_boxes
    flagged = _demo(scene, tmp_path / "flagged", ["--scene-ply"])
    plain = _demo(scene, tmp_path / "plain", ["--no-scene-ply"])
    assert sorted(plain) == [f"{NAME}_combine.jpg", f"{NAME}_dets.json"]
    assert sorted(flagged) == [f"{NAME}_combine.jpg", f"{NAME}_dets.json", f"{NAME}_scene.ply"]
    for f in plain:
        assert flagged[f] == plain[f], f
    dets = json.loads(flagged[f"{NAME}_dets.json"])["detections"]
    n = len(dets)
    assert n >= 2
    # the in-process masks of the kept instances, as tests/test_gpu_demo_geo_masks.py finds them
    im = read_image_device(os.path.join(str(scene[1]), NAME + ".jpg"), "BGR", device)
    res = generator.generate_device(im, "BGR")
    lifted = lift_boxes(torch.from_numpy(_depth()).to(device), _K(), boxes_xyxy=res["boxes"].cpu().numpy().astype(np.float64), masks=list(res["masks"]))
    kept = [k for k, box in enumerate(lifted) if box is not None]
    assert len(kept) == n
    labels = oo.labels(res["masks"][kept].cpu().numpy()).astype(np.int32)
    r = po.read_ply(flagged[f"{NAME}_scene.ply"])
    xyz, rgb = po.point_records(im.cpu().numpy(), _K(), _depth(), labels, po.edge_u8(_box_colors(kept)))
    P = len(xyz)
    assert P == H * W and r["frame"] == "camera" and len(r["xyz"]) == P + 8 * n and len(r["faces"]) == len(r["edges"]) == 12 * n
    corners = np.asarray([d["corners3D"] for d in dets], np.float64).reshape(8 * n, 3).astype(np.float32)
    assert np.array_equal(r["xyz"][P:].view(np.uint32), corners.view(np.uint32))
    assert np.array_equal(r["rgb"][P:], np.repeat(po.edge_u8(_box_colors(kept))[:, ::-1], 8, 0))
    assert np.array_equal(r["xyz"][:P].view(np.uint32), xyz.view(np.uint32)) and np.array_equal(r["rgb"][:P], rgb)
    assert (labels >= 0).any() and not np.array_equal(rgb, im.cpu().numpy().reshape(-1, 3)[:, ::-1])      # some points are tinted
    # the whole file, and the flags: stride, bound and frame reach the library
    assert flagged[f"{NAME}_scene.ply"] == po.scene_ply(im.cpu().numpy(), _K(), _depth(), [d["corners3D"] for d in dets], _box_colors(kept), labels)[0]
    tuned = _demo(scene, tmp_path / "tuned", ["--scene-ply", "--ply-stride", "3", "--ply-max-depth", "2.4", "--ply-frame", "opengl"])
    want, P3 = po.scene_ply(im.cpu().numpy(), _K(), _depth(), [d["corners3D"] for d in dets], _box_colors(kept), labels, stride=3, max_depth=2.4,
                            frame="opengl")
    assert tuned[f"{NAME}_scene.ply"] == want and 0 < P3 < -(-H // 3) * -(-W // 3)
    assert tuned[f"{NAME}_dets.json"] == plain[f"{NAME}_dets.json"] and tuned[f"{NAME}_combine.jpg"] == plain[f"{NAME}_combine.jpg"]


def test_lift_demo_without_depth_writes_a_boxes_only_file(device, tmp_path):
    inp, _ = _lift_setup(tmp_path)
    for out, flags in ((tmp_path / "plain", []), (tmp_path / "ply", ["--depth", "none", "--scene-ply"])):
        r = _lift_demo(tmp_path, inp, out, *flags)
        assert r.returncode == 0, r.stderr[-2000:]
    a, b = tmp_path / "plain", tmp_path / "ply"
    assert sorted(os.listdir(a)) == ["img000_combine.jpg", "img000_dets.json"]
    assert sorted(os.listdir(b)) == ["img000_combine.jpg", "img000_dets.json", "img000_scene.ply"]
    for f in os.listdir(a):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f
    dets = json.loads((b / "img000_dets.json").read_text())["detections"]
    assert len(dets) == 2
    r = po.read_ply((b / "img000_scene.ply").read_bytes())
    corners = np.asarray([d["corners3D"] for d in dets], np.float64).reshape(16, 3).astype(np.float32)
    assert len(r["xyz"]) == 16 and np.array_equal(r["xyz"].view(np.uint32), corners.view(np.uint32))
    assert np.array_equal(r["faces"][:12], np.asarray(po.TRIS)) and np.array_equal(r["edges"][12:], np.asarray(po.EDGES) + 8)
    assert np.array_equal(r["rgb"], np.repeat(po.edge_u8(_box_colors([0, 1]))[:, ::-1], 8, 0))
