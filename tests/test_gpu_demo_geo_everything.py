"""GPU: demo/demo_geo.py --everything (Segment Anything's automatic mask generator instead of names, boxes or clicks) writes what its
parts give in-process: every field of <name>_dets.json is geo.lift_boxes' on generate_device's masks (exact after the JSON round
trip), the 2D box the tight box of the mask, the score the predicted IoU, the category "object"; --threshold is not applied."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from ovmono3d_amd.sam import SamAutomaticMaskGenerator  # noqa: F401  (the feature under test: without it this module does not load)
import sam_oracle as so
from common import ROOT

pytestmark = pytest.mark.gpu

H, W = 96, 128
NAME = "img000"
CONFIG = os.path.join(ROOT, "configs", "OVMono3D_dinov2_SFP.yaml")
# random weights give near-whole-image masks: thresholds that keep several of them
GRID, PRED_IOU, STABILITY, NMS = 3, 0.25, 0.0, 1.0


def _depth():
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    return (2.0 + 0.004 * xx + 0.002 * yy + 0.15 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.float32)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
    root = tmp_path_factory.mktemp("geo_everything")
    inp, maps = root / "in", root / "maps"
    inp.mkdir()
    (maps / "test").mkdir(parents=True)
    Image.fromarray(so.test_image(H, W, seed=20)).save(inp / (NAME + ".jpg"), quality=92)
    np.savez(maps / "test" / (NAME + ".npz"), depth=_depth())
    weights = str(root / "sam_vit_test.pth")
    torch.save(synth_sam_predictor_state_dict("vit_test", seed=3, image_size=128), weights)
    return root, inp, maps, weights


def _K():
    f = 4.0 * H / 2
    return np.array([[f, 0.0, W / 2], [0.0, f, H / 2], [0.0, 0.0, 1.0]])


def test_everything_records_equal_the_in_process_parts(device, scene, tmp_path):
    from ovmono3d_amd.data.gpu_jpeg import read_image_device
    from ovmono3d_amd.geo import lift_boxes
    from ovmono3d_amd.sam import SamAutomaticMaskGenerator, build_sam
    root, inp, maps, weights = scene
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), "--config-file", CONFIG, "--input-folder", str(inp), "--depth", "files",
           "--depth-dir", str(maps), "--mask", "sam", "--sam-weights", weights, "--sam-arch", "vit_test", "--sam-image-size", "128", "--everything",
           "--points-per-side", str(GRID), "--pred-iou-thresh", str(PRED_IOU), "--stability-score-thresh", str(STABILITY), "--box-nms-thresh", str(NMS),
           "--threshold", "5.0", "OUTPUT_DIR", str(out)]                      # no labels, boxes or clicks; a threshold no score reaches
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    pred = build_sam("vit_test", weights, device=device, image_size=128)
    gen = SamAutomaticMaskGenerator(pred, points_per_side=GRID, pred_iou_thresh=PRED_IOU, stability_score_thresh=STABILITY, box_nms_thresh=NMS)
    res = gen.generate_device(read_image_device(os.path.join(str(inp), NAME + ".jpg"), "BGR", device), "BGR")
    boxes = res["boxes"].cpu().numpy().astype(np.float64)
    scores = res["scores"].cpu().tolist()
    lifted = lift_boxes(torch.from_numpy(_depth()).to(device), _K(), boxes_xyxy=boxes, masks=list(res["masks"]))
    expected = []
    for b, sc, box in zip(boxes, scores, lifted):
        if box is None:
            continue
        expected.append({"category": "object", "score": float(sc), "bbox3D": list(box["center_cam"]) + list(box["dimensions"]), "pose": box["pose"],
                         "corners3D": box["bbox3D"], "center_2D": list(box["center_2D"]), "bbox2D": [float(v) for v in b]})
    expected = json.loads(json.dumps(expected))
    d = json.loads((out / f"{NAME}_dets.json").read_text())
    assert d["K"] == _K().tolist()
    assert len(boxes) >= 3 and len(expected) >= 2 and d["detections"] == expected
    assert f"File: {NAME} with {len(expected)} dets ({len(boxes)} boxes at or above the threshold, {len(boxes) - len(expected)} not lifted)" in r.stdout
    assert np.asarray(Image.open(out / f"{NAME}_combine.jpg")).shape == (H, W + H, 3)
