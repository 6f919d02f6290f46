"""GPU: demo/demo_geo.py --points-file (clicks instead of the detector) and --sam-refine write what their parts give in-process: every
field of <name>_dets.json is geo.lift_boxes' on the masks predict_prompts returns for the same clicks (exact after the JSON round
trip), the 2D box the entry's own or mask_boxes' of its mask; --sam-refine 1 is the in-process two-pass result and --sam-refine 0 the
run without the flag, byte for byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import sam_oracle as so
from common import ROOT

pytestmark = pytest.mark.gpu

H, W = 96, 128
NAME = "img000"
CONFIG = os.path.join(ROOT, "configs", "OVMono3D_dinov2_SFP.yaml")
# two one-click prompts, one two-click prompt, one click inside a box, one below the threshold: three groups of one shape each
ENTRIES = [{"points": [[40.0, 30.0]], "labels": [1], "category_name": "chair"},
           {"points": [[90.0, 60.0], [20.0, 80.0]], "labels": [1, 0], "category_name": "table", "score": 0.8},
           {"points": [[64.0, 48.0]], "labels": [1], "category_name": "lamp", "bbox": [30.0, 20.0, 70.0, 50.0], "score": 0.6},
           {"points": [[100.0, 20.0]], "labels": [1], "category_name": "chair"},
           {"points": [[10.0, 10.0]], "labels": [1], "category_name": "sofa", "score": 0.1}]


def _depth():
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    return (2.0 + 0.004 * xx + 0.002 * yy + 0.15 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.float32)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
    root = tmp_path_factory.mktemp("geo_points")
    inp, maps = root / "in", root / "maps"
    inp.mkdir()
    (maps / "test").mkdir(parents=True)
    Image.fromarray(so.test_image(H, W, seed=20)).save(inp / (NAME + ".jpg"), quality=92)
    np.savez(maps / "test" / (NAME + ".npz"), depth=_depth())
    (root / "points.json").write_text(json.dumps({NAME: ENTRIES}))
    (root / "boxes.json").write_text(json.dumps({NAME: [{"bbox": [10.0, 8.0, 64.0, 57.0], "category_id": 0, "score": 0.9},
                                                        {"bbox": [38.5, 24.0, 76.0, 67.0], "category_id": 1, "score": 0.6}]}))
    (root / "labels.json").write_text(json.dumps({NAME: ["chair", "table"]}))
    weights = str(root / "sam_vit_test.pth")
    torch.save(synth_sam_predictor_state_dict("vit_test", seed=3, image_size=128), weights)
    return root, inp, maps, weights


def _run(scene, out, *extra):
    root, inp, maps, weights = scene
    cmd = [sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), "--config-file", CONFIG, "--input-folder", str(inp), "--depth", "files",
           "--depth-dir", str(maps), "--mask", "sam", "--sam-weights", weights, "--sam-arch", "vit_test", "--sam-image-size", "128", *extra,
           "OUTPUT_DIR", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return r


def _K():
    f = 4.0 * H / 2
    return np.array([[f, 0.0, W / 2], [0.0, f, H / 2], [0.0, 0.0, 1.0]])


def _image(scene, device):
    from ovmono3d_amd.data.gpu_jpeg import read_image_device
    return read_image_device(os.path.join(str(scene[1]), NAME + ".jpg"), "BGR", device)


def _records(entries, boxes, lifted):
    out = []
    for e, b, box in zip(entries, boxes, lifted):
        if box is None:
            continue
        out.append({"category": e["category_name"], "score": float(e.get("score", 1.0)), "bbox3D": list(box["center_cam"]) + list(box["dimensions"]),
                    "pose": box["pose"], "corners3D": box["bbox3D"], "center_2D": list(box["center_2D"]), "bbox2D": [float(v) for v in b]})
    return json.loads(json.dumps(out))


def _in_process(scene, device, refine):
    """predict_prompts + mask_boxes + lift_boxes, one call per (point count, has box) group, no helper of the tool."""
    from ovmono3d_amd.geo import lift_boxes
    from ovmono3d_amd.sam import build_sam
    pred = build_sam("vit_test", scene[3], device=device, image_size=128)
    pred.set_image(_image(scene, device), image_format="BGR")
    cand = [e for e in ENTRIES if not e.get("score", 1.0) < 0.30]
    planes, boxes = [None] * len(cand), [None] * len(cand)
    for shape in sorted({(len(e["points"]), "bbox" in e) for e in cand}):
        idx = [i for i, e in enumerate(cand) if (len(e["points"]), "bbox" in e) == shape]
        kw = dict(point_coords=np.asarray([cand[i]["points"] for i in idx], np.float32), point_labels=np.asarray([cand[i]["labels"] for i in idx], np.int32))
        if shape[1]:
            kw["boxes"] = np.asarray([[b[0], b[1], b[0] + b[2], b[1] + b[3]] for b in (cand[i]["bbox"] for i in idx)], np.float64)
        masks, _, low = pred.predict_prompts(mask_index=2, want_lowres=refine > 0, **kw)
        for _ in range(refine):
            masks, _, low = pred.predict_prompts(mask_inputs=low[:, 2].contiguous(), mask_index=2, want_lowres=True, **kw)
        tight = pred.mask_boxes(masks)[0].cpu().numpy().astype(np.float64)
        for k, i in enumerate(idx):
            planes[i], boxes[i] = masks[k], (kw["boxes"][k] if shape[1] else tight[k])
    lifted = lift_boxes(torch.from_numpy(_depth()).to(device), _K(), boxes_xyxy=np.asarray(boxes), masks=planes)
    return _records(cand, boxes, lifted), cand


@pytest.mark.parametrize("refine", [0, 1])
def test_points_file_records_equal_the_in_process_parts(device, scene, tmp_path, refine):
    out = tmp_path / "out"
    r = _run(scene, out, "--points-file", str(scene[0] / "points.json"), *(["--sam-refine", str(refine)] if refine else []))
    expected, cand = _in_process(scene, device, refine)
    d = json.loads((out / f"{NAME}_dets.json").read_text())
    assert d["K"] == _K().tolist()
    assert len(expected) >= 3 and d["detections"] == expected
    assert [x["category"] for x in d["detections"]][:2] == ["chair", "table"] and d["detections"][2]["bbox2D"] == [30.0, 20.0, 100.0, 70.0]
    assert f"File: {NAME} with {len(expected)} dets ({len(cand)} boxes at or above the threshold, {len(cand) - len(expected)} not lifted)" in r.stdout
    assert np.asarray(Image.open(out / f"{NAME}_combine.jpg")).shape == (H, W + H, 3)
    if refine:                                                                  # the refinement pass changes the masks: it ran
        assert expected != _in_process(scene, device, 0)[0]


def test_sam_refine_on_boxes_and_refine_0_is_the_run_without_the_flag(device, scene, tmp_path):
    from ovmono3d_amd.geo import lift_boxes
    from ovmono3d_amd.sam import build_sam
    root = scene[0]
    base = ["--boxes-file", str(root / "boxes.json"), "--labels-file", str(root / "labels.json")]
    _run(scene, tmp_path / "plain", *base)
    _run(scene, tmp_path / "zero", *base, "--sam-refine", "0")
    _run(scene, tmp_path / "one", *base, "--sam-refine", "1")
    plain = (tmp_path / "plain" / f"{NAME}_dets.json").read_bytes()
    assert plain == (tmp_path / "zero" / f"{NAME}_dets.json").read_bytes()
    # in-process: the box pass, then the same boxes with plane 2's logits as mask input
    from ovmono3d_amd.geo import sources as geo
    pred = build_sam("vit_test", scene[3], device=device, image_size=128)
    inst = json.loads((root / "boxes.json").read_text())[NAME]
    boxes = np.asarray([geo.xywh_to_xyxy(b["bbox"]) for b in inst], np.float64)
    pred.set_image(_image(scene, device), image_format="BGR")
    _, _, low = pred.predict_prompts(boxes=boxes, mask_index=2, want_lowres=True)
    masks = pred.predict_prompts(boxes=boxes, mask_inputs=low[:, 2].contiguous(), mask_index=2)[0]
    assert torch.equal(masks, geo.sam_masks(pred, None, None, H, W, boxes, bgr=_image(scene, device), refine=1))
    assert torch.equal(pred.predict_boxes(boxes), geo.sam_masks(pred, None, None, H, W, boxes, bgr=_image(scene, device), refine=0))
    lifted = lift_boxes(torch.from_numpy(_depth()).to(device), _K(), boxes_xyxy=boxes, masks=list(masks))
    cats = ["chair", "table"]
    expected = _records([{"category_name": cats[b["category_id"]], "score": b["score"]} for b in inst], boxes, lifted)
    one = json.loads((tmp_path / "one" / f"{NAME}_dets.json").read_text())
    assert len(expected) >= 1 and one["detections"] == expected
    assert one != json.loads(plain)
