"""GPU: demo/demo_geo.py - OVMono3D-GEO on a folder of images - writes what its parts give in-process: every field of
<name>_dets.json is geo.lift_boxes' on the same depth, K, boxes and masks (exact after the JSON round trip), the 2D boxes of the
detector route are build_detector + gdino_postprocess', the picture is demo.py's, and tools/ovmono3d_geo.py on the same boxes gives the same
records."""
import importlib.util
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

SIZES = ((96, 128), (112, 96))                                      # (H, W): the second image gets the first one's focal length
CATS = ["chair", "table"]
CONFIG = os.path.join(ROOT, "configs", "OVMono3D_dinov2_SFP.yaml")


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _depth(H, W):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    return (2.0 + 0.004 * xx + 0.002 * yy + 0.15 * np.sin(xx / 9.0) * np.cos(yy / 7.0)).astype(np.float32)


def _boxes(H, W):
    return [{"bbox": [10.0, 8.0, 0.5 * W, 0.6 * H], "category_id": 0, "score": 0.9},
            {"bbox": [0.3 * W + 0.25, 0.25 * H, 0.6 * W, 0.7 * H], "category_id": 1, "score": 0.6},
            {"bbox": [5.0, 5.0, 20.0, 20.0], "category_id": 0, "score": 0.1},               # below the threshold
            {"bbox": [-60.0, -60.0, 20.0, 20.0], "category_id": 1, "score": 0.7}]           # outside the image: not lifted


def _setup(tmp_path, n=len(SIZES)):
    inp, maps = tmp_path / "in", tmp_path / "maps"
    inp.mkdir()
    (maps / "test").mkdir(parents=True)
    names = []
    for k, (H, W) in enumerate(SIZES[:n]):
        name = f"img{k:03d}"
        Image.fromarray(so.test_image(H, W, seed=20 + k)).save(inp / (name + ".jpg"), quality=92)
        np.savez(maps / "test" / (name + ".npz"), depth=_depth(H, W))
        names.append(name)
    (tmp_path / "labels.json").write_text(json.dumps({n_: CATS for n_ in names}))
    (tmp_path / "boxes.json").write_text(json.dumps({n_: _boxes(*hw) for n_, hw in zip(names, SIZES)}))
    return inp, maps, names


def _run(tmp_path, inp, out, *extra, opts=()):
    cmd = [sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), "--config-file", CONFIG, "--input-folder", str(inp),
           "--labels-file", str(tmp_path / "labels.json"), *extra, *opts, "OUTPUT_DIR", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return r


def _K(k):
    f = 4.0 * SIZES[0][0] / 2                                       # demo.py's convention: the first image's focal length sticks
    H, W = SIZES[k]
    return np.array([[f, 0.0, W / 2], [0.0, f, H / 2], [0.0, 0.0, 1.0]])


def _expected(inst, lifted, threshold=0.30):
    cand = [b for b in inst if not b["score"] < threshold]
    out = []
    for b, box in zip(cand, lifted):
        if box is None:
            continue
        x, y, w, h = b["bbox"]
        out.append({"category": CATS[b["category_id"]], "score": b["score"], "bbox3D": list(box["center_cam"]) + list(box["dimensions"]),
                    "pose": box["pose"], "corners3D": box["bbox3D"], "center_2D": list(box["center_2D"]), "bbox2D": [x, y, x + w, y + h]})
    return json.loads(json.dumps(out))


def _cand_boxes(inst, threshold=0.30):
    return np.asarray([[b["bbox"][0], b["bbox"][1], b["bbox"][0] + b["bbox"][2], b["bbox"][1] + b["bbox"][3]]
                       for b in inst if not b["score"] < threshold], np.float64)


def _check_outputs(out, names, expected, stdout):
    for k, n in enumerate(names):
        H, W = SIZES[k]
        d = json.loads((out / f"{n}_dets.json").read_text())
        assert d["K"] == _K(k).tolist()
        assert len(expected[k]) >= 1 and d["detections"] == expected[k], n
        assert np.asarray(Image.open(out / f"{n}_combine.jpg")).shape == (H, W + H, 3)
        assert f"File: {n} with {len(expected[k])} dets (3 boxes at or above the threshold, {3 - len(expected[k])} not lifted)" in stdout


def test_boxes_file_box_masks(device, tmp_path):
    from ovmono3d_amd.geo import lift_boxes
    inp, maps, names = _setup(tmp_path)
    out = tmp_path / "out"
    r = _run(tmp_path, inp, out, "--boxes-file", str(tmp_path / "boxes.json"), "--depth", "files", "--depth-dir", str(maps), "--mask", "box")
    expected = []
    for k, n in enumerate(names):
        inst = _boxes(*SIZES[k])
        lifted = lift_boxes(torch.from_numpy(_depth(*SIZES[k])).to(device), _K(k), boxes_xyxy=_cand_boxes(inst), masks=None)
        assert lifted[2] is None and lifted[0] is not None and lifted[1] is not None   # the box outside the image is left out and counted
        expected.append(_expected(inst, lifted))
    _check_outputs(out, names, expected, r.stdout)
    # the point cloud is on by default and changes the picture only
    plain = tmp_path / "plain"
    _run(tmp_path, inp, plain, "--boxes-file", str(tmp_path / "boxes.json"), "--depth", "files", "--depth-dir", str(maps), "--mask", "box", "--no-show-points")
    for k, n in enumerate(names):
        W = SIZES[k][1]
        assert (plain / f"{n}_dets.json").read_bytes() == (out / f"{n}_dets.json").read_bytes()
        a, b = np.asarray(Image.open(out / f"{n}_combine.jpg")).astype(int), np.asarray(Image.open(plain / f"{n}_combine.jpg")).astype(int)
        assert (np.abs(a[:, W:] - b[:, W:]).max(-1) > 16).mean() > 0.02    # the boxes are lifted from this cloud: it is in the frame


def test_boxes_file_sam_masks(device, tmp_path):
    from ovmono3d_amd.geo import lift_boxes
    from ovmono3d_amd.geo.sources import sam_masks
    from ovmono3d_amd.sam import build_sam
    from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
    inp, maps, names = _setup(tmp_path)
    weights = str(tmp_path / "sam_vit_test.pth")
    torch.save(synth_sam_predictor_state_dict("vit_test", seed=3, image_size=128), weights)
    out = tmp_path / "out"
    r = _run(tmp_path, inp, out, "--boxes-file", str(tmp_path / "boxes.json"), "--depth", "files", "--depth-dir", str(maps), "--mask", "sam",
             "--sam-weights", weights, "--sam-arch", "vit_test", "--sam-image-size", "128")
    predictor = build_sam("vit_test", weights, device=device, image_size=128)
    expected = []
    for k, n in enumerate(names):
        H, W = SIZES[k]
        inst = _boxes(H, W)
        boxes = _cand_boxes(inst)
        planes = sam_masks(predictor, str(inp), n + ".jpg", H, W, boxes)
        lifted = lift_boxes(torch.from_numpy(_depth(H, W)).to(device), _K(k), boxes_xyxy=boxes, masks=list(planes))
        expected.append(_expected(inst, lifted))
    _check_outputs(out, names, expected, r.stdout)


def test_detector_route(device, tmp_path):
    from ovmono3d_amd.data.feeding import ResizeShortestEdge, read_image
    from ovmono3d_amd.defaults import make_cfg
    from ovmono3d_amd.gdino.detector import build_detector
    from ovmono3d_amd.geo import lift_boxes
    from ovmono3d_amd.modeling.roi_heads import gdino_glue as oracle2d
    inp, maps, names = _setup(tmp_path, n=1)
    opts = ["MODEL.AMD.GDINO_WEIGHTS", "synthetic://gdino?arch=swint&seed=1", "INPUT.MIN_SIZE_TEST", "210", "INPUT.MAX_SIZE_TEST", "280"]
    cfg = make_cfg(CONFIG, opts)
    det = build_detector(cfg, device)
    H, W = SIZES[0]
    net = ResizeShortestEdge(cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)(read_image(str(inp / "img000.jpg"), cfg.INPUT.FORMAT))
    r = det(torch.as_tensor(np.ascontiguousarray(net.transpose(2, 0, 1))).to(device), oracle2d.build_caption(CATS)[0])
    boxes, scores, cls = oracle2d.gdino_postprocess(r["pred_logits"], r["pred_boxes"], oracle2d.phrase_spans(r["input_ids"], r["phrase_ids"]),
                                                    net.shape[:2], box_threshold=0.001, nms_threshold=0.5)
    scores = scores.cpu().tolist()
    assert len(scores) >= 2
    threshold = float(np.float32(sorted(scores)[len(scores) // 2]))  # the median score: a cut that keeps some boxes and drops others
    b = boxes.cpu().numpy() * np.array([W / net.shape[1], H / net.shape[0]] * 2, np.float32)
    want = [[float(v) for v in row] for row, s in zip(b, scores) if not s < threshold]
    want_cat = [CATS[c] for c, s in zip(cls.cpu().tolist(), scores) if not s < threshold]
    assert 0 < len(want) < len(scores) or min(scores) == max(scores)
    out = tmp_path / "out"
    run = _run(tmp_path, inp, out, "--depth", "files", "--depth-dir", str(maps), "--mask", "box", "--threshold", repr(threshold), opts=opts)
    d = json.loads((out / "img000_dets.json").read_text())["detections"]
    assert f"({len(want)} boxes at or above the threshold" in run.stdout
    # the lift leaves out what it has no answer for
    lifted = lift_boxes(torch.from_numpy(_depth(H, W)).to(device), _K(0), boxes_xyxy=np.asarray(want, np.float64), masks=None)
    keep = [i for i, box in enumerate(lifted) if box is not None]
    assert len(keep) > 0
    assert [x["bbox2D"] for x in d] == [want[i] for i in keep]
    assert [x["category"] for x in d] == [want_cat[i] for i in keep]
    assert [x["corners3D"] for x in d] == json.loads(json.dumps([lifted[i]["bbox3D"] for i in keep]))


@pytest.mark.parametrize("mask", ["box", "sam"])
def test_tool_and_demo_are_the_same_pipeline(device, tmp_path, mask):
    """tools/ovmono3d_geo.py and demo/demo_geo.py --boxes-file on the same images, depth files, boxes and K: every lifted instance's
    record fields are equal, value for value, and the two leave out the same instances."""
    inp, maps, names = _setup(tmp_path)
    f, px, py = 110.0, 60.5, 50.25                                   # one K for both images: the demo's flags hold for the whole folder
    Kmat = [[f, 0.0, px], [0.0, f, py], [0.0, 0.0, 1.0]]
    images = [{"id": 10 + k, "file_path": n + ".jpg", "height": H, "width": W, "K": Kmat, "dataset_id": 0} for k, (n, (H, W)) in enumerate(zip(names, SIZES))]
    oracle = [{"image_id": 10 + k, "K": Kmat, "instances": _boxes(*hw)} for k, hw in enumerate(SIZES)]
    (tmp_path / "synth.json").write_text(json.dumps({"info": {"name": "synth"}, "images": images, "annotations": [], "categories": []}))
    (tmp_path / "oracle_2d.json").write_text(json.dumps(oracle))
    sam = []
    if mask == "sam":
        from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
        weights = str(tmp_path / "sam_vit_test.pth")
        torch.save(synth_sam_predictor_state_dict("vit_test", seed=3, image_size=128), weights)
        sam = ["--sam-weights", weights, "--sam-arch", "vit_test", "--sam-image-size", "128"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ovmono3d_geo.py"), "--oracle2d", str(tmp_path / "oracle_2d.json"), "--dataset",
                        str(tmp_path / "synth.json"), "--depth", "files", "--depth-dir", str(maps), "--image-root", str(inp), "--mask", mask, *sam,
                        "--output", str(tmp_path / "tool.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    out = tmp_path / "out"
    run = _run(tmp_path, inp, out, "--boxes-file", str(tmp_path / "boxes.json"), "--depth", "files", "--depth-dir", str(maps), "--mask", mask, *sam,
               "--focal-length", repr(f), "--principal-point", repr(px), repr(py))
    tool = json.loads((tmp_path / "tool.json").read_text())
    n_lifted = 0
    for rec, n in zip(tool, names):
        d = json.loads((out / f"{n}_dets.json").read_text())
        assert d["K"] == Kmat
        ins, dets = rec["instances"], d["detections"]
        # the same instances are lifted, in the same order: the tool keeps the xywh box it was given, the demo writes it as xyxy
        assert [[b[0], b[1], b[0] + b[2], b[1] + b[3]] for b in (i["bbox"] for i in ins)] == [x["bbox2D"] for x in dets], n
        assert len(ins) >= 1
        for i, x in zip(ins, dets):
            assert i["center_cam"] == x["bbox3D"][:3] and i["dimensions"] == x["bbox3D"][3:], n
            assert i["pose"] == x["pose"] and i["bbox3D"] == x["corners3D"] and i["center_2D"] == x["center_2D"], n
        assert f"File: {n} with {len(ins)} dets (3 boxes at or above the threshold, {3 - len(ins)} not lifted)" in run.stdout
        n_lifted += len(ins)
    assert stats["lifted"] == n_lifted and stats["skipped"] == 3 * len(names) - n_lifted
    if mask == "box":
        assert stats["skipped"] == len(names)                        # the box outside the image, in both


def test_threshold_above_every_score_writes_boxes_jpg(device, tmp_path):
    inp, maps, names = _setup(tmp_path, n=1)
    out = tmp_path / "out"
    _run(tmp_path, inp, out, "--boxes-file", str(tmp_path / "boxes.json"), "--depth", "files", "--depth-dir", str(maps), "--mask", "box",
         "--threshold", "0.95")
    assert json.loads((out / "img000_dets.json").read_text())["detections"] == []
    assert not (out / "img000_combine.jpg").exists()
    assert np.asarray(Image.open(out / "img000_boxes.jpg")).shape == (*SIZES[0], 3)
