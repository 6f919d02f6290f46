"""GPU: masks as outputs of the GEO route. demo/demo_geo.py --segmentation rle --show-masks writes each record's mask as a COCO RLE
that decodes to the in-process mask of that instance and <name>_masks.jpg, the restated overlay as Pillow encodes it; without the
flags the files are what they were. SamAutomaticMaskGenerator.generate_rle is generate() after decoding, and tools/ovmono3d_geo.py
gives the same 3D records from --mask-format rle files as from the .npz files of the same masks. Same synthetic tiny weights and
sizes as tests/test_gpu_demo_geo_everything.py."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import mask_overlay_oracle as oo
import mask_rle_oracle as mo
import sam_oracle as so
from common import ROOT
from ovmono3d_amd import masks as M
from test_gpu_demo_geo_everything import CONFIG, GRID, H, NAME, NMS, PRED_IOU, STABILITY, W, _K, _depth
from test_gpu_geo_sam import _dataset, _tool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
    root = tmp_path_factory.mktemp("geo_masks")
    inp, maps = root / "in", root / "maps"
    inp.mkdir()
    (maps / "test").mkdir(parents=True)
    Image.fromarray(so.test_image(H, W, seed=20)).save(inp / (NAME + ".jpg"), quality=92)
    np.savez(maps / "test" / (NAME + ".npz"), depth=_depth())
    weights = str(root / "sam_vit_test.pth")
    torch.save(synth_sam_predictor_state_dict("vit_test", seed=3, image_size=128), weights)
    return root, inp, maps, weights


def _demo(scene, out, extra):
    root, inp, maps, weights = scene
    cmd = [sys.executable, os.path.join(ROOT, "demo", "demo_geo.py"), "--config-file", CONFIG, "--input-folder", str(inp), "--depth", "files",
           "--depth-dir", str(maps), "--mask", "sam", "--sam-weights", weights, "--sam-arch", "vit_test", "--sam-image-size", "128", "--everything",
           "--points-per-side", str(GRID), "--pred-iou-thresh", str(PRED_IOU), "--stability-score-thresh", str(STABILITY), "--box-nms-thresh", str(NMS),
           *extra, "OUTPUT_DIR", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    return {f: (out / f).read_bytes() for f in sorted(os.listdir(out))}


@pytest.fixture(scope="module")
def generator(device, scene):
    from ovmono3d_amd.sam import SamAutomaticMaskGenerator, build_sam
    pred = build_sam("vit_test", scene[3], device=device, image_size=128)
    return SamAutomaticMaskGenerator(pred, points_per_side=GRID, pred_iou_thresh=PRED_IOU, stability_score_thresh=STABILITY, box_nms_thresh=NMS)


def test_demo_geo_writes_rle_records_and_the_mask_picture(device, scene, generator, tmp_path):
    from ovmono3d_amd import vis
    from ovmono3d_amd.data.gpu_jpeg import read_image_device
    from ovmono3d_amd.geo import lift_boxes
    flagged = _demo(scene, tmp_path / "flagged", ["--segmentation", "rle", "--show-masks"])
    plain = _demo(scene, tmp_path / "plain", [])
    again = _demo(scene, tmp_path / "again", [])
    # without the flags: the same files with the same bytes, run after run, and no mask picture
    assert plain == again and sorted(plain) == [f"{NAME}_combine.jpg", f"{NAME}_dets.json"]
    assert sorted(flagged) == [f"{NAME}_combine.jpg", f"{NAME}_dets.json", f"{NAME}_masks.jpg"]
    assert flagged[f"{NAME}_combine.jpg"] == plain[f"{NAME}_combine.jpg"]
    d, p = json.loads(flagged[f"{NAME}_dets.json"]), json.loads(plain[f"{NAME}_dets.json"])
    assert d["K"] == p["K"] and len(d["detections"]) == len(p["detections"]) >= 2
    assert [{k: v for k, v in r.items() if k != "segmentation"} for r in d["detections"]] == p["detections"]
    # the in-process masks of the kept instances
    im = read_image_device(os.path.join(str(scene[1]), NAME + ".jpg"), "BGR", device)
    res = generator.generate_device(im, "BGR")
    boxes = res["boxes"].cpu().numpy().astype(np.float64)
    lifted = lift_boxes(torch.from_numpy(_depth()).to(device), _K(), boxes_xyxy=boxes, masks=list(res["masks"]))
    kept = [k for k, box in enumerate(lifted) if box is not None]
    assert len(kept) == len(d["detections"])
    planes = res["masks"][kept]
    for r, plane in zip(d["detections"], planes.cpu().numpy()):
        seg = r["segmentation"]
        assert seg == mo.encode(plane) and isinstance(seg["counts"], str)
    assert torch.equal(M.decode_rle([r["segmentation"] for r in d["detections"]], device), planes.ne(0).to(torch.uint8))
    # the picture: the restated overlay (BGR, colours as for the boxes, alpha 0.5 -> 128), saved as Pillow saves its RGB at quality 95
    colors = np.asarray([vis.get_color(i) for i in kept], np.uint8)
    want = oo.overlay(im.cpu().numpy(), oo.labels(planes.cpu().numpy()), colors, 128)
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(want[:, :, ::-1])).save(buf, format="JPEG", quality=95)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(flagged[f"{NAME}_masks.jpg"]))), np.asarray(Image.open(buf)))
    assert not np.array_equal(want, im.cpu().numpy())


def test_generate_rle_equals_generate_after_decoding(device, scene, generator):
    from ovmono3d_amd.data.gpu_jpeg import read_image_device
    im = read_image_device(os.path.join(str(scene[1]), NAME + ".jpg"), "BGR", device)
    ref = generator.generate(im, "BGR")
    assert len(ref) >= 3
    for compressed in (True, False):
        got = generator.generate_rle(im, "BGR", compressed=compressed)
        assert len(got) == len(ref)
        for g, r in zip(got, ref):
            assert {k: v for k, v in g.items() if k != "segmentation"} == {k: v for k, v in r.items() if k != "segmentation"}
            assert g["segmentation"] == mo.encode(r["segmentation"].cpu().numpy(), compressed)
            assert M.rle_area(g["segmentation"]) == g["area"]
        dec = M.decode_rle([g["segmentation"] for g in got], device)
        assert torch.equal(dec.bool(), torch.stack([r["segmentation"] for r in ref]))


def test_tool_gives_the_same_records_from_rle_files_as_from_npz(device, tmp_path):
    p = _dataset(str(tmp_path))
    common = ["--oracle2d", p["oracle2d"], "--dataset", p["dataset"], "--depth-dir", p["depth"]]
    sam = ["--mask", "sam", "--sam-weights", p["weights"], "--sam-arch", "vit_test", "--sam-image-size", "128", "--image-root", p["images"]]
    npz, rle = str(tmp_path / "npz"), str(tmp_path / "rle")
    sa = _tool(common + sam + ["--dump-masks", npz, "--output", str(tmp_path / "a.json")])
    sb = _tool(common + sam + ["--dump-masks", rle, "--mask-format", "rle", "--output", str(tmp_path / "b.json")])
    assert sorted(os.listdir(rle)) == ["10.rle.json", "11.rle.json", "12.rle.json"] and sorted(os.listdir(npz)) == ["10.npz", "11.npz", "12.npz"]
    for iid in (10, 11, 12):                                             # the same masks in both forms
        z = np.load(os.path.join(npz, f"{iid}.npz"))
        with open(os.path.join(rle, f"{iid}.rle.json")) as f:
            j = json.load(f)
        assert j["index"] == [int(i) for i in z["index"]] and j["masks"] == [mo.encode(m) for m in z["masks"]]
    # a run that reads the RLE files (the run that reads the .npz files equals run a: tests/test_gpu_geo_sam.py)
    sc = _tool(common + ["--mask-dir", rle, "--output", str(tmp_path / "c.json")])
    assert sa == sb == sc and sa["lifted"] >= 3
    recs = [json.loads((tmp_path / f"{k}.json").read_text()) for k in "abc"]
    assert recs[0] == recs[1] == recs[2]
