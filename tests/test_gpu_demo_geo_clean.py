"""GPU: --min-mask-region-area on the GEO entry points. demo/demo_geo.py with --boxes-file and SAM masks lifts the planes that
masks.remove_small_regions(planes, N, "both") gives: every field of <name>_dets.json is geo.lift_boxes' on those planes (exact after
the JSON round trip) and the RLE segmentation decodes to them; without the flag it lifts the raw planes, as before. With --points-file
the click's plane is cleaned too and a click without a "bbox" gets the tight box of its cleaned mask.
tools/ovmono3d_geo.py cleans --mask-dir planes that carry specks and pinholes the same way, and --dump-masks writes the cleaned
planes. The cleaned planes are checked against tests/mask_cc_oracle.py."""
import json
import os

import numpy as np
import pytest
import torch

import mask_cc_oracle as O
from ovmono3d_amd import masks as M
from test_gpu_demo_geo import SIZES, _boxes, _cand_boxes, _depth, _expected, _K, _run, _setup, _tool
from test_gpu_geo_sam import SIZES as TOOL_SIZES
from test_gpu_geo_sam import _dataset
from test_gpu_geo_sam import _tool as _run_tool

pytestmark = pytest.mark.gpu

AREA = 64


def test_demo_geo_lifts_the_cleaned_planes(device, tmp_path):
    from ovmono3d_amd.geo import lift_boxes
    from ovmono3d_amd.sam import build_sam
    from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
    from ovmono3d_amd.geo import sources as tool
    inp, maps, names = _setup(tmp_path, n=1)
    weights = str(tmp_path / "sam_vit_test.pth")
    torch.save(synth_sam_predictor_state_dict("vit_test", seed=3, image_size=128), weights)
    common = ["--boxes-file", str(tmp_path / "boxes.json"), "--depth", "files", "--depth-dir", str(maps), "--mask", "sam", "--sam-weights", weights,
              "--sam-arch", "vit_test", "--sam-image-size", "128", "--segmentation", "rle"]
    _run(tmp_path, inp, tmp_path / "clean", *common, "--min-mask-region-area", str(AREA))
    _run(tmp_path, inp, tmp_path / "plain", *common)
    predictor = build_sam("vit_test", weights, device=device, image_size=128)
    H, W = SIZES[0]
    inst = _boxes(H, W)
    boxes = _cand_boxes(inst)
    raw = tool.sam_masks(predictor, str(inp), names[0] + ".jpg", H, W, boxes)
    cleaned, changed = M.remove_small_regions(raw, AREA, "both")
    want = [O.remove_small_regions(p, AREA, "both") for p in raw.cpu().numpy()]
    print(f"SAM planes: areas {raw.sum((1, 2)).tolist()}, changed at area {AREA}: {changed.tolist()}, pixels changed {(cleaned != raw.ne(0)).sum((1, 2)).tolist()}")
    assert changed.tolist() == [w[1] for w in want] and np.array_equal(cleaned.cpu().numpy(), np.stack([w[0] for w in want]))
    assert bool(changed.any()) and not torch.equal(cleaned, raw.ne(0).to(torch.uint8))          # the planes carry small regions: the flag matters
    depth = torch.from_numpy(_depth(H, W)).to(device)
    for folder, planes in (("clean", cleaned), ("plain", raw)):
        lifted = lift_boxes(depth, _K(0), boxes_xyxy=boxes, masks=list(planes))
        expected = _expected(inst, lifted)
        d = json.loads((tmp_path / folder / f"{names[0]}_dets.json").read_text())["detections"]
        assert len(expected) >= 1 and [{k: v for k, v in r.items() if k != "segmentation"} for r in d] == expected, folder
        kept = [k for k, box in enumerate(lifted) if box is not None]
        assert torch.equal(M.decode_rle([r["segmentation"] for r in d], device), planes[kept].ne(0).to(torch.uint8)), folder


def test_demo_geo_click_prompts_take_the_cleaned_mask_and_its_tight_box(device, tmp_path):
    """--points-file: the plane is cleaned before the lift, and an entry without a "bbox" gets the tight box of its cleaned mask."""
    from ovmono3d_amd.geo import lift_boxes
    from ovmono3d_amd.sam import build_sam
    from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
    from ovmono3d_amd.data.gpu_jpeg import read_image_device
    inp, maps, names = _setup(tmp_path, n=1)
    weights = str(tmp_path / "sam_vit_test.pth")
    torch.save(synth_sam_predictor_state_dict("vit_test", seed=3, image_size=128), weights)
    entries = [{"points": [[40.0, 30.0]], "labels": [1], "category_name": "chair"},
               {"points": [[64.0, 48.0]], "labels": [1], "category_name": "lamp", "bbox": [30.0, 20.0, 70.0, 50.0], "score": 0.6}]
    (tmp_path / "points.json").write_text(json.dumps({names[0]: entries}))
    _run(tmp_path, inp, tmp_path / "clean", "--points-file", str(tmp_path / "points.json"), "--depth", "files", "--depth-dir", str(maps), "--mask", "sam",
         "--sam-weights", weights, "--sam-arch", "vit_test", "--sam-image-size", "128", "--segmentation", "rle", "--min-mask-region-area", str(AREA))
    H, W = SIZES[0]
    pred = build_sam("vit_test", weights, device=device, image_size=128)
    pred.set_image(read_image_device(str(inp / (names[0] + ".jpg")), "BGR", device), image_format="BGR")
    raw0 = pred.predict_prompts(point_coords=np.asarray([entries[0]["points"]], np.float32), point_labels=np.asarray([entries[0]["labels"]], np.int32))[0]
    given = np.asarray([[30.0, 20.0, 100.0, 70.0]], np.float64)
    raw1 = pred.predict_prompts(point_coords=np.asarray([entries[1]["points"]], np.float32), point_labels=np.asarray([entries[1]["labels"]], np.int32),
                                boxes=given)[0]
    raw = torch.cat([raw0, raw1])
    cleaned, changed = M.remove_small_regions(raw, AREA, "both")
    want = np.stack([O.remove_small_regions(p, AREA, "both")[0] for p in raw.cpu().numpy()])
    assert np.array_equal(cleaned.cpu().numpy(), want)
    tight_raw, tight = pred.mask_boxes(raw)[0].cpu().numpy().astype(np.float64), pred.mask_boxes(cleaned)[0].cpu().numpy().astype(np.float64)
    print(f"click planes: changed {changed.tolist()}, tight box raw {tight_raw[0].tolist()} cleaned {tight[0].tolist()}")
    assert bool(changed[0]) and not torch.equal(cleaned[0], raw[0].ne(0).to(torch.uint8))         # the click's plane carries small regions
    boxes = np.stack([tight[0], given[0]])
    lifted = lift_boxes(torch.from_numpy(_depth(H, W)).to(device), _K(0), boxes_xyxy=boxes, masks=list(cleaned))
    expected = []
    for e, b, box in zip(entries, boxes, lifted):
        if box is not None:
            expected.append({"category": e["category_name"], "score": float(e.get("score", 1.0)), "bbox3D": list(box["center_cam"]) + list(box["dimensions"]),
                             "pose": box["pose"], "corners3D": box["bbox3D"], "center_2D": list(box["center_2D"]), "bbox2D": [float(v) for v in b]})
    d = json.loads((tmp_path / "clean" / f"{names[0]}_dets.json").read_text())["detections"]
    assert len(expected) >= 1 and [{k: v for k, v in r.items() if k != "segmentation"} for r in d] == json.loads(json.dumps(expected))
    assert lifted[0] is not None and d[0]["bbox2D"] == [float(v) for v in tight[0]]              # the cleaned mask's own box
    kept = [k for k, box in enumerate(lifted) if box is not None]
    assert torch.equal(M.decode_rle([r["segmentation"] for r in d], device), cleaned[kept])


def _speckled(H, W, seed):
    """A blob and its specks and pinholes, as uint8 0 / 1"""
    return O.blobs(H, W, n_blobs=2, specks=12, pinholes=12, seed=seed)


def test_tool_cleans_mask_dir_planes_and_dumps_them(device, tmp_path):
    tool = _tool("ovmono3d_geo")
    p = _dataset(str(tmp_path))
    given = tmp_path / "given"
    given.mkdir()
    planes = {}
    for k, (H, W) in enumerate(TOOL_SIZES):
        planes[10 + k] = np.stack([_speckled(H, W, 7 * k), _speckled(H, W, 7 * k + 1)])
        np.savez_compressed(given / f"{10 + k}.npz", masks=planes[10 + k], index=np.asarray([0, 1], np.int64))
    common = ["--oracle2d", p["oracle2d"], "--dataset", p["dataset"], "--depth-dir", p["depth"], "--mask-dir", str(given)]
    sa = _run_tool(common + ["--min-mask-region-area", str(AREA), "--dump-masks", str(tmp_path / "dump_clean"), "--output", str(tmp_path / "a.json")])
    sb = _run_tool(common + ["--dump-masks", str(tmp_path / "dump_plain"), "--output", str(tmp_path / "b.json")])
    assert sa["images"] == sb["images"] == 3 and sa["lifted"] >= 3
    with open(p["oracle2d"]) as f:
        oracle = json.load(f)
    with open(p["dataset"]) as f:
        images = {im["id"]: im for im in json.load(f)["images"]}
    with open(tmp_path / "a.json") as f:
        got = json.load(f)
    for rec, out in zip(oracle, got):
        iid = rec["image_id"]
        want = np.stack([O.remove_small_regions(m, AREA, "both")[0] for m in planes[iid]])
        assert not np.array_equal(want, planes[iid])                     # the specks were there
        z, zp = np.load(tmp_path / "dump_clean" / f"{iid}.npz"), np.load(tmp_path / "dump_plain" / f"{iid}.npz")
        assert np.array_equal(z["masks"], want) and list(z["index"]) == [0, 1] and np.array_equal(zp["masks"], planes[iid])
        cand = [ins for ins in rec["instances"] if not ins["score"] < 0.30]
        boxes = np.asarray([tool.xywh_to_xyxy(ins["bbox"]) for ins in cand], np.float64)
        im = images[iid]
        depth = tool.load_depth(p["depth"], im["file_path"], im["height"], im["width"])
        lifted = tool.lift_image(depth, np.asarray(rec["K"], np.float64), boxes, list(want), tool.GeoParams())
        expected = []
        for ins, box in zip(cand, lifted):
            if box is None:
                continue
            new = {k: v for k, v in ins.items() if k in tool.KEPT_KEYS}
            new["image_id"] = iid
            for k in ("bbox3D", "depth", "center_cam", "dimensions", "pose", "center_2D"):
                new[k] = box[k]
            expected.append(new)
        assert out["instances"] == json.loads(json.dumps(expected)), iid
