"""OVMono3D-GEO with SAM masks end to end: tools/ovmono3d_geo.py --mask sam on a synthetic dataset, and the predictor's call shapes."""
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

SIZES = ((96, 128), (120, 90), (128, 128))          # (H, W) of the three images


def _dataset(root):
    """Three JPEG images of different shapes, a smooth metric depth map each, three boxes per image (one below the score threshold),
    synthetic vit_test SAM weights for a 128-pixel encoder."""
    from ovmono3d_amd.util.synth_sam_weights import synth_sam_predictor_state_dict
    os.makedirs(os.path.join(root, "images", "synth"))
    os.makedirs(os.path.join(root, "depth", "test"))
    images, oracle = [], []
    for k, (H, W) in enumerate(SIZES):
        iid = 10 + k
        Image.fromarray(so.test_image(H, W, seed=20 + k)).save(os.path.join(root, "images", "synth", f"img_{iid}.jpg"), quality=92)
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        depth = 2.0 + 0.004 * xx + 0.002 * yy + 0.15 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
        np.savez(os.path.join(root, "depth", "test", f"img_{iid}.npz"), depth=depth.astype(np.float32))
        Kmat = [[110.0, 0.0, W / 2.0], [0.0, 110.0, H / 2.0], [0.0, 0.0, 1.0]]
        images.append({"id": iid, "file_path": f"synth/img_{iid}.jpg", "height": H, "width": W, "K": Kmat, "dataset_id": 0})
        inst = [{"bbox": [10.0, 8.0, 0.5 * W, 0.6 * H], "category_id": 0, "score": 0.9, "category_name": "a"},
                {"bbox": [0.3 * W, 0.25 * H, 0.6 * W, 0.7 * H], "category_id": 1, "score": 0.6, "category_name": "b"},
                {"bbox": [5.0, 5.0, 20.0, 20.0], "category_id": 0, "score": 0.1, "category_name": "a"}]
        oracle.append({"image_id": iid, "K": Kmat, "instances": inst})
    paths = {"dataset": os.path.join(root, "synth.json"), "oracle2d": os.path.join(root, "oracle_2d.json"), "depth": os.path.join(root, "depth"),
             "images": os.path.join(root, "images"), "weights": os.path.join(root, "sam_vit_test.pth")}
    with open(paths["dataset"], "w") as f:
        json.dump({"info": {"name": "synth"}, "images": images, "annotations": [], "categories": []}, f)
    with open(paths["oracle2d"], "w") as f:
        json.dump(oracle, f)
    torch.save(synth_sam_predictor_state_dict("vit_test", seed=3, image_size=128), paths["weights"])
    return paths


def _tool(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ovmono3d_geo.py")] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_tool_with_sam_masks_equals_the_run_on_its_dumped_masks(device, tmp_path):
    p = _dataset(str(tmp_path))
    common = ["--oracle2d", p["oracle2d"], "--dataset", p["dataset"], "--depth-dir", p["depth"]]
    dump, out_a, out_b = str(tmp_path / "dumped"), str(tmp_path / "a.json"), str(tmp_path / "b.json")
    sa = _tool(common + ["--mask", "sam", "--sam-weights", p["weights"], "--sam-arch", "vit_test", "--sam-image-size", "128", "--image-root",
                         p["images"], "--dump-masks", dump, "--output", out_a])
    assert sa["images"] == 3 and sa["below_threshold"] == 3 and sa["lifted"] >= 3, sa
    for k, (H, W) in enumerate(SIZES):
        z = np.load(os.path.join(dump, f"{10 + k}.npz"))
        assert z["masks"].dtype == np.uint8 and z["masks"].shape == (2, H, W) and list(z["index"]) == [0, 1]
        assert set(np.unique(z["masks"])) <= {0, 1} and 0 < z["masks"].mean() < 1
    sb = _tool(common + ["--mask-dir", dump, "--output", out_b])
    assert sb == sa
    with open(out_a) as f:
        a = json.load(f)
    with open(out_b) as f:
        b = json.load(f)
    assert a == b                                              # value for value
    assert sum(len(r["instances"]) for r in a) == sa["lifted"]
    for r in a:
        for ins in r["instances"]:
            assert len(ins["bbox3D"]) == 8 and np.isfinite(np.asarray(ins["bbox3D"])).all()


@pytest.fixture(scope="module")
def predictor(device):
    from ovmono3d_amd.sam import build_sam
    sd, img = so.case_inputs(so.TINY)
    pred = build_sam("vit_test", sd, device=device, image_size=128)
    pred.set_image(torch.from_numpy(img).to(device))
    return pred


def test_predict_plane_2_equals_predict_boxes(predictor):
    H, W = so.TINY["hw"]
    G = so.TINY["image_size"] // 16
    batch = predictor.predict_boxes(so.TINY["boxes"], mask_index=2)
    for i, box in enumerate(so.TINY["boxes"]):
        masks, iou, low = predictor.predict(box=np.asarray(box))
        assert masks.dtype == torch.bool and tuple(masks.shape) == (3, H, W)
        assert tuple(iou.shape) == (3,) and tuple(low.shape) == (3, 4 * G, 4 * G)
        assert torch.equal(masks[2], batch[i].bool())
    assert not torch.equal(batch[0], batch[2])


def test_two_predict_boxes_calls_after_one_set_image_give_the_same_bytes(predictor):
    a = predictor.predict_boxes(so.TINY["boxes"], mask_index=2)
    b = predictor.predict_boxes(so.TINY["boxes"], mask_index=2)
    assert torch.equal(a, b)
