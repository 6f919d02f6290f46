"""OVMono3D-GEO with Depth Pro end to end: tools/ovmono3d_geo.py --depth depthpro on a synthetic dataset."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import depthpro_oracle as do
from common import ROOT

pytestmark = pytest.mark.gpu

SIZES = ((96, 128), (120, 90))          # (H, W) of the two images


def _dataset(root):
    """Two JPEG images of different shapes, three boxes per image (one below the score threshold), the TINY Depth Pro weights."""
    os.makedirs(os.path.join(root, "images", "synth"))
    images, oracle = [], []
    for k, (H, W) in enumerate(SIZES):
        iid = 10 + k
        Image.fromarray(do.test_image(H, W, seed=30 + k)).save(os.path.join(root, "images", "synth", f"img_{iid}.jpg"), quality=92)
        Kmat = [[110.0, 0.0, W / 2.0], [0.0, 110.0, H / 2.0], [0.0, 0.0, 1.0]]
        images.append({"id": iid, "file_path": f"synth/img_{iid}.jpg", "height": H, "width": W, "K": Kmat, "dataset_id": 0})
        inst = [{"bbox": [10.0, 8.0, 0.5 * W, 0.6 * H], "category_id": 0, "score": 0.9, "category_name": "a"},
                {"bbox": [0.3 * W, 0.25 * H, 0.6 * W, 0.7 * H], "category_id": 1, "score": 0.6, "category_name": "b"},
                {"bbox": [5.0, 5.0, 20.0, 20.0], "category_id": 0, "score": 0.1, "category_name": "a"}]
        oracle.append({"image_id": iid, "K": Kmat, "instances": inst})
    paths = {"dataset": os.path.join(root, "synth.json"), "oracle2d": os.path.join(root, "oracle_2d.json"),
             "images": os.path.join(root, "images"), "weights": os.path.join(root, "depthpro_tiny.pt")}
    with open(paths["dataset"], "w") as f:
        json.dump({"info": {"name": "synth"}, "images": images, "annotations": [], "categories": []}, f)
    with open(paths["oracle2d"], "w") as f:
        json.dump(oracle, f)
    torch.save(do.case_inputs(do.TINY)[0], paths["weights"])
    return paths


def _tool(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ovmono3d_geo.py")] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("focal", ["estimate", "K"])
def test_tool_with_depthpro_equals_the_run_on_its_dumped_depth(device, tmp_path, focal):
    p = _dataset(str(tmp_path))
    common = ["--oracle2d", p["oracle2d"], "--dataset", p["dataset"], "--mask", "box"]
    dump, out_a, out_b = str(tmp_path / "dumped"), str(tmp_path / "a.json"), str(tmp_path / "b.json")
    sa = _tool(common + ["--depth", "depthpro", "--depthpro-weights", p["weights"], "--depthpro-config", json.dumps(do.TINY["config"]),
                         "--depthpro-focal", focal, "--image-root", p["images"], "--dump-depth", dump, "--output", out_a])
    assert sa["images"] == 2 and sa["below_threshold"] == 2 and sa["lifted"] >= 2, sa
    for k, (H, W) in enumerate(SIZES):
        d = np.load(os.path.join(dump, f"img_{10 + k}.npz"))["depth"]
        assert d.dtype == np.float32 and d.shape == (H, W) and np.isfinite(d).all() and d.min() > 0
    sb = _tool(common + ["--depth-dir", dump, "--output", out_b])
    assert sb == sa
    with open(out_a) as f:
        a = json.load(f)
    with open(out_b) as f:
        b = json.load(f)
    assert a == b                                              # value for value
    assert sum(len(r["instances"]) for r in a) == sa["lifted"]
