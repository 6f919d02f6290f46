"""GPU: demo.py writes the reference's picture - <name>_combine.jpg, the front view beside the novel view (H x (W + H) x 3) -
or <name>_boxes.jpg when the threshold keeps nothing; <name>_dets.json does not depend on drawing."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

pytestmark = pytest.mark.gpu


def _setup(tmp_path):
    from PIL import Image
    inp = tmp_path / "in"
    inp.mkdir()
    rng = np.random.default_rng(0)
    names = []
    for i in range(2):
        name = f"img{i:03d}"
        Image.fromarray(rng.integers(0, 255, (120 + 20 * i, 160, 3), dtype=np.uint8)).save(os.path.join(inp, name + ".png"))
        names.append(name)
    labels = {n: ["chair", "table"] for n in names}
    boxes = {n: [{"bbox": [20, 20, 60, 50], "category_id": 0, "score": 0.9}, {"bbox": [70, 40, 50, 60], "category_id": 1, "score": 0.8}]
             for n in names}
    (tmp_path / "labels.json").write_text(json.dumps(labels))
    (tmp_path / "boxes.json").write_text(json.dumps(boxes))
    return inp, names


def _demo(tmp_path, inp, out, threshold, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "demo", "demo.py"), "--config-file", os.path.join(ROOT, "configs", "OVMono3D_dinov2_SFP.yaml"),
           "--input-folder", str(inp), "--labels-file", str(tmp_path / "labels.json"), "--boxes-file", str(tmp_path / "boxes.json"),
           "--threshold", str(threshold), "MODEL.DINO.MODEL_NAME", "vittest14", "MODEL.FPN.SQUARE_PAD", "224", "INPUT.MIN_SIZE_TEST", "140",
           "INPUT.MAX_SIZE_TEST", "224", "MODEL.WEIGHTS", "synthetic://vittest14?seed=3", "OUTPUT_DIR", str(out), *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


def test_demo_writes_combine_jpg(device, tmp_path):
    from PIL import Image
    inp, names = _setup(tmp_path)
    out, plain = tmp_path / "out", tmp_path / "plain"
    _demo(tmp_path, inp, out, 0.0)
    _demo(tmp_path, inp, plain, 0.0, "MODEL.AMD.VIS", "False")
    for i, n in enumerate(names):
        h, w = 120 + 20 * i, 160
        im = np.asarray(Image.open(out / f"{n}_combine.jpg"))
        assert im.shape == (h, w + h, 3)
        assert im[:, w:].std() > 5                       # the novel view: grid, boxes and labels over the 225 canvas
        assert (out / f"{n}_dets.json").read_bytes() == (plain / f"{n}_dets.json").read_bytes()
        assert not (plain / f"{n}_combine.jpg").exists()


def test_demo_writes_boxes_jpg_when_nothing_is_kept(device, tmp_path):
    from PIL import Image
    inp, names = _setup(tmp_path)
    out = tmp_path / "out"
    _demo(tmp_path, inp, out, 1.1)
    for i, n in enumerate(names):
        assert json.loads((out / f"{n}_dets.json").read_text())["detections"] == []
        assert not (out / f"{n}_combine.jpg").exists()
        buf = io.BytesIO()                                # the input itself, through the same encoder (quality 95)
        Image.open(inp / f"{n}.png").convert("RGB").save(buf, format="JPEG", quality=95)
        assert np.array_equal(np.asarray(Image.open(out / f"{n}_boxes.jpg")), np.asarray(Image.open(buf)))
