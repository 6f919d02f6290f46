"""GPU: demo.py --show-points draws the run's depth map under the boxes of the novel view and changes nothing else:
<name>_dets.json keeps its bytes and the front half of <name>_combine.jpg its pixels; without a depth source the flag is refused.

The front half is compared after decoding. The two files share every coefficient of the front half's blocks (W is a multiple of the
16-pixel MCU), so its luma is equal everywhere and its chroma in every column but the last: a decoder interpolates the chroma of
column W - 1 from the first chroma sample of the novel half (libjpeg's h2v2 upsampling), which is not the front view's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from common import ROOT

pytestmark = pytest.mark.gpu

H, W = 112, 160


def _setup(tmp_path):
    from PIL import Image
    inp, maps = tmp_path / "in", tmp_path / "maps"
    inp.mkdir()
    maps.mkdir()
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)).save(os.path.join(inp, "img000.png"))
    ii, jj = np.mgrid[0:H, 0:W]
    # 0.5 .. 2.8 m: the depth range the synthetic weights put their boxes in, so the cloud passes through the novel view's frame
    np.savez(maps / "img000.npz", depth=(0.5 + 2.0 * jj / W + 0.3 * ii / H).astype(np.float32))
    (tmp_path / "labels.json").write_text(json.dumps({"img000": ["chair", "table"]}))
    (tmp_path / "boxes.json").write_text(json.dumps({"img000": [{"bbox": [20, 20, 60, 50], "category_id": 0, "score": 0.9},
                                                                 {"bbox": [70, 40, 50, 60], "category_id": 1, "score": 0.8}]}))
    return inp, maps


def _demo(tmp_path, inp, out, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "demo", "demo.py"), "--config-file", os.path.join(ROOT, "configs", "OVMono3D_dinov2_SFP.yaml"),
           "--input-folder", str(inp), "--labels-file", str(tmp_path / "labels.json"), "--boxes-file", str(tmp_path / "boxes.json"),
           "--threshold", "0.0", *extra, "MODEL.DINO.MODEL_NAME", "vittest14", "MODEL.FPN.SQUARE_PAD", "224", "INPUT.MIN_SIZE_TEST", "140",
           "INPUT.MAX_SIZE_TEST", "224", "MODEL.WEIGHTS", "synthetic://vittest14?seed=3", "OUTPUT_DIR", str(out)]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def _ycc(path):
    from PIL import Image
    im = Image.open(path)
    im.draft("YCbCr", im.size)                                      # the decoder's own planes, no colour conversion on top
    assert im.mode == "YCbCr"
    return np.asarray(im)


def test_show_points_changes_the_novel_half_only(device, tmp_path):
    inp, maps = _setup(tmp_path)
    depth = ["--depth", "files", "--depth-dir", str(maps)]
    for out, flags in ((tmp_path / "plain", depth), (tmp_path / "points", depth + ["--show-points"])):
        r = _demo(tmp_path, inp, out, *flags)
        assert r.returncode == 0, r.stderr[-2000:]
    a, b = tmp_path / "plain", tmp_path / "points"
    assert len(json.loads((a / "img000_dets.json").read_text())["detections"]) == 2
    assert (a / "img000_dets.json").read_bytes() == (b / "img000_dets.json").read_bytes()
    pa, pb = _ycc(a / "img000_combine.jpg"), _ycc(b / "img000_combine.jpg")
    assert pa.shape == pb.shape == (H, W + H, 3)
    assert np.array_equal(pa[:, :W, 0], pb[:, :W, 0])               # front half: luma everywhere,
    assert np.array_equal(pa[:, :W - 1], pb[:, :W - 1])             # chroma up to the column the decoder blends with the novel half
    changed = (pa[:, W:] != pb[:, W:]).any(-1)
    assert changed.mean() > 0.01, f"only {int(changed.sum())} novel pixels differ: no point cloud was drawn"


def test_show_points_without_a_depth_source_exits_2(tmp_path):
    inp, _ = _setup(tmp_path)
    r = _demo(tmp_path, inp, tmp_path / "out", "--show-points", "--depth", "none")
    assert r.returncode == 2 and "--show-points" in r.stderr
    assert not (tmp_path / "out").exists()
    r = _demo(tmp_path, inp, tmp_path / "out", "--show-points")     # --depth none is the default
    assert r.returncode == 2
