"""Shared cases of the depth-prompt tests (test_depth_prompt_cpu.py, test_gpu_depth_prompt.py): the tiny main model (vittest14, canvas
224), the TINY Depth Pro of depthpro_oracle.py (crop 128, canvas 512), two images of both orientations (150 x 200 is TINY's own, 200 x
150 its seeded twin) so that a swapped height and width in the prompt path cannot pass, and a ResizeShortestEdge that changes the size
(150 x 200 -> 140 x 187)."""
from __future__ import annotations

import json
import os
from functools import lru_cache

import numpy as np
import torch

from common import build_cfg, rel_err
from depthpro_oracle import TINY
from sam_oracle import test_image

MIN_SIZE, MAX_SIZE, CANVAS = 140, 224, 224
SIZE_OPTS = ["INPUT.MIN_SIZE_TEST", MIN_SIZE, "INPUT.MAX_SIZE_TEST", MAX_SIZE]
MODEL_SEED = 5                                           # the synthetic checkpoint of test_gpu_model.py's depth-prompt test
TOL = 1e-3                                               # test_gpu_model.py TOL: the parity tolerance of its depth-prompt test
MARGIN = 10 * TOL                                        # what a depth prompt must move, so that a dropped prompt cannot pass parity
FIELDS = ("pred_boxes", "scores", "pred_bbox3D", "pred_center_cam", "pred_center_2D", "pred_dimensions", "pred_pose")
HWS = ((150, 200), (200, 150))
IMAGE_SEEDS = (TINY["image_seed"], 6)
DEPTHPRO_SPEC = f"synthetic://depthpro?seed={TINY['seed']}&crop={TINY['config']['crop']}"
DEPTHPRO_CONFIG_JSON = json.dumps({k: (list(v) if isinstance(v, tuple) else v) for k, v in TINY["config"].items() if k != "crop"})


def model_cfg(roi_heads="ROIHeads3D", extra=(), gpu_resize=True, max_rois=64):
    return build_cfg("vittest14", CANVAS, "f16x3", max_batch=1, max_rois=max_rois, roi_heads=roi_heads,
                     extra=SIZE_OPTS + ["MODEL.AMD.GPU_RESIZE", gpu_resize] + list(extra))


@lru_cache(maxsize=None)
def image_rgb(i: int) -> np.ndarray:
    """uint8 [H, W, 3], RGB (image 0 is depthpro_oracle.TINY's)."""
    return test_image(*HWS[i], seed=IMAGE_SEEDS[i])


def write_images(folder) -> list:
    """The two images as PNG files in cv2's / the mapper's reading (the file holds RGB); returns the base names."""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    names = []
    for i in range(len(HWS)):
        names.append(f"img{i:03d}")
        Image.fromarray(image_rgb(i)).save(os.path.join(folder, names[-1] + ".png"))
    return names


def intrinsics(i: int):
    h, w = HWS[i]
    return [[300.0, 0.0, w / 2], [0.0, 300.0, h / 2], [0.0, 0.0, 1.0]]


def boxes(i: int) -> dict:
    """Given 2D boxes in original-resolution coordinates (tests/common.py synth_inputs' rule)."""
    h, w = HWS[i]
    g = torch.Generator().manual_seed(40 + i)
    n = 6
    x1, y1 = torch.rand(n, generator=g) * (w * 0.6), torch.rand(n, generator=g) * (h * 0.6)
    bw, bh = (0.1 + torch.rand(n, generator=g) * 0.4) * w, (0.1 + torch.rand(n, generator=g) * 0.4) * h
    return {"gt_bbox2D": torch.stack([x1, y1, torch.clamp(x1 + bw, max=float(w)), torch.clamp(y1 + bh, max=float(h))], 1),
            "gt_classes": torch.randint(0, 50, (n,), generator=g), "gt_scores": 0.3 + 0.7 * torch.rand(n, generator=g)}


def dataset_dicts(image_folder, names) -> list:
    return [{"file_name": os.path.join(image_folder, n + ".png"), "height": HWS[i][0], "width": HWS[i][1], "K": intrinsics(i),
             "image_id": 100 + i, "oracle2D": boxes(i)} for i, n in enumerate(names)]


def model_input(i: int, image_format: str = "BGR") -> dict:
    """What the host mapper hands the model for image i (Pillow's resize; the device resize is bit-identical to it)."""
    from ovmono3d_amd.data import ResizeShortestEdge
    im = image_rgb(i)
    im = im[:, :, ::-1] if image_format == "BGR" else im
    im = ResizeShortestEdge(MIN_SIZE, MAX_SIZE)(np.ascontiguousarray(im))
    return {"image": torch.as_tensor(np.ascontiguousarray(im.transpose(2, 0, 1))), "height": HWS[i][0], "width": HWS[i][1],
            "K": intrinsics(i), "image_id": 100 + i, "oracle2D": boxes(i)}


def max_field_move(a: dict, b: dict) -> float:
    """The largest scale-relative difference (common.rel_err, the measure of the parity tolerance) over the float fields of two
    oracle-format results."""
    return max(rel_err(a[f], b[f]) for f in FIELDS)


def instances_as_dict(inst) -> dict:
    out = {}
    for f in FIELDS:
        v = inst.get(f)
        out[f] = (v.tensor if hasattr(v, "tensor") else v).detach().cpu()
    out["pred_classes"] = inst.pred_classes.cpu()
    return out


def assert_instances_equal(a, b, what=""):
    assert len(a) == len(b) and len(a) > 0, what
    assert torch.equal(a.pred_classes.cpu(), b.pred_classes.cpu()), what
    da, db = instances_as_dict(a), instances_as_dict(b)
    for f in FIELDS:
        assert torch.equal(da[f], db[f]), f"{what}: {f} differs"
