"""Where the 2D boxes and the masks of OVMono3D-GEO come from: what ``tools/ovmono3d_geo.py`` and ``demo/demo_geo.py`` put in front of
``geo.lift_boxes``, and the command-line flags of that choice.

Boxes: an oracle-2D or boxes file (``xywh_to_xyxy``), or the native GroundingDINO detector prompted with names (``detect_boxes``:
tools/make_oracle2d.py's caption and thresholds, boxes scaled back to the image). Masks: Segment Anything prompted with the boxes
(``sam_masks``; ``refined_masks`` for the passes of ``--sam-refine``) or with clicks (``point_masks``), the box itself (``box_masks``), or
files some other run wrote (``dump_masks`` / ``load_masks``: ``.npz`` or COCO RLE); ``clean_planes`` is ``--min-mask-region-area``.
``planes_on_device`` makes one device tensor of planes that may come from either side. Depth has its own module,
``ovmono3d_amd.data.depth_prompt`` (files, or Depth Pro on the device), with flags of the same pattern.
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np
import torch

from . import box_to_rect

BOX_THRESHOLD, NMS_THRESHOLD = 0.001, 0.5                            # tools/make_oracle2d.py's defaults


def xywh_to_xyxy(b):
    x, y, w, h = b
    return [x, y, x + w, y + h]


def planes_on_device(planes, dev):
    """One tensor [n, H, W] on ``dev`` of a list of [H, W] planes - numpy arrays of any strides or tensors on either side, mixed - in
    the planes' own dtype (uint8). An [n, H, W] tensor is moved there as it is."""
    if isinstance(planes, torch.Tensor):
        return planes.to(dev)
    return torch.stack([p.to(dev) if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in planes])


# ------------------------------------------------------------------------------------------ boxes
def detect_boxes(det, resize, bgr, cats, input_format="BGR"):
    """The native detector on one device image: (boxes xyxy [n, 4] at the image's resolution - float32 values, as tools/make_oracle2d.py
    writes them -, scores [n], class index [n])."""
    from ..modeling.roi_heads.gdino_glue import build_caption, gdino_postprocess, phrase_spans
    caption, _ = build_caption(cats)
    net = resize(bgr if input_format == "BGR" else bgr.flip(-1))
    r = det(net.permute(2, 0, 1).contiguous(), caption)
    boxes, scores, cls = gdino_postprocess(r["pred_logits"], r["pred_boxes"], phrase_spans(r["input_ids"], r["phrase_ids"]), tuple(net.shape[:2]),
                                           box_threshold=BOX_THRESHOLD, nms_threshold=NMS_THRESHOLD)
    sy, sx = bgr.shape[0] / net.shape[0], bgr.shape[1] / net.shape[1]                      # network resolution -> original resolution
    b = boxes.cpu().numpy() * np.array([sx, sy, sx, sy], np.float32)
    return b.astype(np.float64).reshape(-1, 4), scores.cpu().tolist(), cls.cpu().tolist()


# ------------------------------------------------------------------------------------------ masks from Segment Anything, or the box
def read_bgr(image_root, file_path, height, width, dev):
    """The image as cv2.imread gives it, on the device: uint8 [H, W, 3], BGR."""
    from ..data.gpu_jpeg import read_image_device
    path = os.path.join(image_root, file_path)
    if not os.path.exists(path):
        raise SystemExit(f"no image {path} (--image-root)")
    bgr = read_image_device(path, "BGR", dev)
    if tuple(bgr.shape[:2]) != (height, width):
        raise SystemExit(f"{path}: image is {tuple(bgr.shape[:2])} but the dataset says {(height, width)}")
    return bgr


def refined_masks(predictor, refine, mask_index=2, **prompts):
    """Device uint8 [n, H, W]: plane ``mask_index`` of ``predict_prompts(**prompts)``, then ``refine`` more passes of the same prompts
    with the previous pass's low-resolution logits of that plane as ``mask_inputs``."""
    masks, _, low = predictor.predict_prompts(mask_index=mask_index, want_lowres=refine > 0, **prompts)
    for k in range(refine):
        masks, _, low = predictor.predict_prompts(mask_inputs=low[:, mask_index].contiguous(), mask_index=mask_index, want_lowres=k + 1 < refine,
                                                  **prompts)
    return masks


def sam_masks(predictor, image_root, file_path, height, width, boxes_xyxy, bgr=None, refine=0):
    """Device uint8 [n, H, W]: SAM's plane [2] for every box of one image (one set_image, one predict_boxes; ``refine`` > 0: that many
    refinement passes behind it, ``refined_masks``)."""
    if bgr is None:
        bgr = read_bgr(image_root, file_path, height, width, predictor.engine.dev)
    predictor.set_image(bgr, image_format="BGR")   # the reference's call (run_seg_anything): a cv2 BGR array, declared as such
    if refine > 0 and len(boxes_xyxy):
        return refined_masks(predictor, refine, boxes=boxes_xyxy)
    return predictor.predict_boxes(boxes_xyxy, mask_index=2)


def box_masks(boxes_xyxy, h, w, device):
    """uint8 [n, h, w]: the pixels ``--mask box`` lifts (geo.box_to_rect, clipped to the image)."""
    planes = torch.zeros((len(boxes_xyxy), h, w), dtype=torch.uint8, device=device)
    for i, b in enumerate(boxes_xyxy):
        x0, y0, x1, y1 = box_to_rect(b)
        planes[i, max(y0, 0):max(min(y1, h), 0), max(x0, 0):max(min(x1, w), 0)] = 1
    return planes


def group_point_prompts(entries):
    """{(point count, has box): [positions in ``entries``]}, in order of first appearance. One predict_prompts call takes prompts of one
    shape; no prompt is padded with label -1 points to fit another's, so each sees exactly its own tokens."""
    groups = {}
    for i, e in enumerate(entries):
        if len(e["points"]) != len(e["labels"]):
            raise SystemExit(f"--points-file: entry {i} has {len(e['points'])} points and {len(e['labels'])} labels")
        groups.setdefault((len(e["points"]), "bbox" in e), []).append(i)
    return groups


def point_masks(predictor, bgr, entries, refine=0, min_area=0):
    """SAM's plane [2] for the click prompts ``entries`` of one image: (device uint8 [n, H, W] in the entries' order, xyxy boxes float64
    [n, 4]: the entry's own "bbox", else the tight box of its mask - zeros for an empty one). ``min_area`` > 0: the planes are
    cleaned (``clean_planes``) and the tight boxes are the cleaned masks'."""
    h, w = int(bgr.shape[0]), int(bgr.shape[1])
    planes = torch.zeros((len(entries), h, w), dtype=torch.uint8, device=bgr.device)
    boxes = np.zeros((len(entries), 4), np.float64)
    if not entries:
        return planes, boxes
    predictor.set_image(bgr, image_format="BGR")
    for (_, has_box), idx in group_point_prompts(entries).items():
        given = np.asarray([xywh_to_xyxy(entries[i]["bbox"]) for i in idx], np.float64) if has_box else None
        masks = refined_masks(predictor, refine, point_coords=np.asarray([entries[i]["points"] for i in idx], np.float32),
                              point_labels=np.asarray([entries[i]["labels"] for i in idx], np.int32), boxes=given)
        masks = clean_planes(masks, min_area)
        planes[idx] = masks
        boxes[idx] = given if has_box else predictor.mask_boxes(masks)[0].cpu().numpy().astype(np.float64)
    return planes, boxes


def clean_planes(planes, min_area):
    """``remove_small_regions(planes, min_area, "both")`` on a list of [H, W] planes (numpy arrays or device tensors) or a device
    [n, H, W] tensor: device uint8 [n, H, W] of 0 / 1. ``min_area`` 0, or no plane: what was given."""
    if not min_area or planes is None or len(planes) == 0:
        return planes
    from ..masks import remove_small_regions
    return remove_small_regions(planes_on_device(planes, torch.device("cuda", torch.cuda.current_device())), int(min_area), "both")[0]


# ------------------------------------------------------------------------------------------ masks in files
def dump_masks(mask_dir, image_id, positions, planes, fmt="npz"):
    """The <image_id>.npz file load_masks reads; fmt "rle": <image_id>.rle.json = {"index": [...], "masks": [COCO RLE, ...]} instead,
    encoded on the device (ovmono3d_amd.masks.encode_rle): the planes stay there and only the strings are read back."""
    os.makedirs(mask_dir, exist_ok=True)
    if fmt == "rle":
        from ..masks import encode_rle
        stack = planes_on_device(planes, torch.device("cuda", torch.cuda.current_device()))
        with open(os.path.join(mask_dir, f"{image_id}.rle.json"), "w") as f:
            json.dump({"index": [int(i) for i in positions], "masks": encode_rle(stack)}, f)
        return
    planes = [p.cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p) for p in planes]
    H, W = planes[0].shape
    np.savez_compressed(os.path.join(mask_dir, f"{image_id}.npz"), masks=np.stack(planes).astype(np.uint8).reshape(-1, H, W),
                        index=np.asarray(positions, np.int64))


def load_masks(mask_dir, image_id, height, width):
    """{position in the instance list: uint8 [H, W]} of one image; empty when the image has no mask file. <image_id>.npz when it
    exists (host arrays), else <image_id>.rle.json, decoded on the device (device tensors of 0 / 1)."""
    path = os.path.join(mask_dir, f"{image_id}.npz")
    if not os.path.exists(path):
        path = os.path.join(mask_dir, f"{image_id}.rle.json")
        if not os.path.exists(path):
            return {}
        from ..masks import decode_rle
        with open(path) as f:
            z = json.load(f)
        index, records = z["index"], z["masks"]
        if len(index) != len(records) or any(list(r["size"]) != [height, width] for r in records):
            raise SystemExit(f"{path}: {len(records)} masks / {len(index)} index entries do not fit a {height} x {width} image")
        if not records:
            return {}
        planes = decode_rle(records, torch.device("cuda", torch.cuda.current_device()))
        return {int(i): planes[k] for k, i in enumerate(index)}
    z = np.load(path)
    masks, index = z["masks"], z["index"]
    if masks.ndim != 3 or tuple(masks.shape[1:]) != (height, width) or len(index) != len(masks):
        raise SystemExit(f"{path}: masks {tuple(masks.shape)} / index {tuple(index.shape)} do not fit a {height} x {width} image")
    return {int(i): (masks[k] != 0).astype(np.uint8) for k, i in enumerate(index)}


# ------------------------------------------------------------------------------------------ command line
def add_mask_arguments(parser, choices=("box", "sam"), default=None) -> None:
    """The mask flags of tools/ovmono3d_geo.py and demo/demo_geo.py; ``default`` is ``--mask``'s."""
    parser.add_argument("--mask", choices=tuple(choices), default=default,
                        help="box: the 2D box is the mask - pixels ceil(x0) <= x < ceil(x1), ceil(y0) <= y < ceil(y1), clipped to the image; "
                             "sam: Segment Anything prompted with the box, plane [2] of its multimask outputs (the reference's rule)")
    parser.add_argument("--sam-weights", default=None, help="segment_anything checkpoint (.pth: image_encoder.*, prompt_encoder.*, mask_decoder.*)")
    parser.add_argument("--sam-arch", default="vit_l", help="vit_b or vit_l (vit_h has head dimension 80: refused)")
    parser.add_argument("--sam-image-size", type=int, default=None, help=argparse.SUPPRESS)      # tests: a small encoder input
    parser.add_argument("--sam-refine", type=int, default=0, metavar="N",
                        help="--mask sam: N more passes per prompt with the previous pass's low-resolution logits as mask_input (default 0: the "
                             "reference's single pass)")
    parser.add_argument("--min-mask-region-area", type=int, default=0, metavar="N",
                        help="clean the masks before they are lifted: holes, then islands, of fewer than N pixels are removed (segment_anything's "
                             "remove_small_regions, on the device; a deviation from the reference, which lifts the raw plane). What is dumped, "
                             "encoded or drawn is the cleaned plane. 0 (default): off. Accepted and without effect with --mask box")


def check_mask_arguments(args, parser):
    """argparse errors (exit status 2) for the mask flags that cannot work; host only."""
    if args.sam_refine < 0 or (args.sam_refine > 0 and args.mask != "sam"):
        parser.error("--sam-refine N needs N >= 0 and --mask sam")
    if args.min_mask_region_area < 0:
        parser.error("--min-mask-region-area N needs N >= 0")
    return args
