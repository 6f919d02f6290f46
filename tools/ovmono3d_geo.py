#!/usr/bin/env python3
"""OVMono3D-GEO, the training-free baseline (reference tools/ovmono3d_geo.py): lifts the 2D boxes of an oracle-2D file to 3D from
a metric depth map and a mask per box - un-projection, PCA yaw, DBSCAN outlier removal, extent fit - on the device
(ovmono3d_amd.geo, csrc/geo.hip), and writes the reference's per-image records for tools/eval_ovmono3d_geo.py.

    python tools/ovmono3d_geo.py --oracle2d gdino_kitti_novel_oracle_2d.json --dataset datasets/Omni3D/KITTI_test_novel.json \\
        --depth-dir datasets/depth --mask sam --sam-weights sam_vit_l_0b3195.pth --sam-arch vit_l --image-root datasets \\
        --output output/ovmono3d_geo/KITTI_test_novel.pth

Masks, one of:
  ``--mask sam``   the reference's way (tools/ovmono3d_geo.py:213-217,270-272,308-309): Segment Anything prompted with each 2D box,
                   plane [2] of the multimask outputs, on the device (ovmono3d_amd.sam, csrc/sam.hip). One ``set_image`` per image
                   (the reference repeats it per instance, with the same result) and one ``predict_boxes`` call for all instances at
                   or above the score threshold; the planes go straight to the lifting without leaving the device. Images are read
                   from ``<image-root>/<file_path>`` by the device JPEG decoder (the host reader for files outside its scope) in
                   cv2.imread's BGR order and handed over as the reference does (``set_image(im, image_format="BGR")``). vit_b
                   and vit_l checkpoints; vit_h (head dimension 80) is refused by the library. ``--sam-refine N`` adds
                   segment_anything's refinement pass N times: the same box again with the previous pass's low-resolution logits
                   of plane [2] as ``mask_input``.
  ``--mask-dir``   masks some other program wrote: ``<mask-dir>/<image_id>.npz`` with ``masks`` uint8 [n, H, W] (nonzero = inside)
                   and ``index`` int [n], the positions of the masked instances in the image's instance list. ``--dump-masks DIR``
                   writes exactly these files from a ``--mask sam`` run. With ``--mask-format rle`` it writes
                   ``<image_id>.rle.json`` = ``{"index": [...], "masks": [{"size": [H, W], "counts": str}, ...]}`` instead: COCO RLE,
                   encoded on the device, so no plane is copied to the host. ``--mask-dir`` reads the ``.npz`` when it exists, else
                   the ``.rle.json`` (decoded on the device); the 3D records are the same either way.
  ``--mask box``   the 2D box itself is the mask: the pixels ceil(x0) <= x < ceil(x1), ceil(y0) <= y < ceil(y1) of the xyxy box,
                   clipped to the image (the reference has no such mode; the rule is this project's).

``--min-mask-region-area N`` (default 0: off, the same bytes as without it) cleans every ``--mask sam`` and ``--mask-dir`` plane before
it is lifted: segment_anything's ``remove_small_regions`` on the device (``ovmono3d_amd.masks.remove_small_regions(planes, N, "both")``:
holes below N pixels filled, then islands below N pixels cleared, 8-connected). A declared deviation: the reference lifts the raw
plane [2], specks included. ``--dump-masks`` writes the cleaned planes. With ``--mask box`` the mask is a rectangle: the flag is accepted
and does nothing.

Depth, one of:
  ``--depth files``     (default) read from ``<depth-dir>/test/<image base name>.npz`` (or ``<depth-dir>/<image base name>.npz``), key
                        ``depth``, metres, at the image's own resolution - a map of another shape is refused, the reference never
                        resizes it.
  ``--depth depthpro``  the reference's way (tools/ovmono3d_geo.py:267,290-295): Depth Pro on the device (ovmono3d_amd.depthpro,
                        csrc/depthpro.hip) from ``--depthpro-weights`` (Hugging Face ``apple/DepthPro-hf`` key names; Apple's own
                        ``depth_pro.pt`` names are not mapped). ``--depthpro-focal estimate`` (default) lets the field-of-view head
                        choose the focal length, as the reference does for images without EXIF data (EXIF is not read here);
                        ``--depthpro-focal K`` passes the dataset's ``K[0][0]``. ``--dump-depth DIR`` writes ``<DIR>/<image base
                        name>.npz`` with key ``depth``: the files ``--depth-dir`` and DatasetMapper3D read.

Instances below ``--score-threshold`` are dropped as in the reference. Instances the reference has no answer for (an empty mask,
fewer than 2 points, a non-finite depth under the mask, a box outside the image, no mask in the mask file) are skipped, counted
and logged.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ovmono3d_amd.data.depth_prompt import add_depth_arguments, build_depth_prompt, check_depth_arguments, load_depth  # noqa: E402
from ovmono3d_amd.geo import GeoParams, lift_boxes  # noqa: E402
from ovmono3d_amd.geo.sources import (add_mask_arguments, check_mask_arguments, clean_planes, dump_masks, load_masks, planes_on_device,  # noqa: E402
                                      read_bgr, sam_masks, xywh_to_xyxy)

logger = logging.getLogger("ovmono3d_geo")
KEPT_KEYS = ("category_id", "bbox", "score", "category_name")


def lift_image(depth, K, boxes_xyxy, masks, params):
    """depth: float32 [H, W], numpy or a device tensor; masks: uint8 [H, W] planes (a list of numpy arrays or device tensors, or a device
    [n, H, W] tensor) or None (the box is the mask). One device call."""
    dev = torch.device("cuda", torch.cuda.current_device())
    d = depth.to(dev) if isinstance(depth, torch.Tensor) else torch.from_numpy(depth).to(dev)
    return lift_boxes(d, K, boxes_xyxy=boxes_xyxy, masks=None if masks is None else planes_on_device(masks, dev), params=params)


def run(args):
    with open(args.oracle2d) as f:
        oracle = json.load(f)
    with open(args.dataset) as f:
        images = {im["id"]: im for im in json.load(f)["images"]}
    params = GeoParams()
    use_box, use_sam = args.mask == "box", args.mask == "sam"
    if not use_box and not use_sam and not args.mask_dir:
        raise SystemExit("give --mask-dir DIR, --mask sam or --mask box")
    predictor = None
    if use_sam:
        if not args.sam_weights or not args.image_root:
            raise SystemExit("--mask sam needs --sam-weights FILE and --image-root DIR")
        from ovmono3d_amd.sam import build_sam
        predictor = build_sam(args.sam_arch, args.sam_weights, image_size=args.sam_image_size)
    depth_source = None
    if args.depth == "depthpro":
        if not args.depthpro_weights or not args.image_root:
            raise SystemExit("--depth depthpro needs --depthpro-weights FILE and --image-root DIR")
        depth_source = build_depth_prompt(args.depthpro_weights, args.depthpro_focal, args.depthpro_config, args.dump_depth)
    out, n_in, n_low, n_skip, n_lifted = [], 0, 0, 0, 0
    for rec in oracle:
        im = images.get(rec["image_id"])
        if im is None:
            raise SystemExit(f"image_id {rec['image_id']} of {args.oracle2d} is not in {args.dataset}")
        H, W = int(im["height"]), int(im["width"])
        K = np.asarray(rec.get("K", im["K"]), np.float64).reshape(3, 3)
        cand = [(pos, ins) for pos, ins in enumerate(rec["instances"]) if not ins["score"] < args.score_threshold]
        n_in += len(rec["instances"])
        n_low += len(rec["instances"]) - len(cand)
        new_instances = []
        if cand:
            bgr = None
            if depth_source is not None:
                bgr = read_bgr(args.image_root, im["file_path"], H, W, depth_source.depthpro.dev)
                depth = depth_source(bgr, "BGR", K, file_name=im["file_path"])
            else:
                depth = load_depth(args.depth_dir, im["file_path"], H, W)
            planes = None
            if use_sam:
                boxes = np.asarray([xywh_to_xyxy(ins["bbox"]) for _, ins in cand], np.float64)
                planes = sam_masks(predictor, args.image_root, im["file_path"], H, W, boxes, bgr=bgr, refine=args.sam_refine)
            elif not use_box:
                have = load_masks(args.mask_dir, rec["image_id"], H, W)
                missing = [pos for pos, _ in cand if pos not in have]
                if missing:
                    logger.warning("image %s: no mask for instances %s - skipped", rec["image_id"], missing)
                    n_skip += len(missing)
                cand = [(pos, ins) for pos, ins in cand if pos in have]
                planes = [have[pos] for pos, _ in cand]
            if cand:
                boxes = np.asarray([xywh_to_xyxy(ins["bbox"]) for _, ins in cand], np.float64)
                planes = clean_planes(planes, args.min_mask_region_area)
                lifted = lift_image(depth, K, boxes, planes, params)
                if args.dump_masks and planes is not None:
                    dump_masks(args.dump_masks, rec["image_id"], [pos for pos, _ in cand], planes, args.mask_format)
                for (pos, ins), box in zip(cand, lifted):
                    if box is None:
                        logger.warning("image %s: instance %d has no 3D box (empty mask, < 2 points, non-finite depth or a box outside "
                                       "the image) - skipped", rec["image_id"], pos)
                        n_skip += 1
                        continue
                    new = {k: v for k, v in ins.items() if k in KEPT_KEYS}
                    new["image_id"] = rec["image_id"]
                    for k in ("bbox3D", "depth", "center_cam", "dimensions", "pose", "center_2D"):
                        new[k] = box[k]
                    new_instances.append(new)
        n_lifted += len(new_instances)
        new_rec = dict(rec)
        new_rec["instances"] = new_instances
        out.append(new_rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    if args.output.endswith(".json"):
        with open(args.output, "w") as f:
            json.dump(out, f)
    else:
        torch.save(out, args.output)
    stats = {"images": len(out), "instances": n_in, "below_threshold": n_low, "skipped": n_skip, "lifted": n_lifted}
    logger.info("wrote %s: %s", args.output, json.dumps(stats))
    return stats


def argument_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--oracle2d", required=True, help="oracle-2D file (tools/make_oracle2d.py): [{image_id, instances[{bbox xywh, category_id, score}]}]")
    ap.add_argument("--dataset", required=True, help="Omni3D annotation json of the same images (file_path, height, width, K)")
    add_depth_arguments(ap)
    ap.add_argument("--mask-dir", default=None, help="<image_id>.npz with 'masks' uint8 [n, H, W] and 'index' int [n]")
    add_mask_arguments(ap)
    ap.add_argument("--image-root", default=None, help="directory the dataset's file_path entries are relative to (--mask sam)")
    ap.add_argument("--dump-masks", default=None, metavar="DIR", help="write the masks used as <DIR>/<image_id>.npz, the files --mask-dir reads")
    ap.add_argument("--mask-format", choices=("npz", "rle"), default="npz",
                    help="--dump-masks: npz (planes copied to the host and deflated) or rle (<image_id>.rle.json, COCO RLE encoded on the device); "
                         "--mask-dir reads either")
    ap.add_argument("--score-threshold", type=float, default=0.30)
    ap.add_argument("--output", required=True, help=".pth (torch.save, as the reference) or .json")
    return ap


def check_args(args, parser=None):
    """Exit status 2 for what cannot work, before any device call: the shared depth and mask checks; --depth-dir is required unless
    Depth Pro supplies the depth."""
    parser = parser if parser is not None else argument_parser()
    check_depth_arguments(args, parser, None, files_need_dir=True)
    return check_mask_arguments(args, parser)


def main():
    logging.basicConfig(level=logging.INFO)
    parser = argument_parser()
    args = check_args(parser.parse_args(), parser)
    if not torch.cuda.is_available():
        raise SystemExit("OVMono3D-GEO runs on the HIP device (there is no CPU path)")
    print(json.dumps(run(args)))


if __name__ == "__main__":
    main()
