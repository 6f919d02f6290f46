#!/usr/bin/env python3
"""OVMono3D-GEO, the training-free method, on a folder of images and a list of names per image - what demo/demo.py is for OVMono3D-LIFT.

    python demo/demo_geo.py --config-file configs/OVMono3D_dinov2_SFP.yaml --input-folder datasets/coco_examples \\
        --labels-file datasets/coco_examples/labels.json --depth depthpro --depthpro-weights checkpoints/depthpro_hf.safetensors \\
        --mask sam --sam-weights checkpoints/sam_vit_l_0b3195.pth \\
        MODEL.AMD.GDINO_WEIGHTS checkpoints/groundingdino_swinb_cogcoor.pth MODEL.AMD.BERT_VOCAB bert-base-uncased/vocab.txt OUTPUT_DIR output/geo

Per image, all on the device: read (the device JPEG route) -> K by demo.py's focal-length convention (the first image's focal length
sticks) -> 2D boxes, from ``--boxes-file`` ({image name: [{bbox xywh, category_id, score}]}) or from the native GroundingDINO detector
prompted with the image's names (tools/make_oracle2d.py's detector, caption and thresholds; boxes scaled back to the image) -> boxes
below ``--threshold`` dropped -> metric depth (``--depth depthpro``: Depth Pro on the image; ``--depth files``: ``<depth-dir>/test/<name>.npz``
or ``<depth-dir>/<name>.npz``) -> a mask per box (``--mask sam``: Segment Anything prompted with the box, plane [2]; ``--mask box``: the box
itself) -> ``ovmono3d_amd.geo.lift_boxes``. Written: ``<name>_dets.json`` in demo.py's schema (instances the lift has no answer for are
left out and counted in the printed line) and ``<name>_combine.jpg``, demo.py's picture; with ``--show-points`` (the default) its novel
view shows the depth map as a point cloud under the boxes, each box's points tinted with its colour. ``<name>_boxes.jpg`` (the input)
when nothing is lifted.

``--points-file FILE`` replaces the detector with clicks: ``{image name: [{"points": [[x, y], ...], "labels": [1, 0, ...],
"category_name": str, optional "bbox": xywh, optional "score"}]}`` (labels 1 foreground, 0 background; at most 8 points). Neither
GroundingDINO weights nor a vocabulary nor ``--labels-file`` are needed: Segment Anything masks what was clicked (plane [2], as for
boxes; a "bbox" joins the clicks as a box prompt) and the mask is lifted. The record's 2D box is the entry's "bbox", else the tight box
of its mask; its score the entry's, else 1.0. ``--sam-refine N`` runs N refinement passes behind the first (the same prompt with the
previous low-resolution logits as ``mask_input``), for boxes and for clicks.

``--everything`` needs neither names nor boxes nor clicks: Segment Anything's automatic mask generator (a ``--points-per-side`` grid of
clicks, ``--pred-iou-thresh``, ``--stability-score-thresh``, ``--box-nms-thresh``; ``ovmono3d_amd.sam.SamAutomaticMaskGenerator``) proposes
the masks of the whole image and every one is lifted. The record's 2D box is the tight box of its mask, its score the predicted IoU,
its category "object"; ``--threshold`` is not applied (the generator has its own thresholds). It needs ``--mask sam`` and is refused
together with ``--points-file`` or ``--boxes-file``.

Masks as outputs, both off by default (the files above are then unchanged): ``--segmentation rle`` adds ``"segmentation": {"size": [H, W],
"counts": str}`` to every record of ``<name>_dets.json``, the instance's mask as a COCO RLE string, whatever the mask came from (boxes,
clicks, ``--everything``, ``--mask box``); ``--show-masks`` writes ``<name>_masks.jpg``, the image with the kept instances' masks
overlaid in the boxes' colours (alpha 0.5, contours). Both are computed on the device (``ovmono3d_amd.masks``); no plane is copied to
the host.

``--min-mask-region-area N`` (default 0: off, every file as without it) cleans the masks before they are lifted: segment_anything's
``remove_small_regions``, holes below N pixels filled and then islands below N pixels cleared (8-connected), on the device
(``ovmono3d_amd.masks.remove_small_regions``). With ``--everything`` it is the generator's ``min_mask_region_area`` (cleaned masks, their
boxes and areas, and the second NMS); for box and click prompts the planes are cleaned before ``lift_boxes``, and a click prompt without a
"bbox" takes the tight box of its cleaned mask. The cleaned planes are what ``--segmentation rle``, ``--show-masks`` and the cloud tint
see. A declared deviation: the reference lifts the raw plane [2], specks included. ``--mask box`` is a rectangle: the flag is accepted
and does nothing.

``--scene-ply`` (off by default; the files above are then unchanged) writes ``<name>_scene.ply``: the depth map un-projected as coloured
points - tinted per box as in the novel view - and the kept boxes as vertices, faces and edges, one binary PLY file to orbit in any
viewer. The points are compacted and packed on the device (``ovmono3d_amd.vis.scene_ply``); ``--ply-stride N``, ``--ply-max-depth M`` and
``--ply-frame camera|opengl`` as in demo/demo.py.

``MODEL.AMD.GEO_UPRIGHT True`` among the trailing options (default False: every file as without it, no new file) stands the boxes
upright on the floor: the plane is fitted once per image to its depth map on the device (``ovmono3d_amd.geo.ground_plane``: RANSAC over
plane hypotheses, then a least-squares refinement) and every instance is lifted in the frame in which the floor's normal is the vertical
axis, so a pitched or rolled camera no longer tilts the boxes. A declared deviation: the reference takes the camera for level.
``<name>_ground.json`` holds ``status``, ``upright``, ``normal`` and ``offset`` of the plane in the camera's frame (x right, y down, z
forward: the points with normal . p + offset = 0; offset is the camera's height above the floor), ``n_points``, ``n_inliers`` and
``share``; every record of ``<name>_dets.json`` gets ``height_above_ground`` (metres, the lowest corner; negative: below the floor).
Where no plane is found the image is lifted level, the file says so and ``<name>_dets.json`` is that of a run without the key. The
fit's settings (``ovmono3d_amd.geo.GroundParams``) are defaults nobody has tuned on real depth maps.

The LIFT model is not built: ``MODEL.WEIGHTS`` is not needed, the config supplies the detector's settings and ``OUTPUT_DIR``.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ovmono3d_amd import vis  # noqa: E402
from ovmono3d_amd.data.depth_prompt import add_depth_arguments, build_depth_prompt, check_depth_arguments, load_depth  # noqa: E402
from ovmono3d_amd.data.gpu_jpeg import read_image_device, write_jpeg  # noqa: E402
from ovmono3d_amd.data.gpu_resize import ResizeShortestEdgeGPU  # noqa: E402
from ovmono3d_amd.defaults import make_cfg  # noqa: E402
from ovmono3d_amd.gdino.detector import build_detector  # noqa: E402
from ovmono3d_amd.geo import GROUND_STATUS_NAMES, GeoParams, ground_plane, lift_boxes  # noqa: E402
from ovmono3d_amd.geo.sources import (add_mask_arguments, box_masks, check_mask_arguments, clean_planes, detect_boxes, point_masks,  # noqa: E402
                                      sam_masks, xywh_to_xyxy)
from ovmono3d_amd.masks import encode_rle, overlay_masks  # noqa: E402
from ovmono3d_amd.vis.outputs import add_ply_arguments, write_scene, write_views  # noqa: E402


# ---- step 1: the 2D instances of one image. One of the four below is chosen per run (build_run); each returns (boxes xyxy float64
# [n, 4], scores [n], class index [n], the positions that go on to the lift, masks) where masks(boxes of those positions) is step 2:
# (device uint8 planes [m, H, W] or None: the box is the mask, the positions' boxes)
def candidates(scores, threshold):
    return [i for i, s in enumerate(scores) if not s < threshold]


def box_prompt_masks(args, run, im):
    """Step 2 for boxes from a file or the detector: Segment Anything prompted with them (None with --mask box), cleaned."""
    def masks(cboxes):
        planes = None
        if run.predictor is not None:
            planes = sam_masks(run.predictor, None, None, int(im.shape[0]), int(im.shape[1]), cboxes, bgr=im, refine=args.sam_refine)
        return clean_planes(planes, args.min_mask_region_area), cboxes
    return masks


def everything_instances(args, cfg, run, im, im_name, cats):
    """--everything: the masks come first, their tight boxes are the 2D boxes; --threshold is not applied."""
    auto = run.generator.generate_device(im, "BGR", min_mask_region_area=args.min_mask_region_area)
    boxes = auto["boxes"].cpu().numpy().astype(np.float64).reshape(-1, 4)
    scores = [float(s) for s in auto["scores"].cpu().tolist()]
    return boxes, scores, [0] * len(boxes), list(range(len(boxes))), lambda cboxes: (auto["masks"], cboxes)


def click_instances(args, cfg, run, im, im_name, cats):
    """--points-file: the 2D boxes come with the masks (the entry's "bbox", else the tight box of its mask)."""
    entries = run.points.get(im_name, [])
    scores = [float(e.get("score", 1.0)) for e in entries]
    cand = candidates(scores, args.threshold)

    def masks(cboxes):
        return point_masks(run.predictor, im, [entries[i] for i in cand], args.sam_refine, args.min_mask_region_area)
    return np.zeros((len(entries), 4), np.float64), scores, list(range(len(entries))), cand, masks


def file_instances(args, cfg, run, im, im_name, cats):
    inst = run.boxes.get(im_name, [])
    boxes = np.asarray([xywh_to_xyxy(b["bbox"]) for b in inst], np.float64).reshape(-1, 4)
    scores, classes = [float(b.get("score", 1.0)) for b in inst], [int(b["category_id"]) for b in inst]
    return boxes, scores, classes, candidates(scores, args.threshold), box_prompt_masks(args, run, im)


def detector_instances(args, cfg, run, im, im_name, cats):
    boxes, scores, classes = detect_boxes(run.detector, run.resize, im, cats, cfg.INPUT.FORMAT)
    return boxes, scores, classes, candidates(scores, args.threshold), box_prompt_masks(args, run, im)


def build_run(args, cfg, dev):
    """What a run builds once: the source of the 2D instances and its files or networks, the names per image (None: every image has
    the one name "object"), the depth source (None: files) and the SAM predictor (None: --mask box)."""
    run = SimpleNamespace(names=None, points=None, boxes=None, detector=None, resize=None, depth_source=None, predictor=None, generator=None)
    if args.everything:                                                      # reads neither names nor boxes nor clicks
        run.instances = everything_instances
    elif args.points_file:
        run.instances = click_instances
        with open(args.points_file) as f:
            run.points = json.load(f)
        run.names = {n: [e["category_name"] for e in entries] for n, entries in run.points.items()}
    else:
        with open(args.labels_file) as f:
            run.names = json.load(f)
        if args.boxes_file:
            run.instances = file_instances
            with open(args.boxes_file) as f:
                run.boxes = json.load(f)
        else:
            run.instances = detector_instances
            run.detector = build_detector(cfg, dev)
            run.resize = ResizeShortestEdgeGPU(cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST)
    if args.depth == "depthpro":
        run.depth_source = build_depth_prompt(args.depthpro_weights, args.depthpro_focal, args.depthpro_config, args.dump_depth, dev)
    if args.mask == "sam":
        from ovmono3d_amd.sam import build_sam
        run.predictor = build_sam(args.sam_arch, args.sam_weights, device=dev, image_size=args.sam_image_size)
    if args.everything:
        from ovmono3d_amd.sam import SamAutomaticMaskGenerator
        run.generator = SamAutomaticMaskGenerator(run.predictor, points_per_side=args.points_per_side, pred_iou_thresh=args.pred_iou_thresh,
                                                  stability_score_thresh=args.stability_score_thresh, box_nms_thresh=args.box_nms_thresh)
    return run


# ---- step 3
def lift_records(depth, K, params, cats, boxes, scores, classes, cand, planes, ground=None):
    """lift_boxes on the candidates: (demo.py's records of the lifted ones, their positions among the candidates). ground: the image's
    GroundCall (MODEL.AMD.GEO_UPRIGHT) or None."""
    lifted = lift_boxes(depth, K, boxes_xyxy=boxes[cand], masks=list(planes) if planes is not None else None, params=params, frame=ground)
    out, kept_idx = [], []
    for k, (i, box) in enumerate(zip(cand, lifted)):
        if box is None:
            continue
        kept_idx.append(k)
        ci = classes[i]
        out.append({"category": cats[ci] if 0 <= ci < len(cats) else ci, "score": float(scores[i]),
                    "bbox3D": list(box["center_cam"]) + list(box["dimensions"]), "pose": box["pose"], "corners3D": box["bbox3D"],
                    "center_2D": list(box["center_2D"]), "bbox2D": [float(v) for v in boxes[i]]})
        if "height_above_ground" in box:
            out[-1]["height_above_ground"] = box["height_above_ground"]
    return out, kept_idx


def write_ground(output_dir, im_name, g):
    """<name>_ground.json of a fitted plane (OvmGroundResult), in the camera's frame: the lift's frame with y and z flipped."""
    found = g.status == 0
    with open(os.path.join(output_dir, im_name + "_ground.json"), "w") as f:
        json.dump({"status": GROUND_STATUS_NAMES[g.status], "upright": found, "normal": [g.normal[0], -g.normal[1], -g.normal[2]] if found else None,
                   "offset": g.offset if found else None, "n_points": g.n_points, "n_inliers": g.n_inliers,
                   "share": g.n_inliers / g.n_points if g.n_points else 0.0}, f)


# ---- step 4
def write_outputs(args, cfg, im, K, im_name, out, kept_idx, cboxes, planes, depth):
    """<name>_dets.json, the picture and, where asked for, the scene file and the mask picture; ``planes`` None: the boxes are the masks."""
    h, w, dev = int(im.shape[0]), int(im.shape[1]), im.device
    gpu_jpeg, labels = bool(cfg.MODEL.AMD.get("GPU_JPEG_WRITE", True)), None
    if out and planes is None and (args.show_points or args.segmentation == "rle" or args.show_masks or args.scene_ply):
        planes = box_masks(cboxes, h, w, dev)
    if out and (args.show_points or args.scene_ply):
        labels = vis.labels_from_masks(planes[kept_idx])
    if out and args.segmentation == "rle":                                   # encoded on the device: only the strings are read back
        for rec, rle in zip(out, encode_rle(planes[kept_idx])):
            rec["segmentation"] = rle
    with open(os.path.join(cfg.OUTPUT_DIR, im_name + "_dets.json"), "w") as f:
        json.dump({"K": K.tolist(), "detections": out}, f)
    write_views(im, K, out, kept_idx, cfg.OUTPUT_DIR, im_name, gpu_jpeg=gpu_jpeg, depth=depth if out and args.show_points else None,
                labels=labels if args.show_points else None)
    if args.scene_ply:
        write_scene(args, im, K, out, kept_idx, cfg.OUTPUT_DIR, im_name, depth=depth, labels=labels)
    if args.show_masks:                                                      # the image under the kept instances' masks, in the boxes' colours
        shown = overlay_masks(im, planes[kept_idx] if out else torch.zeros((0, h, w), dtype=torch.uint8, device=dev),
                              [vis.get_color(i) for i in kept_idx], alpha=0.5)
        write_jpeg(os.path.join(cfg.OUTPUT_DIR, im_name + "_masks.jpg"), shown, quality=95, channel_order="BGR", use_device=gpu_jpeg)


def do_test(args, cfg):
    dev = torch.device("cuda", torch.cuda.current_device())
    ims = sorted(f for f in os.listdir(args.input_folder) if not f.endswith(".json"))
    run = build_run(args, cfg, dev)
    params = GeoParams()
    focal_length, principal_point = args.focal_length, args.principal_point
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    for name in ims:
        im_name = os.path.splitext(name)[0]
        cats = ["object"] if run.names is None else run.names.get(im_name, [])
        if cats == []:
            continue
        stages, t0 = {}, time.perf_counter()

        def lap(stage):
            nonlocal t0
            if args.stage_times:
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                stages[stage] = round((t1 - t0) * 1e3, 3)
                t0 = t1

        im = read_image_device(os.path.join(args.input_folder, name), "BGR", dev)
        h, w = int(im.shape[0]), int(im.shape[1])
        if focal_length == 0:
            focal_length = 4.0 * h / 2                                       # demo.py:63-65
        px, py = (w / 2, h / 2) if len(principal_point) == 0 else principal_point
        K = np.array([[focal_length, 0.0, px], [0.0, focal_length, py], [0.0, 0.0, 1.0]])
        lap("read")
        boxes, scores, classes, cand, masks = run.instances(args, cfg, run, im, im_name, cats)
        lap("boxes")
        out, kept_idx, planes, depth, ground = [], [], None, None, None
        if cand:
            if run.depth_source is not None:
                depth = run.depth_source(im, "BGR", K, file_name=name)
            else:
                depth = torch.from_numpy(load_depth(args.depth_dir, name, h, w)).to(dev)
            lap("depth")
            if cfg.MODEL.AMD.get("GEO_UPRIGHT", False):                      # enqueued here, read with the lift's results
                ground = ground_plane(depth, K)
                lap("ground")
            planes, boxes[cand] = masks(boxes[cand])
            lap("masks")
            out, kept_idx = lift_records(depth, K, params, cats, boxes, scores, classes, cand, planes, ground)
            lap("lift")
            if ground is not None:
                write_ground(cfg.OUTPUT_DIR, im_name, ground.read())
        print("File: {} with {} dets ({} boxes at or above the threshold, {} not lifted)".format(im_name, len(out), len(cand), len(cand) - len(out)))
        write_outputs(args, cfg, im, K, im_name, out, kept_idx, boxes[cand], planes, depth)
        lap("views")
        if args.stage_times:
            print("stage_ms " + json.dumps({"image": im_name, **stages}))


def argument_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--config-file", default="", metavar="FILE", help="path to config file")
    parser.add_argument("--input-folder", type=str, help="folder of images to process", required=True)
    parser.add_argument("--labels-file", type=str, default="", help="path to labels file: {image name: [category names]} (required without --points-file)")
    parser.add_argument("--points-file", type=str, default="",
                        help="click prompts per image ({image name: [{points [[x, y]], labels [1 | 0], category_name, optional bbox xywh, optional score}]}) "
                             "instead of the detector: Segment Anything masks what was clicked")
    parser.add_argument("--everything", action="store_true",
                        help="no names, boxes or clicks: Segment Anything's automatic mask generator proposes the masks and each is lifted (needs --mask sam)")
    parser.add_argument("--points-per-side", type=int, default=32, help="--everything: the click grid's side (at most 36)")
    parser.add_argument("--pred-iou-thresh", type=float, default=0.88, help="--everything: keep masks whose predicted IoU is above it")
    parser.add_argument("--stability-score-thresh", type=float, default=0.95, help="--everything: keep masks whose stability score is at least it")
    parser.add_argument("--box-nms-thresh", type=float, default=0.7, help="--everything: box IoU above which the lower-scored mask is dropped")
    parser.add_argument("--boxes-file", type=str, default="", help="2D boxes per image ({image name: [{bbox xywh, category_id, score}]}) instead of the detector")
    parser.add_argument("--focal-length", type=float, default=0, help="focal length for image inputs (in px)")
    parser.add_argument("--principal-point", type=float, default=[], nargs=2, help="principal point for image inputs (in px)")
    parser.add_argument("--threshold", type=float, default=0.30, help="2D boxes scoring below it are dropped (the reference GEO's cut)")
    add_depth_arguments(parser, choices=("depthpro", "files"), default="depthpro",
                        focal_help="the K[0][0] of this run: --focal-length, or without it the reference's convention 4.0 * h / 2 of the first image")
    add_mask_arguments(parser, choices=("sam", "box"), default="sam")
    parser.add_argument("--stage-times", action="store_true", help=argparse.SUPPRESS)            # measurements: synchronise and print per-stage ms
    parser.add_argument("--show-points", default=True, action=argparse.BooleanOptionalAction,
                        help="draw the depth map as a point cloud under the boxes of the novel view, tinted per box")
    parser.add_argument("--segmentation", choices=("none", "rle"), default="none",
                        help="rle: each record of <name>_dets.json gets \"segmentation\": {size, counts}, its mask as a COCO RLE string "
                             "(every mask source; encoded on the device)")
    parser.add_argument("--show-masks", action="store_true",
                        help="also write <name>_masks.jpg: the image with the kept instances' masks overlaid in the boxes' colours (alpha 0.5, contours)")
    add_ply_arguments(parser)
    parser.add_argument("opts", default=None, nargs=argparse.REMAINDER,
                        help="Modify config options by adding 'KEY VALUE' pairs at the end of the command.")
    return parser


def check_arguments(args, parser):
    """Exit status 2 for what cannot work, before any device call."""
    check_depth_arguments(args, parser, None, files_need_dir=True)
    check_mask_arguments(args, parser)
    if args.everything:
        if args.points_file or args.boxes_file:
            parser.error("--everything proposes its own masks: it takes neither --points-file nor --boxes-file")
        if args.mask != "sam":
            parser.error("--everything runs Segment Anything's automatic mask generator: it needs --mask sam, not --mask box")
        if not 1 <= args.points_per_side <= 36:
            parser.error("--points-per-side must be 1 .. 36 (3 candidates per point, 4096 rows in the NMS)")
    if args.points_file and args.mask != "sam":
        parser.error("--points-file prompts Segment Anything with the clicks: it needs --mask sam, not --mask box")
    if args.points_file and args.boxes_file:
        parser.error("--points-file and --boxes-file both replace the detector: give one")
    if not args.points_file and not args.labels_file and not args.everything:
        parser.error("the following arguments are required: --labels-file (or --points-file)")
    if args.mask == "sam" and not args.sam_weights:
        parser.error("--mask sam needs --sam-weights FILE")
    return args


def main():
    parser = argument_parser()
    args = check_arguments(parser.parse_args(), parser)
    print("Command Line Args:", args)
    cfg = make_cfg(args.config_file, args.opts)
    if not torch.cuda.is_available():
        raise SystemExit("OVMono3D-GEO runs on the HIP device (there is no CPU path)")
    with torch.no_grad():
        do_test(args, cfg)


if __name__ == "__main__":
    main()
