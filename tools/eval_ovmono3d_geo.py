#!/usr/bin/env python3
"""Evaluates OVMono3D-GEO prediction files (tools/ovmono3d_geo.py) with the Omni3D evaluator, as the reference's
tools/eval_ovmono3d_geo.py does: its filter settings (visibility and truncation 1/3, min height 0.0625, max height 1.5, max depth
1e8, the ignore names) and its list of 22 novel categories.

    python tools/eval_ovmono3d_geo.py --predictions KITTI_test_novel=output/ovmono3d_geo/KITTI_test_novel.pth \\
        SUNRGBD_test_novel=output/ovmono3d_geo/SUNRGBD_test_novel.pth --datasets-root datasets/Omni3D \\
        --category-meta configs/category_meta.json --output-dir output/ovmono3d_geo

Each prediction file is the list of per-image records ``[{image_id, ..., instances[{image_id, category_id, bbox, score, bbox3D,
depth, center_cam, dimensions, pose, center_2D}]}]``, .pth (torch.save) or .json. ``category_id`` is mapped through
``--category-meta`` exactly as tools/train_net.py maps the model's class index. Written: ``<output-dir>/<dataset>/omni_ap.json``
per dataset and ``<output-dir>/omni_ap_all.json`` over all of them with the collective summary.
"""
import argparse
import json
import logging
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ovmono3d_amd.evaluation import Omni3DGroundTruth, collective_summary, evaluate_omni3d  # noqa: E402
from train_net import category_map_for, uses_proximity  # noqa: E402

logger = logging.getLogger("eval_ovmono3d_geo")

NOVEL_CATEGORIES = ["monitor", "bag", "dresser", "board", "printer", "keyboard", "painting", "drawers", "microwave", "computer", "kitchen pan",
                    "potted plant", "tissues", "rack", "tray", "toys", "phone", "podium", "cart", "soundsystem", "fireplace", "tram"]


def geo_filter_settings():
    """The settings of the reference script (tools/eval_ovmono3d_geo.py:62-63,109-119)."""
    return {"visibility_thres": 0.33333333, "truncation_thres": 0.33333333, "min_height_thres": 0.0625, "max_depth": 100000000.0,
            "category_names": list(NOVEL_CATEGORIES), "ignore_names": ["dontcare", "ignore", "void"], "trunc_2D_boxes": True,
            "modal_2D_boxes": False, "max_height_thres": 1.5}


def load_predictions(path):
    if not os.path.exists(path):
        raise FileNotFoundError(f"Prediction file not found: {path}")
    if path.endswith(".json"):
        with open(path) as f:
            return json.load(f)
    return torch.load(path, map_location="cpu", weights_only=False)


def run(args):
    pairs = []
    for item in args.predictions:
        name, sep, path = item.partition("=")
        if not sep:
            raise SystemExit(f"--predictions takes NAME=FILE, got {item!r}")
        pairs.append((name, path))
    all_files, all_dets, prox_images, written = [], [], set(), {}
    stage3d = "host" if args.only_2d else args.eval_3d                         # no 3D pass, no 3D stages
    matcher = "device" if stage3d == "device" else args.eval_matcher          # the 3D stages ride in the device matcher's upload
    for name, path in pairs:
        gt_file = os.path.join(args.datasets_root, name + ".json")
        dets = [inst for rec in load_predictions(path) for inst in rec["instances"]]
        gt = Omni3DGroundTruth(gt_file, geo_filter_settings())
        all_files.append(gt_file)
        all_dets += dets
        prox = args.eval_prox and uses_proximity(name)
        if prox:
            prox_images |= set(gt.image_ids)
        logger.info("%s: %d detections, %d ground-truth boxes", name, len(dets), len(gt))
        if len(gt):
            cmap = category_map_for(None, "novel", gt, args.category_meta)
            ap = evaluate_omni3d(gt, dets, category_map=cmap, eval_prox=prox, matcher=matcher, stage3d=stage3d, only_2d=args.only_2d)
            os.makedirs(os.path.join(args.output_dir, name), exist_ok=True)
            written[name] = os.path.join(args.output_dir, name, "omni_ap.json")
            with open(written[name], "w") as f:
                json.dump(ap, f)
            with open(os.path.join(args.output_dir, name, "category_meta.json"), "w") as f:
                json.dump(cmap.to_meta(), f)
    gt = Omni3DGroundTruth(all_files, geo_filter_settings())
    if len(gt):
        ap = evaluate_omni3d(gt, all_dets, category_map=category_map_for(None, "novel", gt, args.category_meta), eval_prox=prox_images,
                             matcher=matcher, stage3d=stage3d, only_2d=args.only_2d)
        ap["collective"] = collective_summary(ap)
        os.makedirs(args.output_dir, exist_ok=True)
        written["all"] = os.path.join(args.output_dir, "omni_ap_all.json")
        with open(written["all"], "w") as f:
            json.dump(ap, f)
        logger.info("all %d datasets: %s", len(all_files), json.dumps(ap["collective"]))
    return written


def argument_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--predictions", nargs="+", required=True, metavar="NAME=FILE", help="dataset name = prediction file (.pth or .json)")
    ap.add_argument("--datasets-root", default="datasets/Omni3D", help="folder of the <NAME>.json annotation files")
    ap.add_argument("--category-meta", default=None, help="category_meta.json-style file: thing_classes + thing_dataset_id_to_contiguous_id")
    ap.add_argument("--output-dir", default="output/ovmono3d_geo")
    ap.add_argument("--eval-prox", action="store_true", help="upstream Omni3D's proximity rule for SUNRGBD / Objectron, as tools/train_net.py")
    ap.add_argument("--eval-matcher", choices=("host", "device"), default="host")
    ap.add_argument("--eval-3d", choices=("host", "device"), default="host", help="the evaluator's 3D IoU and NHD stages in HIP; implies "
                    "--eval-matcher device")
    ap.add_argument("--only-2d", action="store_true", help="AP2D only (needs no GPU; the 3D IoU runs on the device)")
    return ap


def main():
    logging.basicConfig(level=logging.INFO)
    print(json.dumps(run(argument_parser().parse_args())))


if __name__ == "__main__":
    main()
