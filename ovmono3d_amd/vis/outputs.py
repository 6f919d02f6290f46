"""What the demos write per image beside ``<name>_dets.json``: ``write_views`` (``<name>_combine.jpg`` or ``<name>_boxes.jpg``) and
``write_scene`` (``<name>_scene.ply``, with the flags of ``add_ply_arguments``), for demo/demo.py and demo/demo_geo.py alike."""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch


def scene_depth(depth, h, w, im_name):
    """The depth map as draw_scene_view(depth=...) takes it: fp32 [h, w]. A map of another size is not a picture of this image."""
    if depth is None:
        return None
    if torch.is_tensor(depth):
        depth = depth.detach().to(torch.float32)
    else:
        depth = np.ascontiguousarray(depth, dtype=np.float32)
    if depth.ndim == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if tuple(depth.shape) != (h, w):
        raise SystemExit(f"--show-points / --scene-ply: the depth map of {im_name} is {tuple(depth.shape)} but the image is {(h, w)}")
    return depth


def write_views(im, K, dets, kept_idx, output_dir, im_name, gpu_jpeg=True, depth=None, labels=None):
    """demo.py:89-121: the kept boxes drawn (front + novel view, scale = H) into <name>_combine.jpg, else <name>_boxes.jpg.
    gpu_jpeg: a picture on the device is encoded there (data/gpu_jpeg.py write_jpeg; the same bytes as the host's Image.save).
    depth: fp32 [H, W] metric depth of the image, drawn as a point cloud under the boxes of the novel view; labels: int32 [H, W], the
    position in ``dets`` of the box a pixel belongs to or -1 (vis.labels_from_masks), tints the points. Both None: the reference's picture."""
    from .. import vis
    from ..data.gpu_jpeg import write_jpeg
    if len(dets) > 0:
        corners = np.asarray([d["corners3D"] for d in dets], np.float64)
        colors = np.asarray([[c / 255.0 for c in vis.get_color(i)] for i in kept_idx], np.float32)
        text = ["{} {:.2f}".format(d["category"], d["score"]) for d in dets]
        points = {} if depth is None else {"depth": depth, "point_labels": labels}
        front, novel = vis.draw_scene_view(im, K, corners, colors, text=text, scale=int(im.shape[0]), blend_weight=0.5,
                                           blend_weight_overlay=0.85, **points)
        bgr, name = vis.concat_views(front, novel), im_name + "_combine.jpg"
    else:
        bgr, name = im, im_name + "_boxes.jpg"
    write_jpeg(os.path.join(output_dir, name), bgr, quality=95, channel_order="BGR", use_device=gpu_jpeg)


def write_scene(args, im, K, dets, kept_idx, output_dir, im_name, depth=None, labels=None):
    """--scene-ply: <name>_scene.ply, the boxes of ``dets`` in the colours of <name>_combine.jpg over the un-projected depth map (fp32
    [H, W] or None: boxes only), its points tinted by ``labels`` as in the picture. Only the point records leave the device."""
    from .. import vis
    corners = np.asarray([d["corners3D"] for d in dets], np.float64).reshape(-1, 8, 3)
    colors = np.asarray([[c / 255.0 for c in vis.get_color(i)] for i in kept_idx], np.float32).reshape(-1, 3)
    vis.write_scene_ply(os.path.join(output_dir, im_name + "_scene.ply"), im, K, depth=depth, corners=corners, colors=colors,
                        point_labels=labels if depth is not None else None, stride=args.ply_stride, max_depth=args.ply_max_depth,
                        frame=args.ply_frame)


def _positive_float(text):
    v = float(text)
    if not (v > 0 and v != float("inf")):
        raise argparse.ArgumentTypeError(f"{text!r} is not a positive finite number")
    return v


def add_ply_arguments(parser):
    """--scene-ply and its settings; a value out of range is an argparse error (exit status 2)."""
    parser.add_argument("--scene-ply", default=False, action=argparse.BooleanOptionalAction,
                        help="(native build) also write <name>_scene.ply: the kept boxes and, where the run has a depth map, its un-projected "
                             "points as a binary PLY file")
    parser.add_argument("--ply-stride", type=int, default=1, choices=range(1, 17), metavar="N",
                        help="--scene-ply: keep every N-th row and column of the depth map (1..16, default 1)")
    parser.add_argument("--ply-max-depth", type=_positive_float, default=None, metavar="M", help="--scene-ply: drop points farther than M metres")
    parser.add_argument("--ply-frame", choices=("camera", "opengl"), default="camera",
                        help="--scene-ply: camera (x right, y down, z forward, as <name>_dets.json) or opengl (y and z negated)")
