"""The depth prompt of the DINOv2 tower's ``depth_fusion`` branch (reference cubercnn/modeling/backbone/dino.py:40-46,82-105), from
its sources to the tensor the model is handed.

Sources: ``.npz`` files made elsewhere (``load_depth``: ``<dir>/test/<image base name>.npz`` or ``<dir>/<image base name>.npz``, key
``depth``, metres - the files the reference's mapper reads, dataset_mapper.py:21,45-58), or ``DepthProPrompt``: Depth Pro on the device
(``ovmono3d_amd.depthpro``, csrc/depthpro.hip) on the image itself, which can also write those files (``dump_depth``).
``prepare_prompt_depth`` is the single place that turns a depth map into what the model takes: the two resizes of the reference's mapper
(to the image's size, dataset_mapper.py:45-52, then ResizeShortestEdge's, :70-72). ``DatasetMapper3D`` and ``demo/demo.py`` both call
it, so one image gets one prompt on either entry point, and the inline route gives the bits of the file route.

``add_depth_arguments`` / ``check_depth_arguments`` are the command-line flags of this choice, declared here alone, for
``demo/demo.py``, ``tools/train_net.py`` and the two OVMono3D-GEO front ends (``tools/ovmono3d_geo.py``, ``demo/demo_geo.py``, which
lift the map instead of prompting a model with it); the checks run on the host, before any device call.
"""
from __future__ import annotations

import json
import os
from typing import Optional, Tuple

import numpy as np
import torch

SYNTHETIC_PREFIX = "synthetic://depthpro"


# ------------------------------------------------------------------------------------------ files
def dump_depth(depth_dir, file_path, depth):
    """The <image base name>.npz file load_depth reads."""
    os.makedirs(depth_dir, exist_ok=True)
    base = os.path.splitext(os.path.basename(file_path))[0]
    np.savez(os.path.join(depth_dir, base + ".npz"), depth=depth.cpu().numpy().astype(np.float32))


def load_depth(depth_dir, file_path, height=None, width=None):
    """float32 [H, W] of ``<depth_dir>/test/<base>.npz`` or ``<depth_dir>/<base>.npz``; ends the run naming the image when neither exists.
    With ``height`` and ``width`` a map of another shape is refused (OVMono3D-GEO: the reference never resizes it)."""
    base = os.path.splitext(os.path.basename(file_path))[0]
    for cand in (os.path.join(depth_dir, "test", base + ".npz"), os.path.join(depth_dir, base + ".npz")):
        if os.path.exists(cand):
            depth = np.load(cand)["depth"]
            if depth.ndim == 3 and depth.shape[0] == 1:
                depth = depth[0]
            if height is not None and tuple(depth.shape) != (height, width):
                raise SystemExit(f"{cand}: depth map is {tuple(depth.shape)} but the image is {(height, width)}; GEO needs the depth at "
                                 "the image's own resolution (the reference never resizes it)")
            return np.ascontiguousarray(depth, dtype=np.float32)
    raise SystemExit(f"no depth file for {file_path} under {depth_dir}")


# ------------------------------------------------------------------------------------------ the two resizes
def resize_to_image_host(depth: np.ndarray, image_hw) -> np.ndarray:
    """dataset_mapper.py:45-52 on the host: a stored map of another size than the image is interpolated to the image's."""
    if depth.shape[:2] != tuple(image_hw):
        depth = torch.nn.functional.interpolate(torch.from_numpy(depth)[None, None], size=tuple(image_hw),
                                                mode="bilinear", align_corners=False)[0, 0].numpy()
    return depth


def prepare_prompt_depth(depth, image_hw, resize) -> torch.Tensor:
    """depth: float32 [h, w] in metres, numpy or a tensor on either side; image_hw: the image's own (H, W), before ResizeShortestEdge;
    resize: ``DepthPromptResizeGPU`` (both resizes are device kernels, the result stays in HBM) or the host ``ResizeShortestEdge``
    (``F.interpolate`` on the CPU). Returns float32 [H', W'] at the network's input size: ``record["depth"]`` without its leading 1."""
    from .gpu_resize import DepthPromptResizeGPU
    image_hw = (int(image_hw[0]), int(image_hw[1]))
    if isinstance(resize, DepthPromptResizeGPU):
        if not torch.is_tensor(depth):
            depth = torch.from_numpy(np.ascontiguousarray(depth))
        return resize(depth.cuda(), image_hw)
    if torch.is_tensor(depth):
        depth = depth.detach().cpu().numpy()
    depth = resize_to_image_host(depth, image_hw)
    return torch.as_tensor(np.ascontiguousarray(resize(depth)))


# ------------------------------------------------------------------------------------------ Depth Pro as the source
class DepthProPrompt:
    """``source(image_hwc_u8, image_format, K, file_name=None)`` -> device fp32 [H, W] in metres: ``DepthPro.infer`` on the original-size
    image (a device tensor of any strides; a numpy image is uploaded). focal "estimate": the field-of-view head chooses the focal
    length (``f_px=None``); "K": ``float(K[0][0])``. With ``dump_dir`` the map is also written as ``<dump_dir>/<image base name>.npz``
    (``dump_depth``), which needs ``file_name``."""

    def __init__(self, depthpro, focal: str = "estimate", dump_dir: Optional[str] = None):
        if focal not in ("estimate", "K"):
            raise ValueError(f"focal must be 'estimate' or 'K', is {focal!r}")
        self.depthpro, self.focal, self.dump_dir = depthpro, focal, dump_dir

    def __call__(self, image_hwc_u8, image_format: str, K, file_name: Optional[str] = None) -> torch.Tensor:
        f_px = float(K[0][0]) if self.focal == "K" else None
        depth = self.depthpro.infer(image_hwc_u8, f_px=f_px, image_format=image_format)["depth"]
        if self.dump_dir:
            if not file_name:
                raise ValueError("DepthProPrompt(dump_dir=...) names the file after the image: pass file_name")
            dump_depth(self.dump_dir, file_name, depth)
        return depth


def synthetic_depthpro_spec(url: str) -> Tuple[int, Optional[int]]:
    """``synthetic://depthpro?seed=N&crop=C`` -> (seed, crop); ``seed`` absent: 0, ``crop`` absent: None (the configuration's)."""
    from urllib.parse import parse_qsl, urlsplit
    parts = urlsplit(url)
    if parts.scheme != "synthetic" or parts.netloc != "depthpro" or parts.path not in ("", "/"):
        raise ValueError(f"{url!r}: a synthetic Depth Pro checkpoint is written {SYNTHETIC_PREFIX}?seed=N&crop=C")
    vals = {"seed": 0, "crop": None}
    seen = set()
    for k, v in parse_qsl(parts.query, keep_blank_values=True, strict_parsing=bool(parts.query)):
        if k not in vals or k in seen:
            raise ValueError(f"{url!r}: unknown or repeated field {k!r} (seed, crop)")
        seen.add(k)
        try:
            vals[k] = int(v)
        except ValueError:
            raise ValueError(f"{url!r}: {k} must be an integer, is {v!r}") from None
    if vals["seed"] < 0 or (vals["crop"] is not None and vals["crop"] < 1):
        raise ValueError(f"{url!r}: seed must be >= 0 and crop >= 1")
    return vals["seed"], vals["crop"]


def build_depth_prompt(weights: str, focal: str = "estimate", config_json: Optional[str] = None, dump_dir: Optional[str] = None,
                       device: Optional[torch.device] = None) -> DepthProPrompt:
    """weights: a checkpoint file in Hugging Face key names (``build_depthpro``) or ``synthetic://depthpro?seed=N&crop=C`` (seeded random
    weights of the configuration, ``util/synth_depthpro_weights.py``); config_json: fields of ``depthpro.DEFAULT_CONFIG`` to override,
    as a JSON object. Precision is ``build_depthpro``'s default (1: the reference runs Depth Pro in half precision)."""
    from ..depthpro import DEFAULT_CONFIG, build_depthpro
    config = json.loads(config_json) if config_json else None
    if weights.startswith("synthetic://"):
        from ..util.synth_depthpro_weights import synth_depthpro_state_dict
        seed, crop = synthetic_depthpro_spec(weights)
        config = dict(config or {})
        if crop is not None:
            config["crop"] = crop
        full = dict(DEFAULT_CONFIG)
        full.update(config)
        checkpoint = synth_depthpro_state_dict(full, seed=seed)
    else:
        if not os.path.isfile(weights):
            raise FileNotFoundError(f"Depth Pro checkpoint {weights!r} not found (--depthpro-weights)")
        checkpoint = weights
    return DepthProPrompt(build_depthpro(checkpoint, device=device, config=config), focal=focal, dump_dir=dump_dir)


# ------------------------------------------------------------------------------------------ command line
def depth_prompt_unread(cfg) -> Optional[str]:
    """None when the model of ``cfg`` reads a depth prompt, else the setting that keeps it from doing so."""
    if cfg.MODEL.BACKBONE.NAME != "build_dino_backbone":
        return (f"MODEL.BACKBONE.NAME {cfg.MODEL.BACKBONE.NAME}: only build_dino_backbone has the depth-fusion branch "
                "(the reference raises for the other towers)")
    if not bool(cfg.MODEL.DINO.USE_DEPTH_FUSION):
        return "MODEL.DINO.USE_DEPTH_FUSION False: the backbone is built without the depth-fusion branch"
    if "_reg" in str(cfg.MODEL.DINO.MODEL_NAME):
        return (f"MODEL.DINO.MODEL_NAME {cfg.MODEL.DINO.MODEL_NAME}: depth fusion is not defined for a register-token model "
                "(it takes x[:, 1:] as the patch tokens)")
    return None


def add_depth_arguments(parser, choices=("files", "depthpro"), default="files", focal_help="the dataset's K[0][0]") -> None:
    """The depth flags of every entry point: the depth prompt of a model that owns a depth branch, or the map OVMono3D-GEO lifts."""
    what = {"none": "none: no depth prompt", "files": "files: read --depth-dir", "depthpro": "depthpro: run Depth Pro on the device on the image itself"}
    parser.add_argument("--depth", choices=tuple(choices), default=default,
                        help="(native build) where the metric depth comes from - the depth prompt of a depth-fusion checkpoint, or the map "
                             "OVMono3D-GEO lifts; " + "; ".join(what[c] for c in choices))
    parser.add_argument("--depth-dir", default=None, help="(native build) folder of depth-prompt .npz files (key 'depth', metres): "
                        "<dir>/test/<image base name>.npz; refused with --depth depthpro, which would not read it")
    parser.add_argument("--depthpro-weights", default=None, help="(native build) Depth Pro checkpoint in Hugging Face key names (torch file or "
                        f".safetensors), or {SYNTHETIC_PREFIX}?seed=N&crop=C for seeded random weights")
    parser.add_argument("--depthpro-focal", choices=("estimate", "K"), default="estimate",
                        help="(native build) estimate: the field-of-view head chooses the focal length; K: " + focal_help)
    parser.add_argument("--depthpro-config", default=None, metavar="JSON", help="(native build) fields of ovmono3d_amd.depthpro.DEFAULT_CONFIG to "
                        "override, as a JSON object: a checkpoint of another size than apple/DepthPro-hf")
    parser.add_argument("--dump-depth", default=None, metavar="DIR", help="(native build) with --depth depthpro: write the depth used as "
                        "<DIR>/<image base name>.npz, the files --depth-dir reads (from <DIR> or <DIR>/test)")


def check_depth_arguments(args, parser, make_cfg=None, files_need_dir: bool = False):
    """argparse errors (exit status 2) for the combinations that cannot work; host only. ``make_cfg()`` builds the configuration and is
    called only when a depth was asked for; None for an entry point without a model (OVMono3D-GEO lifts the depth itself): nothing
    is asked of a configuration."""
    if args.depth == "depthpro":
        if not args.depthpro_weights:
            parser.error("--depth depthpro needs --depthpro-weights FILE")
        if args.depth_dir:
            parser.error("--depth depthpro computes the depth: --depth-dir would not be read (to write depth files use --dump-depth DIR)")
        if args.depthpro_weights.startswith("synthetic://"):
            try:
                synthetic_depthpro_spec(args.depthpro_weights)
            except ValueError as e:
                parser.error(f"--depthpro-weights: {e}")
        if args.depthpro_config:
            try:
                if not isinstance(json.loads(args.depthpro_config), dict):
                    raise ValueError("not a JSON object")
            except ValueError as e:
                parser.error(f"--depthpro-config: {e}")
    elif args.dump_depth:
        parser.error("--dump-depth writes the depth that --depth depthpro computes")
    if args.depth == "files" and files_need_dir and not args.depth_dir:
        parser.error("--depth files needs --depth-dir DIR")
    if args.depth == "none" and args.depth_dir:
        parser.error("--depth-dir is read with --depth files")
    if make_cfg is not None and (args.depth == "depthpro" or (args.depth == "files" and files_need_dir)):
        why = depth_prompt_unread(make_cfg())
        if why:
            parser.error(f"--depth {args.depth}: nothing would read the depth ({why})")
    return args
