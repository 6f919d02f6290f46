#!/usr/bin/env python3
"""Times Depth Pro (ovm_depthpro_infer, csrc/depthpro.hip) on one 1536-wide image with synthetic ViT-L weights, both precisions.

    python tools/bench_depthpro.py [--runs 7] [--warmup 2] [--yardstick] [--small]

Device times are HIP event times around the call alone (image and workspace resident, no read inside), warm, median of the runs.
With ``--yardstick`` the same network - Hugging Face DepthProForDepthEstimation (tests/depthpro_oracle.py) with the same weights,
eager torch on the same card - is timed the same way, preprocessing and post-processing on the device included: fp16 against
precision 1, fp32 against precision 3. ``--small`` swaps in the test architecture (towers of width 128) for a quick check of the
tool itself. One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ovmono3d_amd.depthpro import DEFAULT_CONFIG, build_depthpro  # noqa: E402
from ovmono3d_amd.util.synth_depthpro_weights import synth_depthpro_state_dict  # noqa: E402

H, W = 1024, 1536
# the architecture of the tests (towers of width 128) at the real crop geometry: --small
SMALL = dict(embed_dim=128, depth=4, heads=2, hook_ids=(3, 1), fusion_dim=64, scaled_dims=(128, 128, 64), inter_dims=(64, 64))


def make_image(h, w, seed):
    g = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 128 + 60 * np.sin(xx / 37.0)[..., None] * np.cos(yy / 23.0)[..., None] + g.normal(0, 12, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def event_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick", action="store_true", help="also time Hugging Face DepthProForDepthEstimation, eager torch on this card")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--small", action="store_true", help="the test architecture instead of ViT-L")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "Depth Pro needs the GPU"
    dev = torch.device("cuda", 0)
    config = dict(DEFAULT_CONFIG, **SMALL) if a.small else dict(DEFAULT_CONFIG)
    sd = synth_depthpro_state_dict(config, seed=7)
    img_np = make_image(H, W, seed=6)
    img = torch.from_numpy(img_np).to(dev)
    out = {"image": [H, W], "canvas": 4 * config["crop"], "embed_dim": config["embed_dim"], "depth": config["depth"]}
    depth = {}
    for prec in (1, 3):
        eng = build_depthpro(sd, device=dev, precision=prec, config=config)
        ws = torch.empty(eng.workspace_bytes(H, W), dtype=torch.uint8, device=dev)
        out[f"p{prec}_workspace_mb"] = round(ws.numel() / 2 ** 20, 1)
        out[f"p{prec}_infer_ms"] = round(event_ms(lambda: eng.infer(img, workspace=ws), a.runs, a.warmup), 3)
        eng.profile(True)                                          # the stage split, from separate profiled calls (events between the stages)
        splits = []
        for _ in range(a.runs):
            r = eng.infer(img, workspace=ws)
            splits.append(eng.stage_ms())
        eng.profile(False)
        out[f"p{prec}_stage_ms"] = {k: round(statistics.median(x[k] for x in splits), 3) for k in eng.STAGES}
        depth[prec] = r["depth"].clone()
        out[f"p{prec}_fov_deg"] = round(float(r["fov_deg"]), 4)
        del eng, ws
        torch.cuda.empty_cache()
    out["p1_vs_p3_rel"] = float((depth[1] - depth[3]).abs().max() / depth[3].abs().max())
    if a.yardstick:
        import torch.nn.functional as F
        sys.path.insert(0, os.path.join(ROOT, "tests"))            # the Hugging Face model is built by the tests' checker
        import depthpro_oracle as do
        for name, dtype, prec in (("fp16", torch.float16, 1), ("fp32", torch.float32, 3)):
            model = do.build_model(config, sd, torch.float32).to(dev).to(dtype)
            S = out["canvas"]

            @torch.no_grad()
            def full():
                x = (img.permute(2, 0, 1)[None].to(dtype) / 255.0 - 0.5) / 0.5
                x = F.interpolate(x, size=(S, S), mode="bilinear", align_corners=False)
                o = model(pixel_values=x)
                f = 0.5 * W / torch.tan(0.5 * torch.deg2rad(o.field_of_view.float().reshape(())))
                inv = F.interpolate((o.predicted_depth.float() * W / f)[None], size=(H, W), mode="bilinear", align_corners=False)[0, 0]
                return 1.0 / torch.clamp(inv, min=1e-4, max=1e4)

            out[f"torch_{name}_infer_ms"] = round(event_ms(full, a.runs, a.warmup), 3)
            ref = full()
            out[f"p{prec}_vs_torch_{name}_rel"] = float((depth[prec] - ref).abs().max() / ref.abs().max())
            del model
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
