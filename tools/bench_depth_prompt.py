#!/usr/bin/env python3
"""Times the text-prompted model step with a depth prompt: DINOv2-L + SFP + ROIHeads3DGDINO on one 512 x 512 image (network input
532 x 532 on the 896 canvas, bench.py's headline shapes), Depth Pro at its real size, synthetic weights everywhere.

    python tools/bench_depth_prompt.py [--runs 9] [--warmup 3] [--small] [--json FILE]

Legs, driven through ``model(...)`` on the same image and boxes, in one process, alternated round by round (leg 1, 2, 3, 4, then
again), each step between two HIP events, warm, median over the rounds:

  none            no prompt (ovm_infer, one C call)
  resident        a prompt already in HBM at the network's input size: the file route without its disk read (ovm_infer_depth)
  inline          Depth Pro on the image, prepare_prompt_depth, then the step: ``--depth depthpro``
  resident_staged leg 2 with MODEL.AMD.FUSED_INFER False: the stages sequenced from Python, which is how a prompted step ran before
                  ovm_infer_depth existed

``one_call`` reports for each leg whether the step went through the one-call path. ``--small`` swaps in the test-size main model and
Depth Pro for a quick check of the tool itself. One JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ovmono3d_amd.data.depth_prompt import build_depth_prompt, prepare_prompt_depth  # noqa: E402
from ovmono3d_amd.data.gpu_resize import DepthPromptResizeGPU  # noqa: E402
from ovmono3d_amd.defaults import make_cfg  # noqa: E402
from ovmono3d_amd.modeling import build_model  # noqa: E402
from ovmono3d_amd.util.synth_weights import synth_state_dict  # noqa: E402

CATEGORIES = ("chair", "dining table", "sofa", "potted plant", "television", "bookcase")
SMALL_DEPTHPRO = dict(embed_dim=128, depth=4, heads=2, hook_ids=(3, 1), fusion_dim=64, scaled_dims=(128, 128, 64), inter_dims=(64, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9, help="rounds; every round runs each leg once")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="vittest14 on a 224 canvas and the test-size Depth Pro")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    arch, canvas, net, orig = ("vittest14", 224, 140, 128) if a.small else ("vitl14", 896, 532, 512)
    sd = synth_state_dict(arch, seed=0)

    def make_model(fused, detector=None):
        cfg = make_cfg("OVMono3D_dinov2_SFP.yaml", ["MODEL.DINO.MODEL_NAME", arch, "MODEL.FPN.SQUARE_PAD", canvas, "MODEL.AMD.GEMM_PRECISION", "f16x3",
                                                    "MODEL.AMD.MAX_BATCH", 1, "MODEL.AMD.MAX_ROIS", 1000, "MODEL.ROI_HEADS.NAME", "ROIHeads3DGDINO",
                                                    "MODEL.AMD.GDINO_WEIGHTS", "synthetic://gdino?seed=0", "MODEL.AMD.FUSED_INFER", fused])
        m = build_model(cfg, device=dev)
        m.load_state_dict(sd)
        if detector is None:
            m.roi_heads.load_detector()
        else:
            m.roi_heads.detector = detector                          # one detector serves both models (they never run at the same time)
        calls = []
        inner = m.engine.infer_gdino

        def counted(*args, **kw):
            calls.append(kw.get("prompt_depth") is not None)
            return inner(*args, **kw)
        m.engine.infer_gdino = counted
        return m, calls

    model, calls = make_model(True)
    staged, staged_calls = make_model(False, model.roi_heads.detector)
    source = build_depth_prompt("synthetic://depthpro?seed=7", "estimate", json.dumps(SMALL_DEPTHPRO) if a.small else None, None, dev)
    g = torch.Generator().manual_seed(1000)
    net_img = torch.randint(0, 256, (3, net, net), dtype=torch.uint8, generator=g).to(dev)
    orig_img = torch.randint(0, 256, (orig, orig, 3), dtype=torch.uint8, generator=g).to(dev)       # what Depth Pro reads: the original-size image
    K = [[2.0 * orig, 0.0, orig / 2], [0.0, 2.0 * orig, orig / 2], [0.0, 0.0, 1.0]]                 # demo.py:63-76 focal 4.0*h/2
    inputs = [{"image": net_img, "height": orig, "width": orig, "K": K, "image_id": 0, "category_list": list(CATEGORIES)}]
    resize = DepthPromptResizeGPU(net, net)

    def prompt():
        return prepare_prompt_depth(source(orig_img, "BGR", K), (orig, orig), resize)[None, None]

    resident = prompt().clone()
    legs = {"none": lambda: model(inputs), "resident": lambda: model(inputs, prompt_depth=resident),
            "inline": lambda: model(inputs, prompt_depth=prompt()), "resident_staged": lambda: staged(inputs, prompt_depth=resident)}
    ndet = {}
    for _ in range(a.warmup):
        for k, fn in legs.items():
            ndet[k] = len(fn()[0]["instances"])
    torch.cuda.synchronize()
    one_call = {}
    times = {k: [] for k in legs}
    for _ in range(a.runs):
        for k, fn in legs.items():
            del calls[:], staged_calls[:]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
            one_call[k] = len(calls) + len(staged_calls) == 1
    out = {"model": arch, "canvas": canvas, "net_res": net, "image": [orig, orig], "depthpro_canvas": source.depthpro.canvas, "rounds": a.runs,
           "detections": ndet, "one_call": one_call}
    for k, ts in times.items():
        out[f"{k}_ms"] = round(statistics.median(ts), 3)
        out[f"{k}_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
    # round by round, so that drift between rounds cancels
    out["inline_minus_resident_ms"] = round(statistics.median(i - r for i, r in zip(times["inline"], times["resident"])), 3)
    out["resident_minus_none_ms"] = round(statistics.median(r - n for r, n in zip(times["resident"], times["none"])), 3)
    out["staged_minus_one_call_ms"] = round(statistics.median(s - r for s, r in zip(times["resident_staged"], times["resident"])), 3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    alone = []
    for _ in range(a.runs):                                          # Depth Pro and the two resizes alone, for the comparison
        e0.record()
        prompt()
        e1.record()
        e1.synchronize()
        alone.append(e0.elapsed_time(e1))
    out["depthpro_and_resizes_alone_ms"] = round(statistics.median(alone), 3)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
