#!/usr/bin/env python3
"""Detector-alone timing of the GroundingDINO engine on synthetic weights: Swin-B or Swin-T backbone, the headline's 532 x 532 image and
6-category caption.

    python tools/bench_gdino.py --arch swinb|swint [--steps 50] [--warmup 10] [--rounds 3] [--fused 0,1] [--kernels]

One engine is built per value of ``--fused`` (the ``gdino_swin_fused`` knob while its plan is built: 0 = qkv GEMM + window attention as
two launches, 1 = the projection inside the window kernel). After ``--warmup`` forwards of each (plan built, graph captured) the
engines are timed in turn, ``--rounds`` times over: ``--steps`` forwards between two HIP events on the stream, graph replay, nothing
else on the device. Reported per value: every round's milliseconds per forward, their median, and the kernel launches of one forward.

``--kernels`` adds the window kernel alone (``ovm_g_swin_qkv_attn``, random operands) at the four stage shapes of the 532 x 532 image
(windows x heads x C: 361 x 3 x 96, 100 x 6 x 192, 25 x 12 x 384, 9 x 24 x 768 at window 7; 144 x 4 x 128 ... at window 12): microseconds
per launch over 200 back-to-back launches between two events, per windows-per-workgroup choice. One JSON line is printed."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ovmono3d_amd import lib  # noqa: E402
from ovmono3d_amd.gdino.config import GDinoConfig  # noqa: E402
from ovmono3d_amd.gdino.detector import HashTokenizer  # noqa: E402
from ovmono3d_amd.gdino.engine import GdinoEngine  # noqa: E402
from ovmono3d_amd.util.synth_gdino_weights import synth_gdino_state_dict  # noqa: E402

CAPTION = "chair . dining table . sofa . potted plant . television . bookcase ."
HW = (532, 532)
MEAN, STD = [103.53, 116.28, 123.675], [57.375, 57.12, 58.395]


def _timed(fn, n, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(n):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / n


def bench_engines(cfg, device, fused_values, steps, warmup, rounds, seed):
    L = lib.load()
    sd = synth_gdino_state_dict(seed, cfg)
    ids = HashTokenizer().encode(CAPTION)
    img = torch.randint(0, 256, (3,) + HW, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(device)
    stream = torch.cuda.current_stream(device)
    engines = {}
    try:
        for v in fused_values:
            assert L.ovm_tune_set(b"gdino_swin_fused", v) == 0
            eng = GdinoEngine(device, sd, cfg, pixel_mean=MEAN, pixel_std=STD, flip_channels=True, use_graphs=True)
            for _ in range(warmup):                              # the first forward builds the plan under the knob's value
                eng.forward(img, ids)
            engines[v] = eng
    finally:
        L.ovm_tune_set(b"gdino_swin_fused", 1)
    torch.cuda.synchronize(device)
    ms = {v: [] for v in fused_values}
    for _ in range(rounds):
        for v in fused_values:                                   # alternate within the round
            ms[v].append(_timed(lambda e=engines[v]: e.forward(img, ids), steps, stream))
    return {str(v): {"ms_per_forward": [round(t, 4) for t in ms[v]], "median_ms": round(statistics.median(ms[v]), 4),
                     "launches": engines[v].launches()} for v in fused_values}


def bench_kernels(cfg, device, seed):
    """the fused window kernel alone at the stages' (windows, heads, C) of the 532 x 532 image"""
    L = lib.load()
    ws, T = cfg.swin_window, cfg.swin_window ** 2
    g = torch.Generator().manual_seed(seed)
    stream = torch.cuda.current_stream(device)
    sp = C.c_void_p(stream.cuda_stream)
    h = w = (HW[0] + 3) // 4
    out = []
    for i, nh in enumerate(cfg.swin_heads):
        Cc = cfg.swin_embed << i
        nW = ((h + ws - 1) // ws) * ((w + ws - 1) // ws)
        Kpad = (Cc + 63) // 64 * 64
        row = {"stage": i, "windows": nW, "heads": nh, "C": Cc}
        if Cc == 32 * nh and (ws == 7 or (ws == 12 and Cc % 128 == 0)):
            M = nW * T
            xh = (torch.randn(M, Kpad, generator=g) * 0.5).half().to(device)
            xl = (torch.randn(M, Kpad, generator=g) * 1e-4).half().to(device)
            xh[:, Cc:] = 0
            xl[:, Cc:] = 0
            frag = (torch.randn((3 * Cc + 127) // 128 * 128 * Kpad * 2, generator=g) * 0.05).half().to(device)
            bias = torch.zeros(3 * Cc, device=device)
            rel = (torch.randn(nh, T, T, generator=g) * 0.1).to(device)
            mask = torch.zeros(nW, T, T, device=device)
            ohi = torch.empty(M, Cc, dtype=torch.float16, device=device)
            olo = torch.empty_like(ohi)
            op = lib.OvmSwinQkvAttnOp()
            op.xhi, op.xlo, op.wfrag, op.bias, op.relbias, op.mask = (t.data_ptr() for t in (xh, xl, frag, bias, rel, mask))
            op.ohi, op.olo = ohi.data_ptr(), olo.data_ptr()
            op.ldx, op.KS, op.C, op.nh, op.nW, op.ldo, op.scale, op.ws = Kpad, Kpad // 32, Cc, nh, nW, Cc, 1.0 / math.sqrt(32.0), ws
            for wpg in ((1, 2, 4) if ws == 7 else (0,)):
                op.wpg = wpg

                def launch():
                    rc = L.ovm_g_swin_qkv_attn(C.byref(op), sp)
                    if rc != 0:
                        raise RuntimeError(f"ovm_g_swin_qkv_attn failed with code {rc}")
                for _ in range(20):
                    launch()
                torch.cuda.synchronize(device)
                row[f"us_wpg{wpg}"] = round(min(_timed(launch, 200, stream) for _ in range(3)) * 1e3, 2)
        out.append(row)
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", choices=("swinb", "swint"), default="swinb")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fused", default="0,1", help="comma separated values of gdino_swin_fused to alternate")
    ap.add_argument("--kernels", action="store_true", help="also time the fused window kernel alone at the four stage shapes")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gdino.py needs the GPU: there is no CPU path to time")
    device = torch.device("cuda", torch.cuda.current_device())
    cfg = GDinoConfig.swin_t() if args.arch == "swint" else GDinoConfig()
    res = {"arch": args.arch, "image": list(HW), "caption_tokens": len(HashTokenizer().encode(CAPTION)), "steps": args.steps,
           "rounds": args.rounds, "device": torch.cuda.get_device_name(device),
           "gdino_swin_fused": bench_engines(cfg, device, [int(v) for v in args.fused.split(",")], args.steps, args.warmup, args.rounds, args.seed)}
    if args.kernels:
        res["window_kernel"] = bench_kernels(cfg, device, args.seed)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
