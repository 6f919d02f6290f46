#!/usr/bin/env python3
"""Writes tests/golden/dinov2_plain_control.npz: the pyramid of the PLAIN vittest14 backbone as the library built from the checked-out
commit computes it on the GPU, for a bit-for-bit control (tests/test_gpu_dinov2_variants.py::test_plain_model_bit_identical_to_fixture).

The committed fixture was written at the commit BEFORE the register-token / SwiGLU variants went in, so it pins that the variant work
left every launch of a plain model as it was. Regenerate only at a commit whose plain-model arithmetic is meant to change.
p4 is stored whole; p2 and p3 (too large to commit) as SHA-256 digests of their fp32 bytes.
Run from the repo root on a GPU:  python tests/golden/make_dinov2_control.py [--lib path/to/libovm3d.so]
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from common import build_cfg, synth_inputs  # noqa: E402
from ovmono3d_amd.util.synth_weights import synth_state_dict  # noqa: E402

SEED_W, SEED_IN, HW = 21, 22, ((140, 196), (224, 168))


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def features():
    """Pyramid levels as contiguous NHWC fp32 tensors, plain vittest14 at canvas 224, two images of different size."""
    from ovmono3d_amd.modeling import build_model
    cfg = build_cfg("vittest14", 224, "f16x3", max_batch=2)
    model = build_model(cfg)
    model.load_state_dict(synth_state_dict("vittest14", seed=SEED_W))
    inputs = synth_inputs(2, hw=HW, n_boxes=4, seed=SEED_IN)
    model.backbone.export_features = True
    feats = model.backbone(model.preprocess_image(inputs))
    torch.cuda.synchronize()
    return {k: feats[k].permute(0, 2, 3, 1).contiguous() for k in ("p2", "p3", "p4")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "dinov2_plain_control.npz"))
    a = ap.parse_args()
    if a.lib:
        from ovmono3d_amd import lib
        lib.LIB_PATH = os.path.abspath(a.lib)
    f = features()
    sd = synth_state_dict("vittest14", seed=SEED_W)
    keys = sorted(sd)[:: max(1, len(sd) // 16)]
    np.savez_compressed(a.out, weights_seed=np.array(SEED_W), inputs_seed=np.array(SEED_IN),
                        weights_fp=np.array([float(sd[k].double().sum()) for k in keys]),
                        p4=f["p4"].cpu().numpy(), p2_sha256=np.array(digest(f["p2"])), p3_sha256=np.array(digest(f["p3"])))
    print("wrote", a.out, {k: tuple(v.shape) for k, v in f.items()})


if __name__ == "__main__":
    main()
