"""DINOv2 register-token and SwiGLU variants on the GPU: the fused silu(gate) * value GEMM epilogue against fp64, the variant models
end to end against the fp32 checker of tests/dinov2_variants_oracle.py (pinned to Hugging Face's models in
tests/test_dinov2_variants_cpu.py), the depth-prompt refusal, and a bit-for-bit control of the plain model."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from common import GOLDEN, assert_close, build_cfg, oracle_params, rel_err, synth_inputs

import dinov2_variants_oracle as vo

pytestmark = pytest.mark.gpu

TOL = 1e-3
FIELDS = ("pred_boxes", "scores", "pred_bbox3D", "pred_center_cam", "pred_center_2D", "pred_dimensions", "pred_pose")


def _lib():
    from ovmono3d_amd import lib
    return lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _split_image(x):
    """fp32 [rows][K] (K % 32 == 0) -> interleaved split image [rows][K/32][hi 32 | lo 32] (fp16)."""
    L = _lib()
    hi, lo = torch.empty_like(x, dtype=torch.float16), torch.empty_like(x, dtype=torch.float16)
    assert L.ovm_op_split_f16(x.data_ptr(), x.numel(), hi.data_ptr(), lo.data_ptr(), _stream()) == 0
    out = torch.empty(x.shape[0], 2 * x.shape[1], dtype=torch.float16, device=x.device)
    assert L.ovm_op_interleave(hi.data_ptr(), lo.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), _stream()) == 0
    return out


def _join_image(img, K):
    """interleaved split image [rows][2 K] -> (hi + lo as fp32 [rows][K], hi, lo)."""
    v = img.view(img.shape[0], K // 32, 2, 32)
    hi, lo = v[:, :, 0, :].reshape(-1, K), v[:, :, 1, :].reshape(-1, K)
    return hi.float() + lo.float(), hi, lo


@functools.lru_cache(maxsize=1)
def _swiglu_case(M, Hs, K):
    """Operands, the fp64 reference and the error of the UNFUSED path (ovm_op_gemm storing the 2 Hs wide fp32 product, SiLU and product
    in torch fp32, a split_f16 round trip) for one shape; shared by the routes of that shape."""
    dev = torch.device("cuda")
    L = _lib()
    g = torch.Generator().manual_seed(M + 3 * Hs + K)
    A = torch.randn(M, K, generator=g).to(dev)
    # asymmetric: gates and values differ in scale and offset, and every row has its own scale, so a gate / value or row mispairing
    # is an O(1) error
    ramp = 0.5 + torch.arange(2 * Hs) % 7 / 6.0
    W = torch.randn(2 * Hs, K, generator=g) * ramp[:, None]
    W[:Hs] *= 2.0 / math.sqrt(K)
    W[Hs:] = W[Hs:] * (0.7 / math.sqrt(K)) + 0.3 / K
    bias = torch.randn(2 * Hs, generator=g) * 0.3
    W, bias = W.to(dev), bias.to(dev)
    h = A.double() @ W.double().T + bias.double()
    ref = torch.nn.functional.silu(h[:, :Hs]) * h[:, Hs:]
    # packed operands of the fused entry
    Kp = (Hs + 31) // 32 * 32
    perm = np.empty(2 * Kp, np.int32)
    assert L.ovm_host_swiglu_perm(Hs, perm.ctypes.data) == 0
    pt = torch.from_numpy(perm.astype(np.int64)).to(dev)
    rows = (2 * Kp + 255) // 256 * 256
    Wp = torch.zeros(rows, K, device=dev)
    Wp[: 2 * Kp] = torch.where(pt[:, None] >= 0, W[pt.clamp_min(0)], torch.zeros((), device=dev))
    bp = torch.where(pt >= 0, bias[pt.clamp_min(0)], torch.zeros((), device=dev)).contiguous()
    a_img, w_img = _split_image(A), _split_image(Wp)
    # unfused
    Wu = torch.zeros((2 * Hs + 127) // 128 * 128, K, device=dev)
    Wu[: 2 * Hs] = W
    wu_img = _split_image(Wu)
    prod = torch.empty(M, 2 * Hs, device=dev)
    assert L.ovm_op_gemm(a_img.data_ptr(), a_img.data_ptr() + 64, 2 * K, wu_img.data_ptr(), wu_img.data_ptr() + 64, M, 2 * Hs, K,
                         bias.data_ptr(), 0, prod.data_ptr(), 2 * Hs, 3, _stream()) == 0
    y = (torch.nn.functional.silu(prod[:, :Hs]) * prod[:, Hs:]).contiguous()
    hi, lo = torch.empty_like(y, dtype=torch.float16), torch.empty_like(y, dtype=torch.float16)
    assert L.ovm_op_split_f16(y.data_ptr(), y.numel(), hi.data_ptr(), lo.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    unfused = rel_err(hi.float() + lo.float(), ref)
    return a_img, w_img, bp, ref, Kp, unfused


@pytest.mark.parametrize("M,Hs,K,force256", [(130, 344, 128, False), (4101, 1024, 384, False), (1370, 4096, 1536, False),
                                              (1370, 4096, 1536, True)])
def test_gemm_swiglu_vs_fp64(device, M, Hs, K, force256):
    """ovm_op_gemm_swiglu (precision 3, interleaved activations in and out) against fp64 silu(g) * u.

    (130, 344, 128): ragged N, Kpad 352, one row of tiles plus 2 leftover rows; (4101, 1024, 384): five leftover rows on the
    wave-specialised 128-tile kernel (512 tiles); (1370, 4096, 1536): the ViT-g shape at canvas 518, once on the default route of the
    entry (704 tiles: the symmetric 128-tile kernel) and once forced onto the 256 x 256 kernel (the route the engine takes for it).

    Bound: test_gemm_store's precision-3 bound max(2e-6, 3e-8 sqrt(K)); only if the unfused path on the same inputs exceeds that bound
    does it become twice the unfused error. Unfused path measured on MI355X (max|a-b| / max|b|): 3.887e-07 at (130, 344, 128),
    7.329e-07 at (4101, 1024, 384), 1.394e-06 at (1370, 4096, 1536) - all inside the bound, so it is 2e-6 for every case; the fused
    kernel gave the same figures to four digits (same MFMA sequence, fp32 SiLU in both). Both figures are printed on every run. The
    bound never comes from the fused kernel."""
    L = _lib()
    a_img, w_img, bp, ref, Kp, unfused = _swiglu_case(M, Hs, K)
    bound = max(2e-6, 3e-8 * math.sqrt(K))
    tol = bound if unfused <= bound else 2.0 * unfused
    outs = []
    try:
        if force256:
            assert L.ovm_tune_set(b"op_gemm256", 1) == 0
        for _ in range(3):
            out = torch.full((M, 2 * Kp), float("nan"), dtype=torch.float16, device=device)
            rc = L.ovm_op_gemm_swiglu(a_img.data_ptr(), a_img.data_ptr() + 64, 2 * K, w_img.data_ptr(), w_img.data_ptr() + 64, M, Hs, K,
                                      bp.data_ptr(), out.data_ptr(), out.data_ptr() + 64, 2 * Kp, 3, _stream())
            assert rc == 0
            outs.append(out)
        torch.cuda.synchronize()
    finally:
        L.ovm_tune_set(b"op_gemm256", 0)
    y, hi, lo = _join_image(outs[0], Kp)
    err = rel_err(y[:, :Hs], ref)
    print(f"swiglu {M}x{Hs}x{K} force256={force256}: fused {err:.3e} unfused {unfused:.3e} tol {tol:.3e}")
    assert not torch.isnan(outs[0]).any(), "the epilogue left part of the activation image unwritten"
    if Kp > Hs:
        assert torch.all(hi[:, Hs:] == 0) and torch.all(lo[:, Hs:] == 0), "pad columns [Hs, Kpad) must be written as zeros"
    assert err <= tol, f"fused {err:.3e} > {tol:.3e} (unfused {unfused:.3e})"
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), "launches differ bit for bit"


def test_gemm_swiglu_plain_output_arrays(device):
    """Same entry with separate hi / lo output arrays (ldo = Kp) and plain activation arrays."""
    L = _lib()
    M, Hs, K = 67, 40, 64
    g = torch.Generator().manual_seed(5)
    A = torch.randn(M, K, generator=g).to(device)
    W = (torch.randn(2 * Hs, K, generator=g) / 8).to(device)
    Kp = 64
    perm = np.empty(2 * Kp, np.int32)
    assert L.ovm_host_swiglu_perm(Hs, perm.ctypes.data) == 0
    Wp = torch.zeros(128, K, device=device)
    for n, s in enumerate(perm.tolist()):
        if s >= 0:
            Wp[n] = W[s]
    w_img = _split_image(Wp)
    ah, al = torch.empty_like(A, dtype=torch.float16), torch.empty_like(A, dtype=torch.float16)
    assert L.ovm_op_split_f16(A.data_ptr(), A.numel(), ah.data_ptr(), al.data_ptr(), _stream()) == 0
    hi = torch.full((M, Kp), float("nan"), dtype=torch.float16, device=device)
    lo = torch.full((M, Kp), float("nan"), dtype=torch.float16, device=device)
    assert L.ovm_op_gemm_swiglu(ah.data_ptr(), al.data_ptr(), K, w_img.data_ptr(), w_img.data_ptr() + 64, M, Hs, K, None,
                                hi.data_ptr(), lo.data_ptr(), Kp, 3, _stream()) == 0
    torch.cuda.synchronize()
    h = A.double() @ W.double().T
    ref = torch.nn.functional.silu(h[:, :Hs]) * h[:, Hs:]
    assert_close((hi.float() + lo.float())[:, :Hs], ref, 2e-6, "swiglu plain arrays")
    assert torch.all(hi[:, Hs:] == 0) and torch.all(lo[:, Hs:] == 0)
    # a too-short output row is refused, not overrun
    assert L.ovm_op_gemm_swiglu(ah.data_ptr(), al.data_ptr(), K, w_img.data_ptr(), w_img.data_ptr() + 64, M, Hs, K, None,
                                hi.data_ptr(), lo.data_ptr(), Kp - 32, 3, _stream()) == -4


# ------------------------------------------------------------------------------------------------ models
@pytest.fixture
def variant_oracle(monkeypatch):
    """oracle.pipeline.inference with the variant-aware ViT forward in place of oracle.vit.dino_backbone_forward."""
    import oracle.vit
    from oracle.pipeline import inference
    monkeypatch.setattr(oracle.vit, "dino_backbone_forward", vo.dino_backbone_forward)
    return inference


def _build(cfg, seed=1):
    from ovmono3d_amd.modeling import build_model
    from ovmono3d_amd.util.synth_weights import synth_state_dict
    sd = synth_state_dict(cfg.MODEL.DINO.MODEL_NAME, num_classes=cfg.MODEL.ROI_HEADS.NUM_CLASSES, seed=seed)
    model = build_model(cfg)
    model.load_state_dict(sd)
    return model, sd


def _compare(out, ref, tol=TOL):
    assert len(out) == len(ref)
    for o, r in zip(out, ref):
        inst = o["instances"]
        assert len(inst) == len(r["scores"])
        assert torch.equal(inst.pred_classes.cpu(), r["pred_classes"].to(torch.int64)), "category indices differ"
        for f in FIELDS:
            got = inst.get(f)
            got = got.tensor if hasattr(got, "tensor") else got
            if r[f].numel():
                assert_close(got, r[f], tol, f)


@pytest.mark.parametrize("name", ["vittest14_reg", "vitgtest14", "vitgtest14_reg"])
def test_oracle2d_tiny_variants(device, variant_oracle, name):
    cfg = build_cfg(name, 224, "f16x3", max_batch=2)
    model, sd = _build(cfg)
    inputs = synth_inputs(2, hw=((140, 196), (224, 168)), n_boxes=12, seed=3)
    out = model(inputs)
    ref, aux = variant_oracle(sd, inputs, oracle_params(cfg), return_aux=True)
    model.backbone.export_features = True
    feats = model.backbone(model.preprocess_image(inputs))
    for k in ("p2", "p3", "p4"):
        assert_close(feats[k], aux["features"][k], 2e-4, k)
    _compare(out, ref)


def test_one_pass_precision_tiny_variant(device, variant_oracle):
    """f16 mode (plain fp16 operands and activation images, no lo parts) through both variants: same categories, floats within the
    looser band test_fast_precision_runs uses for the plain towers."""
    cfg = build_cfg("vitgtest14_reg", 224, "f16", max_batch=1)
    model, sd = _build(cfg)
    inputs = synth_inputs(1, n_boxes=8, seed=7)
    out = model(inputs)
    ref = variant_oracle(sd, inputs, oracle_params(cfg))
    _compare(out, ref, tol=5e-2)


def test_rpn_route_tiny_register_model(device, variant_oracle):
    cfg = build_cfg("vittest14_reg", 224, "f16x3", max_batch=2)
    model, sd = _build(cfg, seed=21)
    inputs = synth_inputs(2, hw=((168, 210), (224, 224)), n_boxes=0, seed=24, oracle2d=False)
    out = model(inputs)
    ref = variant_oracle(sd, inputs, oracle_params(cfg))
    assert len(out[0]["instances"]) > 0
    _compare(out, ref)


def test_vitg_width_depth2_canvas518(device, variant_oracle):
    """ViT-g width (D = 1536, Hs = 4096) at depth 2, canvas 518 (T = 1370). The w12 GEMM is M = 1370, N = 8192: 6 x 32 = 192 tiles of
    256 x 256, the dispatcher's threshold, so it runs on the 256-tile kernel with EPI_SWIGLU (csrc/tower.hip gemm()); with the
    "gemm256" tune key off it runs on the 128-tile kernels, and both must give the oracle's answer. The profile shows the two w12
    launches under the fc1 category."""
    L = _lib()
    cfg = build_cfg("vitg14_d2", 518, "f16x3", max_batch=1, max_rois=64)
    model, sd = _build(cfg, seed=2)
    inputs = synth_inputs(1, hw=((512, 384),), orig_scale=1.25, n_boxes=32, seed=4)
    torch.set_num_threads(16)
    ref, aux = variant_oracle(sd, inputs, oracle_params(cfg), return_aux=True)
    model.engine.profile_enable(True)
    out = model(inputs)
    prof = model.engine.profile_read()
    model.engine.profile_enable(False)
    assert prof["fc1"][1] == 2 and prof["fc2"][1] == 2 and prof["qkv"][1] == 2
    _compare(out, ref)
    model.backbone.export_features = True
    try:
        assert L.ovm_tune_set(b"gemm256", 0) == 0
        feats = model.backbone(model.preprocess_image(inputs))
        for k in ("p2", "p3", "p4"):
            assert_close(feats[k], aux["features"][k], 2e-4, f"128-tile route {k}")
    finally:
        L.ovm_tune_set(b"gemm256", 1)
    feats = model.backbone(model.preprocess_image(inputs))
    for k in ("p2", "p3", "p4"):
        assert_close(feats[k], aux["features"][k], 2e-4, f"256-tile route {k}")


def test_vitl_registers_depth2_canvas896(device, variant_oracle):
    """ViT-L width with 4 registers at canvas 896: T = 4101, five leftover queries per head and five leftover GEMM rows."""
    cfg = build_cfg("vitl14_reg_d2", 896, "f16x3", max_batch=1, max_rois=64)
    model, sd = _build(cfg, seed=4)
    inputs = synth_inputs(1, hw=((896, 672),), orig_scale=1.0, n_boxes=24, seed=12)
    out = model(inputs)
    torch.set_num_threads(16)
    ref = variant_oracle(sd, inputs, oracle_params(cfg))
    _compare(out, ref)


def test_vitb14_reg_canvas518(device, variant_oracle):
    """The reference's named register model (dino.py:17-24 'vitb14_reg')."""
    cfg = build_cfg("vitb14_reg", 518, "f16x3", max_batch=1)
    model, sd = _build(cfg, seed=2)
    inputs = synth_inputs(1, hw=((512, 384),), orig_scale=1.25, n_boxes=32, seed=4)
    out = model(inputs)
    torch.set_num_threads(16)
    ref = variant_oracle(sd, inputs, oracle_params(cfg))
    _compare(out, ref)


# ------------------------------------------------------------------------------------- refusals and controls
def test_register_model_refuses_prompt_depth(device):
    """The reference's fusion takes x[:, 1:] as the patch tokens (dino.py:91-105): with registers its torch.cat raises. Loading a
    register checkpoint that carries depth_fusion.* is fine; giving it a depth prompt is refused by the plugin and by the library."""
    from ovmono3d_amd.lib import OvmError
    cfg = build_cfg("vittest14_reg", 224, "f16x3", max_batch=1)
    model, sd = _build(cfg, seed=5)
    assert "backbone.net.depth_fusion.weight" in sd
    inputs = synth_inputs(1, hw=((160, 224),), n_boxes=4, seed=31, depth=True)
    assert len(model(inputs)) == 1
    with pytest.raises(ValueError, match="register-token model"):
        model(inputs, prompt_depth=torch.stack([x["depth"] for x in inputs]))
    native, _keep = model.engine.make_images(inputs)
    with pytest.raises(OvmError, match="register-token model"):
        model.engine.backbone_forward(native, 1, inputs[0]["depth"][None])


def test_plain_model_bit_identical_to_fixture(device):
    """The plain vittest14 pyramid equals, bit for bit, what the library computed before the variants went in
    (tests/golden/dinov2_plain_control.npz, written by tests/golden/make_dinov2_control.py at that commit): with no register tokens and
    the GELU MLP every launch gets the arguments it got then."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_dinov2_control", os.path.join(GOLDEN, "make_dinov2_control.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    z = np.load(os.path.join(GOLDEN, "dinov2_plain_control.npz"))
    from ovmono3d_amd.util.synth_weights import synth_state_dict
    sd = synth_state_dict("vittest14", seed=int(z["weights_seed"]))
    keys = sorted(sd)[:: max(1, len(sd) // 16)]
    assert np.allclose([float(sd[k].double().sum()) for k in keys], z["weights_fp"], rtol=1e-9, atol=1e-9), "synthetic weight stream changed"
    f = mk.features()
    assert np.array_equal(f["p4"].cpu().numpy(), z["p4"]), "p4 differs from the fixture"
    assert mk.digest(f["p3"]) == str(z["p3_sha256"]) and mk.digest(f["p2"]) == str(z["p2_sha256"])
