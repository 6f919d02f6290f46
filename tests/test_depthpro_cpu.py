"""Depth Pro without a GPU: the conditions on the reference that make the GPU comparison meaningful, the synthetic checkpoint's key
names against Hugging Face's model, the ABI mirror, the refusal of unsupported pyramids and the tool's arguments."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import depthpro_oracle as do
from common import ROOT

CASES = [do.TINY, do.GEOM]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_reference_is_decided_everywhere(case):
    """band = 4 x max |fp32 - fp64| of the canonical inverse depth: no fp64 pixel within the band of 0 (the head's last ReLU), no
    pixel of the scaled inverse depth at a clamp limit, field of view in [30, 100] degrees. No pixel is left out."""
    r64, r32, _, _ = do.reference_pair(case)
    band = 4.0 * float((r32["canonical"].double() - r64["canonical"]).abs().max())
    lo = float(r64["canonical"].min())
    print(f"{case['name']}: band {band:.3e}, canonical in [{lo:.4f}, {float(r64['canonical'].max()):.4f}], fov {float(r64['fov']):.3f}")
    assert lo > band
    for key in ("inv_est", "inv_given"):
        assert float(r64[key].min()) > 1e-4 and float(r64[key].max()) < 1e4, key
    assert 30.0 <= float(r64["fov"]) <= 100.0


def test_synthetic_checkpoint_loads_strictly_tiny():
    sd, _ = do.case_inputs(do.TINY)
    do.build_model(do.TINY["config"], sd, torch.float32)          # load_state_dict(strict=True) inside


def test_synthetic_checkpoint_matches_full_size_model_on_meta():
    """ViT-L towers: shapes only, nothing allocated."""
    from transformers import DepthProForDepthEstimation
    from ovmono3d_amd.depthpro import DEFAULT_CONFIG
    from ovmono3d_amd.util.synth_depthpro_weights import synth_depthpro_state_dict
    with torch.device("meta"):
        model = DepthProForDepthEstimation(do.hf_config(DEFAULT_CONFIG))
        sd = synth_depthpro_state_dict(DEFAULT_CONFIG, seed=0)
    want = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in sd.items()}
    assert got == want, (sorted(set(want) ^ set(got))[:8], [k for k in want if k in got and want[k] != got[k]][:8])


def test_package_does_not_import_transformers():
    code = "import sys; import ovmono3d_amd.depthpro, ovmono3d_amd.util.synth_depthpro_weights; assert 'transformers' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))


def test_abi_size_of_config_matches_mirror():
    from ovmono3d_amd import lib
    assert lib.load().ovm_abi_sizeof(b"OvmDepthProConfig") == C.sizeof(lib.OvmDepthProConfig) == 4 * 5 + 8 + 4 + 12 + 8 + 12 + 12 + 4 * 4 + 4


def test_device_wiring_restated_in_torch_matches_hugging_face():
    """The order the device code works in (csrc/depthpro.hip), restated with torch fp64 ops on the TINY case: crops as views of the three
    pyramid levels (high resolution first), merge by the merged-cell rule + bilinear resize, low-resolution | image halves of the
    concatenation, hook i -> upsample chain i, the fusion plumbing, the field-of-view neck on the tokens before the reshape."""
    import torch.nn.functional as F
    r64, _, sd, _ = do.reference_pair(do.TINY)
    cfg = do.TINY["config"]
    c, D = cfg["crop"], cfg["embed_dim"]
    g = c // 16
    m = do.build_model(cfg, sd, torch.float64)
    W = {k: v.double() for k, v in sd.items()}
    P = [r64["pyramid0"], r64["pyramid1"], r64["pyramid2"]]
    ncrop, stride, pad = [5, 3, 1], [int(c * 0.75), c // 2, c], [min(g // 4, 3), min(g // 4, 6), 0]
    crops = [P[l][i * stride[l]:i * stride[l] + c, j * stride[l]:j * stride[l] + c].permute(2, 0, 1)
             for l in range(3) for i in range(ncrop[l]) for j in range(ncrop[l])]
    with torch.no_grad():
        enc = m.depth_pro.encoder.patch_encoder.model(torch.stack(crops), output_hidden_states=True)
        taps = [enc.hidden_states[h + 1] for h in cfg["hook_ids"]]
        whole = P[2].permute(2, 0, 1)[None]
        tok_i = m.depth_pro.encoder.image_encoder.model(whole).last_hidden_state
        tok_f = m.fov_model.fov_encoder.model(whole).last_hidden_state

    def cell(mm, n, pd):
        if n == 1 or mm < g - pd:
            return 0, mm
        r, w = mm - (g - pd), g - 2 * pd
        i = min(1 + r // w, n - 1)
        return i, pd + r - (i - 1) * w

    def merge(tok, crop0, l):
        n, pd = ncrop[l], pad[l]
        ms, out = (g if n == 1 else n * g - 2 * (n - 1) * pd), g << (2 - l)
        M = torch.zeros(ms, ms, D, dtype=torch.float64)
        for y in range(ms):
            cy, ly = cell(y, n, pd)
            for x in range(ms):
                cx, lx = cell(x, n, pd)
                M[y, x] = tok[crop0 + cy * n + cx, 1 + ly * g + lx]
        if ms != out:
            M = F.interpolate(M.permute(2, 0, 1)[None], size=(out, out), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
        return M

    def close(a, b, name):
        assert float((a - b).abs().max() / b.abs().max()) < 1e-12, name

    feats = [merge(tok_i, 0, 2), merge(enc.last_hidden_state, 34, 2), merge(enc.last_hidden_state, 25, 1), merge(enc.last_hidden_state, 0, 0),
             merge(taps[0], 0, 0), merge(taps[1], 0, 0)]
    for i, f in enumerate(feats):
        close(f, r64[f"features{i}"], f"features{i}")
    nchw, nhwc = (lambda t: t.permute(2, 0, 1)[None]), (lambda t: t[0].permute(1, 2, 0))
    ct = lambda t, k: F.conv_transpose2d(t, W[k + ".weight"], W.get(k + ".bias"), stride=2)                      # noqa: E731
    cv = lambda t, k, p=0, s=1: F.conv2d(t, W[k + ".weight"], W.get(k + ".bias"), padding=p, stride=s)           # noqa: E731
    U = "depth_pro.neck.feature_upsample."
    img_up = ct(nchw(feats[0]), U + "image_block.layers.0")
    low_up = ct(cv(nchw(feats[1]), U + "scaled_images.0.layers.0"), U + "scaled_images.0.layers.1")
    up = [cv(torch.cat([low_up, img_up], 1), "depth_pro.neck.fuse_image_with_low_res")]
    for i in (1, 2):
        up.append(ct(cv(nchw(feats[i + 1]), U + f"scaled_images.{i}.layers.0"), U + f"scaled_images.{i}.layers.1"))
    for i in (0, 1):
        t = cv(nchw(feats[4 + i]), U + f"intermediate.{i}.layers.0")
        for k in range(2 + i):
            t = ct(t, U + f"intermediate.{i}.layers.{1 + k}")
        up.append(t)
    neck = [cv(up[i], f"depth_pro.neck.feature_projection.projections.{i}", 1) for i in range(4)] + [up[4]]
    for i, f in enumerate(neck):
        close(nhwc(f), r64[f"neck{i}"], f"neck{i}")

    def unit(x, p):
        return x + cv(F.relu(cv(F.relu(x), p + ".convolution1", 1)), p + ".convolution2", 1)

    hid = None
    for i in range(5):
        p = f"fusion_stage.intermediate.{i}" if i < 4 else "fusion_stage.final"
        hs = neck[i] if i == 0 else hid + unit(neck[i], p + ".residual_layer1")
        y = unit(hs, p + ".residual_layer2")
        hid = cv(ct(y, p + ".deconv") if i < 4 else y, p + ".projection")
    close(nhwc(hid), r64["fused"], "fused")
    h = ct(cv(hid, "head.layers.0", 1), "head.layers.1")
    close(F.relu(cv(F.relu(cv(h, "head.layers.2", 1)), "head.layers.4"))[0, 0], r64["canonical"], "canonical")
    fovf = (tok_f[0] @ W["fov_model.fov_encoder.neck.weight"].T + W["fov_model.fov_encoder.neck.bias"])[1:].reshape(g, g, -1)
    x0 = F.relu(cv(neck[0], "fov_model.conv", 1, 2)) + nchw(fovf)
    for i in range(2):
        x0 = F.relu(cv(x0, f"fov_model.head.layers.{2 * i}", 1, 2))
    close(cv(x0, "fov_model.head.layers.4").flatten(), r64["fov"], "fov")


@pytest.mark.parametrize("change", [dict(ratios=(0.25, 0.5, 0.75)), dict(overlaps=(0.0, 0.25, 0.25)), dict(ratios=(0.5, 1.0, 1.0))])
def test_unsupported_pyramid_is_refused_before_any_device_call(change):
    from ovmono3d_amd import lib
    from ovmono3d_amd.depthpro import build_depthpro, check_config, depthpro_config
    cfg = dict(do.TINY["config"], **change)
    with pytest.raises(lib.OvmError) as e:
        check_config(depthpro_config(cfg))
    assert "unsupported pyramid" in str(e.value) and "0.25 / 0.5 / 1" in str(e.value)
    with pytest.raises(lib.OvmError) as e:                       # the constructor refuses before it touches the device or the weights
        build_depthpro({}, device=torch.device("cuda", 0), config=cfg)
    assert "unsupported pyramid" in str(e.value)
    h = C.c_void_p()
    assert lib.load().ovm_depthpro_create(C.byref(depthpro_config(cfg)), None, 0, 0, C.byref(h)) == -6
    assert b"unsupported pyramid" in lib.load().ovm_depthpro_last_error(h)
    lib.load().ovm_depthpro_destroy(h)


def _tool():
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ovmono3d_geo
    return ovmono3d_geo


BASE_ARGS = ["--oracle2d", "o.json", "--dataset", "d.json", "--mask", "box", "--output", "out.pth"]


def test_tool_accepts_depthpro_without_depth_dir():
    tool = _tool()
    parser = tool.argument_parser()
    args = tool.check_args(parser.parse_args(BASE_ARGS + ["--depth", "depthpro", "--depthpro-weights", "w.pt", "--image-root", "."]), parser)
    assert args.depth == "depthpro" and args.depth_dir is None and args.depthpro_focal == "estimate" and args.dump_depth is None
    args = tool.check_args(parser.parse_args(BASE_ARGS + ["--depth-dir", "depth"]), parser)          # an existing invocation
    assert args.depth == "files" and args.depth_dir == "depth"
    with pytest.raises(SystemExit):                                # a directory that would be ignored is refused, not dropped silently
        tool.check_args(parser.parse_args(BASE_ARGS + ["--depth", "depthpro", "--depthpro-weights", "w.pt", "--depth-dir", "depth"]), parser)


def test_tool_still_rejects_files_without_depth_dir(capsys):
    tool = _tool()
    parser = tool.argument_parser()
    for extra in ([], ["--depth", "files"]):
        with pytest.raises(SystemExit) as e:
            tool.check_args(parser.parse_args(BASE_ARGS + extra), parser)
        assert e.value.code == 2 and "--depth-dir" in capsys.readouterr().err
