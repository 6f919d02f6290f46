"""GPU: ovm_render_scene (ovmono3d_amd/csrc/render.hip) against the numpy restatement tests/scene_oracle.py.

Every pixel is equal, or differs by at most 1 on a silhouette pixel (fp32 shading on the device, fp64 in the oracle, before
truncation), or lies in the oracle's ambiguity band (centre within 1e-3 px of a triangle edge or of a line's radius, or a depth
near-tie) - and such band pixels that differ are at most 0.1 % of the canvas. Labels use the same glyph masks on both sides."""
import numpy as np
import pytest
import torch

import scene_oracle as so

pytestmark = pytest.mark.gpu


def _check(dev, ref, band, sil, what):
    assert dev.shape == ref.shape, what
    d = np.abs(dev.astype(np.int64) - ref.astype(np.int64)).max(-1)
    off = d > 0
    shading = sil & (d <= 1)
    rest = off & ~shading
    assert not (rest & ~band).any(), f"{what}: {int((rest & ~band).sum())} pixels differ outside the tolerances " \
                                     f"(first at {np.argwhere(rest & ~band)[:3].tolist()}, max diff {int(d.max())})"
    assert (rest & band).sum() <= 1e-3 * d.size, f"{what}: {int((rest & band).sum())} band pixels differ"


def _run(seed, n, kind, H, W, scale=None, mode="front_and_novel", bw=0.5, bwo=0.85, labels=True, device_image=False):
    from ovmono3d_amd import vis
    scale = H if scale is None else scale
    corners, colors, K, kw = so.make_scene(seed, n, kind, H, W)
    img = np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    text = [f"obj{i} {((i * 37) % 100) / 100:.2f}" for i in range(n)] if labels else None
    bits = vis.MODES[mode]
    masks = [[vis.text_mask(t, 0.5 * hh / 500) if bits & on else np.zeros((0, 0), np.uint8) for t in text]
             for hh, on in ((H, so.FRONT), (scale, so.NOVEL))] if labels else None
    sizes = np.array([[(m.shape[1], m.shape[0]) for m in mv] for mv in masks]).reshape(2, n, 2) if labels else None
    bits = vis.MODES[mode]
    o = so.layout(corners, colors, K, H, W, scale, mode=bits, label_size=sizes, blend_weight=bw, blend_weight_overlay=bwo, **kw)
    f, nv, band, sil = so.render(o, o["grid"], img, masks)
    im = torch.from_numpy(img).cuda() if device_image else img
    out = vis.draw_scene_view(im, K, corners, colors, text=text, scale=scale, mode=mode, blend_weight=bw, blend_weight_overlay=bwo, **kw)
    torch.cuda.synchronize()
    outs = {"front": (out,), "novel": (out,), "front_and_novel": out}[mode]
    want = {"front": (0,), "novel": (1,), "front_and_novel": (0, 1)}[mode]
    refs = (f, nv)
    for t, v in zip(outs, want):
        assert t.is_cuda and t.dtype == torch.uint8
        _check(t.cpu().numpy(), refs[v], band[v], sil[v], f"seed {seed} n {n} {kind} {H}x{W} scale {scale} view {v}")
    return o, outs


SMALL = [(120, 160), (97, 131), (427, 640)]


@pytest.mark.parametrize("H,W", SMALL)
@pytest.mark.parametrize("kind", so.KINDS)
@pytest.mark.parametrize("n", (1, 7, 100))
def test_render_matches_oracle(H, W, kind, n):
    seed = 10_000 + 97 * n + 13 * so.KINDS.index(kind) + H
    o, _ = _run(seed, n, kind, H, W, scale=H if W != 131 else 150)
    if kind == "early":
        assert o["early_return"] == 1


@pytest.mark.parametrize("kind,n", (("plain", 100), ("crossing", 7)))
def test_render_full_hd(kind, n):
    _run(77, n, kind, 1080, 1920)


def test_render_modes_and_inputs():
    _run(5, 7, "plain", 120, 160, mode="front")
    _run(6, 7, "plain", 120, 160, mode="novel", scale=200)
    _run(7, 7, "crossing", 120, 160, bw=0.0, bwo=1.0, labels=False, device_image=True)
    _run(8, 0, "plain", 120, 160)                                  # no boxes: the input, and the bare (white) novel render


def test_views_share_one_buffer_when_scale_is_height():
    from ovmono3d_amd import vis
    _, (front, novel) = _run(9, 7, "plain", 120, 160)
    both = vis.concat_views(front, novel)
    assert both.shape == (120, 280, 3) and both.data_ptr() == front.data_ptr()
    assert torch.equal(both[:, 160:], novel)
