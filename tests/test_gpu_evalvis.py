"""GPU: ovm_render_panels (ovmono3d_amd/csrc/panels.hip) against the numpy restatement tests/panels_oracle.py, and
visualize_from_instances end to end.

Every byte of the mosaic is equal outside the oracle's line band (pixel centres within 1e-3 px of a line's radius, exact ties
excluded - see panels_oracle.render), and the band pixels that differ are at most 0.1 % of the mosaic (the cap of
tests/test_gpu_render.py). tests/test_evalvis_cpu.py checks that the band itself stays below that share on these scenes."""
import os

import numpy as np
import pytest
import torch

import panels_oracle as po

pytestmark = pytest.mark.gpu

CATS = list(po.NAMES)


def image(H, W):
    return np.random.default_rng(H * 1000 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)


def scenes():
    """(name, H, W, (K, gt_all, gt_eval, preds)): seeded scenes at the three sizes, and the constructed edge cases."""
    out = []
    for H, W in ((96, 128), (250, 334), (120, 161)):
        for n_gt, n_pred in ((12, 20), (4, 3)):
            out.append((f"seeded {n_gt}+{n_pred} {H}x{W}", H, W, po.make_scene(2000 + 31 * n_gt + n_pred + H, n_gt, n_pred, H, W)))
    for H, W in ((96, 128), (60, 81), (250, 334)):
        out += [(f"{k} {H}x{W}", H, W, v) for k, v in po.constructed(H, W).items()]
    return out


def _check(dev, ref, band, what):
    assert dev.shape == ref.shape and dev.dtype == np.uint8, what
    off = (dev != ref).any(-1)
    bad = off & ~band
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ outside the line band (first at {np.argwhere(bad)[:3].tolist()})"
    assert (off & band).sum() <= 1e-3 * off.size, f"{what}: {int((off & band).sum())} band pixels differ"


def _render(img, scene, **kw):
    from ovmono3d_amd import vis
    K, gt_all, gt_eval, preds = scene
    out = vis.render_panels(torch.from_numpy(img).cuda() if isinstance(img, np.ndarray) else img, K, gt_all, gt_eval, preds, **kw)
    torch.cuda.synchronize()
    return out


def test_panels_match_oracle():
    for what, H, W, scene in scenes():
        img = image(H, W)
        ref, band = po.render(img, po.layout(scene[0], H, W, *scene[1:]))
        out = _render(img, scene)
        assert out.is_cuda and tuple(out.shape) == (2 * H, 3 * W, 3)
        _check(out.cpu().numpy(), ref, band, what)


def test_padded_row_pitches_and_second_call():
    H, W = 120, 161
    scene = po.make_scene(2000 + 31 * 12 + 20 + H, 12, 20, H, W)
    img = image(H, W)
    ref, band = po.render(img, po.layout(scene[0], H, W, *scene[1:]))
    src = torch.full((H, W + 5, 3), 7, dtype=torch.uint8, device="cuda")
    src[:, :W] = torch.from_numpy(img).cuda()
    buf = torch.full((2 * H, 3 * W + 11, 3), 201, dtype=torch.uint8, device="cuda")
    out = _render(src[:, :W], scene, out=buf[:, :3 * W])
    assert out.data_ptr() == buf.data_ptr() and out.stride(0) == 3 * (3 * W + 11)
    _check(out.cpu().numpy(), ref, band, "padded pitch")
    assert bool((buf[:, 3 * W:] == 201).all()), "the padding of the mosaic's rows was written"
    first = out.clone()
    again = _render(src[:, :W], scene, out=buf[:, :3 * W])                   # same buffers, same stream
    assert torch.equal(again, first)
    assert torch.equal(_render(img, scene), first)                           # and from packed buffers


def test_twenty_labels_on_one_spot():
    """The blend is sequential and truncates after every label: 20 rectangles over one spot give the oracle's bytes."""
    H, W = 250, 334
    K = po.intrinsics(H, W)
    one = po.box(K, 1, [0.0, 0.0, 4.0], [1.0, 1.0, 1.0], 0.3, bbox=[140.0, 150.0, 30.0, 20.0])
    gts = [dict(one, category_id=c % 9) for c in range(20)]                      # one name (one rectangle), nine colours
    img = image(H, W)
    scene = (K, gts, [True] * 20, gts)
    panels = po.layout(K, H, W, *scene[1:])
    rects = {p[1:5] for p in panels[3] if p[0] == "blend"}
    assert len(rects) == 1 and len([p for p in panels[3] if p[0] == "blend"]) == 20  # 20 rectangles with one corner
    x0, y0, x1, y1 = rects.pop()
    ref, band = po.render(img, panels)
    once, _ = po.render(img, po.layout(K, H, W, gts[-1:], [True], gts[-1:]))
    assert (ref[H + y0:H + y1, x0:x1] != once[H + y0:H + y1, x0:x1]).any()       # the bytes depend on the labels below the last
    _check(_render(img, scene).cpu().numpy(), ref, band, "20 labels")


def test_panel_isolation_and_empty_lists():
    H, W = 96, 128
    K, gt_all, gt_eval, preds = po.make_scene(11, 0, 9, H, W)
    img = image(H, W)
    out = _render(img, (K, [], [], preds)).cpu().numpy()
    for p in (0, 1, 3, 4):                                                       # the four ground-truth panels: the input image
        r, c = divmod(p, 3)
        assert np.array_equal(out[r * H:(r + 1) * H, c * W:(c + 1) * W], img), f"panel {p}"
    assert (out[:H, 2 * W:] != img).any() and (out[H:, 2 * W:] != img).any()
    out = _render(img, (K, [], [], [])).cpu().numpy()
    assert np.array_equal(out, np.tile(img, (2, 3, 1)))


def test_visualize_from_instances_end_to_end(tmp_path):
    from PIL import Image
    from ovmono3d_amd import vis
    H, W, n = 64, 96, 51
    rng = np.random.default_rng(3)
    records, dets = [], []
    for i in range(n):
        path = str(tmp_path / f"img_{i:03d}.jpg")
        yy, xx = np.mgrid[0:H, 0:W]
        Image.fromarray(np.stack([xx * 2 + i, yy * 3, xx + yy], -1).astype(np.uint8)).save(path, quality=90)
        K, gt_all, _, preds = po.make_scene(300 + i, 3, 4, H, W)
        annos = [{k: b[k] for k in ("category_id", "bbox", "center_cam", "dimensions", "pose")} for b in gt_all]
        insts = []
        for a, p in zip(gt_all, preds):                                          # predictions near the first ground-truth boxes
            z = a["center_cam"][2] + 0.25
            insts.append({"category_id": a["category_id"], "score": float(rng.uniform(0.2, 1.0)), "bbox": [v + 1.0 for v in a["bbox"]],
                          "center_2D": [a["bbox"][0] + a["bbox"][2] / 2, a["bbox"][1] + a["bbox"][3] / 2], "center_cam": [0.0, 0.0, z],
                          "dimensions": p["dimensions"], "pose": p["pose"]})
        records.append({"file_name": path, "image_id": i, "annotations": annos})
        dets.append({"image_id": i, "K": K.tolist(), "height": H, "width": W, "instances": insts})
    ds = vis.SampleDataset(records)
    out_dir = tmp_path / "out"
    s = vis.visualize_from_instances(dets, ds, "SYNTH_test", 512, str(out_dir), CATS, CATS[:5], "final", every=50)
    files = sorted(os.listdir(out_dir / "vis"))
    assert files == ["SYNTH_test_000000.jpg", "SYNTH_test_000050.jpg"]
    for f in files:
        with Image.open(out_dir / "vis" / f) as im:
            assert im.size == (3 * W, 2 * H) == (288, 128) and im.mode == "RGB"
    cpu = vis.visualize_from_instances(dets, ds, "SYNTH_test", 512, str(tmp_path / "cpu"), CATS, CATS[:5], "final", every=0)
    assert s == cpu and "nan" not in s and s.startswith("SYNTH_testiter=final, xy(")
    assert os.listdir(tmp_path / "cpu" / "vis") == []
    # the picture that was written is the mosaic of that sample
    K, gt_all, gt_eval, preds = vis.panel_boxes(dets[50], records[50]["annotations"], CATS, CATS[:5])
    from ovmono3d_amd.data.gpu_jpeg import read_image_device
    bgr = read_image_device(records[50]["file_name"], "BGR", torch.device("cuda"))
    ref, band = po.render(bgr.cpu().numpy(), po.layout(K, H, W, gt_all, gt_eval, preds))
    _check(vis.render_panels(bgr, K, gt_all, gt_eval, preds).cpu().numpy(), ref, band, "sample 50")
    with Image.open(out_dir / "vis" / files[1]) as im:
        got = np.asarray(im)[:, :, ::-1].astype(np.int64)
    plain = np.tile(bgr.cpu().numpy(), (2, 3, 1)).astype(np.int64)
    drawn = (ref != plain).any(-1)                                               # JPEG at quality 95 of THAT mosaic: where something
    assert drawn.sum() > 500                                                     # was drawn, the file is nearer to it than to the input
    assert np.abs(got - ref)[drawn].mean() < np.abs(got - plain)[drawn].mean()
