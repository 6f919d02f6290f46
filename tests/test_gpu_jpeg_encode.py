"""GPU: the device JPEG encoder (ovmono3d_amd/csrc/jpeg_enc.hip) against Pillow = libjpeg-turbo, live and byte for byte, on the
cases of tests/jpeg_enc_ref.py (whose conditions tests/test_jpeg_encode_cpu.py asserts on the oracle alone)."""
import ctypes as C
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_enc_ref as R
from ovmono3d_amd import lib as _lib
from ovmono3d_amd.data import gpu_jpeg

pytestmark = pytest.mark.gpu

SUB = {2: "4:2:0", 0: "4:4:4"}


def _dev(arr, device):
    return torch.from_numpy(np.array(arr)).to(device)                # a copy: the shared case pictures are read-only


def _first_diff(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return f"lengths {len(a)} / {len(b)}, first differing byte {int(d[0]) if len(d) else n}"


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_forward_coefficients_equal_pillows(device, case):
    """Stages 1-2 (colour, edges, downsampling, FDCT, quantisation, dummy blocks): the planes Pillow's file decodes to."""
    rgb, ref = R.case(*case)
    want, info = gpu_jpeg.entropy_decode(ref)
    got = gpu_jpeg.jpeg_forward(_dev(rgb, device), case[3], SUB[case[4]]).cpu()
    assert got.shape == want.shape and got.dtype == torch.int16
    bad = (got != want).any(1).nonzero().flatten()
    assert len(bad) == 0, f"{len(bad)} of {len(want)} blocks differ, first {bad[:4].tolist()} (planes start at 0, " \
                          f"{info.bw[0] * info.bh[0]}, {info.bw[0] * info.bh[0] + info.bw[1] * info.bh[1]})"


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_encode_equals_pillow(device, case):
    rgb, ref = R.case(*case)
    got = gpu_jpeg.encode_jpeg(_dev(rgb, device), case[3], SUB[case[4]])
    assert got == ref, _first_diff(got, ref)


@pytest.mark.parametrize("h,w", [(37, 53), (250, 333)])
def test_input_forms(device, h, w):
    rgb = R.picture("noise", h, w, seed=3)
    ref = R.pillow_bytes(rgb, 95, 2)
    x = _dev(rgb, device)
    assert gpu_jpeg.encode_jpeg(x) == ref
    bgr = x.flip(-1).contiguous()                                    # BGR memory, read with a negative channel stride
    assert gpu_jpeg.encode_jpeg(bgr, channel_order="BGR") == ref
    assert gpu_jpeg.encode_jpeg(bgr) == R.pillow_bytes(np.ascontiguousarray(rgb[:, :, ::-1]), 95, 2)
    big = torch.randint(0, 256, (h + 3, w + 5, 3), dtype=torch.uint8, device=device)
    big[3:, 5:] = x
    crop = big[3:, 5:]
    assert not crop.is_contiguous() and gpu_jpeg.encode_jpeg(crop) == ref
    pitched = torch.zeros((h, 3 * w + 13), dtype=torch.uint8, device=device)
    view = pitched[:, :3 * w].view(h, w, 3)
    view.copy_(x)
    assert view.stride(0) == 3 * w + 13 and gpu_jpeg.encode_jpeg(view) == ref
    planar = x.permute(2, 0, 1).contiguous().permute(1, 2, 0)        # channel stride h * w
    assert planar.stride(2) == h * w and gpu_jpeg.encode_jpeg(planar, 75, "4:4:4") == R.pillow_bytes(rgb, 75, 0)


def test_repeat_and_second_size(device):
    """Two calls give equal bytes; a picture of another size through the same path is right too (no state is left behind)."""
    a, ra = R.case("noise", 250, 333, 95, 2)
    b, rb = R.case("coco", 480, 640, 95, 2)
    c, rc = R.case("noise", 17, 9, 95, 2)
    xa = _dev(a, device)
    first = gpu_jpeg.encode_jpeg(xa)
    assert first == ra and gpu_jpeg.encode_jpeg(xa) == first
    assert gpu_jpeg.encode_jpeg(_dev(b, device)) == rb
    assert gpu_jpeg.encode_jpeg(_dev(c, device)) == rc
    assert gpu_jpeg.encode_jpeg(xa) == first


def test_round_trip_through_the_device_decoder(device):
    rgb, ref = R.case("coco", 480, 640, 95, 2)
    data = gpu_jpeg.encode_jpeg(_dev(rgb, device))
    with Image.open(io.BytesIO(ref)) as im:
        want = np.asarray(im.convert("RGB"))
    assert np.array_equal(gpu_jpeg.decode_jpeg(data, device).cpu().numpy(), want)


def test_capacity_one_byte_short_is_refused_and_launches_nothing(device):
    L = _lib.load()
    rgb = R.picture("noise", 37, 53)
    x = _dev(rgb, device)
    info = _lib.OvmJpegEncInfo()
    hdr = (C.c_uint8 * 640)()
    assert L.ovm_host_jpeg_encode_plan(53, 37, 95, 2, C.byref(info), hdr, 640) == 0
    wsb, cap = C.c_int64(), C.c_int64()
    assert L.ovm_jpeg_encode_workspace(C.byref(info), C.byref(wsb), C.byref(cap)) == 0
    ws = torch.full((wsb.value,), 0x5a, dtype=torch.uint8, device=device)
    out = torch.full((cap.value,), 0x5a, dtype=torch.uint8, device=device)
    n = torch.full((1,), -7, dtype=torch.int64, device=device)
    args = (x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), C.byref(info), hdr, ws.data_ptr())
    assert L.ovm_jpeg_encode(*args, ws.numel(), out.data_ptr(), cap.value - 1, n.data_ptr(), None) == -5
    assert L.ovm_jpeg_encode(*args, ws.numel() - 1, out.data_ptr(), cap.value, n.data_ptr(), None) == -5
    torch.cuda.synchronize()
    assert int(n.item()) == -7 and bool((out == 0x5a).all()) and bool((ws == 0x5a).all())
    assert L.ovm_jpeg_encode(*args, ws.numel(), out.data_ptr(), cap.value, n.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert out[:int(n.item())].cpu().numpy().tobytes() == R.pillow_bytes(rgb, 95, 2)


def test_write_jpeg_and_render_panels_write_the_same_file_either_way(device, tmp_path):
    import panels_oracle as po
    import scene_oracle as so
    from ovmono3d_amd import vis
    H, W = 120, 160
    corners, colors, K, kw = so.make_scene(5, 7, "plain", H, W)
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(device)
    front, novel = vis.draw_scene_view(img, K, corners, colors, text=[f"obj{i} 0.50" for i in range(7)], scale=H, blend_weight=0.5,
                                       blend_weight_overlay=0.85, **kw)
    pic = vis.concat_views(front, novel)
    assert pic.is_cuda and tuple(pic.shape) == (H, W + H, 3)
    gpu_jpeg.write_jpeg(str(tmp_path / "dev.jpg"), pic, quality=95, channel_order="BGR", use_device=True)
    gpu_jpeg.write_jpeg(str(tmp_path / "host.jpg"), pic, quality=95, channel_order="BGR", use_device=False)
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(pic.cpu().numpy()[:, :, ::-1])).save(b, format="JPEG", quality=95)
    assert (tmp_path / "dev.jpg").read_bytes() == (tmp_path / "host.jpg").read_bytes() == b.getvalue()
    Kp, gt_all, gt_eval, preds = po.make_scene(2000 + 31 * 4 + 3 + 96, 4, 3, 96, 128)
    im2 = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (96, 128, 3), dtype=np.uint8)).to(device)
    m1 = vis.render_panels(im2, Kp, gt_all, gt_eval, preds, save_path=str(tmp_path / "p_dev.jpg"), gpu_jpeg=True)
    m2 = vis.render_panels(im2, Kp, gt_all, gt_eval, preds, save_path=str(tmp_path / "p_host.jpg"), gpu_jpeg=False)
    assert torch.equal(m1, m2)
    assert (tmp_path / "p_dev.jpg").read_bytes() == (tmp_path / "p_host.jpg").read_bytes()
    with Image.open(tmp_path / "p_dev.jpg") as im:
        assert im.size == (3 * 128, 2 * 96)
