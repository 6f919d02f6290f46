"""GPU: <name>_scene.ply from ``ovmono3d_amd.vis.scene_ply`` is byte-equal to the numpy restatement (tests/scene_ply_oracle.py) - no
tolerance - on the smallest shapes that cross the kernel's boundaries: one pixel, exactly one 2,048-pixel tile, one pixel past a
tile, one short of two, several tiles with about 30 % of the depth NaN, +-inf, 0 or negative. ``ovm_scene_ply_points`` is also
called directly into a buffer pre-filled with 0xA5 and one guard page beyond the worst case: the device count is the oracle's P,
the first 15 P bytes are the oracle's records, every byte at or past 15 P is untouched, and a second call gives the same bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import scene_ply_oracle as po
from ovmono3d_amd import lib
from ovmono3d_amd import vis

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0xA5


def _views(device, s, H, W):
    """The [H, W] maps as column slices of the (possibly wider) device buffers."""
    return tuple(torch.from_numpy(s[k]).to(device)[:, :W] for k in ("im", "depth", "labels"))


def _host(s, H, W):
    return s["im"][:, :W], s["depth"][:, :W], s["labels"][:, :W]


def _records(s, H, W, n, labels=True, **kw):
    """The oracle's P and point bytes."""
    im, depth, lab = _host(s, H, W)
    frame = kw.get("frame", "camera")
    data, P = po.scene_ply(im, s["K"], depth, s["corners"][:n], s["colors"][:n], lab if labels else None, **kw)
    h = len(po.header(P, n, frame))
    return P, data[h:h + 15 * P]


def _device_points(device, s, H, W, n, labels=True, stride=1, max_depth=None, frame="camera"):
    """One direct call: (count, the output buffer with its guard page as numpy)."""
    L = lib.load()
    im, depth, lab = _views(device, s, H, W)
    tint = np.zeros((max(n, 1), 4), np.uint8)
    tint[:n, :3] = po.edge_u8(s["colors"][:n])
    K = np.ascontiguousarray(s["K"].reshape(9))
    worst = -(-H // stride) * -(-W // stride) * 15
    ws_bytes = C.c_int64()
    assert L.ovm_scene_ply_points_workspace(H, W, stride, n, C.byref(ws_bytes)) == 0
    out = torch.full((worst + GUARD,), FILL, dtype=torch.uint8, device=device)
    count = torch.full((1,), -1, dtype=torch.int64, device=device)
    ws = torch.empty(int(ws_bytes.value), dtype=torch.uint8, device=device)
    rc = L.ovm_scene_ply_points(im.data_ptr(), im.stride(0), depth.data_ptr(), 4 * depth.stride(0), lab.data_ptr() if labels else None,
                                4 * lab.stride(0) if labels else 0, tint.ctypes.data, n, H, W, K.ctypes.data, stride,
                                0.0 if max_depth is None else float(max_depth), int(frame == "opengl"), out.data_ptr(), worst, count.data_ptr(),
                                ws.data_ptr(), ws.numel(), C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize(device)
    return int(count.item()), out.cpu().numpy()


def _check_direct(device, s, H, W, n, **kw):
    P, want = _records(s, H, W, n, **kw)
    got_P, buf = _device_points(device, s, H, W, n, **kw)
    assert got_P == P
    assert buf[:15 * P].tobytes() == want
    assert (buf[15 * P:] == FILL).all(), f"{int((buf[15 * P:] != FILL).sum())} bytes at or past 15 P were written"
    again_P, again = _device_points(device, s, H, W, n, **kw)
    assert again_P == P and np.array_equal(again, buf)
    return P


def _check_file(device, s, H, W, n, labels=True, **kw):
    im, depth, lab = _views(device, s, H, W)
    hi, hd, hl = _host(s, H, W)
    got = vis.scene_ply(im, s["K"], depth=depth, corners=s["corners"][:n], colors=s["colors"][:n], point_labels=lab if labels else None, **kw)
    want, P = po.scene_ply(hi, s["K"], hd, s["corners"][:n], s["colors"][:n], hl if labels else None, **kw)
    assert isinstance(got, bytes) and got == want
    return P


SHAPES = [(1, 1, 0.0), (3, 5, 0.0), (32, 64, 0.0), (1, 2049, 0.0), (45, 91, 0.0), (64, 65, 0.3), (257, 263, 0.3)]


@pytest.mark.parametrize("frame", ["camera", "opengl"])
@pytest.mark.parametrize("H,W,bad", SHAPES)
def test_file_and_records_equal_the_oracle(device, H, W, bad, frame):
    s = po.scene(H, W, seed=100 + H + W, bad=bad, n=3)
    P = _check_direct(device, s, H, W, 3, frame=frame)
    assert P == H * W if bad == 0 else 0.5 * H * W < P < 0.9 * H * W
    assert _check_file(device, s, H, W, 3, frame=frame) == P


def test_no_valid_pixel_gives_a_boxes_only_file_and_count_zero(device):
    H, W = 45, 91
    s = po.scene(H, W, seed=7, n=2)
    s["depth"][:] = np.array([np.nan, np.inf, -np.inf, 0.0, -3.0], np.float32)[np.arange(H * W).reshape(H, W) % 5]
    assert _check_direct(device, s, H, W, 2) == 0
    im, depth, lab = _views(device, s, H, W)
    got = vis.scene_ply(im, s["K"], depth=depth, corners=s["corners"], colors=s["colors"], point_labels=lab)
    assert got == vis.scene_ply(s["im"], s["K"], corners=s["corners"], colors=s["colors"]) == po.scene_ply(s["im"], s["K"], None, s["corners"], s["colors"])[0]
    assert len(po.read_ply(got)["xyz"]) == 16


def test_a_tiles_byte_range_starts_at_every_alignment(device):
    """Two tiles of 2,048 pixels. With the first o pixels of the first tile invalid the second tile's range starts at byte
    15 * (2048 - o): every alignment mod 4 - and mod 16, the width of the interior stores - for o = 0 .. 15. With only the first o
    pixels of the second tile invalid, the first valid pixel sits at tile offset o and the tile's range ends o records early."""
    H, W = 2, 2048
    for o in range(16):
        s = po.scene(H, W, seed=40 + o, n=1)
        s["depth"][0, :o] = np.nan
        assert _check_direct(device, s, H, W, 1) == 2 * 2048 - o
        s = po.scene(H, W, seed=60 + o, n=1)
        s["depth"][1, :o] = 0.0
        assert _check_direct(device, s, H, W, 1) == 2 * 2048 - o
    # a lone valid pixel at tile offsets 0 .. 3 of the second tile
    for o in range(4):
        s = po.scene(H, W, seed=80 + o, n=1)
        s["depth"][:] = -1.0
        s["depth"][1, o] = 2.5
        assert _check_direct(device, s, H, W, 1) == 1


@pytest.mark.parametrize("stride", [1, 2, 3, 16])
@pytest.mark.parametrize("H,W", [(45, 91), (257, 263)])
def test_strides_on_sizes_that_are_no_multiples(device, H, W, stride):
    s = po.scene(H, W, seed=H + stride, bad=0.3, n=2)
    P = _check_direct(device, s, H, W, 2, stride=stride)
    assert 0 < P <= -(-H // stride) * -(-W // stride)
    assert _check_file(device, s, H, W, 2, stride=stride, frame="opengl") == P


def test_max_depth_keeps_the_bound_itself(device):
    H, W = 64, 65
    s = po.scene(H, W, seed=9, bad=0.3, n=1)
    valid = np.isfinite(s["depth"]) & (s["depth"] > 0)
    bound = float(np.median(s["depth"][valid]))                            # the median of an odd or even count: make it occur
    bound = float(s["depth"][valid][np.argmin(np.abs(s["depth"][valid] - bound))])
    s["depth"][5, 7] = s["depth"][40, 2] = np.float32(bound)
    P = _check_direct(device, s, H, W, 1, max_depth=bound)
    keep = po.valid_mask(s["depth"], 1, bound)
    assert keep[5, 7] and keep[40, 2] and P == int(keep.sum()) and 0 < P < int(valid.sum())
    assert _check_file(device, s, H, W, 1, max_depth=bound) == P


@pytest.mark.parametrize("n", [0, 1, 3])
def test_labels_tint_valid_indices_only(device, n):
    H, W = 45, 91
    s = po.scene(H, W, seed=20 + n, bad=0.3, n=n)
    assert (s["labels"] == -1).any() and (s["labels"] >= n).any() and (n == 0 or ((s["labels"] >= 0) & (s["labels"] < n)).any())
    P = _check_direct(device, s, H, W, n)
    assert _check_file(device, s, H, W, n) == P
    plain = _records(s, H, W, n, labels=False)[1]
    assert _check_direct(device, s, H, W, n, labels=False) == P and (_records(s, H, W, n)[1] != plain) == (n > 0)


def test_pitched_rows_and_numpy_uploads(device):
    H, W = 64, 65
    s = po.scene(H, W, seed=31, bad=0.3, n=3, wide=7)                      # the maps are column slices of [H, W + 7] buffers
    im, depth, lab = _views(device, s, H, W)
    assert depth.stride(0) == W + 7 and im.stride(0) == 3 * (W + 7) and not depth.is_contiguous()
    P = _check_direct(device, s, H, W, 3, stride=2)
    assert _check_file(device, s, H, W, 3, stride=2) == P
    hi, hd, hl = _host(s, H, W)
    up = vis.scene_ply(hi, s["K"], depth=hd, corners=s["corners"], colors=s["colors"], point_labels=hl, stride=2)
    assert up == po.scene_ply(hi, s["K"], hd, s["corners"], s["colors"], hl, stride=2)[0]
    # points only
    assert vis.scene_ply(im, s["K"], depth=depth) == po.scene_ply(hi, s["K"], hd)[0]


def test_refusals_on_the_device_write_nothing(device):
    L = lib.load()
    H, W = 8, 8
    s = po.scene(H, W, seed=3, n=1)
    im, depth, lab = _views(device, s, H, W)
    K = np.ascontiguousarray(s["K"].reshape(9))
    tint = np.zeros((1, 4), np.uint8)
    out = torch.full((H * W * 15 + GUARD,), FILL, dtype=torch.uint8, device=device)
    count = torch.full((1,), -1, dtype=torch.int64, device=device)
    ws = torch.full((1 << 16,), FILL, dtype=torch.uint8, device=device)

    def call(ob=H * W * 15, wb=1 << 16, stride=1, dp=4 * W):
        return L.ovm_scene_ply_points(im.data_ptr(), im.stride(0), depth.data_ptr(), dp, lab.data_ptr(), 4 * W, tint.ctypes.data, 1, H, W, K.ctypes.data,
                                      stride, 0.0, 0, out.data_ptr(), ob, count.data_ptr(), ws.data_ptr(), wb, None)
    assert call(ob=H * W * 15 - 1) == lib.OVM_ERR_CAPACITY and call(wb=16) == lib.OVM_ERR_CAPACITY
    assert call(stride=17) == lib.OVM_ERR_INVALID and call(dp=4 * W + 2) == lib.OVM_ERR_INVALID
    torch.cuda.synchronize(device)
    assert int(count.item()) == -1 and bool((out == FILL).all()) and bool((ws == FILL).all())
