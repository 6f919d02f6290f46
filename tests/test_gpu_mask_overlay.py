"""GPU: the label map and the mask picture (ovm_mask_labels, ovm_render_mask_overlay through ovmono3d_amd.masks) against
vis.labels_from_masks and the numpy restatement tests/mask_overlay_oracle.py: integer rules, equal to the byte."""
import numpy as np
import pytest
import torch

import mask_overlay_oracle as oo
import mask_rle_oracle as mo
from ovmono3d_amd import masks as M
from ovmono3d_amd import vis

pytestmark = pytest.mark.gpu


def _planes(n, H, W, seed=0):
    """Overlapping blobs; plane 0 leaves room so that later planes show."""
    return np.stack([mo.blobs(H, W, seed=seed + i, k=2) for i in range(n)]) if n else np.zeros((0, H, W), np.uint8)


def _image(H, W, seed=1):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


@pytest.mark.parametrize("H,W", [(48, 64), (37, 53)])
@pytest.mark.parametrize("n", [0, 1, 40])
def test_labels_equal_labels_from_masks(device, n, H, W):
    planes = _planes(n, H, W)
    if n:
        planes[n // 2] *= 200                                            # any nonzero value is inside
    t = torch.from_numpy(planes).to(device)
    got = M.mask_labels(t)
    assert got.dtype == torch.int32 and torch.equal(got, vis.labels_from_masks(t))
    assert np.array_equal(got.cpu().numpy(), oo.labels(planes))
    if n:
        assert torch.equal(M.mask_labels(t != 0), got)
        wide = torch.zeros((n, H + 3, W + 5), dtype=torch.uint8, device=device)
        wide[:, 2:2 + H, 4:4 + W] = t
        assert torch.equal(M.mask_labels(wide[:, 2:2 + H, 4:4 + W]), got)      # pitched planes


def _colors(n):
    return np.asarray([vis.get_color(i) for i in range(n)], np.uint8).reshape(-1, 3)


@pytest.mark.parametrize("alpha", [0, 128, 255])
def test_overlay_equals_the_restatement(device, alpha):
    H, W = 37, 53
    planes = _planes(5, H, W, seed=20)
    img = _image(H, W)
    lab = oo.labels(planes)
    want = oo.overlay(img, lab, _colors(5), alpha)
    got = M.overlay_masks(torch.from_numpy(img).to(device), torch.from_numpy(planes).to(device), _colors(5), alpha=alpha / 255)
    assert np.array_equal(got.cpu().numpy(), want)
    got = M.overlay_masks(torch.from_numpy(img).to(device), torch.from_numpy(lab).to(device), _colors(5), alpha=alpha / 255)
    assert np.array_equal(got.cpu().numpy(), want)
    if alpha == 0:                                                        # only the contours show
        inner = want != img
        assert inner.any() and not np.array_equal(want, img)


def test_overlay_borders_single_pixels_and_foreign_labels(device):
    H, W = 48, 64
    img = _image(H, W, seed=2)
    full = np.ones((1, H, W), np.uint8)                                   # touches all four borders: the border is not contour by itself
    want = oo.overlay(img, oo.labels(full), _colors(1), 128)
    col = _colors(1)[0].astype(np.int64)
    assert np.array_equal(want, ((img.astype(np.int64) * 127 + col * 128 + 127) // 255).astype(np.uint8))       # blended everywhere, no contour
    got = M.overlay_masks(torch.from_numpy(img).to(device), torch.from_numpy(full).to(device), _colors(1), alpha=128 / 255)
    assert np.array_equal(got.cpu().numpy(), want)
    one = np.zeros((2, H, W), np.uint8)
    one[1, 17, 31] = 1                                                    # a one-pixel mask is all contour
    one[0, 0, 0] = 1
    want = oo.overlay(img, oo.labels(one), _colors(2), 128)
    assert tuple(want[17, 31]) == tuple(_colors(2)[1]) and tuple(want[0, 0]) == tuple(_colors(2)[0])
    got = M.overlay_masks(torch.from_numpy(img).to(device), torch.from_numpy(one).to(device), _colors(2), alpha=128 / 255)
    assert np.array_equal(got.cpu().numpy(), want)
    # labels at or above n: those pixels are unchanged, but they still make their neighbours contour
    lab = oo.labels(_planes(4, H, W, seed=30))
    want = oo.overlay(img, lab, _colors(2), 128)
    assert (lab >= 2).any() and np.array_equal(want[lab >= 2], img[lab >= 2])
    got = M.overlay_masks(torch.from_numpy(img).to(device), torch.from_numpy(lab).to(device), _colors(2), alpha=128 / 255)
    assert np.array_equal(got.cpu().numpy(), want)


def test_overlay_pitched_rows(device):
    H, W = 37, 53
    img = _image(H, W, seed=3)
    planes = _planes(3, H, W, seed=40)
    lab = oo.labels(planes)
    want = oo.overlay(img, lab, _colors(3), 128)
    wide_img = torch.zeros((H, W + 11, 3), dtype=torch.uint8, device=device)
    wide_img[:, 3:3 + W] = torch.from_numpy(img).to(device)
    wide_lab = torch.full((H, W + 7), 9, dtype=torch.int32, device=device)
    wide_lab[:, 2:2 + W] = torch.from_numpy(lab).to(device)
    got = M.overlay_masks(wide_img[:, 3:3 + W], wide_lab[:, 2:2 + W], _colors(3), alpha=128 / 255)
    assert np.array_equal(got.cpu().numpy(), want)
