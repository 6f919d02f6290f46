"""numpy restatement of the label map and the mask picture (ovm_mask_labels, ovm_render_mask_overlay; rules in include/ovm3d.h).
A layer of this project - the reference draws no masks - so there is nothing outside to pin it to: the rules are the statement."""
import numpy as np


def labels(masks: np.ndarray) -> np.ndarray:
    """uint8 / bool [n, H, W] -> int32 [H, W]: the lowest plane index covering the pixel, -1 where none does."""
    n, H, W = masks.shape
    out = np.full((H, W), -1, np.int32)
    for i in range(n - 1, -1, -1):
        out[masks[i] != 0] = i
    return out


def overlay(image: np.ndarray, lab: np.ndarray, colors: np.ndarray, alpha: int) -> np.ndarray:
    """image uint8 [H, W, 3], lab int32 [H, W], colors uint8 [n, 3] in the image's channel order, alpha 0..255."""
    H, W = lab.shape
    n = len(colors)
    differs = np.zeros((H, W), bool)                     # a 4-neighbour inside the image carries another label
    differs[:, 1:] |= lab[:, 1:] != lab[:, :-1]
    differs[:, :-1] |= lab[:, :-1] != lab[:, 1:]
    differs[1:, :] |= lab[1:, :] != lab[:-1, :]
    differs[:-1, :] |= lab[:-1, :] != lab[1:, :]
    out = image.copy()
    valid = (lab >= 0) & (lab < n)
    if n == 0 or not valid.any():
        return out
    col = np.asarray(colors, np.int64).reshape(-1, 3)[np.clip(lab, 0, n - 1)]
    blend = (image.astype(np.int64) * (255 - alpha) + col * alpha + 127) // 255
    out[valid] = blend[valid].astype(np.uint8)
    out[valid & differs] = col[valid & differs].astype(np.uint8)
    return out
