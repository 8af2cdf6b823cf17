"""The affine warp rule of include/mtbt_hip.h (`mtbt_warp_batch`) restated in numpy int64: what the kernel must reproduce bit for bit.
TEST INFRASTRUCTURE.  The reference project has no augmentation and cv2 is absent; the rule is the project's own (modelled on cv2's
warpAffine(INTER_LINEAR)) and has no counterpart in oracle/.

Position   X = a dx + b dy + c, Y = d dx + e dy + f (1/65536 source px, pixel-index coordinates); Xs = (X + 1024) >> 11, Ys likewise: 1/32 px.
Inside     -16 <= Xs <= 32 W0 - 17 and -16 <= Ys <= 32 H0 - 17.
Image      sx = Xs >> 5, fx = Xs & 31; taps x0 = clamp(sx), x1 = clamp(sx + 1), rows the same;
           v = ((32-fx)(32-fy) S00 + fx (32-fy) S01 + (32-fx) fy S10 + fx fy S11 + 512) >> 10; the table; / 255 once; BGR -> RGB planes.
Mask       the byte at (clamp((Xs + 16) >> 5), clamp((Ys + 16) >> 5)) >= 128.
Outside    114 / 255, never through the table; mask 0.
"""
import numpy as np

LIN_MAX, OFF_MAX = 1 << 26, 1 << 47


def positions(coef_row, S: int, H0: int, W0: int):
    """(Xs, Ys, inside): int64 [S, S] positions in 1/32 px and the bool inside test, canvas pixel (dx, dy) at [dy, dx]."""
    a, b, c, d, e, f = (int(v) for v in coef_row[:6])
    assert all(int(v) == 0 for v in coef_row[6:]) and max(abs(a), abs(b), abs(d), abs(e)) <= LIN_MAX and max(abs(c), abs(f)) <= OFF_MAX
    dy, dx = np.mgrid[0:S, 0:S].astype(np.int64)
    Xs, Ys = (a * dx + b * dy + c + 1024) >> 11, (d * dx + e * dy + f + 1024) >> 11
    inside = (Xs >= -16) & (Xs <= 32 * W0 - 17) & (Ys >= -16) & (Ys <= 32 * H0 - 17)
    return Xs, Ys, inside


def warp_bytes(img: np.ndarray, coef_row, S: int):
    """(v, inside): the blended bytes uint8 [S, S, C] in the source's channel order (0 outside) and the inside test; img is [H0, W0, C]."""
    H0, W0 = img.shape[:2]
    Xs, Ys, inside = positions(coef_row, S, H0, W0)
    sx, sy, fx, fy = Xs >> 5, Ys >> 5, (Xs & 31)[..., None], (Ys & 31)[..., None]
    x0, x1, y0, y1 = np.clip(sx, 0, W0 - 1), np.clip(sx + 1, 0, W0 - 1), np.clip(sy, 0, H0 - 1), np.clip(sy + 1, 0, H0 - 1)
    src = img.astype(np.int64)
    v = ((32 - fx) * (32 - fy) * src[y0, x0] + fx * (32 - fy) * src[y0, x1] + (32 - fx) * fy * src[y1, x0] + fx * fy * src[y1, x1] + 512) >> 10
    assert v.min() >= 0 and v.max() <= 255
    return np.where(inside[..., None], v, 0).astype(np.uint8), inside


def warp_nearest(mask: np.ndarray, coef_row, S: int):
    """(bytes, inside): the mask byte the rule reads for every canvas pixel, uint8 [S, S] (0 outside)."""
    H0, W0 = mask.shape
    Xs, Ys, inside = positions(coef_row, S, H0, W0)
    mx, my = np.clip((Xs + 16) >> 5, 0, W0 - 1), np.clip((Ys + 16) >> 5, 0, H0 - 1)
    return np.where(inside, mask[my, mx], 0).astype(np.uint8), inside


def warp(img_bgr: np.ndarray, mask, coef_row, S: int, lut=None):
    """One canvas.  img_bgr uint8 [H0, W0, 3], mask uint8 [H0, W0] or None, lut uint8 [3, 256] or None.
    Returns (img_t [3, S, S] float32 RGB, mask_t [1, S, S] float32)."""
    v, inside = warp_bytes(img_bgr, coef_row, S)
    if lut is not None:
        v = np.stack([np.asarray(lut)[c][v[:, :, c]] for c in range(3)], axis=2)
    canvas = np.where(inside[..., None], v, 114).astype(np.uint8)
    img_t = (canvas[:, :, ::-1].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
    mask_t = np.zeros((1, S, S), dtype=np.float32)
    if mask is not None:
        mask_t[0] = warp_nearest(mask, coef_row, S)[0] >= 128
    return np.ascontiguousarray(img_t), mask_t
