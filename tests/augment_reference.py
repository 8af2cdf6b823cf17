"""Numpy restatement of the training augmentation (`mtbt_augment_batch`, include/mtbt_hip.h).  TEST INFRASTRUCTURE.

The reference project has no augmentation, so this arithmetic is the project's own definition and has no counterpart in
oracle/.  It is built from the oracle's resize (`oracle.preprocess.resize_linear_u8` / `resize_nearest_u8`, the restated
cv2 8-bit paths) so that at the identity geometry it is `oracle.preprocess.letterbox`:

  R = the source resized to new_w x new_h;  Q = R transposed (orient bit 2), then flipped in x (bit 0) and y (bit 1), which is
  Q[y][x] = R[y'][x'] with x1 = qw-1-x | x, y1 = qh-1-y | y, (x', y') = (y1, x1) | (x1, y1);  the canvas shows Q at
  (off_x, off_y), 114 / 0 elsewhere;  the table remaps the resized bytes (BGR order), never the pad;  then BGR -> RGB, / 255, CHW.
"""
import numpy as np

from oracle import preprocess as O


def orient_array(a: np.ndarray, orient: int) -> np.ndarray:
    """R -> Q for an [H, W] or [H, W, C] array."""
    if orient & 4:
        a = a.transpose((1, 0) + tuple(range(2, a.ndim)))
    if orient & 1:
        a = a[:, ::-1]
    if orient & 2:
        a = a[::-1]
    return a


def paste(canvas: np.ndarray, q: np.ndarray, off_x: int, off_y: int) -> None:
    """canvas[dy][dx] = q[dy - off_y][dx - off_x] where that index lies inside q."""
    S = canvas.shape[0]
    qh, qw = q.shape[:2]
    y0, y1, x0, x1 = max(off_y, 0), min(off_y + qh, S), max(off_x, 0), min(off_x + qw, S)
    if y0 < y1 and x0 < x1:
        canvas[y0:y1, x0:x1] = q[y0 - off_y:y1 - off_y, x0 - off_x:x1 - off_x]


def augment(img_bgr: np.ndarray, mask, geom_row, S: int, lut=None):
    """One image.  geom_row = (new_w, new_h, off_x, off_y, orient, 0, 0, 0); lut uint8 [3, 256] or None.
    Returns (img_t [3,S,S] float32 RGB, mask_t [1,S,S] float32)."""
    new_w, new_h, off_x, off_y, orient = (int(v) for v in geom_row[:5])
    assert 0 <= orient <= 7 and all(int(v) == 0 for v in geom_row[5:])
    R = O.resize_linear_u8(img_bgr, new_w, new_h)
    if lut is not None:
        R = np.stack([np.asarray(lut)[c][R[:, :, c]] for c in range(3)], axis=2)
    canvas = np.full((S, S, 3), 114, dtype=np.uint8)
    paste(canvas, orient_array(R, orient), off_x, off_y)
    mcanvas = np.zeros((S, S), dtype=np.uint8)
    if mask is not None:
        paste(mcanvas, orient_array(O.resize_nearest_u8(mask, new_w, new_h), orient), off_x, off_y)
    img_t = (canvas[:, :, ::-1].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
    mask_t = ((mcanvas.astype(np.float32) / np.float32(255.0)) > 0.5).astype(np.float32)[None]
    return np.ascontiguousarray(img_t), mask_t
