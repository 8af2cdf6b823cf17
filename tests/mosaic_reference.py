"""Numpy restatement of the four-image mosaic (`mtbt_mosaic_batch`, include/mtbt_hip.h).  TEST INFRASTRUCTURE.

Like the augmentation it is the project's own definition (the reference's dataset class augments nothing), so it has no counterpart in
oracle/.  It is `augment_reference.augment` per tile on a whole canvas, with the canvas's table, and a copy of the tile's rectangle:

  centre (cx, cy);  tile 0 [0,cx) x [0,cy), tile 1 [cx,S) x [0,cy), tile 2 [0,cx) x [cy,S), tile 3 [cx,S) x [cy,S), x then y.
"""
import numpy as np

from augment_reference import augment


def rectangles(centre, S: int):
    """(x0, y0, x1, y1), half-open, of tiles 0..3."""
    cx, cy = int(centre[0]), int(centre[1])
    assert 0 <= cx <= S and cx % 4 == 0 and 0 <= cy <= S
    return [(0, 0, cx, cy), (cx, 0, S, cy), (0, cy, cx, S), (cx, cy, S, S)]


def mosaic(imgs4, masks4, geom4, centre, S: int, lut=None):
    """One canvas.  imgs4 / masks4: the four tiles' sources (a mask may be None); geom4 [4][8]; lut uint8 [3, 256] or None.
    Returns (img_t [3,S,S] float32 RGB, mask_t [1,S,S] float32)."""
    img_t, mask_t = np.empty((3, S, S), np.float32), np.empty((1, S, S), np.float32)
    for t, (x0, y0, x1, y1) in enumerate(rectangles(centre, S)):
        x, m = augment(imgs4[t], masks4[t], geom4[t], S, lut=lut)
        img_t[:, y0:y1, x0:x1] = x[:, y0:y1, x0:x1]
        mask_t[:, y0:y1, x0:x1] = m[:, y0:y1, x0:x1]
    return img_t, mask_t
