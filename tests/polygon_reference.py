"""The polygon fill rule of include/mtbt_hip.h (`mtbt_fill_polygons`) restated in numpy: what the kernel must reproduce bit for bit.

Quantisation   q = rint(float32(v) * 16), round half to even, int32; pixel (X, Y) has its centre at (16 X + 8, 16 Y + 8).
Crossing       an edge a -> b of the closed polygon crosses the scanline yc = 16 Y + 8 when (ay <= yc) != (by <= yc).
Left           with ay < by: (bx - ax) * (yc - ay) - (xc - ax) * (by - ay) > 0, in int64.
Even-odd       inside = odd number of crossing edges the pixel is left of.
Planes         OR of the polygons, each filled on its own; fewer than 3 vertices fill nothing.
Clip           (x0, y0, x1, y1) half-open in pixel indices zeroes everything outside.
"""
import numpy as np


def quantise(v) -> np.ndarray:
    """Pixel coordinates -> the fixed-point int32 the kernel reads (float32(v) * 16 is exact; np.rint rounds half to even)."""
    return np.rint(np.asarray(v, dtype=np.float32) * np.float32(16.0)).astype(np.int32)


def _edges(poly):
    """[n, 2] pixel coordinates -> the upward (ay < by) int64 edges of the closed polygon, horizontal ones dropped."""
    q = quantise(poly).astype(np.int64).reshape(-1, 2)
    if q.shape[0] < 3:
        return []
    out = []
    for i in range(q.shape[0]):
        (ax, ay), (bx, by) = q[i], q[(i + 1) % q.shape[0]]
        if ay == by:
            continue
        out.append((ax, ay, bx, by) if ay < by else (bx, by, ax, ay))
    return out


def _apply_clip(m: np.ndarray, clip) -> np.ndarray:
    if clip is None:
        return m
    H, W = m.shape
    x0, y0, x1, y1 = (int(v) for v in clip)
    keep = np.zeros_like(m)
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
    if x0 < x1 and y0 < y1:
        keep[y0:y1, x0:x1] = True
    return m & keep


def fill(polygons, H: int, W: int, clip=None) -> np.ndarray:
    """One plane: bool [H, W], the union of `polygons` (a list of [n, 2] pixel-coordinate arrays).  Vectorised over the pixels of the
    rows an edge crosses, looping over edges."""
    xc = 16 * np.arange(W, dtype=np.int64) + 8
    plane = np.zeros((H, W), dtype=bool)
    for poly in polygons:
        m = np.zeros((H, W), dtype=bool)
        for ax, ay, bx, by in _edges(poly):
            # rows with ay <= 16 Y + 8 < by: Y >= ceil((ay - 8) / 16), Y <= ceil((by - 8) / 16) - 1
            y_lo, y_hi = max(-((8 - ay) // 16), 0), min(-((8 - by) // 16), H)
            if y_lo >= y_hi:
                continue
            yc = 16 * np.arange(y_lo, y_hi, dtype=np.int64) + 8
            left = (bx - ax) * (yc[:, None] - ay) - (xc[None, :] - ax) * (by - ay) > 0
            m[y_lo:y_hi] ^= left
        plane |= m
    return _apply_clip(plane, clip)


def fill_scalar(polygons, H: int, W: int, clip=None) -> np.ndarray:
    """`fill` with the rule spelled out per pixel in Python integers (tiny shapes only)."""
    plane = np.zeros((H, W), dtype=bool)
    for poly in polygons:
        q = [(int(x), int(y)) for x, y in quantise(poly).reshape(-1, 2)]
        if len(q) < 3:
            continue
        for Y in range(H):
            for X in range(W):
                xc, yc, n = 16 * X + 8, 16 * Y + 8, 0
                for i in range(len(q)):
                    (ax, ay), (bx, by) = q[i], q[(i + 1) % len(q)]
                    if (ay <= yc) == (by <= yc):
                        continue
                    if ay > by:
                        ax, ay, bx, by = bx, by, ax, ay
                    n += (bx - ax) * (yc - ay) - (xc - ax) * (by - ay) > 0
                plane[Y, X] |= bool(n & 1)
    return _apply_clip(plane, clip)


def pack_bits(mask: np.ndarray) -> np.ndarray:
    """bool [..., H, W] -> uint8 [..., H, pitch], pitch = 8 * ceil(W / 64): pixel X is bit X & 7 of byte X >> 3, padding zero."""
    W = mask.shape[-1]
    pitch = 8 * ((W + 63) // 64)
    out = np.zeros(mask.shape[:-1] + (pitch,), dtype=np.uint8)
    bits = np.packbits(mask, axis=-1, bitorder="little")
    out[..., :bits.shape[-1]] = bits
    return out


def records(mask: np.ndarray):
    """bool [H, W] -> (area, [x1, y1, x2, y2] with exclusive maxima; zeros for an empty plane)."""
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return 0, [0, 0, 0, 0]
    return int(ys.size), [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1]


def circle(cx: float, cy: float, r: float, n: int, phase: float = 0.0) -> np.ndarray:
    t = phase + 2.0 * np.pi * np.arange(n) / n
    return np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], axis=1)


def polygon_cases(rng: np.random.Generator, H: int, W: int):
    """Named planes, each a list of [n, 2] float64 polygons in pixels of an H x W plane: the places where a fill can go wrong."""
    A = lambda pts: np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    w, h = float(W), float(H)
    rect = lambda x1, y1, x2, y2: A([[x1, y1], [x2, y1], [x2, y2], [x1, y2]])
    tri_a, tri_b = A([[0, 0], [w, 0], [w, h]]), A([[0, 0], [w, h], [0, h]])       # share the diagonal of the plane's square
    star = circle(w / 2, h / 2, 0.45 * min(w, h) + 1.0, 5)[[0, 2, 4, 1, 3]]
    cases = [
        ("no_polygons", []),
        ("two_vertices", [A([[0, 0], [w, h]])]),
        ("triangle", [A([[0.2 * w, 0.1 * h], [0.9 * w, 0.4 * h], [0.3 * w, 0.95 * h]])]),
        ("rect_integer", [rect(W // 4, H // 4, W // 4 + (W + 1) // 2, H // 4 + (H + 1) // 2)]),
        ("rect_on_centres", [rect(W // 4 + 0.5, H // 4 + 0.5, W // 4 + (W + 1) // 2 + 0.5, H // 4 + (H + 1) // 2 + 0.5)]),
        ("rect_larger", [rect(-3.0, -2.0, w + 70.0, h + 5.0)]),
        ("left_of", [rect(-w - 5, 0.0, -0.25, h)]),
        ("right_of", [rect(w + 0.25, 0.0, 2 * w + 3, h)]),
        ("above", [rect(0.0, -h - 4, w, -0.25)]),
        ("below", [rect(0.0, h + 0.25, w, 2 * h + 9)]),
        ("negative_far", [A([[-30000.0, -20000.0], [32768.0, 0.3 * h], [0.5 * w, 31000.0], [-100.5, 0.7 * h]])]),
        ("bow_tie", [A([[0.1 * w, 0.1 * h], [0.9 * w, 0.9 * h], [0.9 * w, 0.1 * h], [0.1 * w, 0.9 * h]])]),
        ("pentagram", [star]),
        ("duplicates_closed", [A([[1, 1], [1, 1], [w - 1, 1.25], [w - 1, 1.25], [w - 1, 1.25], [0.5 * w, h - 0.5], [1, 1]])]),
        ("sliver", [A([[0.3 * w, -1.0], [0.3 * w + 0.4, -1.0], [0.6 * w + 0.4, h + 1.0], [0.6 * w, h + 1.0]])]),
        ("bar_word_boundaries", [rect(62.5, 0.2 * h, 129.5, 0.8 * h)]),
        ("diagonal_word_boundaries", [A([[60.0, 0.0], [66.0, 0.0], [131.0, h], [125.0, h]])]),
        ("circle_3000", [circle(0.5 * w, 0.5 * h, 0.45 * min(w, h) + 0.7, 3000)]),
        ("seven_circles_500", [circle(w * (0.2 + 0.1 * i), h * (0.3 + 0.07 * i), 0.18 * max(w, h) + 0.3, 500, 0.1 * i) for i in range(7)]),
        ("shared_diagonal_a", [tri_a]),
        ("shared_diagonal_b", [tri_b]),
        ("shared_diagonal_both", [tri_a, tri_b]),
    ]
    for i in range(4):
        n = int(rng.integers(3, 12))
        cases.append((f"random_{i}", [np.stack([rng.uniform(-2 * w, 2 * w, n), rng.uniform(-2 * h, 2 * h, n)], axis=1)
                                      for _ in range(1 + i % 2)]))
    return cases
