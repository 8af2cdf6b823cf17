"""Restatement of THE MEASURE RULE (include/mtbt_hip.h, `mtbt_measure_regions`; `postprocess.measure_regions`), written for clarity: the
yardstick of tests/test_cpu_measure.py (against scipy.spatial and closed forms) and tests/test_gpu_measure.py (bit for bit).

Every product is a Python int and every fraction a `fractions.Fraction`: the compared products reach 2^87 and numpy's int64 wraps
silently.  A region is a list of pixels (x, y); the dense forms below only collect such lists, so a plane of 16384 x 16384 with four set
pixels needs no array.

  sums        area, perimeter (pixel sides whose 4-neighbour is not in the region), sum X, sum Y, sum X^2, sum X Y, sum Y^2, 0
  hull        the strictly convex hull of the corners of the pixel squares, from the vertex with the smallest key y * (W + 1) + x, in the
              sense E -> S -> W -> N (clockwise on the screen, area2 > 0 by the contour rule's formula)
  calipers    d2 and its pair (smallest i, then smallest j), perp across it, the minimum width h^2 / len2 and the minimum rectangle
              h t / len2 over the hull's edges as exact fractions, ties to the smallest edge
"""
from fractions import Fraction

import numpy as np

from surface_reference import pack_bits  # noqa: F401  (the packed layout is the same)

CALIPER = ("d2", "perp", "w_num", "w_len2", "r_h", "r_t", "r_tmin", "r_len2")
CALIPER_AT = ("xa", "ya", "xb", "yb", "w_edge", "w_vertex", "r_edge", "zero")


def cross(ax, ay, bx, by):
    return ax * by - ay * bx


def sums(pixels):
    """The eight sums of a list of pixels (x, y), Python ints."""
    inside = set(pixels)
    per = sum((x + dx, y + dy) not in inside for x, y in pixels for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)))
    return [len(pixels), per, sum(x for x, _ in pixels), sum(y for _, y in pixels), sum(x * x for x, _ in pixels),
            sum(x * y for x, y in pixels), sum(y * y for _, y in pixels), 0]


def corner_set(pixels):
    return {(x + dx, y + dy) for x, y in pixels for dx in (0, 1) for dy in (0, 1)}


def area2_of(poly):
    """The contour rule's formula: sum of x_i y_{i+1} - x_{i+1} y_i."""
    return sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1] for i in range(len(poly)))


def hull_of(points, W):
    """The strictly convex hull of a set of lattice points (Andrew's monotone chain, collinear points dropped), listed by the rule."""
    pts = sorted(set(points))
    if len(pts) < 3:
        return pts
    half = []
    for seq in (pts, pts[::-1]):
        chain = []
        for p in seq:
            while len(chain) >= 2 and cross(chain[-1][0] - chain[-2][0], chain[-1][1] - chain[-2][1], p[0] - chain[-1][0], p[1] - chain[-1][1]) <= 0:
                chain.pop()
            chain.append(p)
        half.append(chain[:-1])
    poly = half[0] + half[1]
    if area2_of(poly) < 0:
        poly = poly[::-1]
    k = min(range(len(poly)), key=lambda i: poly[i][1] * (W + 1) + poly[i][0])
    return poly[k:] + poly[:k]


def calipers(poly):
    """-> (caliper, caliper_at): two lists of eight Python ints over the FULL hull."""
    h = len(poly)
    d2, ia, ib = -1, 0, 0
    for i in range(h):
        for j in range(i + 1, h):
            d = (poly[i][0] - poly[j][0]) ** 2 + (poly[i][1] - poly[j][1]) ** 2
            if d > d2:
                d2, ia, ib = d, i, j
    (xa, ya), (xb, yb) = poly[ia], poly[ib]
    cr = [cross(xb - xa, yb - ya, qx - xa, qy - ya) for qx, qy in poly]
    perp = max(cr) - min(cr)
    best_w = best_r = None
    for i in range(h):
        (px, py), (nx, ny) = poly[i], poly[(i + 1) % h]
        ex, ey = nx - px, ny - py
        len2 = ex * ex + ey * ey
        hs = [abs(cross(ex, ey, qx - px, qy - py)) for qx, qy in poly]
        ts = [ex * (qx - px) + ey * (qy - py) for qx, qy in poly]
        hi, t = max(hs), max(ts) - min(ts)
        w = (Fraction(hi * hi, len2), i, hi, len2, hs.index(hi))
        r = (Fraction(hi * t, len2), i, hi, t, min(ts), len2)
        if best_w is None or w[0] < best_w[0]:
            best_w = w
        if best_r is None or r[0] < best_r[0]:
            best_r = r
    return ([d2, perp, best_w[2], best_w[3], best_r[2], best_r[3], best_r[4], best_r[5]],
            [xa, ya, xb, yb, best_w[1], best_w[4], best_r[1], 0])


def measure_pixels(pixels, W):
    """One region from its list of pixels (x, y) -> dict of Python ints: sums [8], hull (list of (x, y), the full hull), hull_area2,
    caliper [8], caliper_at [8].  An empty list gives zeros."""
    pixels = [(int(x), int(y)) for x, y in pixels]
    if not pixels:
        return {"sums": [0] * 8, "hull": [], "hull_area2": 0, "caliper": [0] * 8, "caliper_at": [0] * 8}
    poly = hull_of(corner_set(pixels), W)
    cal, at = calipers(poly)
    return {"sums": sums(pixels), "hull": poly, "hull_area2": area2_of(poly), "caliper": cal, "caliper_at": at}


def pixels_of(m):
    ys, xs = np.nonzero(np.asarray(m, bool))
    return list(zip(xs.tolist(), ys.tolist()))


def measure_plane(m):
    """Plane mode: the set pixels of a dense bool plane, connected or not, as one region."""
    m = np.asarray(m, bool)
    return measure_pixels(pixels_of(m), m.shape[1])


def measure_labels(lab, max_regions):
    """Label mode: -> list of C region dicts, region i = {label == i} at [i - 1]; labels <= 0 and > C are reported nowhere."""
    lab = np.asarray(lab)
    groups = {}
    ys, xs = np.nonzero((lab >= 1) & (lab <= max_regions))
    for x, y, v in zip(xs.tolist(), ys.tolist(), lab[ys, xs].tolist()):
        groups.setdefault(v, []).append((x, y))
    return [measure_pixels(groups.get(i, []), lab.shape[1]) for i in range(1, max_regions + 1)]


def tables(regions, max_hull):
    """A [n][C] nested list of region dicts -> what mtbt_measure_regions writes: sums int64 [n, C, 8] (the words of the uint64 table),
    n_hull int32 [n, C], hull int32 [n, C, Vh, 2], hull_area2 int64 [n, C], caliper int64 [n, C, 8], caliper_at int32 [n, C, 8]."""
    n, C = len(regions), len(regions[0]) if regions else 0
    out = {"sums": np.zeros((n, C, 8), np.int64), "n_hull": np.zeros((n, C), np.int32), "hull": np.zeros((n, C, max_hull, 2), np.int32),
           "hull_area2": np.zeros((n, C), np.int64), "caliper": np.zeros((n, C, 8), np.int64), "caliper_at": np.zeros((n, C, 8), np.int32)}
    for b in range(n):
        for r, rec in enumerate(regions[b]):
            out["sums"][b, r] = rec["sums"]
            out["n_hull"][b, r] = len(rec["hull"])
            k = min(len(rec["hull"]), max_hull)
            if k:
                out["hull"][b, r, :k] = rec["hull"][:k]
            out["hull_area2"][b, r] = rec["hull_area2"]
            out["caliper"][b, r] = rec["caliper"]
            out["caliper_at"][b, r] = rec["caliper_at"]
    return out


def plane_tables(planes, max_hull=512):
    """Plane mode over a list of dense planes (C = 1)."""
    return tables([[measure_plane(m)] for m in planes], max_hull)


def label_tables(label_maps, max_regions, max_hull=512):
    """Label mode over a list of dense label maps."""
    return tables([measure_labels(lab, max_regions) for lab in label_maps], max_hull)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
def disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def diamond(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return abs(yy - cy) + abs(xx - cx) <= r


def extra_cases(rng, H, W):
    """-> list of (name, dense bool plane) beside `components_reference.plane_cases`: a pixel in each corner alone, a disc, a diamond, a
    bar across the word boundaries 63|64 and 127|128."""
    z = np.zeros((H, W), bool)
    out = []
    for name, (y, x) in (("pixel_tl", (0, 0)), ("pixel_tr", (0, W - 1)), ("pixel_bl", (H - 1, 0)), ("pixel_br", (H - 1, W - 1))):
        m = z.copy()
        m[y, x] = True
        out.append((name, m))
    r = max(min(H, W) // 2 - 1, 0)
    out.append(("disc", disc(H, W, H // 2, W // 2, r)))
    out.append(("diamond", diamond(H, W, H // 2, W // 2, r)))
    bar = z.copy()
    bar[H // 2, min(60, W - 1):min(W, 132)] = True
    out.append(("bar", bar))
    return out


BIG_FOUR = ((0, 0), (16383, 1), (16382, 16383), (1, 16382))     # (x, y): four pixels near the corners of a 16384 x 16384 plane


def width_products(poly):
    """Every cross-multiplied pair h_i^2 * len2_j the width comparison of a hull can form, Python ints: to show that some exceed 2^64."""
    h = len(poly)
    hs, ls = [], []
    for i in range(h):
        (px, py), (nx, ny) = poly[i], poly[(i + 1) % h]
        ex, ey = nx - px, ny - py
        hs.append(max(abs(cross(ex, ey, qx - px, qy - py)) for qx, qy in poly))
        ls.append(ex * ex + ey * ey)
    return [hs[i] * hs[i] * ls[j] for i in range(h) for j in range(h) if i != j]
