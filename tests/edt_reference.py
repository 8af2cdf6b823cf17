"""Numpy restatement of the distance transform and of the region terms of the segmentation loss (include/mtbt_hip.h,
`mtbt_distance_transform`, `mtbt_seg_region_loss`), written for clarity and by exhaustive search: the yardstick of
tests/test_cpu_edt.py (against scipy, Kervadec's formula and torch autograd) and of the GPU tests (maps bit for bit).

  d2 maps   d2_set[y, x] = min over the set pixels (y', x') of (y - y')^2 + (x - x')^2, d2_unset over the unset pixels inside the
            image; NONE = 0xFFFFFFFF everywhere when there is no such pixel.  Exact integers.
  phi       +sqrt(d2_set) on an unset pixel, -(sqrt(d2_unset) - 1) on a set pixel, 0 where the needed map is NONE
  terms     dice = mean_b [1 - (2 I + s) / (P + T + s)], boundary = (1 / (B N)) sum phi p, with p = sigmoid(z), in float64, and
            the analytic gradient of w_dice * dice + w_boundary * boundary with respect to z
"""
import numpy as np

NONE = 0xFFFFFFFF


def d2_pairs(targets: np.ndarray) -> np.ndarray:
    """int64 [H, W]: at every pixel the least squared distance to a True pixel of `targets`, every pair of pixels tried (small planes
    only); NONE everywhere when `targets` holds none."""
    t = np.asarray(targets, bool)
    H, W = t.shape
    pts = np.argwhere(t).astype(np.int64)
    if len(pts) == 0:
        return np.full((H, W), NONE, np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty(H * W, np.int64)
    py, px = yy.reshape(-1).astype(np.int64), xx.reshape(-1).astype(np.int64)
    block = max(1, (1 << 22) // len(pts))
    for i in range(0, H * W, block):
        dy, dx = py[i:i + block, None] - pts[None, :, 0], px[i:i + block, None] - pts[None, :, 1]
        out[i:i + block] = (dy * dy + dx * dx).min(1)
    return out.reshape(H, W)


def d2_separable(targets: np.ndarray) -> np.ndarray:
    """The same map by two exhaustive minima, for planes too large for `d2_pairs`: g[y', x] = min over the targets of row y' of
    |x - x'| (every x' tried), then d2[y, x] = min over every row y' of (y - y')^2 + g[y', x]^2.  min over (y', x') of a sum of a term
    in y' and a term in (y', x') is the min over y' of the first plus the min over x' of the second: still exact, still no cleverness."""
    t = np.asarray(targets, bool)
    H, W = t.shape
    if not t.any():
        return np.full((H, W), NONE, np.int64)
    BIG = np.int64(1) << 20                                   # a row without a target: beyond every distance, its square fits int64
    xs = np.arange(W, dtype=np.int64)
    g = np.empty((H, W), np.int64)
    for y in range(H):
        tx = xs[t[y]]
        g[y] = np.abs(xs[:, None] - tx[None, :]).min(1) if len(tx) else BIG
    g2 = g * g
    ys = np.arange(H, dtype=np.int64)
    out = np.empty((H, W), np.int64)
    for y in range(H):
        out[y] = (((ys - y) ** 2)[:, None] + g2).min(0)
    return out


def d2_maps(m: np.ndarray, pairs: bool = None):
    """(d2_set, d2_unset) of one dense boolean plane as int64; `pairs` picks the all-pairs search (default: planes up to 96 x 160)."""
    m = np.asarray(m, bool)
    if pairs is None:
        pairs = m.size <= 96 * 160
    f = d2_pairs if pairs else d2_separable
    return f(m), f(~m)


def phi_of(m: np.ndarray, d2_set: np.ndarray, d2_unset: np.ndarray) -> np.ndarray:
    """float64 [H, W] signed distance of the boundary term."""
    m = np.asarray(m, bool)
    d2 = np.where(m, d2_unset, d2_set)
    d = np.sqrt(d2.astype(np.float64))
    return np.where(d2 == NONE, 0.0, np.where(m, -(d - 1.0), d))


def region_terms(z: np.ndarray, masks: np.ndarray, phi: np.ndarray, *, w_dice: float = 1.0, w_boundary: float = 0.0, smooth: float = 1.0):
    """z, phi float64 [B, H, W] (z = logits + bias), masks bool [B, H, W] -> (dice, boundary, weighted, d weighted / d z)."""
    z, t, phi = np.asarray(z, np.float64), np.asarray(masks, bool).astype(np.float64), np.asarray(phi, np.float64)
    B, N = z.shape[0], z.shape[1] * z.shape[2]
    p = 1.0 / (1.0 + np.exp(-z))
    I, P, T = (p * t).sum((1, 2)), p.sum((1, 2)), t.sum((1, 2))
    num, den = 2.0 * I + smooth, P + T + smooth
    dice = float(np.mean(1.0 - num / den))
    boundary = float((phi * p).sum() / (B * N))
    d_dice = -(2.0 * t * den[:, None, None] - num[:, None, None]) / (den[:, None, None] ** 2) / B
    grad = p * (1.0 - p) * (w_dice * d_dice + w_boundary * phi / (B * N))
    return dice, boundary, w_dice * dice + w_boundary * boundary, grad


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 65), (2, 63), (37, 64), (70, 130))     # 1 pixel, a second word, an odd tail, a full word, several of both


def blobs(rng, H: int, W: int, k: int) -> np.ndarray:
    """k filled ellipses somewhere in the plane (never empty: each keeps its centre pixel)."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(k):
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        ry, rx = max(1.0, H / rng.uniform(4, 12)), max(1.0, W / rng.uniform(4, 12))
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        m[cy, cx] = True
    return m


def plane_cases(rng, H: int, W: int):
    """-> list of (name, dense boolean plane): the contents the two passes of the kernel can go wrong on."""
    z = np.zeros((H, W), bool)
    cases = [("empty", z), ("full", ~z)]
    for name, (y, x) in (("corner_tl", (0, 0)), ("corner_tr", (0, W - 1)), ("corner_bl", (H - 1, 0)), ("corner_br", (H - 1, W - 1))):
        c = z.copy()
        c[y, x] = True
        cases.append((name, c))
    row, col = z.copy(), z.copy()
    row[H // 2, :] = True
    col[:, W // 3] = True
    yy, xx = np.mgrid[0:H, 0:W]
    cases += [("row", row), ("column", col), ("checker", (yy + xx) % 2 == 0), ("blobs2", blobs(rng, H, W, 2)), ("blobs3", blobs(rng, H, W, 3)),
              ("noise_sparse", rng.uniform(size=(H, W)) < 0.002), ("noise_half", rng.uniform(size=(H, W)) < 0.5)]
    return cases


def pack_bits(m: np.ndarray, pad_ones: bool = False) -> np.ndarray:
    """Dense [..., H, W] bool -> packed uint8 [..., H, 8 * ceil(W / 64)]; `pad_ones` sets the padding bits X >= W."""
    m = np.asarray(m, bool)
    W = m.shape[-1]
    Wp = 64 * ((W + 63) // 64)
    full = np.full(m.shape[:-1] + (Wp,), pad_ones, bool)
    full[..., :W] = m
    return np.packbits(full, axis=-1, bitorder="little")
