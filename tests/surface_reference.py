"""Numpy restatement of the surface-distance metrics (include/mtbt_hip.h, `mtbt_surface_distances`; `metrics.surface_metrics`), written
for clarity and by brute force: the yardstick of tests/test_cpu_surface.py (against scipy) and tests/test_gpu_surface.py (bit for bit).

  edge set      the set pixels with at least one of their four neighbours unset or outside the image
  directed d2   for every edge pixel of A in row-major order, min over the edge pixels of B of dy^2 + dx^2 (exact integers)
  order stats   of a list of length m at quantile q: the items at lo = floor(q (m - 1)) and min(lo + 1, m - 1) of the sorted list
  metrics       hd, hd95 (pooled: MedPy; max: MONAI), assd, nsd, with the `undefined` rules "skip" and "diagonal"
"""
import numpy as np


def edge_set(m: np.ndarray) -> np.ndarray:
    m = np.asarray(m, bool)
    p = np.pad(m, 1, constant_values=False)
    interior = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m & ~interior


def directed_d2(ea: np.ndarray, eb: np.ndarray) -> np.ndarray:
    """int64 [|ea|]: for every pixel of `ea` in row-major order the least squared distance to a pixel of `eb` (which is not empty).
    Every pair of pixels is tried, a block of `ea` at a time (int32 is exact: the planes here are far smaller than 2^15 a side)."""
    pa, pb = np.argwhere(ea).astype(np.int32), np.argwhere(eb).astype(np.int32)
    out = np.empty(len(pa), np.int64)
    block = max(1, (1 << 22) // max(1, len(pb)))
    for i in range(0, len(pa), block):
        dy = pa[i:i + block, None, 0] - pb[None, :, 0]
        dx = pa[i:i + block, None, 1] - pb[None, :, 1]
        out[i:i + block] = (dy * dy + dx * dx).min(1)
    return out


def order_stats(values: np.ndarray, q: float):
    """(item at lo, item at min(lo + 1, m - 1)) of the sorted list, lo = floor(q * (m - 1)); (0, 0) for an empty list."""
    v = np.sort(np.asarray(values, np.int64))
    m = len(v)
    if m == 0:
        return 0, 0
    lo = int(np.floor(np.float64(q) * np.float64(m - 1)))
    return int(v[lo]), int(v[min(lo + 1, m - 1)])


def records(a: np.ndarray, b: np.ndarray, quantiles=(0.95,), tol2: int = 0) -> dict:
    """What mtbt_surface_distances writes for ONE pair of dense boolean planes, plus the lists themselves (`lists`)."""
    ea, eb = edge_set(a), edge_set(b)
    n_edge = [int(ea.sum()), int(eb.sum())]
    Q = len(quantiles)
    rec = {"n_edge": n_edge, "max_d2": [0, 0], "n_within": [0, 0], "sum_d": [0.0, 0.0], "rank_d2": np.zeros((Q, 3, 2), np.int64),
           "lists": (np.zeros(0, np.int64), np.zeros(0, np.int64))}
    if min(n_edge) == 0:
        return rec
    ab, ba = directed_d2(ea, eb), directed_d2(eb, ea)
    rec["lists"] = (ab, ba)
    for s, l in enumerate((ab, ba)):
        rec["max_d2"][s] = int(l.max())
        rec["n_within"][s] = int((l <= tol2).sum())
        rec["sum_d"][s] = float(np.sqrt(l.astype(np.float64)).sum())
    for qi, q in enumerate(quantiles):
        for s, l in enumerate((ab, ba, np.concatenate([ab, ba]))):
            rec["rank_d2"][qi, s] = order_stats(l, q)
    return rec


def batch_records(pairs, quantiles=(0.95,), tol2: int = 0) -> dict:
    """`records` of a list of (a, b) stacked as the device lays them out: n_edge / max_d2 / n_within [n,2], sum_d [n,2], rank_d2 [n,Q,3,2]."""
    recs = [records(a, b, quantiles, tol2) for a, b in pairs]
    n, Q = len(recs), len(quantiles)
    out = {k: np.array([r[k] for r in recs], np.int64).reshape(n, 2) for k in ("n_edge", "max_d2", "n_within")}
    out["sum_d"] = np.array([r["sum_d"] for r in recs], np.float64).reshape(n, 2)
    out["rank_d2"] = np.array([r["rank_d2"] for r in recs], np.int64).reshape(n, Q, 3, 2)
    return out


def metrics(a: np.ndarray, b: np.ndarray, *, spacing: float = 1.0, tolerance: float = 2.0, quantile: float = 0.95,
            percentile_mode: str = "pooled", undefined: str = "skip") -> dict:
    """hd, hd95, assd, nsd and `defined` of one pair, from the lists directly (np.percentile, np.mean): NaN where the pair does not
    contribute."""
    ea, eb = edge_set(a), edge_set(b)
    na, nb = int(ea.sum()), int(eb.sum())
    if na == 0 or nb == 0:
        if undefined == "diagonal" and (na > 0) != (nb > 0):
            diag = spacing * float(np.sqrt(float(a.shape[0]) ** 2 + float(a.shape[1]) ** 2))
            return {"hd": diag, "hd95": diag, "assd": diag, "nsd": 0.0, "defined": False}
        return {"hd": np.nan, "hd95": np.nan, "assd": np.nan, "nsd": np.nan, "defined": False}
    d2ab, d2ba = directed_d2(ea, eb), directed_d2(eb, ea)
    ab, ba = spacing * np.sqrt(d2ab.astype(np.float64)), spacing * np.sqrt(d2ba.astype(np.float64))
    if percentile_mode == "pooled":
        hd95 = float(np.percentile(np.concatenate([ab, ba]), 100 * quantile))
    else:
        hd95 = float(max(np.percentile(ab, 100 * quantile), np.percentile(ba, 100 * quantile)))
    tol2 = int(np.floor((tolerance / spacing) ** 2))
    return {"hd": float(max(ab.max(), ba.max())), "hd95": hd95, "assd": float(0.5 * (ab.mean() + ba.mean())),
            "nsd": float(((d2ab <= tol2).sum() + (d2ba <= tol2).sum()) / (na + nb)), "defined": True}


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
def blob(rng, H: int, W: int, thin: bool = True) -> np.ndarray:
    """A plane of one to three rectangles, lightly thinned (`thin`) but never to nothing: its edge set is not empty."""
    m = np.zeros((H, W), bool)
    for _ in range(int(rng.integers(1, 4))):
        h, w = int(rng.integers(1, max(2, H // 2 + 1))), int(rng.integers(1, max(2, W // 2 + 1)))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        m[y:y + h, x:x + w] = True
    if not thin:
        return m
    t = m & (rng.uniform(size=(H, W)) < 0.9)
    return t if t.any() else m


def plane_cases(rng, H: int, W: int):
    """-> (list of (name, a, b) dense boolean pairs of one shape, number of pairs with an empty side).  The contents the kernel can go
    wrong on: see tests/test_gpu_surface.py."""
    z = np.zeros((H, W), bool)
    full = np.ones((H, W), bool)
    c0, c1 = z.copy(), z.copy()
    c0[0, 0], c1[H - 1, W - 1] = True, True
    hole = full.copy()
    if H * W > 1:                      # a single pixel stays: the plane must keep an edge
        hole[H // 3:max(H // 3 + 1, 2 * H // 3), W // 3:max(W // 3 + 1, 2 * W // 3)] = False
    b1, b2 = z.copy(), z.copy()
    b1[:max(1, H // 4), :max(1, W // 4)] = True
    b2[H - max(1, H // 3):, W - max(1, W // 5):] = True
    noise_a, noise_b = rng.uniform(size=(H, W)) < 0.5, rng.uniform(size=(H, W)) < 0.5
    noise_a[0, 0] = noise_b[H - 1, 0] = True
    inner = z.copy()
    inner[H // 4:max(H // 4 + 1, H // 2), W // 4:max(W // 4 + 1, W // 2)] = True
    outer = inner.copy()
    outer[max(0, H // 4 - 2):H // 2 + 2, max(0, W // 4 - 3):W // 2 + 3] = True
    cases = [("corners", c0, c1), ("full_vs_corner", full, c0), ("hole_vs_full", hole, full), ("blobs_apart", b1, b2),
             ("noise", noise_a, noise_b), ("identical", b1, b1.copy()), ("subset", inner, outer), ("blob_pair", blob(rng, H, W), blob(rng, H, W)),
             ("a_empty", z, b2), ("b_empty", b1, z), ("both_empty", z, z)]
    return cases, 3


def pack_bits(m: np.ndarray, pad_ones: bool = False) -> np.ndarray:
    """Dense [..., H, W] bool -> packed uint8 [..., H, 8 * ceil(W / 64)]; `pad_ones` sets the padding bits X >= W."""
    m = np.asarray(m, bool)
    W = m.shape[-1]
    Wp = 64 * ((W + 63) // 64)
    full = np.full(m.shape[:-1] + (Wp,), pad_ones, bool)
    full[..., :W] = m
    return np.packbits(full, axis=-1, bitorder="little")
