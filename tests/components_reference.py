"""Numpy restatement of connected-component labelling of binary planes (include/mtbt_hip.h, `mtbt_label_components` and
`mtbt_select_components`; `metrics.LesionMetrics`), written for clarity as a plain flood fill: the yardstick of
tests/test_cpu_components.py (against scipy.ndimage) and tests/test_gpu_components.py (bit for bit).

  labels        0 = background; the components are numbered 1, 2, ... in row-major order of their first pixel
  records       per id: area, box x1 y1 x2 y2 (exclusive maxima), flat index of the first pixel, overlap with a second plane
  select rule   a component is kept when area >= min_area and, with keep_largest = k > 0, fewer than k components come before it in
                the order (larger area first, lower id first among equal areas)
  lesion counts found ground-truth components and true predicted components, the integers behind `LesionMetrics`
"""
import numpy as np

from surface_reference import pack_bits  # noqa: F401  (the packed layout is the same)


def label(m: np.ndarray, connectivity: int = 4):
    """-> (int32 [H, W] label map, number of components) of a dense boolean plane."""
    assert connectivity in (4, 8)
    m = np.asarray(m, bool)
    H, W = m.shape
    P = W + 2
    pad = np.zeros((H + 2, P), np.int64)
    pad[1:-1, 1:-1] = -m.astype(np.int64)                     # -1: set and not yet labelled
    flat = pad.ravel().tolist()
    steps = (-P, -1, 1, P) + ((-P - 1, -P + 1, P - 1, P + 1) if connectivity == 8 else ())
    n = 0
    for s in np.flatnonzero(pad.ravel()).tolist():            # ascending flat index = row-major order
        if flat[s] != -1:
            continue
        n += 1
        flat[s] = n
        stack = [s]
        while stack:
            v = stack.pop()
            for o in steps:
                if flat[v + o] == -1:
                    flat[v + o] = n
                    stack.append(v + o)
    return np.array(flat, np.int32).reshape(H + 2, P)[1:-1, 1:-1].copy(), n


def records(m: np.ndarray, connectivity: int = 4, max_components: int = 1024, other=None) -> dict:
    """What mtbt_label_components writes for ONE dense plane: labels, n_components, and the tables area [C], box [C, 4], first [C],
    inter [C] (None without `other`) with zeros in the rows beyond n_components; `areas` holds the area of EVERY id."""
    lab, n = label(m, connectivity)
    H, W = lab.shape
    C = int(max_components)
    areas = np.bincount(lab.ravel(), minlength=n + 1)[1:].astype(np.int64)
    area, box, first = np.zeros(C, np.int64), np.zeros((C, 4), np.int64), np.zeros(C, np.int64)
    inter = None if other is None else np.zeros(C, np.int64)
    ys, xs = np.nonzero(lab)
    ids = lab[ys, xs]
    for i in range(1, min(n, C) + 1):
        sel = ids == i
        y, x = ys[sel], xs[sel]
        area[i - 1] = len(y)
        box[i - 1] = (x.min(), y.min(), x.max() + 1, y.max() + 1)
        first[i - 1] = (y * W + x).min()
        if other is not None:
            inter[i - 1] = int(np.asarray(other, bool)[y, x].sum())
    return {"labels": lab, "n_components": n, "area": area, "box": box, "first": first, "inter": inter, "areas": areas}


def keep_rule(areas: np.ndarray, min_area: int = 0, keep_largest=None) -> np.ndarray:
    """bool [n_components]: which ids (id i at [i - 1]) the select rule keeps.  Written as counts, not as a sort."""
    a = np.asarray(areas, np.int64)
    keep = a >= int(min_area)
    k = int(keep_largest or 0)
    if k > 0:
        before = np.zeros(len(a), np.int64)                   # components that come before id i: larger, or equal and of a lower id
        for v in np.unique(a):
            idx = np.flatnonzero(a == v)
            before[idx] = int((a > v).sum()) + np.arange(len(idx))
        keep &= before < k
    return keep


def select(m: np.ndarray, connectivity: int = 4, min_area: int = 0, keep_largest=None):
    """-> (dense bool plane of the kept components, their number)."""
    lab, n = label(m, connectivity)
    keep = keep_rule(np.bincount(lab.ravel(), minlength=n + 1)[1:], min_area, keep_largest)
    return np.concatenate([[False], keep])[lab], int(keep.sum())


def lesion_counts(pred: np.ndarray, gt: np.ndarray, overlap: float = 0.0, min_area: int = 0, connectivity: int = 4,
                  max_components: int = 1024) -> dict:
    """The integers `LesionMetrics` pools for ONE image: n_gt, n_found, n_pred, n_true and `truncated` (a side with more than
    max_components components: the excess counts as not found / false)."""
    pred, gt = np.asarray(pred, bool), np.asarray(gt, bool)
    if min_area > 0:
        pred = select(pred, connectivity, min_area)[0]
    out = {}
    trunc = False
    for name, hit, a, b in (("gt", "found", gt, pred), ("pred", "true", pred, gt)):
        r = records(a, connectivity, max_components, other=b)
        n = min(r["n_components"], max_components)
        area, inter = r["area"][:n], r["inter"][:n]
        ok = (inter >= 1) & (inter.astype(np.float64) >= np.float64(overlap) * area.astype(np.float64))
        out[f"n_{name}"], out[f"n_{hit}"] = r["n_components"], int(ok.sum())
        trunc |= r["n_components"] > max_components
    out["truncated"] = bool(trunc)
    return out


def lesion_metrics(counts) -> dict:
    """`LesionMetrics.compute()` from a list of `lesion_counts`."""
    tot = {k: sum(int(c[k]) for c in counts) for k in ("n_gt", "n_found", "n_pred", "n_true")}
    rec = tot["n_found"] / tot["n_gt"] if tot["n_gt"] else 0.0
    prec = tot["n_true"] / tot["n_pred"] if tot["n_pred"] else 0.0
    return {"lesion_recall": rec, "lesion_precision": prec, "lesion_f1": 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0,
            "fp_per_image": (tot["n_pred"] - tot["n_true"]) / len(counts) if counts else 0.0,
            "n_gt": tot["n_gt"], "n_pred": tot["n_pred"], "n_images": len(counts), "n_truncated": sum(bool(c["truncated"]) for c in counts)}


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
def plane_cases(rng, H: int, W: int):
    """-> list of (name, dense bool plane) of one shape: the contents a labelling kernel can go wrong on (tests/test_gpu_components.py)."""
    z = np.zeros((H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    corners = z.copy()
    corners[0, 0] = corners[0, W - 1] = corners[H - 1, 0] = corners[H - 1, W - 1] = True
    serp = z.copy()                                           # one component: the longest chain of links
    serp[0::2] = True
    serp[1::4, W - 1] = True
    serp[3::4, 0] = True
    u = z.copy()                                              # the arms join only in the last row
    u[:, 0] = u[:, W - 1] = u[H - 1] = True
    comb = z.copy()
    comb[:, 0::4] = True
    comb[H - 1] = True
    if H >= 3:
        comb[0, 2::8] = True                                  # detached single pixels between the teeth: components of equal area
    bar = z.copy()                                            # a bar and a diagonal across the word boundaries 63|64 and 127|128
    bar[H - 1, min(60, W - 1):min(W, 132)] = True
    for x0 in (60, 124):
        for i in range(min(8, max(H - 2, 0))):
            if x0 + i < W:
                bar[i, x0 + i] = True
    diag = z.copy()
    d = np.arange(min(H, W))
    diag[d, d] = True
    return [("empty", z), ("full", ~z), ("corners", corners), ("checker", (yy + xx) % 2 == 0), ("serpentine", serp), ("u", u),
            ("comb", comb), ("bar_diagonal", bar), ("diagonal", diag), ("noise_500", rng.uniform(size=(H, W)) < 0.5),
            ("noise_593", rng.uniform(size=(H, W)) < 0.593)]


def big_plane(rng, S: int = 640) -> np.ndarray:
    """A blob with a hole, a detached island and specks at p = 0.02."""
    yy, xx = np.mgrid[0:S, 0:S]
    m = (yy - 0.45 * S) ** 2 + (xx - 0.5 * S) ** 2 < (0.3 * S) ** 2
    m &= ~((yy - 0.4 * S) ** 2 + (xx - 0.55 * S) ** 2 < (0.08 * S) ** 2)
    m[S - 40:S - 30, 5:9] = True
    return m | (rng.uniform(size=(S, S)) < 0.02)
