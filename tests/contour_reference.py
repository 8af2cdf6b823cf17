"""The contour rule and the COCO run-length rule of include/mtbt_hip.h (`mtbt_trace_contours`, `mtbt_rle_encode`) restated in plain
Python: what the kernels must reproduce bit for bit (tests/test_cpu_contours.py holds the restatement against independent code,
tests/test_gpu_contours.py holds the kernels against the restatement).

Lattice      pixel (X, Y) is the square [X, X + 1] x [Y, Y + 1]; a vertex is an integer point (x, y), 0 <= x <= W, 0 <= y <= H, with
             key y * (W + 1) + x.
Edges        a set pixel contributes its top side heading E when the pixel above is unset, its right side heading S when the pixel to
             the right is unset, its bottom side heading W when the pixel below is unset and its left side heading N when the pixel to
             the left is unset: the set pixel lies to the right of the direction of travel.  Outside the plane is unset.
Successor    the edge that starts where e ends; where two start there (a saddle: two diagonal pixels set), connectivity 4 turns right
             (E -> S -> W -> N -> E) and connectivity 8 turns left.  The cycles of the successor are the contours.
Vertices     the start points of the edges whose predecessor has another direction.
Start        the start point of the contour's E-heading edge with the smallest key; the vertices are listed from there.
Order        the contours of a plane by the key of their start, ascending.
Area         area2 = sum(x_i * y_{i+1} - x_{i+1} * y_i): > 0 for an outer contour, < 0 for a hole.
RLE          runs of equal pixels over the plane read column-major (index x * H + y), the first run counting unset pixels.
"""
import numpy as np

E, S, W_, N = 0, 1, 2, 3
STEP = ((1, 0), (0, 1), (-1, 0), (0, -1))           # dx, dy of E, S, W, N: y grows downwards, so E -> S is a right turn


def edges(m: np.ndarray) -> dict:
    """-> {(x, y, direction)}: every directed boundary edge of a dense boolean plane, by its start point."""
    m = np.asarray(m, bool)
    H, W = m.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = m
    out = set()
    for Y, X in zip(*np.nonzero(m)):
        Y, X = int(Y), int(X)
        if not p[Y, X + 1]:
            out.add((X, Y, E))                      # top side (X, Y) -> (X + 1, Y)
        if not p[Y + 1, X + 2]:
            out.add((X + 1, Y, S))                  # right side (X + 1, Y) -> (X + 1, Y + 1)
        if not p[Y + 2, X + 1]:
            out.add((X + 1, Y + 1, W_))             # bottom side (X + 1, Y + 1) -> (X, Y + 1)
        if not p[Y + 1, X]:
            out.add((X, Y + 1, N))                  # left side (X, Y + 1) -> (X, Y)
    return out


def successor(e, all_edges, connectivity: int):
    x, y, d = e
    x, y = x + STEP[d][0], y + STEP[d][1]
    for turn in ((1, 0, 3) if connectivity == 4 else (3, 0, 1)):   # right, straight, left  /  left, straight, right
        n = (x, y, (d + turn) % 4)
        if n in all_edges:
            return n
    raise AssertionError("a boundary edge without a successor")


def trace(m: np.ndarray, connectivity: int = 4) -> list:
    """-> the contours of one dense plane in order, each a dict: `vertices` int64 [k, 2] (x, y), `start` (key), `area2`, `box`
    (x1, y1, x2, y2 of the vertices)."""
    assert connectivity in (4, 8)
    m = np.asarray(m, bool)
    H, W = m.shape
    es = edges(m)
    seen, contours = set(), []
    for e in sorted((e for e in es if e[2] == E), key=lambda e: e[1] * (W + 1) + e[0]):   # E edges by key: the first unseen one is a start
        if e in seen:
            continue
        cyc, c = [], e
        while c not in seen:
            seen.add(c)
            cyc.append(c)
            c = successor(c, es, connectivity)
        assert c == e, "the successor is a permutation"
        v = [(x, y) for i, (x, y, d) in enumerate(cyc) if cyc[i - 1][2] != d]
        assert v[0] == e[:2], "the start is a vertex"
        v = np.asarray(v, np.int64)
        nx = np.roll(v, -1, axis=0)
        contours.append({"vertices": v, "start": e[1] * (W + 1) + e[0], "area2": int((v[:, 0] * nx[:, 1] - nx[:, 0] * v[:, 1]).sum()),
                         "box": (int(v[:, 0].min()), int(v[:, 1].min()), int(v[:, 0].max()), int(v[:, 1].max()))})
    assert len(seen) == len(es)                     # every cycle holds an E-heading edge
    return contours


def records(m: np.ndarray, connectivity: int = 4, max_contours: int = 1024, max_vertices=None) -> dict:
    """What mtbt_trace_contours writes for ONE dense plane: n_vertices, n_contours, vertices [n_vertices, 2] and the tables offset [C],
    count [C], area2 [C], box [C, 4], start [C] with zeros in the rows beyond min(n_contours, C).  With n_vertices > max_vertices:
    n_contours = -1, zero tables and no vertices."""
    cs = trace(m, connectivity)
    C = int(max_contours)
    nv = sum(len(c["vertices"]) for c in cs)
    out = {"n_vertices": nv, "n_contours": len(cs), "vertices": np.zeros((0, 2), np.int64), "offset": np.zeros(C, np.int64),
           "count": np.zeros(C, np.int64), "area2": np.zeros(C, np.int64), "box": np.zeros((C, 4), np.int64), "start": np.zeros(C, np.int64)}
    if max_vertices is not None and nv > int(max_vertices):
        out["n_contours"] = -1
        return out
    if cs:
        out["vertices"] = np.concatenate([c["vertices"] for c in cs], axis=0)
    off = 0
    for i, c in enumerate(cs):
        if i < C:
            out["offset"][i], out["count"][i], out["area2"][i], out["box"][i], out["start"][i] = off, len(c["vertices"]), c["area2"], c["box"], c["start"]
        off += len(c["vertices"])
    return out


def stack_records(planes, connectivity: int = 4, max_contours: int = 1024, max_vertices=None) -> dict:
    """`records` of a stack of equally shaped planes in the layout `postprocess.trace_contours` returns: n_vertices [n], n_contours [n],
    vertices [n, V, 2] (rows from n_vertices on are zero here, unspecified on the device; V = the largest count when not given), the
    tables [n, C(, 4)] and hole [n, C]."""
    rs = [records(m, connectivity, max_contours, max_vertices) for m in planes]
    V = max([r["n_vertices"] for r in rs], default=0) if max_vertices is None else int(max_vertices)
    verts = np.zeros((len(rs), V, 2), np.int64)
    for i, r in enumerate(rs):
        verts[i, :len(r["vertices"])] = r["vertices"]
    out = {k: np.stack([r[k] for r in rs]) for k in ("offset", "count", "area2", "box", "start")}
    out.update(n_vertices=np.array([r["n_vertices"] for r in rs]), n_contours=np.array([r["n_contours"] for r in rs]), vertices=verts,
               hole=out["area2"] < 0)
    return out


def count_vertices(m: np.ndarray) -> int:
    """n_vertices of a plane from the 2 x 2 pixels around every lattice vertex: one contour vertex where one or three of them are set,
    two where exactly two diagonal ones are (either connectivity)."""
    m = np.asarray(m, bool)
    p = np.zeros((m.shape[0] + 2, m.shape[1] + 2), np.int64)
    p[1:-1, 1:-1] = m
    a, b, c, d = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    s = a + b + c + d
    return int(((s == 1) | (s == 3)).sum() + 2 * ((s == 2) & (a == d)).sum())


# ---- COCO run lengths -----------------------------------------------------------------------------------------------------------------
def rle_counts(m: np.ndarray) -> list:
    """Run lengths of a dense plane read column-major, the first run counting unset pixels (0 when pixel (0, 0) is set)."""
    flat = np.asarray(m, bool).T.ravel().tolist()
    counts, cur, run = [], False, 0
    for v in flat:
        if v != cur:
            counts.append(run)
            cur, run = v, 0
        run += 1
    counts.append(run)
    return counts


def rle_decode(counts, H: int, W: int) -> np.ndarray:
    flat = np.zeros(H * W, bool)
    pos, val = 0, False
    for c in counts:
        flat[pos:pos + int(c)] = val
        pos += int(c)
        val = not val
    assert pos == H * W
    return flat.reshape(W, H).T.copy()


def rle_to_string(counts) -> str:
    """The pycocotools compression of a count list: x[i] -= x[i - 2] for i > 2, then 5-bit groups, least significant first, 0x20 the
    continuation bit, the last group's bit 0x10 the sign, each group + 48 as ASCII."""
    out = []
    counts = [int(c) for c in counts]
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1F
            x >>= 5                                 # arithmetic: -1 stays -1
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def rle_from_string(s: str) -> list:
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
def hand_planes() -> list:
    """-> list of (name, dense bool plane): the contents the rule is read off by hand on."""
    single = np.zeros((3, 3), bool)
    single[1, 1] = True
    saddle = np.array([[1, 0], [0, 1]], bool)
    ring = np.zeros((5, 5), bool)
    ring[1:4, 1:4] = True
    ring[2, 2] = False
    island = np.zeros((7, 9), bool)
    island[1:6, 1:8] = True
    island[2:5, 2:7] = False
    island[3, 4] = True
    touch = np.ones((4, 4), bool)                   # the hole at (1, 1) meets the outer contour at the vertex (1, 1): pixel (0, 0) is unset
    touch[0, 0] = touch[1, 1] = False
    border = np.zeros((6, 8), bool)
    border[0] = border[-1] = border[:, 0] = border[:, -1] = True
    return [("single", single), ("saddle", saddle), ("ring", ring), ("ring_island", island), ("hole_touches_outer", touch),
            ("border", border)]
