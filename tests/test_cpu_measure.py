"""THE MEASURE RULE without a GPU: the restatement (tests/measure_reference.py) against independent routes -- scipy.spatial.ConvexHull and
pdist over ALL corners, float64 projections on every hull-edge normal, np.nonzero sums, padded differences, scipy.ndimage.label, closed
forms, ties, the eight dihedral views -- then csrc/measure_exact.h as a host program against Python ints, the C ABI's refusals, and
`region_properties` on the restatement's tables."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage
from scipy.spatial import ConvexHull
from scipy.spatial.distance import pdist

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import measure_components, measure_detections, measure_regions, region_properties   # exported  # noqa: F401
from multitask_bonetumor_yolo_amd import postprocess as P

import components_reference as CR
import measure_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
PTR = 4096                                       # non-null, aligned dummy: every call below is refused before any launch
SHAPES = [(1, 1), (1, 70), (37, 64), (33, 65), (40, 130), (96, 200)]
RTOL = 1e-9                                      # float64 rounding of a few operations on values <= 2^30


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def all_cases():
    """(name, plane) over the six shapes plus one disc."""
    out = []
    for i, (H, W) in enumerate(SHAPES):
        rng = np.random.default_rng(40 + i)
        out += [(f"{H}x{W}:{name}", m) for name, m in CR.plane_cases(rng, H, W) + R.extra_cases(rng, H, W)]
    out.append(("disc_r30", R.disc(70, 80, 33, 41, 30)))
    return out


CASES = all_cases()


# ---- the restatement against independent routes ------------------------------------------------------------------------------------
def _max_d2(corners):
    """The largest squared distance over ALL corners: pdist, or the same in row blocks where its matrix would not fit."""
    if len(corners) <= 4000:
        return int(round(pdist(corners, "sqeuclidean").max()))
    sq = (corners ** 2).sum(axis=1)                                                        # integers below 2^53: float64 holds them exactly
    return max(int((sq[i:i + 1024, None] + sq[None, :] - 2.0 * (corners[i:i + 1024] @ corners.T)).max()) for i in range(0, len(corners), 1024))


def _independent(name, m):
    rec = R.measure_plane(m)
    H, W = m.shape
    ys, xs = np.nonzero(m)
    if len(xs) == 0:
        assert rec == {"sums": [0] * 8, "hull": [], "hull_area2": 0, "caliper": [0] * 8, "caliper_at": [0] * 8}, name
        return
    # sums against np.nonzero, the perimeter against padded differences
    x, y = xs.astype(np.int64), ys.astype(np.int64)
    pad = np.pad(m, 1).astype(np.int8)
    per = int(np.abs(np.diff(pad, axis=0)).sum() + np.abs(np.diff(pad, axis=1)).sum())
    assert rec["sums"] == [len(x), per, int(x.sum()), int(y.sum()), int((x * x).sum()), int((x * y).sum()), int((y * y).sum()), 0], name
    # hull vertex set and area against scipy over the corner set
    corners = np.array(sorted(R.corner_set(list(zip(xs.tolist(), ys.tolist())))), dtype=np.float64)
    hull = ConvexHull(corners)
    poly = np.array(rec["hull"], dtype=np.float64)
    assert {tuple(v) for v in corners[hull.vertices].astype(int).tolist()} == set(rec["hull"]), name
    assert rec["hull_area2"] > 0 and abs(hull.volume - rec["hull_area2"] / 2) <= 1e-9 * hull.volume, name
    h = len(poly)
    assert h >= 4 and len(set(rec["hull"])) == h
    keys = [py * (W + 1) + px for px, py in rec["hull"]]
    assert keys[0] == min(keys) and rec["hull"][1][1] == rec["hull"][0][1] and rec["hull"][1][0] > rec["hull"][0][0], name   # leaves its start heading E
    e = np.roll(poly, -1, axis=0) - poly
    turn = e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0]
    assert (turn > 0).all(), name                                                          # strictly convex, one sense
    # d2 against pdist over ALL corners; the pair attains it and is the first such pair
    cal, at = rec["caliper"], rec["caliper_at"]
    assert cal[0] == _max_d2(corners), name
    pa, pb = (at[0], at[1]), (at[2], at[3])
    ia, ib = rec["hull"].index(pa), rec["hull"].index(pb)
    assert ia < ib and (pa[0] - pb[0]) ** 2 + (pa[1] - pb[1]) ** 2 == cal[0], name
    firsts = [(i, j) for i in range(h) for j in range(i + 1, h) if int(((poly[i] - poly[j]) ** 2).sum()) == cal[0]]
    assert firsts[0] == (ia, ib), name
    # perp: the spread of ALL corners across the diameter
    u = np.array([pb[0] - pa[0], pb[1] - pa[1]], dtype=np.float64)
    c = u[0] * (corners[:, 1] - pa[1]) - u[1] * (corners[:, 0] - pa[0])
    assert cal[1] == int(round(c.max() - c.min())), name
    # width and minimum rectangle against float64 projections of all corners on every hull-edge normal
    ln = np.sqrt((e ** 2).sum(axis=1))
    rel = corners[None, :, :] - poly[:, None, :]
    hs = np.abs(e[:, None, 0] * rel[:, :, 1] - e[:, None, 1] * rel[:, :, 0]).max(axis=1) / ln
    ts = (e[:, None, 0] * rel[:, :, 0] + e[:, None, 1] * rel[:, :, 1])
    spans = (ts.max(axis=1) - ts.min(axis=1)) / ln
    width, rect = cal[2] / math.sqrt(cal[3]), cal[4] * cal[5] / cal[7]
    assert abs(width - hs.min()) <= RTOL * width and abs(rect - (hs * spans).min()) <= RTOL * rect, name
    for k, vals, edge in ((0, hs, at[4]), (1, hs * spans, at[6])):
        order = np.sort(vals)
        if order[1] - order[0] > RTOL * order[1]:                                          # the argmin only where float64 can tell
            assert int(np.argmin(vals)) == edge, (name, k)
        assert vals[edge] - order[0] <= RTOL * order[1], (name, k)
    (px, py), (nx, ny) = rec["hull"][at[4]], rec["hull"][(at[4] + 1) % h]
    assert cal[3] == (nx - px) ** 2 + (ny - py) ** 2
    qx, qy = rec["hull"][at[5]]
    assert abs((nx - px) * (qy - py) - (ny - py) * (qx - px)) == cal[2], name              # w_vertex attains w_num


@pytest.mark.parametrize("k", range(len(CASES)), ids=[n for n, _ in CASES])
def test_restatement_against_scipy_and_numpy(k):
    _independent(*CASES[k])


def test_label_mode_is_plane_mode_per_component():
    rng = np.random.default_rng(3)
    for H, W in ((37, 64), (40, 130)):
        for name, m in CR.plane_cases(rng, H, W):
            for structure in (ndimage.generate_binary_structure(2, 1), np.ones((3, 3), bool)):
                lab, n = ndimage.label(m, structure=structure)
                C_ = 16
                got = R.measure_labels(lab, C_)
                for i in range(1, C_ + 1):
                    want = R.measure_plane(lab == i)
                    if i <= n:
                        # the perimeter of a component alone is its perimeter in the map: other labels are "not this region"
                        assert got[i - 1] == want, (name, i)
                    else:
                        assert got[i - 1]["sums"] == [0] * 8 and got[i - 1]["hull"] == []
    lab = rng.integers(-2, 9, size=(33, 65))                                              # an arbitrary map: regions need not be connected
    got = R.measure_labels(lab, 5)
    for i in range(1, 6):
        assert got[i - 1] == R.measure_plane(lab == i)


def test_closed_forms_and_ties():
    for a, b, x0, y0 in ((5, 3, 2, 1), (1, 1, 0, 0), (7, 7, 3, 4), (2, 9, 60, 0), (70, 1, 0, 5)):
        m = np.zeros((12, 140), bool)
        m[y0:y0 + b, x0:x0 + a] = True
        rec = R.measure_plane(m)
        assert rec["hull"] == [(x0, y0), (x0 + a, y0), (x0 + a, y0 + b), (x0, y0 + b)] and rec["hull_area2"] == 2 * a * b
        cal, at = rec["caliper"], rec["caliper_at"]
        assert cal[0] == a * a + b * b and at[:4] == [x0, y0, x0 + a, y0 + b]             # of the two diagonals the one from vertex 0
        assert cal[1] == 2 * a * b                                                        # both other corners, a b off the diagonal each
        assert cal[2] ** 2 * 1 == min(a, b) ** 2 * cal[3] and cal[4] * cal[5] == a * b * cal[7]
        assert at[4] == (0 if b <= a else 1) and at[6] == 0                                # ties go to the smallest edge
        assert rec["sums"][:2] == [a * b, 2 * (a + b)]
        props = region_properties({k: torch.from_numpy(v) for k, v in R.tables([[rec]], 8).items()})
        assert abs(props["mu20"][0, 0] - a * a / 12) < 1e-9 and abs(props["mu02"][0, 0] - b * b / 12) < 1e-9
        assert abs(props["feret_min"][0, 0] - min(a, b)) < 1e-12 and abs(props["min_rect_area"][0, 0] - a * b) < 1e-9
        assert np.allclose(props["centroid"][0, 0], [x0 + a / 2, y0 + b / 2]) and props["solidity"][0, 0] == 1.0
        assert np.allclose(props["min_rect"][0, 0], [(x0, y0), (x0 + a, y0), (x0 + a, y0 + b), (x0, y0 + b)], atol=1e-9)
    for Ld in (1, 2, 5, 33):                                                              # a one-pixel diagonal: collinear corners all along
        m = np.zeros((Ld + 2, Ld + 3), bool)
        d = np.arange(Ld)
        m[d + 1, d + 2] = True
        rec = R.measure_plane(m)
        want = [(2, 1), (3, 1), (Ld + 2, Ld), (Ld + 2, Ld + 1), (Ld + 1, Ld + 1), (2, 2)]
        assert rec["hull"] == (want if Ld > 1 else [(2, 1), (3, 1), (3, 2), (2, 2)])
        assert rec["caliper"][0] == 2 * Ld * Ld
    dm = R.diamond(21, 21, 10, 10, 6)                                                     # equal widths on several edges: the smallest wins
    rec = R.measure_plane(dm)
    per_edge = []
    h = len(rec["hull"])
    for i in range(h):
        (px, py), (nx, ny) = rec["hull"][i], rec["hull"][(i + 1) % h]
        hi = max(abs(R.cross(nx - px, ny - py, qx - px, qy - py)) for qx, qy in rec["hull"])
        per_edge.append(R.Fraction(hi * hi, (nx - px) ** 2 + (ny - py) ** 2))
    assert per_edge.count(min(per_edge)) >= 2 and rec["caliper_at"][4] == per_edge.index(min(per_edge))


def test_sizes_are_invariant_under_the_dihedral_views():
    rng = np.random.default_rng(9)
    blob = R.disc(40, 50, 18, 22, 13) | R.disc(40, 50, 25, 30, 9)                         # one pair attains its diameter
    for m in (CR.big_plane(rng, 48), blob, R.disc(40, 50, 18, 22, 13), dict(CR.plane_cases(rng, 33, 65))["noise_593"]):
        base = R.measure_plane(m)
        hp = base["hull"]
        ties = sum((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 == base["caliper"][0] for i, a in enumerate(hp) for b in hp[i + 1:])
        # the extent across the diameter is a size only where one pair attains the diameter: among several the rule picks by index
        perp = (lambda r: r["caliper"][1]) if ties == 1 else (lambda r: None)
        want = (base["sums"][:2], len(base["hull"]), base["hull_area2"], base["caliper"][0], perp(base),
                R.Fraction(base["caliper"][2] ** 2, base["caliper"][3]), R.Fraction(base["caliper"][4] * base["caliper"][5], base["caliper"][7]))
        for k in range(4):
            for flip in (False, True):
                v = np.rot90(m, k)
                v = v[:, ::-1] if flip else v
                rec = R.measure_plane(np.ascontiguousarray(v))
                got = (rec["sums"][:2], len(rec["hull"]), rec["hull_area2"], rec["caliper"][0], perp(rec),
                       R.Fraction(rec["caliper"][2] ** 2, rec["caliper"][3]), R.Fraction(rec["caliper"][4] * rec["caliper"][5], rec["caliper"][7]))
                assert got == want, (k, flip)


def test_the_big_quadrilateral_needs_more_than_64_bits():
    rec = R.measure_pixels(R.BIG_FOUR, 16384)
    assert rec["sums"][0] == 4 and len(rec["hull"]) >= 4
    assert max(R.width_products(rec["hull"])) > 2 ** 64                                    # a 64-bit word would wrap


# ---- csrc/measure_exact.h as a host program ------------------------------------------------------------------------------------------
def _exact_lines(rng):
    lines, want = [], []
    big = lambda bits: int(rng.integers(0, 2 ** 62)) % (2 ** bits)
    for _ in range(300):
        a, b = big(int(rng.integers(1, 64))), big(int(rng.integers(1, 64)))
        lines.append(f"mul {a} {b}")
        want.append(f"{(a * b) >> 64} {(a * b) & (2 ** 64 - 1)}")
    lines.append(f"mul {2 ** 64 - 1} {2 ** 64 - 1}")
    want.append(f"{((2 ** 64 - 1) ** 2) >> 64} {((2 ** 64 - 1) ** 2) & (2 ** 64 - 1)}")
    sign = lambda v: (v > 0) - (v < 0)
    for _ in range(300):
        h1, h2, l1, l2 = big(29) + 1, big(29) + 1, big(29) + 1, big(29) + 1
        lines.append(f"width {h1} {l1} {h2} {l2}")
        want.append(str(sign(h1 * h1 * l2 - h2 * h2 * l1)))
        t1, t2 = big(30) + 1, big(30) + 1
        lines.append(f"rect {h1} {t1} {l1} {h2} {t2} {l2}")
        want.append(str(sign(h1 * t1 * l2 - h2 * t2 * l1)))
    # pairs that differ only below bit 64: h1^2 l2 and h2^2 l1 with equal high words
    for h, l in ((2 ** 29 - 1, 2 ** 29 - 3), (2 ** 29 - 5, 2 ** 28 + 1), (2 ** 28 + 12345, 2 ** 29 - 7)):
        for dl in (-1, 0, 1):
            a, b = h * h * (l + dl), h * h * l
            assert a >> 64 == b >> 64 and a >= 2 ** 64
            lines.append(f"width {h} {l} {h} {l + dl}")
            want.append(str(sign(a - b)))
            lines.append(f"rect {h} {h} {l} {h} {h} {l + dl}")
            want.append(str(sign(a - b)))
    return lines, want


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan"])
def test_measure_exact_alone_against_python_ints(tmp_path, sanitize):
    exe = str(tmp_path / "measure_exact")
    flags = ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + flags + ["-I" + B.CSRC, os.path.join(ROOT, "tests", "measure_exact_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines, want = _exact_lines(np.random.default_rng(11))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    got = r.stdout.strip().splitlines()
    assert re.fullmatch(rf"measure_exact: {len(lines)} lines ok", got[-1]) and got[:-1] == want


# ---- the entry point's refusals, without a GPU ------------------------------------------------------------------------------------------
def _call(lib, **over):
    a = L.MeasureArgs()
    H, W = over.get("H", 37), over.get("W", 70)
    vals = dict(packed=PTR, labels=None, workspace=PTR, workspace_bytes=1 << 40, sums=PTR, n_hull=PTR, hull=PTR, hull_area2=PTR, caliper=PTR,
                caliper_at=PTR, n=2, H=H, W=W, pitch=8 * ((W + 63) // 64), max_regions=1, max_hull=64)
    vals.update(over)
    reserved = vals.pop("reserved", (0, 0))
    for k, v in vals.items():
        setattr(a, k, v)
    a.reserved[0], a.reserved[1] = reserved
    return lib.mtbt_measure_regions(C.byref(a), None)


def test_entry_point_refuses_bad_arguments_before_any_launch(lib):
    assert lib.mtbt_sizeof_measure_args(0) == C.sizeof(L.MeasureArgs) and lib.mtbt_sizeof_measure_args(1) == -1
    assert lib.mtbt_measure_regions(None, None) == EINVAL
    assert _call(lib, n=0) == 0                                                            # n == 0 launches nothing
    for k in ("sums", "n_hull", "hull_area2", "caliper", "caliper_at", "workspace"):
        assert _call(lib, **{k: None}) == EINVAL, k
    assert _call(lib, packed=None) == EINVAL                                               # neither planes nor labels
    assert _call(lib, pitch=8) == EINVAL and _call(lib, pitch=24) == EINVAL
    for dim in ("H", "W"):
        for v in (0, 16385, -1):
            assert _call(lib, **{dim: v, "pitch": 16}) == EINVAL, (dim, v)
    for c in (0, 65537, -3):
        assert _call(lib, labels=PTR, max_regions=c) == EINVAL, c
    assert _call(lib, max_regions=2) == EINVAL                                             # plane mode has one region
    assert _call(lib, max_hull=3) == EINVAL and _call(lib, n=-1) == EINVAL
    assert _call(lib, reserved=(0, 1)) == EINVAL and _call(lib, reserved=(7, 0)) == EINVAL
    need = lib.mtbt_measure_workspace_bytes(2, 37, 70, 5)
    assert need == 16 * ((2 * 5 * 2 * 38 * 4 + 15) // 16)                                  # 8 bytes per (region, lattice row)
    assert _call(lib, labels=PTR, max_regions=5, workspace_bytes=need - 1) == EINVAL
    for k, off in (("packed", 4), ("sums", 4), ("hull_area2", 4), ("caliper", 4), ("workspace", 8), ("n_hull", 2), ("hull", 2), ("caliper_at", 2)):
        assert _call(lib, **{k: PTR + off}) == EALIGN, k
    assert _call(lib, labels=PTR + 2, max_regions=5) == EALIGN
    assert _call(lib, sums=PTR + 4, max_hull=3) == EINVAL                                  # invalid and misaligned together is MTBT_EINVAL
    for bad in ((-1, 37, 70, 1), (1, 0, 70, 1), (1, 37, 16385, 1), (1, 37, 70, 0), (1, 37, 70, 65537)):
        assert lib.mtbt_measure_workspace_bytes(*bad) == EINVAL, bad
    assert lib.mtbt_measure_workspace_bytes(0, 37, 70, 1) == 0
    assert lib.mtbt_measure_workspace_bytes(1, 16384, 16384, 1) == 16 * ((2 * 16385 * 4 + 15) // 16)


def test_python_refusals_need_no_device():
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.measure_regions(torch.zeros(1, 4, 8, dtype=torch.uint8), 40)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.measure_regions(None, 40, labels=torch.zeros(1, 4, 40, dtype=torch.int32))


def test_region_properties_on_the_restatement():
    m = R.disc(70, 80, 33, 41, 30)
    rec = R.measure_plane(m)
    tabs = {k: torch.from_numpy(v) for k, v in R.tables([[rec], [R.measure_plane(np.zeros((70, 80), bool))]], 512).items()}
    p1, p2 = region_properties(tabs), region_properties(tabs, spacing=0.5)
    A = float(m.sum())
    assert p1["area"][0, 0] == A and p2["area"][0, 0] == A / 4 and p2["feret_max"][0, 0] == p1["feret_max"][0, 0] / 2
    assert abs(p1["feret_max"][0, 0] - math.sqrt(rec["caliper"][0])) < 1e-12 and 60 < p1["feret_min"][0, 0] <= p1["feret_perp"][0, 0] + 1e-9
    assert abs(p1["feret_perp"][0, 0] - rec["caliper"][1] / math.sqrt(rec["caliper"][0])) < 1e-9
    assert np.allclose(p1["centroid"][0, 0], [41.5, 33.5]) and abs(p1["major_axis"][0, 0] - p1["equivalent_diameter"][0, 0]) < 0.2 and p1["eccentricity"][0, 0] < 0.05
    assert abs(p1["equivalent_diameter"][0, 0] - math.sqrt(4 * A / math.pi)) < 1e-9 and 0.95 < p1["solidity"][0, 0] < 1.0
    assert abs(p1["who_product"][0, 0] - p1["feret_max"][0, 0] * p1["feret_perp"][0, 0]) < 1e-9
    # the rectangle: four corners, its area h t / len2, every hull vertex inside it
    rect = p1["min_rect"][0, 0]
    side = lambda a, b: math.hypot(*(rect[b] - rect[a]))
    assert abs(side(0, 1) * side(1, 2) - p1["min_rect_area"][0, 0]) < 1e-6
    for qx, qy in rec["hull"]:
        for i in range(4):
            e, d = rect[(i + 1) % 4] - rect[i], np.array([qx, qy]) - rect[i]
            assert e[0] * d[1] - e[1] * d[0] > -1e-6
    # the empty region: sizes 0, ratios NaN
    assert p1["area"][1, 0] == 0 and p1["feret_max"][1, 0] == 0 and p1["hull_area"][1, 0] == 0 and p1["major_axis"][1, 0] == 0
    assert all(np.isnan(p1[k][1, 0]).all() for k in ("centroid", "solidity", "orientation", "eccentricity", "min_rect"))
    # orientation of a bar along x and along the diagonal
    bar = np.zeros((20, 40), bool)
    bar[5:8, 3:30] = True
    t = {k: torch.from_numpy(v) for k, v in R.plane_tables([bar, np.eye(20, dtype=bool)], 16).items()}
    o = region_properties(t)["orientation"]
    assert abs(o[0, 0]) < 1e-12 and abs(o[1, 0] - math.pi / 4) < 1e-12
