"""The polygon fill rule (include/mtbt_hip.h `mtbt_fill_polygons`) and the host label movement, on the CPU: the restatement in
tests/polygon_reference.py against its own scalar form, against a float64 crossing number and matplotlib, the properties the rule
promises, `augment_polygons` / `mosaic_polygons` against the box rule, and the entry point's early returns and struct layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import polygon_reference as R
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import preprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_polygon(rng, H, W, n=None, spread=1.3):
    n = int(rng.integers(3, 10)) if n is None else n
    return np.stack([rng.uniform(-(spread - 1) * W, spread * W, n), rng.uniform(-(spread - 1) * H, spread * H, n)], axis=1)


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (7, 9), (12, 70), (40, 130)])
def test_fill_equals_the_scalar_rule(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    cases = [(n, p) for n, p in R.polygon_cases(rng, H, W) if sum(len(q) for q in p) <= 40]
    assert len(cases) >= 20
    for k, (name, plane) in enumerate(cases):
        clip = None if k % 3 else (W // 4, H // 3, W - W // 5, H - H // 4)
        assert np.array_equal(R.fill(plane, H, W, clip), R.fill_scalar(plane, H, W, clip)), name


def _crossing_number_float(poly, H, W):
    """The textbook even-odd test with a division, in float64, on the quantised vertices and pixel centres."""
    q = R.quantise(poly).astype(np.float64)
    xc, yc = np.meshgrid(16.0 * np.arange(W) + 8.0, 16.0 * np.arange(H) + 8.0)
    inside = np.zeros((H, W), dtype=bool)
    for i in range(len(q)):
        (ax, ay), (bx, by) = q[i], q[(i + 1) % len(q)]
        if ay == by:
            continue
        cross = (ay <= yc) != (by <= yc)
        xi = ax + (yc - ay) * (bx - ax) / (by - ay)
        inside ^= cross & (xc < xi)
    return inside


def test_fill_equals_a_float64_crossing_number_on_random_polygons():
    rng = np.random.default_rng(5)
    pixels = 0
    for k in range(60):
        H, W = int(rng.integers(20, 70)), int(rng.integers(20, 90))
        poly = _random_polygon(rng, H, W)
        assert np.array_equal(R.fill([poly], H, W), _crossing_number_float(poly, H, W)), k
        pixels += H * W
    assert pixels > 100000


def test_fill_agrees_with_matplotlib_away_from_the_edges():
    mpath = pytest.importorskip("matplotlib.path")
    rng = np.random.default_rng(6)
    H, W = 48, 80
    xc, yc = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    pts = np.stack([xc.ravel(), yc.ravel()], axis=1)
    for k in range(12):
        tri = _random_polygon(rng, H, W, n=3)
        q = R.quantise(tri) / 16.0
        a, b = q, np.roll(q, -1, axis=0)
        d = b - a
        t = np.clip(((pts[:, None, :] - a[None]) * d[None]).sum(-1) / np.maximum((d * d).sum(-1), 1e-30)[None], 0.0, 1.0)
        dist = np.linalg.norm(pts[:, None, :] - (a[None] + t[..., None] * d[None]), axis=-1).min(axis=1)
        far = (dist >= 0.125).reshape(H, W)
        want = mpath.Path(q).contains_points(pts).reshape(H, W)
        got = R.fill([tri], H, W)
        assert far.sum() > 0.8 * H * W and np.array_equal(got[far], want[far]), k


# ---- the properties the rule promises --------------------------------------------------------------------------------------------------
def test_start_vertex_and_direction_do_not_matter():
    rng = np.random.default_rng(7)
    for k in range(20):
        H, W = 33, 70
        poly = _random_polygon(rng, H, W)
        want = R.fill([poly], H, W)
        for s in range(len(poly)):
            assert np.array_equal(R.fill([np.roll(poly, s, axis=0)], H, W), want)
            assert np.array_equal(R.fill([np.roll(poly, s, axis=0)[::-1]], H, W), want)


def test_a_shared_edge_is_watertight():
    rng = np.random.default_rng(8)
    H, W = 40, 70
    for k in range(30):
        a, b = rng.uniform(-5, 75, 2), rng.uniform(-5, 75, 2)          # the shared edge; c and d on either side of it
        a[1], b[1] = rng.uniform(-5, 45), rng.uniform(-5, 45)
        nrm = np.array([-(b - a)[1], (b - a)[0]])
        c, d = (a + b) / 2 + rng.uniform(0.2, 1.0) * nrm, (a + b) / 2 - rng.uniform(0.2, 1.0) * nrm
        one, two = R.fill([[a, b, c]], H, W), R.fill([[b, a, d]], H, W)
        assert not (one & two).any(), k
        assert np.array_equal(one | two, R.fill([[a, d, b, c]], H, W)), k       # the quadrilateral without the diagonal (convex at a and b)


def test_a_rectangle_sets_exactly_the_centres_inside_its_quantised_sides():
    rng = np.random.default_rng(9)
    H, W = 37, 130
    for k in range(40):
        x1, x2 = np.sort(rng.uniform(-10, W + 10, 2))
        y1, y2 = np.sort(rng.uniform(-10, H + 10, 2))
        if k % 4 == 0:
            x1, y1, x2, y2 = np.floor(x1) + 0.5, np.floor(y1) + 0.5, np.floor(x2) + 0.5, np.floor(y2) + 0.5   # sides on pixel centres
        qx1, qy1, qx2, qy2 = (int(v) for v in R.quantise([x1, y1, x2, y2]))
        xc, yc = 16 * np.arange(W) + 8, 16 * np.arange(H) + 8
        want = ((qy1 <= yc) & (yc < qy2))[:, None] & ((qx1 <= xc) & (xc < qx2))[None, :]
        assert np.array_equal(R.fill([[[x1, y1], [x2, y1], [x2, y2], [x1, y2]]], H, W), want), k


def test_the_threshold_form_equals_the_pixel_form():
    """What the kernel evaluates per 64-pixel word: a crossing edge toggles X < t, t = ceil(num / den) clamped to [0, W]."""
    rng = np.random.default_rng(10)
    H, W = 30, 150
    for k in range(30):
        poly = _random_polygon(rng, H, W, spread=2.0)
        q = [(int(x), int(y)) for x, y in R.quantise(poly)]
        got = np.zeros((H, W), dtype=bool)
        for Y in range(H):
            yc = 16 * Y + 8
            for i in range(len(q)):
                (ax, ay), (bx, by) = q[i], q[(i + 1) % len(q)]
                if (ay <= yc) == (by <= yc):
                    continue
                if ay > by:
                    ax, ay, bx, by = bx, by, ax, ay
                num, den = (bx - ax) * (yc - ay) + (ax - 8) * (by - ay), 16 * (by - ay)
                t = min(max(-((-num) // den), 0), W)
                got[Y, :t] ^= True
        assert np.array_equal(got, R.fill([poly], H, W)), k


def test_pack_bits_and_records():
    m = np.zeros((5, 70), dtype=bool)
    m[1, 3] = m[3, 69] = m[2, 64] = True
    p = R.pack_bits(m)
    assert p.shape == (5, 16) and p[1, 0] == 8 and p[3, 8] == 32 and p[2, 8] == 1 and int(p.sum()) == 41
    assert R.records(m) == (3, [3, 1, 70, 4]) and R.records(np.zeros((4, 4), dtype=bool)) == (0, [0, 0, 0, 0])


def test_the_3000_gon_is_quick():
    import time
    t0 = time.perf_counter()
    m = R.fill([R.circle(320.0, 320.0, 300.3, 3000)], 640, 640)
    assert time.perf_counter() - t0 < 1.0
    assert abs(int(m.sum()) - np.pi * 300.3 ** 2) < 2000


# ---- the host label movement -----------------------------------------------------------------------------------------------------------
def _rect_row(cls, xc, yc, w, h):
    x1, y1, x2, y2 = xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2
    return [cls, x1, y1, x2, y1, x2, y2, x1, y2]


def _predicted(vertices, S, rect):
    """The pixel set of an axis-parallel rectangle given by its moved corners, by the rectangle property, inside `rect`."""
    q = R.quantise(vertices)
    (qx1, qy1), (qx2, qy2) = q.min(axis=0), q.max(axis=0)
    c = 16 * np.arange(S) + 8
    want = ((qy1 <= c) & (c < qy2))[:, None] & ((qx1 <= c) & (c < qx2))[None, :]
    keep = np.zeros((S, S), dtype=bool)
    keep[max(rect[1], 0):rect[3], max(rect[0], 0):rect[2]] = True
    return want & keep


def test_augment_polygons_moves_a_rectangle_like_the_box_rule():
    rng = np.random.default_rng(11)
    S, kept, dropped, seen = 64, 0, 0, set()
    for it in range(1600):
        W0, H0 = int(rng.integers(20, 200)), int(rng.integers(20, 200))
        g = P.sample_geometry([(H0, W0)], S, rng, scale=(0.5, 2.5), aspect=0.3, fliplr=0.5, flipud=0.5, transpose=0.5)[0]
        g[4] = it % 8                                                   # every orientation, evenly
        qw, qh = (g[1], g[0]) if g[4] & 4 else (g[0], g[1])
        g[2], g[3] = int(np.floor(rng.random() * (S - qw))), int(np.floor(rng.random() * (S - qh)))     # crops once q > S
        xc, yc, w, h = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.02, 0.6), rng.uniform(0.02, 0.6)
        rect = None if it % 3 else tuple(int(v) for v in (rng.integers(0, 32), rng.integers(0, 32), rng.integers(32, 65), rng.integers(32, 65)))
        box = P.augment_yolo_labels([[1, xc, yc, w, h]], W0, H0, g, S, clip_rect=rect)
        pol = P.augment_polygons([_rect_row(1, xc, yc, w, h)], W0, H0, g, S, clip_rect=rect)
        assert len(box) == len(pol), it
        dropped += not box
        if box:
            kept += 1
            seen.add((int(g[4]), rect is None, bool(qw > S or qh > S)))
            row6, v = pol[0]
            assert v.shape == (4, 2) and v.dtype == np.float64
            assert max(abs(a - b) for a, b in zip(box[0], row6)) <= 1e-9, it
            assert np.array_equal(R.fill([v], S, S, rect), _predicted(v, S, rect or (0, 0, S, S))), it
    assert kept > 300 and dropped > 100
    assert {o for o, _, _ in seen} == set(range(8)) and {(a, b) for _, a, b in seen} == {(True, True), (True, False), (False, True), (False, False)}


def test_augment_polygons_drop_rules():
    g = [64, 64, 0, 0, 0, 0, 0, 0]
    tri = [0, 0.1, 0.1, 0.5, 0.1, 0.3, 0.6]
    assert len(P.augment_polygons([tri], 64, 64, g, 64)) == 1
    assert P.augment_polygons([[0, 0.1, 0.1, 0.5, 0.5]], 64, 64, g, 64) == []                              # two points
    assert P.augment_polygons([[0, 0.1, 0.1, 0.3, 0.3, 0.5, 0.5]], 64, 64, g, 64) == []                     # no area
    assert P.augment_polygons([[0, 0.1, 0.1, 0.12, 0.1, 0.11, 0.6]], 64, 64, g, 64) == []                   # under min_px wide
    assert P.augment_polygons([tri], 64, 64, g, 64, clip_rect=(0, 0, 8, 8)) == []                           # mostly cut away
    bar = [[0, 0.0, 0.25, 1.0, 0.25, 1.0, 0.2578125, 0.0, 0.2578125]]                                    # 640 x 5 pixels: side ratio 128
    assert P.augment_polygons(bar, 640, 640, [640, 640, 0, 0, 0, 0, 0, 0], 640) == []
    assert len(P.augment_polygons(bar, 640, 640, [640, 640, 0, 0, 0, 0, 0, 0], 640, max_aspect=200.0)) == 1
    (row6, v), = P.augment_polygons([[2, -0.5, 0.25, 0.5, 0.25, 0.5, 0.75, -0.5, 0.75]], 64, 64, g, 64)    # clipped box, unclipped vertices
    assert row6 == [0.0, 2.0, 0.25, 0.5, 0.5, 0.5] and v[:, 0].min() == -32.0


def test_mosaic_polygons_per_tile():
    rng = np.random.default_rng(12)
    S, kept = 64, 0
    for it in range(200):
        sizes = [(int(rng.integers(20, 200)), int(rng.integers(20, 200))) for _ in range(4)]
        index, geom, centres = P.sample_mosaic(sizes, S, rng, prob=0.8, scale=(0.5, 1.5), fliplr=0.5, flipud=0.5, transpose=0.5)
        boxes = [[[float(t % 2), rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(0.1, 0.7), rng.uniform(0.1, 0.7)]
                  for _ in range(int(rng.integers(0, 3)))] for t in range(4)]
        polys = [[_rect_row(*b) for b in tile] for tile in boxes]
        tiles_sizes = [sizes[k] for k in index[0]]
        want = P.mosaic_yolo_labels(boxes, tiles_sizes, geom[0], centres[0], S)
        got = P.mosaic_polygons(polys, tiles_sizes, geom[0], centres[0], S)
        assert len(got) == len(want), it
        rects = P.tile_rects(centres[0], S)
        for w6, (row6, v, rect) in zip(want, got):
            kept += 1
            assert rect in rects and max(abs(a - b) for a, b in zip(w6, row6)) <= 1e-9, it
            m = R.fill([v], S, S, rect)
            assert np.array_equal(m, _predicted(v, S, rect)), it
            outside = np.ones((S, S), dtype=bool)
            outside[rect[1]:rect[3], rect[0]:rect[2]] = False
            assert not (m & outside).any()
    assert kept > 100


# ---- the C ABI, without a GPU ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


PTR = 4096   # a non-null, 8-byte aligned dummy: every check below returns before anything is dereferenced


def _args(**kw):
    a = L.FillPolygonsArgs()
    a.vertices = a.poly_offsets = a.plane_offsets = a.out = PTR
    a.n, a.n_polys, a.n_vertices, a.H, a.W, a.pitch = 1, 1, 3, 4, 70, 16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_fill_polygons_early_returns(lib):
    assert lib.mtbt_fill_polygons(None, None) == -1
    for bad in (dict(out=None), dict(vertices=None), dict(poly_offsets=None), dict(plane_offsets=None), dict(n=-1), dict(n_polys=-1),
                dict(n_vertices=-1), dict(H=0), dict(W=0), dict(H=65536, W=32768, pitch=4096), dict(pitch=8), dict(pitch=24), dict(W=64)):
        assert lib.mtbt_fill_polygons(C.byref(_args(**bad)), None) == -1, bad
    for bad in (dict(out=PTR + 4), dict(vertices=PTR + 2), dict(poly_offsets=PTR + 1), dict(plane_offsets=PTR + 3), dict(clip=PTR + 2),
                dict(area=PTR + 2), dict(box=PTR + 1)):
        assert lib.mtbt_fill_polygons(C.byref(_args(**bad)), None) == -2, bad
    assert lib.mtbt_fill_polygons(C.byref(_args(out=PTR + 4, H=0)), None) == -1          # invalid and misaligned: invalid
    # n == 0 launches nothing (a launch would fail without a device); NULL vertices are fine when there are none
    assert lib.mtbt_fill_polygons(C.byref(_args(n=0)), None) == 0
    assert lib.mtbt_fill_polygons(C.byref(_args(n=0, n_vertices=0, vertices=None, n_polys=0, clip=PTR, area=PTR, box=PTR)), None) == 0


def test_sizeof_query(lib):
    assert lib.mtbt_sizeof_fill_polygons_args(0) == C.sizeof(L.FillPolygonsArgs) == 80
    assert lib.mtbt_sizeof_fill_polygons_args(1) == -1 and lib.mtbt_sizeof_fill_polygons_args(-1) == -1
    assert lib.mtbt_abi_version() == 5


def test_ctypes_mirror_matches_the_header(tmp_path):
    fields = [f for f, _ in L.FillPolygonsArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){',
             'printf("sizeof %zu\\n", sizeof(mtbt_fill_polygons_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(mtbt_fill_polygons_args, {f}));' for f in fields]
    lines.append('return 0;}')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(L.FillPolygonsArgs)
    assert fields == ["vertices", "poly_offsets", "plane_offsets", "clip", "out", "area", "box", "n", "n_polys", "n_vertices", "H", "W", "pitch"]
    for f in fields:
        assert int(out[f]) == getattr(L.FillPolygonsArgs, f).offset, f


def test_fill_polygons_checks_its_arguments_before_the_device():
    from multitask_bonetumor_yolo_amd import postprocess as pp
    for bad in ([[0, 0], [1, np.nan], [2, 2]], [[0, 0], [1, np.inf], [2, 2]], [[0, 0], [40000.0, 1], [2, 2]]):
        with pytest.raises(ValueError, match="finite"):
            pp.fill_polygons([bad], 8, 8, device="cuda:0")
    with pytest.raises(ValueError):
        pp.fill_polygons([], 0, 8, device="cuda:0")
    with pytest.raises(ValueError, match="clip"):
        pp.fill_polygons([[]], 8, 8, clip=[[0, 0, 1, 1], [0, 0, 1, 1]], device="cuda:0")
    with pytest.raises(RuntimeError, match="no CPU path"):
        pp.fill_polygons([[]], 8, 8, device="cpu")
