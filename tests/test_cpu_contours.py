"""CPU checks of contour tracing and COCO run lengths (postprocess.trace_contours / rle_encode, csrc/contours.hip): the numpy restatement
(tests/contour_reference.py) against independent code -- the project's fill rule, the component labelling and scipy.ndimage -- on every
plane the GPU tests use; the run-length rule and its string form; the host helpers on reference results; the C-ABI structs against the
header through gcc and the argument checks of the entry points (nothing is launched)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import (coco_segm_results, contour_polygons, count_contour_vertices, labelme_shapes, rle_encode,   # exported
                                          rle_from_string, rle_to_string, trace_contours, yolo_seg_polygons, yolo_seg_rows)

import components_reference as CR
import contour_reference as R
import polygon_reference as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
PTR = 4096                                       # non-null, aligned dummy: every call below is refused before any launch
SHAPES = [(1, 1), (1, 70), (37, 64), (33, 65), (40, 130), (96, 200)]
STRUCTURE = {4: ndimage.generate_binary_structure(2, 1), 8: np.ones((3, 3), bool)}


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


# ---- the restatement against independent code: the consequences A to D of the rule ----------------------------------------------------
def _consequences(m, conn):
    H, W = m.shape
    cs = R.trace(m, conn)
    back = np.zeros((H, W), bool)
    for c in cs:
        assert len(c["vertices"]) >= 4 and len(c["vertices"]) % 2 == 0
        d = np.roll(c["vertices"], -1, axis=0) - c["vertices"]
        assert ((d != 0).sum(axis=1) == 1).all() and ((d[:, 0] != 0) != (np.roll(d, -1, axis=0)[:, 0] != 0)).all()   # axis-parallel, alternating
        back ^= PR.fill([c["vertices"].astype(np.float64)], H, W)
    assert np.array_equal(back, m)                                                          # A
    assert sum(c["area2"] for c in cs) == 2 * int(m.sum())                                  # B
    assert [c["start"] for c in cs] == sorted(c["start"] for c in cs) and all(c["area2"] != 0 for c in cs)
    comp = CR.records(m, conn, max_components=max(1, m.size))
    outer = [c for c in cs if c["area2"] > 0]
    assert len(outer) == comp["n_components"]                                               # C
    for k, c in enumerate(outer):
        first = int(comp["first"][k])
        assert c["start"] == (first // W) * (W + 1) + first % W and tuple(c["box"]) == tuple(comp["box"][k])
    _, n_bg = ndimage.label(np.pad(~m, 1, constant_values=True), structure=STRUCTURE[12 - conn])
    assert len(cs) - len(outer) == n_bg - 1                                                 # D
    assert sum(len(c["vertices"]) for c in cs) == R.count_vertices(m)
    return cs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_satisfies_the_consequences_on_every_case(shape):
    H, W = shape
    for name, m in CR.plane_cases(np.random.default_rng(20 + SHAPES.index(shape)), H, W):
        for conn in (4, 8):
            cs = _consequences(m, conn)
            if name == "empty":
                assert cs == []
            if name == "full":
                assert len(cs) == 1 and cs[0]["vertices"].tolist() == [[0, 0], [W, 0], [W, H], [0, H]] and cs[0]["area2"] == 2 * H * W


def test_reference_on_hand_written_planes():
    planes = dict(R.hand_planes())
    got = {(name, conn): _consequences(m, conn) for name, m in planes.items() for conn in (4, 8)}
    lens = lambda k: [len(c["vertices"]) for c in got[k]]
    holes = lambda k: [c["area2"] < 0 for c in got[k]]
    for conn in (4, 8):
        assert got[("single", conn)][0]["vertices"].tolist() == [[1, 1], [2, 1], [2, 2], [1, 2]] and got[("single", conn)][0]["start"] == 1 * 4 + 1
        assert lens(("ring", conn)) == [4, 4] and holes(("ring", conn)) == [False, True]
        assert got[("ring", conn)][1]["vertices"].tolist() == [[2, 3], [3, 3], [3, 2], [2, 2]]      # a hole starts on its BOTTOM side and runs the other way
        assert lens(("ring_island", conn)) == [4, 4, 4] and holes(("ring_island", conn)) == [False, False, True]   # the island starts above the hole's bottom
        assert lens(("border", conn)) == [4, 4] and holes(("border", conn)) == [False, True]
    assert lens(("saddle", 4)) == [4, 4] and lens(("saddle", 8)) == [8]
    assert got[("saddle", 8)][0]["vertices"].tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]   # (1, 1) twice
    assert lens(("hole_touches_outer", 4)) == [10] and holes(("hole_touches_outer", 4)) == [False]   # 4: the hole opens to the outside
    assert lens(("hole_touches_outer", 8)) == [6, 4] and holes(("hole_touches_outer", 8)) == [False, True]


def test_records_tables_and_capacities():
    m = dict(CR.plane_cases(np.random.default_rng(2), 37, 64))["noise_500"]
    full = R.records(m, 4, max_contours=4096)
    n, nv = full["n_contours"], full["n_vertices"]
    assert 5 < n < 4096 and np.array_equal(np.cumsum(full["count"][:n]) - full["count"][:n], full["offset"][:n]) and full["count"][:n].sum() == nv
    assert not full["count"][n:].any() and not full["box"][n:].any() and not full["start"][n:].any()
    cut = R.records(m, 4, max_contours=5)
    assert cut["n_contours"] == n and np.array_equal(cut["count"], full["count"][:5]) and np.array_equal(cut["vertices"], full["vertices"])
    over = R.records(m, 4, max_contours=5, max_vertices=nv - 1)
    assert over["n_contours"] == -1 and over["n_vertices"] == nv and not over["count"].any() and len(over["vertices"]) == 0
    assert R.records(m, 4, max_contours=5, max_vertices=nv)["n_contours"] == n


# ---- run lengths ----------------------------------------------------------------------------------------------------------------------
def test_rle_rule_and_round_trip():
    m = np.zeros((3, 4), bool)
    m[0, 0] = True
    assert R.rle_counts(m) == [0, 1, 11]
    for shape in SHAPES:
        for name, p in CR.plane_cases(np.random.default_rng(5), *shape):
            c = R.rle_counts(p)
            assert sum(c) == p.size and (c[0] == 0) == bool(p[0, 0]) and all(v > 0 for v in c[1:])
            assert np.array_equal(R.rle_decode(c, *shape), p)
            s = rle_to_string(c)
            assert s == R.rle_to_string(c) and rle_from_string(s) == c == R.rle_from_string(s)
            assert all(48 <= ord(ch) < 48 + 64 for ch in s)
    assert R.rle_counts(np.zeros((5, 7), bool)) == [35] and R.rle_counts(np.ones((5, 7), bool)) == [0, 35]


def test_rle_string_handles_large_counts_and_negative_deltas():
    for c in ([0, 1, 11], [5, 40000, 3, 2, 70000, 1], [2 ** 15, 2 ** 15 - 1, 2 ** 15 + 1, 1, 1, 2 ** 28], [100000, 1, 1, 100000, 7, 3, 5],
              [16, 15, 17, 31, 32, 33, 1, 1024, 2, 1023]):
        s = rle_to_string(c)
        assert rle_from_string(s) == c and R.rle_from_string(s) == c and s == R.rle_to_string(c)
    assert rle_to_string([0, 1, 11]) == "01;"                    # 0 -> '0', 1 -> '1', 11 -> chr(48 + 11)
    assert rle_to_string([3, 1, 2, 1]) == "3120"                 # from the 4th value on the difference to two back: 1 - 1 = 0
    assert rle_to_string([3, 5, 2, 1]) == "352L"                 # 1 - 5 = -4: one group 0b11100 = 28, its bit 0x10 the sign, chr(48 + 28)
    assert rle_to_string([0, 32]) == "0P1"                       # 32: group 0 with the continuation bit (chr(48 + 32)), then group 1


# ---- host helpers over a result --------------------------------------------------------------------------------------------------------
def _as_result(planes, conn, **kw):
    r = R.stack_records(planes, conn, **kw)
    out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in r.items()}
    out["shape"] = planes[0].shape
    return out


def test_helpers_on_reference_results():
    named = dict(R.hand_planes())
    island = named["ring_island"]
    H, W = island.shape
    planes = [island, np.zeros_like(island), ~np.zeros_like(island)]
    res = _as_result(planes, 4, max_contours=8)
    polys = contour_polygons(res, 0)
    assert [p.tolist() for p in polys] == [c["vertices"].tolist() for c in R.trace(island, 4) if c["area2"] > 0] and len(polys) == 2
    assert polys[0].dtype == np.int32 and len(contour_polygons(res, 0, holes=True)) == 3 and contour_polygons(res, 1) == []
    rows = yolo_seg_rows(res, [3, 4, 5], W, H)
    assert [r[0] for r in rows] == [3, 3, 5] and all(0.0 <= v <= 1.0 for r in rows for v in r[1:])
    back, classes = yolo_seg_polygons(rows, H, W)               # the parser behind yolo_seg_planes
    assert classes == [3, 3, 5]
    want = polys + contour_polygons(res, 2)
    for b, w in zip(back, want):
        assert np.array_equal(PR.quantise(b), 16 * w)            # exactly the lattice points, in the fill's fixed point
    filled = PR.fill(back[:2], H, W)                             # the formats cannot carry the hole: the ring comes back filled, the island in it
    assert np.array_equal(filled, ndimage.binary_fill_holes(island))
    shapes = labelme_shapes(res, 0, "tumor")
    assert [s["points"] for s in shapes] == [p.tolist() for p in polys]
    assert all(s["label"] == "tumor" and s["shape_type"] == "polygon" for s in shapes)
    with pytest.raises(ValueError):
        contour_polygons(_as_result(planes, 4, max_contours=1), 0)            # three contours, a table of one
    nv = int(res["n_vertices"][0])
    with pytest.raises(ValueError):
        contour_polygons(_as_result(planes, 4, max_contours=8, max_vertices=nv - 1), 0)
    with pytest.raises(ValueError):
        yolo_seg_rows(res, [1], W, H)


def test_yolo_rows_round_trip_at_awkward_sizes():
    rng = np.random.default_rng(9)
    for H, W in ((37, 70), (96, 200), (3000, 2999)):
        m = np.zeros((min(H, 40), min(W, 40)), bool)
        m[:] = rng.uniform(size=m.shape) < 0.5
        big = np.zeros((H, W), bool)
        big[H - m.shape[0]:, W - m.shape[1]:] = m                 # against the far corner: the largest coordinates
        cs = [c for c in R.trace(big, 8) if c["area2"] > 0]
        rows = [[0] + (c["vertices"].astype(np.float64) / np.asarray([float(W), float(H)])).reshape(-1).tolist() for c in cs]
        back, _ = yolo_seg_polygons(rows, H, W)
        assert len(back) == len(cs) and all(np.array_equal(PR.quantise(b), 16 * c["vertices"]) for b, c in zip(back, cs))


def test_refusals_without_a_device():
    p = torch.zeros(1, 8, 8, dtype=torch.uint8)
    for call in (lambda: trace_contours(p, 8), lambda: count_contour_vertices(p, 8), lambda: rle_encode(p, 8)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        coco_segm_results({"masks_frame": [p], "counts": torch.zeros(1), "scores": torch.zeros(1, 1), "labels": torch.zeros(1, 1),
                           "boxes_frame": torch.zeros(1, 1, 4)}, [7])           # the frames are missing


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(tmp_path, lib):
    structs = {"mtbt_contours_args": L.ContoursArgs, "mtbt_rle_args": L.RleArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){']
    for name, st in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in st._fields_]
    lines.append('return 0;}')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for which, (name, st) in enumerate(structs.items()):
        assert int(out[name]) == C.sizeof(st) == lib.mtbt_sizeof_contours_args(which)
        for f, _ in st._fields_:
            assert int(out[f"{name}.{f}"]) == getattr(st, f).offset, f
    assert L.CONTOURS_STRUCTS == tuple(structs.values())


def test_symbols_and_additive_abi(lib):
    assert lib.mtbt_sizeof_contours_args(-1) == -1 and lib.mtbt_sizeof_contours_args(2) == -1
    assert lib.mtbt_abi_version() == 5 == L.ABI_VERSION
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("mtbt_trace_contours", "mtbt_contours_workspace_bytes", "mtbt_rle_encode", "mtbt_rle_workspace_bytes", "mtbt_sizeof_contours_args"):
        assert name in L.SYMBOLS and hasattr(lib, name) and name in text
    assert L.DISTANCE_STRUCTS == (L.DistanceTransformArgs, L.SegRegionArgs) and lib.mtbt_sizeof_distance_args(2) == -1   # the earlier tables did not move
    assert "contours.hip" in B.SOURCES and "contours.hip" not in B.EXTRA_FLAGS


TABLES = ("n_contours", "vertices", "offset", "count", "area2", "box", "start")


def _trace_args(lib, n=3, H=37, W=70, V=500, full=True):
    a = L.ContoursArgs()
    for f in ("packed", "n_vertices") + (("workspace",) + TABLES if full else ()):
        setattr(a, f, PTR)
    a.n, a.H, a.W, a.pitch, a.connectivity, a.max_contours, a.max_vertices = n, H, W, 8 * ((W + 63) // 64), 4, 16, V
    a.workspace_bytes = lib.mtbt_contours_workspace_bytes(n, H, W, V) if full else 0
    return a


@pytest.mark.parametrize("field,value", [("packed", None), ("n_vertices", None), ("workspace", None), ("n_contours", None), ("vertices", None),
                                         ("offset", None), ("count", None), ("area2", None), ("box", None), ("start", None), ("n", -1),
                                         ("H", 0), ("H", 16385), ("W", 0), ("W", 16385), ("pitch", 8), ("pitch", 24), ("connectivity", 0),
                                         ("connectivity", 6), ("max_contours", 0), ("max_contours", 65537), ("max_vertices", -1),
                                         ("workspace_bytes", 16)])
def test_trace_rejects_bad_arguments_without_launching(lib, field, value):
    assert lib.mtbt_trace_contours(None, None) == EINVAL
    a = _trace_args(lib)
    setattr(a, field, value)
    assert lib.mtbt_trace_contours(C.byref(a), None) == EINVAL


def test_trace_count_only_argument_checks(lib):
    for field, value in (("packed", None), ("n_vertices", None), ("n", -1), ("H", 0), ("W", 16385), ("pitch", 8), ("connectivity", 5)):
        a = _trace_args(lib, full=False)
        setattr(a, field, value)
        assert lib.mtbt_trace_contours(C.byref(a), None) == EINVAL, field
    for table in TABLES[2:]:                                                   # a table without vertices is not a count-only call
        a = _trace_args(lib, full=False)
        setattr(a, table, PTR)
        assert lib.mtbt_trace_contours(C.byref(a), None) == EINVAL, table
    for f, off in (("packed", 4), ("n_vertices", 2)):
        a = _trace_args(lib, full=False)
        setattr(a, f, PTR + off)
        assert lib.mtbt_trace_contours(C.byref(a), None) == EALIGN, f
    a = _trace_args(lib, n=0, full=False)
    assert lib.mtbt_trace_contours(C.byref(a), None) == 0


def test_trace_workspace_query_alignment_and_empty_calls(lib):
    ws = lib.mtbt_contours_workspace_bytes
    assert ws(-1, 8, 8, 10) == EINVAL and ws(1, 0, 8, 10) == EINVAL and ws(1, 8, 16385, 10) == EINVAL and ws(1, 8, 8, -1) == EINVAL
    assert ws(0, 8, 8, 10) == 0 and 0 < ws(1, 37, 70, 0) < ws(1, 37, 70, 100) < ws(1, 37, 70, 1000) < ws(2, 37, 70, 1000)
    assert ws(1, 37, 70, 2 * 37 * 70 + 2) == ws(1, 37, 70, 2 ** 31 - 1)          # no plane has more vertices than 2 H W + 2
    assert ws(1, 37, 70, 1000) >= 32 * 1000 and ws(1, 16384, 16384, 2 ** 31 - 1) > 2 ** 34
    a = _trace_args(lib)
    a.workspace_bytes -= 1
    assert lib.mtbt_trace_contours(C.byref(a), None) == EINVAL
    for f, off in (("packed", 4), ("workspace", 8), ("n_vertices", 2), ("n_contours", 2), ("vertices", 2), ("offset", 2), ("count", 2),
                   ("area2", 4), ("box", 2), ("start", 2)):
        a = _trace_args(lib)
        setattr(a, f, PTR + off)
        assert lib.mtbt_trace_contours(C.byref(a), None) == EALIGN, f
    a = _trace_args(lib, n=0)                                   # nothing to do is not an error, and launches nothing
    a.workspace, a.workspace_bytes = None, 0
    assert lib.mtbt_trace_contours(C.byref(a), None) == 0


def _rle_args(lib, n=3, H=37, W=70, R=64):
    a = L.RleArgs()
    for f in ("packed", "workspace", "counts", "n_runs"):
        setattr(a, f, PTR)
    a.n, a.H, a.W, a.pitch, a.max_runs = n, H, W, 8 * ((W + 63) // 64), R
    a.workspace_bytes = lib.mtbt_rle_workspace_bytes(n, H, W)
    return a


@pytest.mark.parametrize("field,value", [("packed", None), ("workspace", None), ("n_runs", None), ("n", -1), ("H", 0), ("H", 16385), ("W", 0),
                                         ("W", 16385), ("pitch", 8), ("pitch", 24), ("max_runs", -1), ("workspace_bytes", 16)])
def test_rle_rejects_bad_arguments_without_launching(lib, field, value):
    assert lib.mtbt_rle_encode(None, None) == EINVAL
    a = _rle_args(lib)
    setattr(a, field, value)
    assert lib.mtbt_rle_encode(C.byref(a), None) == EINVAL


def test_rle_workspace_query_alignment_and_empty_calls(lib):
    ws = lib.mtbt_rle_workspace_bytes
    assert ws(-1, 8, 8) == EINVAL and ws(1, 0, 8) == EINVAL and ws(1, 8, 16385) == EINVAL and ws(0, 8, 8) == 0
    assert 8 * 70 <= ws(1, 37, 70) < ws(1, 129, 70) < ws(2, 129, 70) and ws(1, 128, 70) == ws(1, 37, 70)
    a = _rle_args(lib)
    a.workspace_bytes -= 1
    assert lib.mtbt_rle_encode(C.byref(a), None) == EINVAL
    for f, off in (("packed", 4), ("workspace", 8), ("counts", 2), ("n_runs", 2)):
        a = _rle_args(lib)
        setattr(a, f, PTR + off)
        assert lib.mtbt_rle_encode(C.byref(a), None) == EALIGN, f
    a = _rle_args(lib, n=0)
    a.workspace, a.workspace_bytes = None, 0
    assert lib.mtbt_rle_encode(C.byref(a), None) == 0            # nothing to do is not an error, and launches nothing
