"""CPU checks of the surface-distance metrics (metrics.SurfaceDistanceMetrics, csrc/surface_dist.hip): the numpy restatement
(tests/surface_reference.py) against scipy, the host finalisation (`metrics.surface_metrics`) on hand-made records and against the
restatement, the C-ABI struct against the header through gcc, the argument checks of the entry point (nothing is launched) and the
option checks of `ValidationStep(surface=...)`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import SurfaceDistanceMetrics, ValidationStep, surface_distances, surface_metrics   # exported
from multitask_bonetumor_yolo_amd.metrics import surface_tol2

import surface_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
PTR = 4096                                       # non-null, aligned dummy: every call below is refused before any launch


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def _random_pairs(n, seed=0):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        H, W = int(rng.integers(1, 40)), int(rng.integers(1, 140))
        yield R.blob(rng, H, W), R.blob(rng, H, W)


# ---- the restatement against scipy --------------------------------------------------------------------------------------------
def test_reference_edges_and_distances_equal_scipy():
    cross = ndimage.generate_binary_structure(2, 1)
    n_undefined = 0
    for a, b in _random_pairs(60):
        ea, eb = R.edge_set(a), R.edge_set(b)
        assert np.array_equal(ea, a ^ ndimage.binary_erosion(a, cross, border_value=0))
        assert np.array_equal(eb, b ^ ndimage.binary_erosion(b, cross, border_value=0))
        n_undefined += not (ea.any() and eb.any())
        edt = ndimage.distance_transform_edt(~eb)
        assert np.array_equal(R.directed_d2(ea, eb), np.rint(edt[ea] ** 2).astype(np.int64))
    assert n_undefined == 0                                  # the generator keeps at least one rectangle per plane


def test_reference_metrics_equal_medpy_formulas_with_scipy():
    cross = ndimage.generate_binary_structure(2, 1)
    for (a, b), spacing in zip(_random_pairs(40, seed=1), np.tile([1.0, 0.7], 20)):
        ea, eb = (m ^ ndimage.binary_erosion(m, cross, border_value=0) for m in (a, b))
        ab = ndimage.distance_transform_edt(~eb, sampling=spacing)[ea]       # MedPy's __surface_distances
        ba = ndimage.distance_transform_edt(~ea, sampling=spacing)[eb]
        for mode in ("pooled", "max"):
            got = R.metrics(a, b, spacing=spacing, tolerance=1.5, percentile_mode=mode)
            want95 = np.percentile(np.hstack((ab, ba)), 95) if mode == "pooled" else max(np.percentile(ab, 95), np.percentile(ba, 95))
            assert got["hd"] == pytest.approx(max(ab.max(), ba.max()), rel=1e-9, abs=1e-9)
            assert got["assd"] == pytest.approx(np.mean((ab.mean(), ba.mean())), rel=1e-9, abs=1e-9)
            assert got["hd95"] == pytest.approx(want95, rel=1e-9, abs=1e-9)
            within = (ab <= 1.5 + 1e-12).sum() + (ba <= 1.5 + 1e-12).sum()  # no d lies within 1e-12 of 1.5 at these spacings
            assert got["nsd"] == pytest.approx(within / (len(ab) + len(ba)), rel=1e-12)


def test_order_statistics_reproduce_numpy_percentile():
    rng = np.random.default_rng(2)
    for m in (1, 2, 3, 20, 21, 101, 1000):
        v = rng.integers(0, 50, size=m)
        d = np.sqrt(v.astype(np.float64))
        for q in (0.0, 0.5, 0.95, 1.0, 0.37):
            lo, hi = R.order_stats(v, q)
            pos = q * (m - 1)
            t = pos - np.floor(pos)
            assert np.sqrt(lo) + (np.sqrt(hi) - np.sqrt(lo)) * t == pytest.approx(np.percentile(d, 100 * q), rel=1e-9, abs=1e-9)


# ---- the host finalisation ------------------------------------------------------------------------------------------------------
def _host_records(pairs, quantile=0.95, tol2=4):
    rec = R.batch_records(pairs, (quantile,), tol2)
    rec.update(quantiles=(quantile,), tol2=tol2, shape=pairs[0][0].shape)
    return rec


@pytest.mark.parametrize("mode", ["pooled", "max"])
@pytest.mark.parametrize("undefined", ["skip", "diagonal"])
def test_finalisation_equals_the_restatement(mode, undefined):
    rng = np.random.default_rng(3)
    for H, W in ((1, 1), (7, 70), (33, 65)):
        cases, n_empty = R.plane_cases(rng, H, W)
        pairs = [(a, b) for _, a, b in cases]
        for spacing, tolerance in ((1.0, 2.0), (0.5, 1.2)):
            rec = _host_records(pairs, tol2=surface_tol2(tolerance, spacing))
            got = surface_metrics(rec, spacing=spacing, tolerance=tolerance, percentile_mode=mode, undefined=undefined)
            assert int((~got["defined"]).sum()) == n_empty
            for i, (a, b) in enumerate(pairs):
                want = R.metrics(a, b, spacing=spacing, tolerance=tolerance, percentile_mode=mode, undefined=undefined)
                assert bool(got["defined"][i]) == want["defined"]
                for k in ("hd", "hd95", "assd", "nsd"):
                    assert got[k][i] == pytest.approx(want[k], rel=1e-9, abs=1e-12, nan_ok=True), (cases[i][0], k)


def test_finalisation_on_hand_made_records():
    # pair 0: one edge pixel a side (m = 1 in each direction: lo = hi), 3-4-5 apart; pair 1: A empty; pair 2: both empty
    rec = {"n_edge": np.array([[1, 1], [0, 4], [0, 0]]), "max_d2": np.array([[25, 25], [0, 0], [0, 0]]),
           "n_within": np.array([[0, 0], [0, 0], [0, 0]]), "sum_d": np.array([[5.0, 5.0], [0.0, 0.0], [0.0, 0.0]]),
           "rank_d2": np.array([[[[25, 25], [25, 25], [25, 25]]], np.zeros((1, 3, 2)), np.zeros((1, 3, 2))]),
           "quantiles": (0.95,), "tol2": 4, "shape": (30, 40)}
    got = surface_metrics(rec, spacing=1.0, tolerance=2.0)
    assert got["defined"].tolist() == [True, False, False]
    assert (got["hd"][0], got["hd95"][0], got["assd"][0], got["nsd"][0]) == (5.0, 5.0, 5.0, 0.0)
    assert all(np.isnan(got[k][1:]).all() for k in ("hd", "hd95", "assd", "nsd"))
    got = surface_metrics(rec, spacing=1.0, tolerance=2.0, undefined="diagonal")
    assert (got["hd"][1], got["hd95"][1], got["assd"][1], got["nsd"][1]) == (50.0, 50.0, 50.0, 0.0)
    assert not got["defined"][1] and np.isnan(got["hd"][2]) and np.isnan(got["nsd"][2])       # both empty: always skipped
    # spacing: distances scale, and the tolerance is compared in pixels
    rec["tol2"] = surface_tol2(2.0, 0.25)
    assert rec["tol2"] == 64
    got = surface_metrics(rec, spacing=0.25, tolerance=2.0, undefined="diagonal")
    assert (got["hd"][0], got["assd"][0], got["hd"][1]) == (1.25, 1.25, 12.5)
    with pytest.raises(ValueError, match="tol2"):
        surface_metrics(rec, spacing=1.0, tolerance=2.0)
    with pytest.raises(ValueError):
        surface_metrics(rec, spacing=0.25, tolerance=2.0, percentile_mode="median")
    with pytest.raises(ValueError):
        surface_metrics(rec, spacing=0.25, tolerance=2.0, undefined="zero")


def test_tolerance_between_two_square_roots():
    assert [surface_tol2(t) for t in (0.0, 0.99, 1.0, 1.5, 2.0, 2.23, 2.24)] == [0, 0, 1, 2, 4, 4, 5]   # sqrt(5) = 2.236...
    assert surface_tol2(1.0, 0.5) == 4 and surface_tol2(3.0, 2.0) == 2
    a = np.zeros((9, 9), bool)
    b = a.copy()
    a[4, 4] = True
    b[4, 5], b[5, 6], b[6, 6] = True, True, True          # from b to a: d2 = 1, 5, 8; from a to b: 1
    for tol, want in ((0.5, 0.0), (1.0, 0.5), (2.23, 0.5), (2.24, 0.75), (2.9, 1.0)):
        rec = _host_records([(a, b)], tol2=surface_tol2(tol))
        assert surface_metrics(rec, tolerance=tol)["nsd"][0] == want
        assert R.metrics(a, b, tolerance=tol)["nsd"] == want


def test_metric_object_without_updates_and_its_refusals():
    m = SurfaceDistanceMetrics()
    assert m.compute() == {"hd": -1.0, "hd95": -1.0, "assd": -1.0, "nsd": -1.0, "n_pairs": 0, "n_undefined": 0}
    assert m.tol2 == 4 and SurfaceDistanceMetrics(tolerance=3.0, spacing=2.0).tol2 == 2
    for kw in (dict(quantile=1.5), dict(percentile_mode="both"), dict(undefined="nan"), dict(spacing=0.0), dict(tolerance=-1.0)):
        with pytest.raises(ValueError):
            SurfaceDistanceMetrics(**kw)
    import torch
    with pytest.raises(RuntimeError):
        m.update(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(RuntimeError):
        surface_distances(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8), 8)


def test_validation_step_surface_options():
    for bad in ("yes", 3, dict(tolerence=2.0), dict(percentile_mode="both"), dict(quantile=2.0), dict(dist_sync=False)):
        with pytest.raises(ValueError):
            ValidationStep(None, surface=bad)
    assert ValidationStep._surface_options(None) is None and ValidationStep._surface_options(True) == {}
    assert ValidationStep._surface_options(dict(tolerance=1.0, undefined="diagonal")) == dict(tolerance=1.0, undefined="diagonal")
    with pytest.raises(NotImplementedError):                 # valid options: the constructor gets as far as the model
        ValidationStep(None, surface=dict(quantile=0.9))


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_header(tmp_path, lib):
    name, st = "mtbt_surface_args", L.SurfaceArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){',
             f'printf("{name} %zu\\n", sizeof({name}));']
    lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in st._fields_]
    lines.append('return 0;}')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out[name]) == C.sizeof(st) == lib.mtbt_sizeof_surface_args(0)
    for f, _ in st._fields_:
        assert int(out[f"{name}.{f}"]) == getattr(st, f).offset, f
    assert L.SURFACE_STRUCTS == (st,)


def test_symbols_and_additive_abi(lib):
    assert lib.mtbt_sizeof_surface_args(-1) == -1 and lib.mtbt_sizeof_surface_args(1) == -1
    assert lib.mtbt_abi_version() == 5 == L.ABI_VERSION
    for name in ("mtbt_surface_distances", "mtbt_surface_distances_workspace_bytes", "mtbt_sizeof_surface_args"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert len(L.MASK_EVAL_STRUCTS) == 4 and lib.mtbt_sizeof_mask_eval_args(4) == -1        # the earlier tables did not move


def _args(lib, n=3, H=37, W=70, Q=2):
    a = L.SurfaceArgs()
    for f in ("a", "b", "workspace", "n_edge", "max_d2", "n_within", "sum_d", "rank_d2"):
        setattr(a, f, PTR)
    a.n, a.H, a.W, a.pitch, a.tol2, a.Q = n, H, W, 8 * ((W + 63) // 64), 4, Q
    a.q[0], a.q[1] = 0.5, 0.95
    a.workspace_bytes = lib.mtbt_surface_distances_workspace_bytes(n, H, W)
    return a


@pytest.mark.parametrize("field,value", [("a", None), ("b", None), ("workspace", None), ("n_edge", None), ("max_d2", None), ("n_within", None),
                                         ("sum_d", None), ("rank_d2", None), ("n", -1), ("H", 0), ("H", 16385), ("W", 0), ("W", 16385),
                                         ("pitch", 8), ("pitch", 24), ("Q", -1), ("Q", 5), ("workspace_bytes", 16)])
def test_rejects_bad_arguments_without_launching(lib, field, value):
    assert lib.mtbt_surface_distances(None, None) == EINVAL
    a = _args(lib)
    setattr(a, field, value)
    assert lib.mtbt_surface_distances(C.byref(a), None) == EINVAL


def test_quantile_range_workspace_query_and_alignment(lib):
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        a = _args(lib)
        a.q[1] = bad
        assert lib.mtbt_surface_distances(C.byref(a), None) == EINVAL
    a = _args(lib)
    a.q[3] = float("nan")                                    # beyond Q: not read
    a.workspace_bytes -= 1
    assert lib.mtbt_surface_distances(C.byref(a), None) == EINVAL
    ws = lib.mtbt_surface_distances_workspace_bytes
    assert ws(-1, 8, 8) == EINVAL and ws(1, 0, 8) == EINVAL and ws(1, 8, 16385) == EINVAL and ws(0, 8, 8) == 0
    assert 0 < ws(1, 37, 70) < ws(2, 37, 70) and ws(64, 37, 70) == ws(1000, 37, 70)          # the pairs go in groups of at most 64
    assert ws(100, 16384, 16384) == ws(1, 16384, 16384) > 2 ** 31                            # ... and of at least one
    for f, off in (("a", 4), ("b", 4), ("workspace", 8), ("n_edge", 2), ("max_d2", 2), ("n_within", 2), ("sum_d", 4), ("rank_d2", 2)):
        a = _args(lib)
        setattr(a, f, PTR + off)
        assert lib.mtbt_surface_distances(C.byref(a), None) == EALIGN, f
    a = _args(lib, n=0)                                      # nothing to do is not an error, and launches nothing
    a.workspace, a.workspace_bytes = None, 0
    assert lib.mtbt_surface_distances(C.byref(a), None) == 0
    a = _args(lib, Q=0)
    a.rank_d2 = None
    a.n = 0
    assert lib.mtbt_surface_distances(C.byref(a), None) == 0
