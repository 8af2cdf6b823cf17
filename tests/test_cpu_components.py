"""CPU checks of connected-component labelling (postprocess.label_components / filter_components, metrics.LesionMetrics,
csrc/components.hip): the numpy restatement (tests/components_reference.py) against scipy.ndimage on every plane the GPU tests use, the
select rule against a sort, the host arithmetic of `LesionMetrics` on hand-made record tables, the C-ABI structs against the header
through gcc, the argument checks of the entry points (nothing is launched) and the option checks of `ValidationStep(lesions=...)`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import (LesionMetrics, ValidationStep, components_to_instances, filter_components, label_components,   # exported
                                          lesion_hits)

import components_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
PTR = 4096                                       # non-null, aligned dummy: every call below is refused before any launch
SHAPES = [(1, 1), (1, 70), (37, 64), (33, 65), (40, 130), (96, 200)]
STRUCTURE = {4: ndimage.generate_binary_structure(2, 1), 8: np.ones((3, 3), bool)}


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


# ---- the restatement against scipy --------------------------------------------------------------------------------------------
def _against_scipy(m, conn, other):
    r = R.records(m, conn, max_components=m.size, other=other)
    lab, n = ndimage.label(m, structure=STRUCTURE[conn])
    assert r["n_components"] == n and np.array_equal(r["labels"], lab)
    assert np.array_equal(r["areas"], np.bincount(lab.ravel(), minlength=n + 1)[1:]) and np.array_equal(r["area"][:n], r["areas"])
    for i, sl in enumerate(ndimage.find_objects(lab)):
        assert tuple(r["box"][i]) == (sl[1].start, sl[0].start, sl[1].stop, sl[0].stop)
        assert lab.ravel()[r["first"][i]] == i + 1 and not (lab.ravel()[:r["first"][i]] == i + 1).any()
    assert np.array_equal(r["inter"][:n], np.bincount(lab[other], minlength=n + 1)[1:])
    assert not r["area"][n:].any() and not r["box"][n:].any() and not r["first"][n:].any() and not r["inter"][n:].any()
    return n


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_equals_scipy_on_every_case(shape):
    H, W = shape
    rng = np.random.default_rng(3)
    counts = {}
    for name, m in R.plane_cases(np.random.default_rng(20 + SHAPES.index(shape)), H, W):
        other = rng.uniform(size=(H, W)) < 0.3
        for conn in (4, 8):
            counts[(name, conn)] = _against_scipy(m, conn, other)
    assert counts[("empty", 4)] == 0 and counts[("full", 8)] == 1 and counts[("serpentine", 4)] == 1 and counts[("u", 4)] == 1
    assert counts[("checker", 4)] == (H * W + 1) // 2 and counts[("checker", 8)] == (1 if H > 1 else (W + 1) // 2)   # one row has no diagonals
    assert counts[("diagonal", 4)] == min(H, W) and counts[("diagonal", 8)] == 1
    if H >= 3:
        assert counts[("comb", 4)] == counts[("comb", 8)] == 1 + len(range(2, W, 8))      # the comb and its detached single pixels


def test_reference_equals_scipy_on_the_large_plane_and_truncates_its_tables():
    m = R.big_plane(np.random.default_rng(6))
    for conn in (4, 8):
        lab, n = ndimage.label(m, structure=STRUCTURE[conn])
        got, n_got = R.label(m, conn)
        assert n_got == n > 1024 and np.array_equal(got, lab)
    r = R.records(m[:64, :64], 4, max_components=5)
    lab, n = ndimage.label(m[:64, :64])
    assert r["n_components"] == n > 5 and len(r["area"]) == 5 and np.array_equal(r["area"], np.bincount(lab.ravel())[1:6])


# ---- the select rule -------------------------------------------------------------------------------------------------------------
def test_select_rule_equals_a_sort():
    rng = np.random.default_rng(4)
    for _ in range(200):
        a = rng.integers(1, 6, size=int(rng.integers(0, 30)))            # few values: many ties
        for k in (None, 0, 1, 3, 7, 100):
            for min_area in (0, 2, 6):
                got = R.keep_rule(a, min_area, k)
                order = sorted(range(len(a)), key=lambda i: (-a[i], i))   # larger first, lower id first among equals
                want = np.zeros(len(a), bool)
                want[order[:k] if k else order] = True
                want &= a >= min_area
                assert np.array_equal(got, want), (a, k, min_area)


def test_select_on_a_plane_with_ties():
    names, planes = zip(*R.plane_cases(np.random.default_rng(0), 37, 64))
    comb = planes[names.index("comb")]
    lab, n = ndimage.label(comb)
    assert n == 9 and (np.bincount(lab.ravel())[2:] == 1).all()            # the comb, then eight single pixels
    kept, k = R.select(comb, 4, keep_largest=3)
    assert k == 3 and np.array_equal(kept, np.isin(lab, (1, 2, 3)))         # ties go to the lower ids
    kept, k = R.select(comb, 4, min_area=2)
    assert k == 1 and np.array_equal(kept, lab == 1)
    kept, k = R.select(comb, 4, min_area=2, keep_largest=3)
    assert k == 1 and np.array_equal(kept, lab == 1)


# ---- LesionMetrics: host arithmetic ------------------------------------------------------------------------------------------------
def test_lesion_hits_on_hand_made_tables():
    n_comp = np.array([3, 0, 6, 1])                                          # plane 2 has more components than the table holds
    area = np.array([[10, 4, 3, 0], [0, 0, 0, 0], [5, 5, 5, 5], [7, 0, 0, 0]])
    inter = np.array([[5, 0, 1, 9], [0, 0, 0, 0], [1, 2, 3, 5], [0, 0, 0, 0]])  # [0, 3] lies beyond n_components: never read
    hits, cut = lesion_hits(n_comp, area, inter, 0.0)
    assert hits.tolist() == [2, 0, 4, 0] and cut.tolist() == [False, False, True, False]
    hits, _ = lesion_hits(n_comp, area, inter, 0.5)                          # 5 >= 5.0, 1 < 1.5; 1 < 2.5, 2 < 2.5, 3 >= 2.5, 5 >= 2.5
    assert hits.tolist() == [1, 0, 2, 0]
    hits, _ = lesion_hits(n_comp, area, inter, 1.0)
    assert hits.tolist() == [0, 0, 1, 0]
    hits, cut = lesion_hits(np.zeros(0), np.zeros((0, 4)), np.zeros((0, 4)), 0.0)
    assert hits.shape == (0,) and cut.shape == (0,)


def test_lesion_metrics_compute_from_records():
    m = LesionMetrics(overlap=0.5, max_components=4)
    assert m.compute() == {"lesion_recall": 0.0, "lesion_precision": 0.0, "lesion_f1": 0.0, "fp_per_image": 0.0, "n_gt": 0, "n_pred": 0,
                           "n_images": 0, "n_truncated": 0}
    t = lambda v: torch.tensor(v, dtype=torch.int32)
    m._records.append({"gt_n_components": t([3, 0, 6, 1]), "gt_area": t([[10, 4, 3, 0], [0, 0, 0, 0], [5, 5, 5, 5], [7, 0, 0, 0]]),
                       "gt_inter": t([[5, 0, 1, 9], [0, 0, 0, 0], [1, 2, 3, 5], [0, 0, 0, 0]]),
                       "pred_n_components": t([2, 1, 1, 0]), "pred_area": t([[6, 2, 0, 0], [3, 0, 0, 0], [20, 0, 0, 0], [0, 0, 0, 0]]),
                       "pred_inter": t([[5, 1, 0, 0], [0, 0, 0, 0], [11, 0, 0, 0], [0, 0, 0, 0]])})
    got = m.compute()                                                        # found 1 + 0 + 2 + 0 of 10; true 2 + 0 + 1 + 0 of 4
    assert got["n_gt"] == 10 and got["n_pred"] == 4 and got["n_images"] == 4 and got["n_truncated"] == 1
    assert got["lesion_recall"] == 3 / 10 and got["lesion_precision"] == 3 / 4 and got["fp_per_image"] == 1 / 4
    assert got["lesion_f1"] == 2 * 0.75 * 0.3 / (0.75 + 0.3)
    m.reset()
    assert m.compute()["n_images"] == 0


def test_reference_lesion_counts_by_hand():
    pred, gt = np.zeros((12, 20), bool), np.zeros((12, 20), bool)
    gt[1:5, 1:5], gt[8:10, 8:10], gt[0, 19] = True, True, True                # 16 pixels, 4 pixels, 1 pixel
    pred[2:5, 2:9], pred[9, 9], pred[11, 0], pred[6, 15:17] = True, True, True, True   # covers 9 of 16, 1 of 4; a speck and a pair are false
    c = R.lesion_counts(pred, gt, overlap=0.0)
    assert c == {"n_gt": 3, "n_found": 2, "n_pred": 4, "n_true": 2, "truncated": False}
    assert R.lesion_counts(pred, gt, overlap=0.5)["n_found"] == 1 and R.lesion_counts(pred, gt, overlap=0.5)["n_true"] == 1
    c = R.lesion_counts(pred, gt, min_area=2)                                # the two single pixels of the prediction go
    assert c == {"n_gt": 3, "n_found": 1, "n_pred": 2, "n_true": 1, "truncated": False}
    c = R.lesion_counts(pred, gt, max_components=2)
    assert c["truncated"] and c["n_gt"] == 3 and c["n_pred"] == 4
    got = R.lesion_metrics([R.lesion_counts(pred, gt), R.lesion_counts(gt, gt)])
    assert got["lesion_recall"] == 5 / 6 and got["lesion_precision"] == 5 / 7 and got["fp_per_image"] == 1.0 and got["n_images"] == 2


def test_refusals_without_a_device():
    for kw in (dict(overlap=1.5), dict(overlap=-0.1), dict(min_area=-1), dict(min_area=1.5), dict(connectivity=6), dict(max_components=0),
               dict(max_components=65537)):
        with pytest.raises(ValueError):
            LesionMetrics(**kw)
    m = LesionMetrics()
    with pytest.raises(RuntimeError):
        m.update(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    p = torch.zeros(1, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        m.update_packed(p, p, 8)
    for call in (lambda: label_components(p, 8), lambda: filter_components(p, 8, min_area=2), lambda: components_to_instances(p, 8)):
        with pytest.raises(RuntimeError):
            call()


def test_validation_step_lesion_options():
    for bad in ("yes", 3, dict(overlop=0.5), dict(overlap=2.0), dict(connectivity=5), dict(dist_sync=False)):
        with pytest.raises(ValueError):
            ValidationStep(None, lesions=bad)
    assert ValidationStep._lesion_options(None) is None and ValidationStep._lesion_options(True) == {}
    assert ValidationStep._lesion_options(dict(overlap=0.1, min_area=4)) == dict(overlap=0.1, min_area=4)
    with pytest.raises(NotImplementedError):                 # valid options: the constructor gets as far as the model
        ValidationStep(None, lesions=dict(connectivity=8))


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(tmp_path, lib):
    structs = {"mtbt_components_args": L.ComponentsArgs, "mtbt_select_components_args": L.SelectComponentsArgs}
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
        assert int(out[name]) == C.sizeof(st) == lib.mtbt_sizeof_components_args(which)
        for f, _ in st._fields_:
            assert int(out[f"{name}.{f}"]) == getattr(st, f).offset, f
    assert L.COMPONENTS_STRUCTS == tuple(structs.values())


def test_symbols_and_additive_abi(lib):
    assert lib.mtbt_sizeof_components_args(-1) == -1 and lib.mtbt_sizeof_components_args(2) == -1
    assert lib.mtbt_abi_version() == 5 == L.ABI_VERSION
    for name in ("mtbt_label_components", "mtbt_select_components", "mtbt_components_workspace_bytes", "mtbt_sizeof_components_args"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert L.SURFACE_STRUCTS == (L.SurfaceArgs,) and lib.mtbt_sizeof_surface_args(1) == -1     # the earlier tables did not move
    assert "components.hip" in B.SOURCES


def _label_args(lib, n=3, H=37, W=70, with_other=True):
    a = L.ComponentsArgs()
    for f in ("packed", "workspace", "labels", "n_components", "area", "box", "first") + (("other", "inter") if with_other else ()):
        setattr(a, f, PTR)
    a.n, a.H, a.W, a.pitch, a.connectivity, a.max_components = n, H, W, 8 * ((W + 63) // 64), 4, 16
    a.workspace_bytes = lib.mtbt_components_workspace_bytes(n, H, W)
    return a


def _select_args(lib, n=3, H=37, W=70):
    a = L.SelectComponentsArgs()
    for f in ("packed", "workspace", "out", "n_kept"):
        setattr(a, f, PTR)
    a.n, a.H, a.W, a.pitch, a.min_area, a.keep_largest = n, H, W, 8 * ((W + 63) // 64), 2, 1
    a.workspace_bytes = lib.mtbt_components_workspace_bytes(n, H, W)
    return a


@pytest.mark.parametrize("field,value", [("packed", None), ("workspace", None), ("n_components", None), ("area", None), ("box", None),
                                         ("first", None), ("other", None), ("inter", None), ("n", -1), ("H", 0), ("H", 16385), ("W", 0),
                                         ("W", 16385), ("pitch", 8), ("pitch", 24), ("connectivity", 0), ("connectivity", 6),
                                         ("max_components", 0), ("max_components", 65537), ("workspace_bytes", 16)])
def test_label_rejects_bad_arguments_without_launching(lib, field, value):
    assert lib.mtbt_label_components(None, None) == EINVAL
    a = _label_args(lib)
    setattr(a, field, value)
    assert lib.mtbt_label_components(C.byref(a), None) == EINVAL


@pytest.mark.parametrize("field,value", [("packed", None), ("workspace", None), ("out", None), ("n_kept", None), ("n", -1), ("H", 0),
                                         ("H", 16385), ("W", 0), ("W", 16385), ("pitch", 8), ("keep_largest", -1), ("workspace_bytes", 16)])
def test_select_rejects_bad_arguments_without_launching(lib, field, value):
    assert lib.mtbt_select_components(None, None) == EINVAL
    a = _select_args(lib)
    setattr(a, field, value)
    assert lib.mtbt_select_components(C.byref(a), None) == EINVAL


def test_workspace_query_alignment_and_empty_calls(lib):
    ws = lib.mtbt_components_workspace_bytes
    assert ws(-1, 8, 8) == EINVAL and ws(1, 0, 8) == EINVAL and ws(1, 8, 16385) == EINVAL and ws(0, 8, 8) == 0
    assert 0 < ws(1, 37, 70) < ws(2, 37, 70) < ws(70, 37, 70)            # every plane keeps its own slice: select reads it afterwards
    assert ws(1, 37, 70) >= 4 * 37 * 70 + 4 * ((37 * 70 + 1) // 2) and ws(1, 16384, 16384) > 2 ** 30
    a = _label_args(lib)
    a.workspace_bytes -= 1
    assert lib.mtbt_label_components(C.byref(a), None) == EINVAL
    for f, off in (("packed", 4), ("other", 4), ("workspace", 8), ("labels", 2), ("n_components", 2), ("area", 2), ("box", 2), ("first", 2),
                   ("inter", 2)):
        a = _label_args(lib)
        setattr(a, f, PTR + off)
        assert lib.mtbt_label_components(C.byref(a), None) == EALIGN, f
    for f, off in (("packed", 4), ("out", 4), ("workspace", 8), ("n_kept", 2)):
        a = _select_args(lib)
        setattr(a, f, PTR + off)
        assert lib.mtbt_select_components(C.byref(a), None) == EALIGN, f
    a = _label_args(lib, n=0, with_other=False)               # nothing to do is not an error, and launches nothing
    a.workspace, a.workspace_bytes, a.labels = None, 0, None
    assert lib.mtbt_label_components(C.byref(a), None) == 0
    a = _select_args(lib, n=0)
    a.workspace, a.workspace_bytes = None, 0
    assert lib.mtbt_select_components(C.byref(a), None) == 0
