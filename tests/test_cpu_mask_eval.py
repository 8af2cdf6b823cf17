"""CPU checks of the instance-mask mAP (metrics.DeviceMaskMeanAveragePrecision, csrc/mask_eval.hip): the four C-ABI structs against the
header through gcc, their size table, that the ABI grew without moving, the argument checks of the three entry points (nothing is
launched), the constructor's refusals and the host layout helper that maps a list of images to launches."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd.metrics import (MASK_EVAL_MAX_IMAGES, DeviceMaskMeanAveragePrecision, DeviceMeanAveragePrecision,
                                                  _mask_launch_layout)

from coco_reference import COCO, coco_loop_iou
from mask_reference import loop_images, mask_case, pack_np, pair_counts_np, unpack_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = (("mtbt_pack_masks_args", L.PackMasksArgs), ("mtbt_mask_image", L.MaskImage), ("mtbt_mask_pair_args", L.MaskPairArgs),
           ("mtbt_mask_eval_args", L.MaskEvalArgs))
EINVAL, EALIGN = -1, -2
PTR = 4096                                       # non-null, aligned dummy: every call below is refused before any launch


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def test_struct_layouts_match_the_header(tmp_path, lib):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){']
    for name, st in STRUCTS:
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in st._fields_]
    lines.append('return 0;}')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for which, (name, st) in enumerate(STRUCTS):
        assert int(out[name]) == C.sizeof(st) == lib.mtbt_sizeof_mask_eval_args(which), name
        for f, _ in st._fields_:
            assert int(out[f"{name}.{f}"]) == getattr(st, f).offset, (name, f)
    assert L.MASK_EVAL_STRUCTS == tuple(st for _, st in STRUCTS)


def test_size_table_range_and_additive_abi(lib):
    assert lib.mtbt_sizeof_mask_eval_args(-1) == -1 and lib.mtbt_sizeof_mask_eval_args(4) == -1
    assert lib.mtbt_abi_version() == 5 == L.ABI_VERSION
    assert len(L.ARG_STRUCTS) == 10 and lib.mtbt_sizeof_args(9) > 0 and lib.mtbt_sizeof_args(10) == -1
    assert len(L.FRAME_STRUCTS) == 2 and lib.mtbt_sizeof_frame_args(1) > 0 and lib.mtbt_sizeof_frame_args(2) == -1
    for name in ("mtbt_pack_masks", "mtbt_mask_pair_counts", "mtbt_mask_eval", "mtbt_sizeof_mask_eval_args"):
        assert name in L.SYMBOLS


# ---- mtbt_pack_masks -----------------------------------------------------------------------------------------------------------
def _pack_args():
    a = L.PackMasksArgs()
    a.src = a.out = PTR
    a.plane_stride, a.row_stride = 5 * 70, 70
    a.n_src, a.n_out, a.H, a.W, a.pitch, a.dtype = 2, 2, 5, 70, 16, 0
    return a


@pytest.mark.parametrize("field,value", [("src", None), ("out", None), ("pitch", 8), ("pitch", 24), ("H", 0), ("W", 0), ("dtype", 2),
                                         ("row_stride", 69), ("n_out", 3), ("n_src", -1), ("n_out", -1), ("plane_stride", -1)])
def test_pack_masks_rejects_bad_arguments_without_launching(lib, field, value):
    assert lib.mtbt_pack_masks(None, None) == EINVAL
    a = _pack_args()
    setattr(a, field, value)
    assert lib.mtbt_pack_masks(C.byref(a), None) == EINVAL


def test_pack_masks_size_and_alignment_limits(lib):
    a = _pack_args()
    a.H, a.W, a.pitch, a.row_stride, a.plane_stride = 1 << 16, 1 << 15, (1 << 15) // 8, 1 << 15, 1 << 31     # H * W == 2^31
    assert lib.mtbt_pack_masks(C.byref(a), None) == EINVAL
    a = _pack_args()
    a.out = PTR + 4
    assert lib.mtbt_pack_masks(C.byref(a), None) == EALIGN
    a = _pack_args()
    a.dtype, a.src = 1, PTR + 2
    assert lib.mtbt_pack_masks(C.byref(a), None) == EALIGN
    a = _pack_args()
    a.n_out = 0                                                          # nothing to do is not an error, and launches nothing
    assert lib.mtbt_pack_masks(C.byref(a), None) == 0


# ---- mtbt_mask_pair_counts -----------------------------------------------------------------------------------------------------
def _pair_args(n=2, K=17, M=3):
    a = L.MaskPairArgs()
    a.counts = a.gt_image = a.inter = a.det_area = a.gt_area = PTR
    a.B, a.K, a.M = n, K, M
    im = (L.MaskImage * max(n, 1))()
    for i in range(n):
        im[i].det = im[i].gt_base = PTR
        im[i].H, im[i].W, im[i].pitch, im[i].g0, im[i].gt_planes = 5, 40, 8, 0, M
    return a, im


@pytest.mark.parametrize("field,value", [("inter", None), ("det_area", None), ("gt_image", None), ("gt_area", None), ("K", 0), ("K", 1025),
                                         ("M", -1), ("B", 1)])
def test_pair_counts_rejects_bad_arguments_without_launching(lib, field, value):
    a, im = _pair_args()
    assert lib.mtbt_mask_pair_counts(None, im, 2, None) == EINVAL
    assert lib.mtbt_mask_pair_counts(C.byref(a), None, 2, None) == EINVAL
    setattr(a, field, value)
    assert lib.mtbt_mask_pair_counts(C.byref(a), im, 2, None) == EINVAL


@pytest.mark.parametrize("field,value", [("det", None), ("gt_base", None), ("pitch", 16), ("H", 0), ("W", 0), ("gt_planes", -1)])
def test_pair_counts_rejects_bad_images_without_launching(lib, field, value):
    a, im = _pair_args()
    setattr(im[1], field, value)
    assert lib.mtbt_mask_pair_counts(C.byref(a), im, 2, None) == EINVAL


def test_pair_counts_image_count_size_and_alignment_limits(lib):
    a, im = _pair_args(n=33)
    assert lib.mtbt_mask_pair_counts(C.byref(a), im, 33, None) == EINVAL
    a, im = _pair_args(n=0)
    assert lib.mtbt_mask_pair_counts(C.byref(a), im, 0, None) == EINVAL
    a, im = _pair_args()
    im[0].H, im[0].W, im[0].pitch = 1 << 16, 1 << 15, (1 << 15) // 8     # H * W == 2^31
    assert lib.mtbt_mask_pair_counts(C.byref(a), im, 2, None) == EINVAL
    a, im = _pair_args()
    im[1].det = PTR + 4                                                  # planes are 8-byte aligned ...
    assert lib.mtbt_mask_pair_counts(C.byref(a), im, 2, None) == EALIGN
    a, im = _pair_args()
    a.inter = PTR + 2
    assert lib.mtbt_mask_pair_counts(C.byref(a), im, 2, None) == EALIGN


# ---- mtbt_mask_eval ------------------------------------------------------------------------------------------------------------
def _eval_args():
    a = L.MaskEvalArgs()
    for f in ("inter", "det_area", "gt_px", "scores", "labels", "counts", "gt_image", "gt_label", "rank", "match", "ignore", "gt_area", "status"):
        setattr(a, f, PTR)
    a.B, a.K, a.M, a.T, a.max_det = 1, 100, 3, 10, 100
    return a


@pytest.mark.parametrize("field,value", [("T", 0), ("T", 33), ("K", 0), ("K", 1025), ("max_det", 0), ("B", -1), ("M", -1), ("inter", None),
                                         ("det_area", None), ("gt_px", None), ("gt_image", None), ("gt_label", None), ("scores", None),
                                         ("status", None)])
def test_mask_eval_rejects_bad_arguments_without_launching(lib, field, value):
    assert lib.mtbt_mask_eval(None, None) == EINVAL
    a = _eval_args()
    setattr(a, field, value)
    assert lib.mtbt_mask_eval(C.byref(a), None) == EINVAL


def test_mask_eval_alignment_and_empty_batch(lib):
    a = _eval_args()
    a.labels = PTR + 4
    assert lib.mtbt_mask_eval(C.byref(a), None) == EALIGN
    a = _eval_args()
    a.B = 0                                                              # nothing to do: no launch
    assert lib.mtbt_mask_eval(C.byref(a), None) == 0


# ---- Python ----------------------------------------------------------------------------------------------------------------------
def test_constructor_refusals():
    with pytest.raises(ValueError):
        DeviceMaskMeanAveragePrecision(iou_thresholds=np.linspace(0.1, 0.9, 33))
    with pytest.raises(ValueError):
        DeviceMaskMeanAveragePrecision(iou_thresholds=[])
    with pytest.raises(ValueError):
        DeviceMaskMeanAveragePrecision(max_detection_thresholds=[0, 10])
    with pytest.raises(TypeError):
        DeviceMaskMeanAveragePrecision(box_format="xyxy")
    with pytest.raises(TypeError):
        DeviceMaskMeanAveragePrecision(iou_type="segm")
    with pytest.raises(ValueError, match="DeviceMaskMeanAveragePrecision"):
        DeviceMeanAveragePrecision(iou_type="segm")                      # still refused there, and says where to go
    m = DeviceMaskMeanAveragePrecision(iou_thresholds=[0.5, 0.75], max_detection_thresholds=[100, 1, 10], class_metrics=True)
    assert m.max_dets == [1, 10, 100] and m.class_metrics and list(m.iou_thresholds) == [0.5, 0.75]
    r = m.compute()                                                      # no update: the empty key set, no device needed
    assert r["map"] == -1.0 and r["classes"] == []


def test_launch_layout_of_a_list_of_images():
    (c0, c1, g0, gi), = _mask_launch_layout([0, 1, 5, 9])
    assert (c0, c1) == (0, 4) and g0 == [0, 0, 1, 6]
    assert gi.dtype == np.int32 and gi.tolist() == [1] + [2] * 5 + [3] * 9
    # image b's plane j is flat row g0[b] + j: the kernel reads it at gt_base_b + (m - g0_b) planes
    for b, n in enumerate([0, 1, 5, 9]):
        assert [m - g0[b] for m in np.nonzero(gi == b)[0]] == list(range(n))
    assert _mask_launch_layout([]) == []
    with pytest.raises(ValueError):
        _mask_launch_layout([1, -1])


def test_launch_layout_chunks_at_32_images():
    n_gt = [b % 3 for b in range(70)]
    chunks = _mask_launch_layout(n_gt)
    assert MASK_EVAL_MAX_IMAGES == 32 and [(c[0], c[1]) for c in chunks] == [(0, 32), (32, 64), (64, 70)]
    for c0, c1, g0, gi in chunks:
        assert len(gi) == sum(n_gt[c0:c1]) and (gi.max() < c1 - c0 if len(gi) else True)     # indices are local to the launch
        assert g0 == np.cumsum([0] + n_gt[c0:c1])[:-1].tolist()
        assert np.bincount(gi, minlength=c1 - c0).tolist() == n_gt[c0:c1]


# ---- the GPU tests' case set, checked with the restatement alone ------------------------------------------------------------------
def test_mask_case_set_is_not_degenerate():
    """tests/test_gpu_mask_eval.py compares the device path with `coco_loop_iou` on this set (seed 1): it must exercise every area
    range, all ten thresholds and the planted cases, whatever the device computes."""
    case = mask_case(1)
    images = loop_images(case)
    r = coco_loop_iou(images, COCO, [1, 10, 100], class_metrics=True)
    assert 0 < r["map"] < 1 and all(r[k] != -1 for k in ("map_small", "map_medium", "map_large"))
    assert r["classes"] == [0, 1, 2] and r["map_per_class"][2] == -1.0                        # class 2: detections without GT
    ious = np.array([v for im in images for row in im[5] for v in row])
    assert all(((ious >= lo) & (ious < lo + 0.05)).any() for lo in np.linspace(0.5, 0.95, 10))  # matches at every threshold step
    assert {1024.0, 9216.0} <= set(images[0][2]) and {1024.0, 9216.0} <= set(images[0][4])     # inclusive area bounds
    assert np.array_equal(case[1]["gt"][0], case[1]["gt"][-1])                                 # two identical GT masks
    assert not case[2]["det"][0].any() and not case[2]["gt"][-1].any() and images[2][5][0][-1] == 0.0   # union 0 -> IoU 0
    assert any(len(set(c["scores"][:c["count"]].tolist())) < c["count"] for c in case)         # duplicated scores
    assert {len(c["gt"]) for c in case} >= {0, 1, 6} and max(len(c["gt"]) for c in case) == 6


def test_host_packers_round_trip():
    bits = np.random.default_rng(0).uniform(size=(3, 5, 70)) < 0.5
    p = pack_np(bits)
    assert p.shape == (3, 5, 16) and np.array_equal(unpack_np(p, 70), bits) and not np.unpackbits(p, axis=-1, bitorder="little")[:, :, 70:].any()
    inter, da, ga = pair_counts_np(bits[:2], bits[1:])
    assert inter[0, 1] == bits[1].sum() == da[1] == ga[0] and inter.shape == (2, 2)
