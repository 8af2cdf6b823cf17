"""CPU checks of the device box mAP (metrics.DeviceMeanAveragePrecision, csrc/box_eval.hip): the C-ABI struct and its argument
checks, the constructor's refusals, and the host accumulation (`_accumulate`, pycocotools accumulate / summarize) on hand-built
records.  torchmetrics / pycocotools are absent: PARITY UNPINNED against them; the algorithm is pycocotools' published one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd.metrics import DeviceMeanAveragePrecision, _accumulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL, SMALL, MEDIUM, LARGE = 1, 2, 4, 8          # gt_area bits / match-ignore word index = area range


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def test_box_eval_struct_layout_matches_header(tmp_path, lib):
    fields = [f for f, _ in L.BoxEvalArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(mtbt_box_eval_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(mtbt_box_eval_args, {f}));' for f in fields]
    lines.append('return 0;}')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(L.BoxEvalArgs)
    for f in fields:
        assert int(out[f]) == getattr(L.BoxEvalArgs, f).offset, f
    assert lib.mtbt_sizeof_args(9) == C.sizeof(L.BoxEvalArgs)
    assert L.ARG_STRUCTS[9] is L.BoxEvalArgs


def _valid_args():
    a = L.BoxEvalArgs()
    a.boxes = a.scores = a.labels = a.gt = a.rank = a.match = a.ignore = a.gt_area = a.status = 4096   # non-null, aligned dummies
    a.B, a.K, a.M, a.T, a.max_det, a.gt_format, a.img_size = 1, 100, 3, 10, 100, 0, 640.0
    return a


@pytest.mark.parametrize("field,value", [("T", 0), ("T", 33), ("K", 1025), ("max_det", 0), ("boxes", None), ("status", None),
                                         ("gt", None), ("gt_format", 2)])
def test_box_eval_rejects_bad_arguments_without_launching(lib, field, value):
    assert lib.mtbt_box_eval(None, None) == -1
    a = _valid_args()
    setattr(a, field, value)
    assert lib.mtbt_box_eval(C.byref(a), None) == -1


def test_constructor_refuses_what_it_does_not_compute():
    with pytest.raises(ValueError):
        DeviceMeanAveragePrecision(box_format="cxcywh")
    with pytest.raises(ValueError):
        DeviceMeanAveragePrecision(iou_type="segm")
    with pytest.raises(ValueError):
        DeviceMeanAveragePrecision(iou_thresholds=np.linspace(0.1, 0.9, 33))
    m = DeviceMeanAveragePrecision(iou_thresholds=[0.5, 0.75], max_detection_thresholds=[100, 1, 10], class_metrics=True)
    assert m.max_dets == [1, 10, 100]


def _records(dets, gts):
    """dets: (image, rank, score, label, match words [4], ignore words [4]); gts: (label, area bits)."""
    d = list(zip(*dets)) if dets else [[]] * 6
    g = list(zip(*gts)) if gts else [[]] * 2
    return {"image": np.array(d[0], np.int64), "rank": np.array(d[1], np.int64), "score": np.array(d[2], np.float64),
            "label": np.array(d[3], np.int64), "match": np.array(d[4], np.uint32).reshape(-1, 4),
            "ignore": np.array(d[5], np.uint32).reshape(-1, 4), "gt_label": np.array(g[0], np.int64), "gt_area": np.array(g[1], np.uint32)}


def test_hand_computed_ap_all_areas():
    # two small GT boxes (10 x 10); detections by score: hit, miss, hit -> recall .5 .5 1, precision 1 .5 2/3, envelope 1 2/3 2/3
    hit, miss = [1, 1, 0, 0], [0, 0, 0, 0]
    rec = _records([(0, 0, 0.9, 0, hit, miss), (0, 1, 0.8, 0, miss, miss), (0, 2, 0.7, 0, hit, miss)], [(0, ALL | SMALL), (0, ALL | SMALL)])
    r = _accumulate(rec, [0.5], [1, 10, 100])
    want = (51 * 1.0 + 50 * (2.0 / 3.0)) / 101
    assert abs(r["map"] - want) < 1e-12 and abs(r["map_50"] - want) < 1e-12 and r["map_75"] == -1.0
    assert abs(r["map_small"] - want) < 1e-12
    assert r["map_medium"] == -1.0 and r["map_large"] == -1.0 and r["mar_medium"] == -1.0     # no medium / large GT
    assert r["mar_1"] == 0.5 and r["mar_10"] == 1.0 and r["mar_100"] == 1.0 and r["mar_small"] == 1.0
    assert "map_per_class" not in r


def test_class_without_gt_is_left_out_and_per_class_values():
    hit, miss = [3, 0, 0, 3], [0, 0, 0, 0]              # matched at both thresholds, in "all" and "large"
    rec = _records([(0, 0, 0.5, 0, hit, miss), (0, 0, 0.9, 7, miss, miss), (1, 0, 0.4, 3, miss, miss)], [(0, ALL | LARGE), (3, ALL | LARGE)])
    r = _accumulate(rec, [0.5, 0.75], [1, 10, 100], class_metrics=True)
    assert r["classes"] == [0, 3, 7]
    assert r["map_per_class"] == pytest.approx([1.0, 0.0, -1.0], abs=1e-12) and r["mar_100_per_class"] == [1.0, 0.0, -1.0]
    assert abs(r["map"] - 0.5) < 1e-12 and abs(r["map_large"] - 0.5) < 1e-12
    assert r["map_small"] == -1.0 and r["mar_small"] == -1.0


def test_ignored_detections_count_neither_way_and_max_det_prefix():
    # "small" range: detection 0 matched a large (ignored) GT box -> ignored; detection 1 unmatched but large -> ignored;
    # detection 2 matched the small GT box.  In "all": 0 and 2 are hits, 1 is a false positive.
    rec = _records([(0, 0, 0.9, 0, [1, 0, 0, 0], [0, 1, 0, 0]), (0, 1, 0.8, 0, [0, 0, 0, 0], [0, 1, 0, 0]),
                    (0, 2, 0.7, 0, [1, 1, 0, 0], [0, 0, 0, 0])], [(0, ALL | LARGE), (0, ALL | SMALL)])
    r = _accumulate(rec, [0.5], [1, 2, 100])
    assert abs(r["map_small"] - 1.0) < 1e-12 and r["mar_small"] == 1.0
    assert abs(r["map"] - (51 + 50 * 2 / 3) / 101) < 1e-12
    assert r["mar_1"] == 0.5 and r["mar_2"] == 0.5 and r["mar_100"] == 1.0     # max-det 1 / 2 keep ranks 0 / 0-1 only


def test_empty_records():
    r = _accumulate(_records([], []), [0.5], [1, 10, 100], class_metrics=True)
    assert r["map"] == -1.0 and r["map_small"] == -1.0 and r["mar_100"] == -1.0 and r["classes"] == []
