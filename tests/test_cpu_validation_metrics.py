"""CPU checks of the validation metrics: the argument checks of the two confusion-matrix entry points (`mtbt_det_confusion`,
`mtbt_cls_confusion`), the host arithmetic of ImageClassificationMetrics / DetectionConfusionMatrix on injected counts,
SegmentationMetrics.compute_map on hand-built pixel counts and against the plain-loop COCO restatement, and the data-parallel reduction
of the new classes and of the loss means under gloo."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd.metrics import DetectionConfusionMatrix, ImageClassificationMetrics, SegmentationMetrics
from multitask_bonetumor_yolo_amd.validate import BatchWeightedMeans

from coco_reference import COCO, coco_loop_iou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def _det_args():
    a = L.LossArgs()
    a.n_levels, a.N, a.nc, a.reg_max, a.img_size, a.iou_thresh = 1, 2, 2, 16, 640.0, 0.5
    a.map[0], a.h[0], a.w[0], a.map_pixel_stride[0] = 4096, 20, 20, 66
    a.gt_xyxy = a.gt_cls = a.gt_off = 4096                                   # non-null, aligned dummies: never launched
    return a


@pytest.mark.parametrize("field,value", [("N", 0), ("nc", 0), ("nc", L.CONFUSION_MAX_NC + 1), ("n_levels", 0), ("reg_max", 0),
                                         ("gt_xyxy", None), ("gt_cls", None), ("gt_off", None), ("counts", None), ("status", None)])
def test_det_confusion_rejects_bad_arguments_without_launching(lib, field, value):
    assert lib.mtbt_det_confusion(None, 4096, 4096, None) == -1
    a, counts, status = _det_args(), 4096, 4096
    if field == "counts":
        counts = value
    elif field == "status":
        status = value
    else:
        setattr(a, field, value)
    assert lib.mtbt_det_confusion(C.byref(a), counts, status, None) == -1
    a = _det_args()
    a.map[0] = None
    assert lib.mtbt_det_confusion(C.byref(a), 4096, 4096, None) == -1


# ---- the level table every loss entry point builds with one function (csrc/loss_match.h, fill_levels) --------------------------------
def _loss_args():
    a = _det_args()
    a.img_logits = a.img_gt = a.out = a.workspace = 4096
    a.n_img_classes, a.workspace_bytes = 2, 1 << 40
    return a


def _tal_args():
    a = L.TalLossArgs()
    a.n_levels, a.N, a.nc, a.reg_max, a.img_size, a.n_gt, a.topk = 1, 2, 2, 16, 640.0, 1, 10
    a.map[0], a.h[0], a.w[0], a.map_pixel_stride[0] = 4096, 20, 20, 66
    a.gt_xyxy = a.gt_cls = a.gt_off = a.out = a.workspace = 4096
    a.workspace_bytes = 1 << 40
    return a


def _mask_args():
    a = L.MaskLossArgs()
    a.n_levels, a.N, a.reg_max, a.img_size, a.iou_thresh, a.n_gt = 1, 2, 16, 640.0, 0.5, 1
    a.map[0], a.h[0], a.w[0], a.map_pixel_stride[0] = 4096, 20, 20, 66
    a.gt_xyxy = a.gt_off = a.mc = a.protos = a.gt_masks = a.workspace = a.out = 4096
    a.mc_batch_stride, a.mc_anchor_stride, a.mc_channel_stride = 400 * 32, 32, 1
    a.hp, a.wp, a.nm, a.weight, a.workspace_bytes = 160, 160, 32, 1.0, 1 << 40
    return a


def _grad_maps():
    return (C.c_void_p * 3)(4096, None, None), (C.c_int32 * 3)(66, 0, 0)


# (arguments with one valid level, the call on them, the narrowest pixel stride the entry point accepts: 0 = it reads no map)
LEVEL_USERS = {
    "multitask_loss": (_loss_args, lambda lib, a: lib.mtbt_multitask_loss(C.byref(a), None), 66),
    "multitask_loss_grad": (_loss_args, lambda lib, a: lib.mtbt_multitask_loss_grad(C.byref(a), *_grad_maps(), 4096, 4096, None), 66),
    "det_confusion": (_det_args, lambda lib, a: lib.mtbt_det_confusion(C.byref(a), 4096, 4096, None), 66),
    "tal_det_loss": (_tal_args, lambda lib, a: lib.mtbt_tal_det_loss(C.byref(a), None), 66),
    "instance_mask_loss": (_mask_args, lambda lib, a: lib.mtbt_instance_mask_loss(C.byref(a), None), 64),
    "instance_mask_loss_assigned": (_mask_args, lambda lib, a: lib.mtbt_instance_mask_loss_assigned(C.byref(a), 4096, None), 0),
}
BAD_LEVELS = ["n_levels=0", "n_levels=4", "h=0", "w=0", "narrow_stride", "null_map", "hw_above_int_max"]
# a narrow stride and a null map are no errors of an entry point that reads no map: those rows do not exist for it
LEVEL_CASES = [(u, b) for u, (_, _, min_ld) in LEVEL_USERS.items() for b in BAD_LEVELS if min_ld or b not in ("narrow_stride", "null_map")]


@pytest.mark.parametrize("user,bad", LEVEL_CASES)
def test_every_loss_entry_point_rejects_bad_level_fields_without_launching(lib, user, bad):
    """One table of bad level fields against all the entry points that fill their level table with `fill_levels`: MTBT_EINVAL before any
    launch (the pointers are dummies).  46341 * 46341 anchors on one level exceed INT_MAX: the sum is taken in 64 bits and refused."""
    make, call, min_ld = LEVEL_USERS[user]
    a = make()
    if bad.startswith("n_levels"):
        a.n_levels = int(bad[-1])
    elif bad in ("h=0", "w=0"):
        setattr(a, bad[0], (C.c_int32 * 3)(0, 0, 0))
    elif bad == "narrow_stride":
        a.map_pixel_stride[0] = min_ld - 1
    elif bad == "null_map":
        a.map[0] = None
    else:
        a.h[0] = a.w[0] = 46341
    assert call(lib, a) == -1


@pytest.mark.parametrize("args", [(None, 4096, 8, 2, 4096, 4096), (4096, None, 8, 2, 4096, 4096), (4096, 4096, 0, 2, 4096, 4096),
                                  (4096, 4096, 8, 0, 4096, 4096), (4096, 4096, 8, L.CONFUSION_MAX_NC + 1, 4096, 4096),
                                  (4096, 4096, 8, 2, None, 4096), (4096, 4096, 8, 2, 4096, None)])
def test_cls_confusion_rejects_bad_arguments_without_launching(lib, args):
    assert lib.mtbt_cls_confusion(*args, None) == -1


def test_constructors_refuse_unsupported_class_counts():
    for bad in (0, L.CONFUSION_MAX_NC + 1):
        with pytest.raises(ValueError):
            ImageClassificationMetrics(bad)
        with pytest.raises(ValueError):
            DetectionConfusionMatrix(bad, 640)


def _inject(m, counts, status=0):
    m._state = torch.tensor(list(np.asarray(counts).ravel()) + [status], dtype=torch.int64)
    return m


def test_image_metrics_from_injected_counts():
    # rows = target, columns = prediction; class 2 never occurs (neither target nor prediction)
    m = _inject(ImageClassificationMetrics(3, dist_sync=False), [[5, 1, 0], [2, 2, 0], [0, 0, 0]])
    out = m.compute()
    assert out["accuracy"] == 7 / 10
    assert np.array_equal(out["confusion_counts"], [[5, 1, 0], [2, 2, 0], [0, 0, 0]])
    assert np.allclose(out["confusion_matrix"], [[5 / 6, 1 / 6, 0], [0.5, 0.5, 0], [0, 0, 0]], rtol=0, atol=1e-15)
    assert out["precision_macro"] == pytest.approx((5 / 7 + 2 / 3) / 2, abs=1e-15)
    assert out["recall_macro"] == pytest.approx((5 / 6 + 1 / 2) / 2, abs=1e-15)
    assert out["f1_macro"] == pytest.approx((10 / 13 + 4 / 7) / 2, abs=1e-15)
    # a class that is only ever predicted counts (tp + fp + fn > 0) with zeros where its denominator is 0
    out = _inject(ImageClassificationMetrics(2, dist_sync=False), [[3, 1], [0, 0]]).compute()
    assert out["precision_macro"] == pytest.approx((3 / 3 + 0) / 2) and out["recall_macro"] == pytest.approx((3 / 4 + 0) / 2)
    assert out["f1_macro"] == pytest.approx((6 / 7 + 0) / 2) and out["accuracy"] == 3 / 4
    # nothing seen at all
    out = ImageClassificationMetrics(2, dist_sync=False).compute()
    assert out["accuracy"] == 0.0 and out["f1_macro"] == 0.0 and not out["confusion_matrix"].any()


def test_nonzero_status_raises():
    with pytest.raises(ValueError):
        _inject(ImageClassificationMetrics(2, dist_sync=False), [[1, 0], [0, 1]], status=1).compute()
    with pytest.raises(ValueError):
        _inject(DetectionConfusionMatrix(2, 640, dist_sync=False), [[1, 0], [0, 1]], status=1).compute()
    out = _inject(DetectionConfusionMatrix(2, 640, dist_sync=False), [[3, 1], [0, 0]]).compute()
    assert np.allclose(out["confusion_matrix"], [[0.75, 0.25], [0, 0]], rtol=0, atol=1e-15)


def _seg(counts, scores):
    """SegmentationMetrics holding per-image counts (TP, FP, FN, TN) and mask scores (score = psum / (TP + FP + 1e-6))."""
    s = SegmentationMetrics(dist_sync=False)
    c = torch.tensor(counts, dtype=torch.int64).reshape(-1, 4)
    s._counts.append(c)
    s._psum.append(torch.tensor(scores, dtype=torch.float32) * (c[:, 0] + c[:, 1]).float())
    return s


KEYS = {"map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium",
        "mar_large"}


def test_compute_map_gt_of_exactly_32_squared_is_small_and_medium():
    out = _seg([[1024, 0, 0, 4096 - 1024]], [0.9]).compute_map()
    assert set(out) == KEYS
    one = pytest.approx(1.0, abs=1e-12)                                  # precision = tp / (tp + fp + eps), as pycocotools
    assert out["map"] == one and out["map_small"] == one and out["map_medium"] == one and out["map_large"] == -1.0
    assert out["mar_small"] == one and out["mar_medium"] == one and out["mar_large"] == -1.0


def test_compute_map_ignores_a_detection_matched_to_an_out_of_range_gt():
    # image A: det 1000 px (small) inside a 2000 px GT (medium), IoU 0.5, score 0.9; image B: a 100 px hit, score 0.8
    out = _seg([[1000, 0, 1000, 0], [100, 0, 0, 0]], [0.9, 0.8]).compute_map()
    # small: at IoU 0.50 A matches the (medium) GT and is ignored -> B alone, AP 1; at 0.55..0.95 A is unmatched, inside the small
    # range, a false positive ranked above B -> AP 0.5
    assert out["map_small"] == pytest.approx((1.0 + 9 * 0.5) / 10, abs=1e-12)
    # medium: A is a hit at 0.50 only; B's det matches an ignored GT and A's unmatched det lies outside the range (both ignored)
    assert out["map_medium"] == pytest.approx(0.1, abs=1e-12) and out["mar_medium"] == pytest.approx(0.1, abs=1e-12)


def test_compute_map_empty_against_empty_is_iou_zero():
    out = _seg([[0, 0, 0, 4096]], [0.0]).compute_map()
    assert out["map"] == 0.0 and out["map_50"] == 0.0 and out["mar_100"] == 0.0 and out["map_small"] == 0.0
    assert _seg(np.zeros((0, 4)), []).compute_map()["map"] == -1.0


def _seg_on_random_counts():
    rng = np.random.default_rng(11)
    n = 60
    tp, fp, fn = rng.integers(0, 3000, n), rng.integers(0, 1500, n), rng.integers(0, 1500, n)
    tp[:5] = 0
    fp[:3] = 0
    counts = np.stack([tp, fp, fn, 128 * 128 - tp - fp - fn], 1)
    return _seg(counts, rng.uniform(0.5, 1.0, n).round(3))


def test_compute_map_agrees_with_compute_on_random_counts():
    s = _seg_on_random_counts()
    full, segm = s.compute(), s.compute_map()
    assert abs(segm["map"] - full["seg_map"]) <= 1e-12 and abs(segm["map_50"] - full["seg_map_50"]) <= 1e-12
    assert 0.0 < segm["map"] < 1.0


def test_segm_map_equals_coco_reference_restatement():
    """compute_map and compute's seg_map / seg_map_50 against the plain-loop restatement (no code shared with `_accumulate`), fed what
    the metric defines per image: one detection (its mask score, area TP + FP) and one GT (area TP + FN), both class 0, mask IoU
    TP / (TP + FP + FN) (0 for an empty union)."""
    s = _seg_on_random_counts()
    c, score = s.per_image()
    images = [([float(p)], [0], [tp + fp], [0], [tp + fn], [[tp / (tp + fp + fn) if tp + fp + fn else 0.0]])
              for (tp, fp, fn, _), p in zip(c.tolist(), score)]
    want = coco_loop_iou(images, COCO, [1, 10, 100])
    full, segm = s.compute(), s.compute_map()
    assert set(segm) == set(want) == KEYS and 0.0 < want["map"] < 1.0
    for k in KEYS:
        assert abs(segm[k] - want[k]) <= 1e-12, (k, segm[k], want[k])
    assert abs(full["seg_map"] - want["map"]) <= 1e-12 and abs(full["seg_map_50"] - want["map_50"]) <= 1e-12


def test_batch_weighted_means():
    m = BatchWeightedMeans(2, dist_sync=False)
    m.update((torch.tensor(1.0), torch.tensor(4.0)), 4)
    m.update((torch.tensor(3.0), torch.tensor(-2.0)), 2)
    assert np.allclose(m.compute(), [(4 + 6) / 6, (16 - 4) / 6], rtol=0, atol=1e-15)
    m.reset()
    assert not m.compute().any()


def test_gloo_world_size_2_validation_metric_sync(tmp_path):
    """Two gloo ranks hold different counts: `compute()` on each returns the global value (the counts summed over ranks, the loss means
    weighted over every rank's batches) and leaves the local state as it was."""
    script = tmp_path / "w.py"
    script.write_text(
        "import sys, numpy as np, torch, torch.distributed as dist\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "from multitask_bonetumor_yolo_amd.metrics import DetectionConfusionMatrix, ImageClassificationMetrics\n"
        "from multitask_bonetumor_yolo_amd.validate import BatchWeightedMeans\n"
        "dist.init_process_group('gloo')\n"
        "r, w = dist.get_rank(), dist.get_world_size()\n"
        "def state(rank, nc):\n"
        "    g = torch.Generator().manual_seed(31 + rank * 7 + nc)\n"
        "    return torch.cat([torch.randint(0, 50, (nc * nc,), generator=g), torch.zeros(1, dtype=torch.int64)])\n"
        "def losses(rank):\n"
        "    g = torch.Generator().manual_seed(5 + rank)\n"
        "    return [(torch.rand(6, generator=g).unbind(), 2 + rank + k) for k in range(3)]\n"
        "img, det = ImageClassificationMetrics(3), DetectionConfusionMatrix(2, 640)\n"
        "img._state, det._state = state(r, 3), state(r, 2)\n"
        "lm = BatchWeightedMeans(6)\n"
        "for v, b in losses(r): lm.update(v, b)\n"
        "local = (img._state.clone(), det._state.clone(), lm._sum.clone(), lm._count)\n"
        "gi, gd, gl = img.compute(), det.compute(), lm.compute()\n"
        "ri, rd, rl = ImageClassificationMetrics(3, dist_sync=False), DetectionConfusionMatrix(2, 640, dist_sync=False), BatchWeightedMeans(6, dist_sync=False)\n"
        "ri._state = sum(state(k, 3) for k in range(w)); rd._state = sum(state(k, 2) for k in range(w))\n"
        "for k in range(w):\n"
        "    for v, b in losses(k): rl.update(v, b)\n"
        "wi, wd, wl = ri.compute(), rd.compute(), rl.compute()\n"
        "assert all(np.array_equal(gi[k], wi[k]) for k in wi) and all(np.array_equal(gd[k], wd[k]) for k in wd)\n"
        "assert np.allclose(gl, wl, rtol=1e-15, atol=0)\n"
        "assert torch.equal(img._state, local[0]) and torch.equal(det._state, local[1]) and torch.equal(lm._sum, local[2]) and lm._count == local[3]\n"
        "print(f'RANK{r} ok {gi[\"accuracy\"]:.9f} {gi[\"f1_macro\"]:.9f} {int(gd[\"confusion_counts\"].sum())} {gl[0]:.9f}', flush=True)\n"
        "dist.destroy_process_group()\n")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29571", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=180)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    rows = sorted(l.split() for o in outs for l in o.splitlines() if l.startswith("RANK"))
    assert len(rows) == 2 and rows[0][1:] == rows[1][1:]
