"""Device box mAP (metrics.DeviceMeanAveragePrecision, csrc/box_eval.hip) against the host MeanAveragePrecision (the keys both
compute), against the plain-loop restatement of pycocotools evaluateImg / accumulate / summarize with area ranges and per-class
output (tests/coco_reference.py), and the batch path against the list path on real model output."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multitask_bonetumor_yolo_amd.metrics import DeviceMeanAveragePrecision, MeanAveragePrecision

from coco_reference import AREAS, COCO, _random_set, coco_loop

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- data --------------------------------------------------------------------------------------------------------------------
def _t(lst):
    return [{k: torch.as_tensor(v) for k, v in d.items()} for d in lst]


def _device_map(preds, targets, **kw):
    m = DeviceMeanAveragePrecision(**kw)
    m.update(_t(preds), _t(targets))
    return m


def _close(got, want, tol=1e-12):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, v in want.items():
        if isinstance(v, list):
            assert len(got[k]) == len(v) and all(abs(a - b) <= tol for a, b in zip(got[k], v)), (k, got[k], v)
        else:
            assert abs(got[k] - v) <= tol, (k, got[k], v)


# ---- tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [[0.5], COCO])
@pytest.mark.parametrize("max_dets", [[1, 3, 10], [1, 10, 100]])
def test_shared_keys_equal_host_class(thr, max_dets):
    preds, targets = _random_set(1)
    got = _device_map(preds, targets, iou_thresholds=thr, max_detection_thresholds=max_dets).compute()
    host = MeanAveragePrecision(iou_thresholds=thr, max_detection_thresholds=max_dets)
    host.update(_t(preds), _t(targets))
    want = host.compute()
    assert want["map"] > 0.05
    _close({k: got[k] for k in want}, want)


@pytest.mark.parametrize("seed", [2, 3])
def test_all_keys_equal_loop_restatement(seed):
    preds, targets = _random_set(seed)
    for thr, md in ((COCO, [1, 10, 100]), ([0.5, 0.75], [1, 3, 10])):
        got = _device_map(preds, targets, iou_thresholds=thr, max_detection_thresholds=md, class_metrics=True).compute()
        want = coco_loop(preds, targets, thr, md, class_metrics=True)
        assert got["classes"] == want["classes"] == [0, 1, 2] and want["map_per_class"][2] == -1.0
        assert min(want[k] for k in ("map_small", "map_medium", "map_large")) > 0.0
        _close(got, want)


def _one(dets, gts, thr=(0.5,)):
    """dets: [(box, score)], gts: [box], all class 0 -> compute() of the device class and of the loop restatement."""
    p = [dict(boxes=np.array([d[0] for d in dets], np.float32).reshape(-1, 4), scores=np.array([d[1] for d in dets], np.float32),
              labels=np.zeros(len(dets), np.int64))]
    t = [dict(boxes=np.array(gts, np.float32).reshape(-1, 4), labels=np.zeros(len(gts), np.int64))]
    got = _device_map(p, t, iou_thresholds=list(thr), class_metrics=True).compute()
    _close(got, coco_loop(p, t, list(thr), [1, 10, 100], class_metrics=True))
    return got


def test_hand_built_area_and_tie_cases():
    one = pytest.approx(1.0 / (1.0 + np.spacing(1)), abs=1e-12)               # pycocotools' precision of a lone true positive
    r = _one([([0, 0, 32, 32], 0.9)], [[0, 0, 32, 32]])                        # area exactly 32^2: small AND medium
    assert r["map_small"] == one and r["map_medium"] == one and r["mar_small"] == r["mar_medium"] == 1.0 and r["map_large"] == -1.0
    r = _one([([0, 0, 96, 96], 0.9)], [[0, 0, 96, 96]])                        # exactly 96^2: medium AND large
    assert r["map_medium"] == one and r["map_large"] == one and r["map_small"] == -1.0
    r = _one([([0, 0, 100, 100], 0.9), ([200, 200, 210, 210], 0.8)], [[0, 0, 100, 100], [200, 200, 210, 210]])
    assert r["map_small"] == one and r["map_large"] == one                     # the large match is neither TP nor FP in "small"
    r = _one([([300, 300, 400, 400], 0.9), ([200, 200, 210, 210], 0.8)], [[200, 200, 210, 210]])
    assert r["map_small"] == one and r["map"] == pytest.approx(0.5, abs=1e-12) and r["map_large"] == -1.0
    #        (an unmatched large detection: ignored in "small", a false positive in "all")
    # det A has IoU 90/110 with both GT boxes (a tie) and takes the LATER one, so det B (== the first GT box) still finds its box
    # at 0.75; taking the earlier one would leave B with IoU 80/120 < 0.75
    r = _one([([1, 0, 11, 10], 0.9), ([0, 0, 10, 10], 0.8)], [[0, 0, 10, 10], [2, 0, 12, 10]], thr=(0.75,))
    assert r["map"] == one and r["mar_100"] == 1.0


def _model_batch(B=4, S=128):
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, postprocess as pp
    from oracle.model import ConvNeXtBiFPNYOLO as OracleModel, randomize_
    torch.manual_seed(0)
    ora = randomize_(OracleModel(2, 2, pretrained_backbone=False)).eval()
    hip = ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)
    hip.load_state_dict(ora.state_dict(), strict=True)
    hip = hip.to(DEV).eval()
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        out = hip(x, "infer")
        res = pp.detect_and_segment(out["detect_features"], out["segment_protos"][1], out["segment_protos"][2], S, masks=False)
    torch.cuda.synchronize()
    # GT rows (batch_idx, cls, cx, cy, w, h) normalised: jittered copies of some kept boxes, one random box, image 1 without GT
    rng = np.random.default_rng(5)
    rows = []
    for b in range(B):
        if b == 1:
            continue
        n = int(res["counts"][b])
        kb = res["boxes"][b, :n].cpu().numpy()
        kl = res["labels"][b, :n].cpu().numpy()
        for j in rng.choice(n, min(n, 3), replace=False):
            x1, y1, x2, y2 = kb[j] + rng.normal(0, 1.5, 4)
            rows.append([b, kl[j], (x1 + x2) / 2 / S, (y1 + y2) / 2 / S, abs(x2 - x1) / S, abs(y2 - y1) / S])
        rows.append([b, int(rng.integers(0, 2)), 0.5, 0.5, 0.3, 0.2])
    return res, torch.tensor(rows, dtype=torch.float32), S


def _reference_lists(res, gt_rows, S):
    """validation_step's per-image dicts (:535-570); the GT conversion is :566's per-box formula in torch fp32."""
    preds, targets = [], []
    for b, n in enumerate(res["counts"].tolist()):
        preds.append(dict(boxes=res["boxes"][b, :n].cpu(), scores=res["scores"][b, :n].cpu(), labels=res["labels"][b, :n].cpu()))
        g = gt_rows[gt_rows[:, 0] == b]
        c = g[:, 2:6]
        xyxy = torch.stack([(c[:, 0] - c[:, 2] / 2) * S, (c[:, 1] - c[:, 3] / 2) * S, (c[:, 0] + c[:, 2] / 2) * S,
                            (c[:, 1] + c[:, 3] / 2) * S], dim=1).clamp_(0, S)
        targets.append(dict(boxes=xyxy, labels=g[:, 1].long()))
    return preds, targets


def test_batch_path_equals_list_path():
    res, gt_rows, S = _model_batch()
    a = DeviceMeanAveragePrecision(class_metrics=True)
    a.update_batched(res, gt_rows.to(DEV), S)
    b = DeviceMeanAveragePrecision(class_metrics=True)
    b.update(*_reference_lists(res, gt_rows, S))
    ra, rb = a.compute(), b.compute()
    assert ra == rb and ra["map"] > 0.0, (ra, rb)


def test_update_batched_does_not_synchronise():
    res, gt_rows, S = _model_batch(B=2)
    gt = gt_rows.to(DEV)
    m = DeviceMeanAveragePrecision()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update_batched(res, gt, S)
        m.update_batched(res, gt, S)
        with pytest.raises(RuntimeError):                                      # positive control: the mode fires on this build
            res["counts"].sum().item()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert m.compute()["map"] >= 0.0


def test_caps():
    preds, targets = _random_set(4, n_img=2)
    rng = np.random.default_rng(6)
    gb, gl = targets[0]["boxes"], targets[0]["labels"]
    src = rng.integers(0, len(gb), 300)
    db = (gb[src] + np.round(rng.normal(0, 2.0, (300, 4)))).astype(np.float32)
    db[:, 2:] = np.maximum(db[:, 2:], db[:, :2] + 1)
    sc, dl = np.round(rng.uniform(0, 1, 300), 2).astype(np.float32), gl[src]
    boxes, scores, labels = torch.zeros(1, 1024, 4), torch.zeros(1, 1024), torch.zeros(1, 1024, dtype=torch.int64)
    boxes[0, :300], scores[0, :300], labels[0, :300] = torch.from_numpy(db), torch.from_numpy(sc), torch.from_numpy(dl)
    det = dict(boxes=boxes.to(DEV), scores=scores.to(DEV), labels=labels.to(DEV), counts=torch.tensor([300], dtype=torch.int32, device=DEV))
    c = torch.from_numpy(gb)
    rows = torch.cat([torch.zeros(len(gb), 1), torch.from_numpy(gl).float()[:, None], (c[:, :2] + c[:, 2:]) / 2 / 640, (c[:, 2:] - c[:, :2]) / 640], 1)
    m = DeviceMeanAveragePrecision(class_metrics=True)
    m.update_batched(det, rows.to(DEV), 640)
    xyxy = torch.cat([(rows[:, 2:4] - rows[:, 4:6] / 2) * 640, (rows[:, 2:4] + rows[:, 4:6] / 2) * 640], 1).clamp_(0, 640)
    host = [dict(boxes=db, scores=sc, labels=dl)], [dict(boxes=xyxy.numpy(), labels=gl)]
    _close(m.compute(), coco_loop(host[0], host[1], COCO, [1, 10, 100], class_metrics=True))
    many = torch.cat([torch.zeros(1025, 1), torch.zeros(1025, 1), torch.full((1025, 2), 0.5), torch.full((1025, 2), 0.1)], 1)
    m = DeviceMeanAveragePrecision()
    m.update_batched(det, many.to(DEV), 640)
    with pytest.raises(RuntimeError, match="more than 1024 GT"):
        m.compute()


def _padded(preds, K):
    B = len(preds)
    boxes, scores, labels = torch.zeros(B, K, 4), torch.zeros(B, K), torch.zeros(B, K, dtype=torch.int64)
    counts = torch.zeros(B, dtype=torch.int32)
    for b, p in enumerate(preds):
        n = len(p["scores"])
        boxes[b, :n], scores[b, :n], labels[b, :n], counts[b] = torch.as_tensor(p["boxes"]), torch.as_tensor(p["scores"]), torch.as_tensor(p["labels"]), n
    return dict(boxes=boxes.to(DEV), scores=scores.to(DEV), labels=labels.to(DEV), counts=counts.to(DEV))


def _rows(targets, S):
    """xyxy pixel GT -> collated (batch_idx, cls, cx, cy, w, h) normalised rows, and the xyxy the per-box formula gives back."""
    rows = [[b, float(l), (x1 + x2) / 2 / S, (y1 + y2) / 2 / S, (x2 - x1) / S, (y2 - y1) / S]
            for b, t in enumerate(targets) for (x1, y1, x2, y2), l in zip(t["boxes"].tolist(), t["labels"].tolist())]
    rows = torch.tensor(rows, dtype=torch.float32).reshape(-1, 6)
    back = []
    for b in range(len(targets)):
        g = rows[rows[:, 0] == b]
        c = g[:, 2:6]
        xyxy = torch.stack([(c[:, 0] - c[:, 2] / 2) * S, (c[:, 1] - c[:, 3] / 2) * S, (c[:, 0] + c[:, 2] / 2) * S,
                            (c[:, 1] + c[:, 3] / 2) * S], dim=1).clamp_(0, S)
        back.append(dict(boxes=xyxy.numpy(), labels=g[:, 1].long().numpy()))
    return rows, back


def test_batches_without_gt_rows():
    """M == 0 (a validation batch with no tumour boxes): ranks and ignore bits of a full batch (K = 1024, 1000 detections, 3
    classes, tied scores) equal the host's stable per-class order, every run; mixed with batches that carry GT, compute()
    equals the loop restatement; the list path with every target empty gives M == 0 as well."""
    rng = np.random.default_rng(11)
    n, K, S, md = 1000, 1024, 640, [1, 10, 100]
    xy = rng.integers(0, 600, (2, n, 2))
    db = np.concatenate([xy.min(0), xy.max(0) + 1], 1).astype(np.float32)
    sc, dl = np.round(rng.uniform(0, 1, n), 2).astype(np.float32), rng.integers(0, 3, n)
    det = _padded([dict(boxes=db, scores=sc, labels=dl)], K)
    rank = -np.ones(K, np.int64)
    for c in range(3):
        idx = np.nonzero(dl == c)[0]
        idx = idx[np.argsort(-sc[idx], kind="mergesort")]
        rank[idx[:md[-1]]] = np.arange(min(len(idx), md[-1]))
    area = (db[:, 2].astype(np.float64) - db[:, 0]) * (db[:, 3].astype(np.float64) - db[:, 1])
    want_ig = np.zeros((K, 4), np.int64)
    for a, (lo, hi) in enumerate(AREAS):
        want_ig[:n, a] = np.where((area < lo) | (area > hi), (1 << 10) - 1, 0)
    want_ig[rank < 0] = 0
    m = DeviceMeanAveragePrecision()
    no_gt = torch.zeros((0, 6), dtype=torch.float32, device=DEV)
    for _ in range(8):
        m.update_batched(det, no_gt, S)
    for rec in m._dets:
        r = rec.cpu().numpy()
        assert np.array_equal(r[:, 2], rank) and not r[:, 3:7].any()
        assert np.array_equal(r[:, 7:11].view(np.uint32), want_ig)
    assert m.compute()["map"] == -1.0

    preds, targets = _random_set(7, n_img=12)
    parts = [slice(0, 5), slice(5, 8), slice(8, 12)]
    empty = [dict(boxes=np.zeros((0, 4), np.float32), labels=np.zeros(0, np.int64)) for _ in range(3)]
    m, loop_t = DeviceMeanAveragePrecision(class_metrics=True), []
    for i, sl in enumerate(parts):
        tg = empty if i == 1 else targets[sl]
        rows, back = _rows(tg, S)
        assert (rows.shape[0] == 0) == (i == 1)
        m.update_batched(_padded(preds[sl], 32), rows.to(DEV), S)
        loop_t += back
    _close(m.compute(), coco_loop(preds, loop_t, COCO, md, class_metrics=True))
    lst = DeviceMeanAveragePrecision(class_metrics=True)
    lst.update(_t(preds[:5]), _t(targets[:5]))
    lst.update(_t(preds[5:8]), _t(empty))
    lst.update(_t(preds[8:]), _t(targets[8:]))
    _close(lst.compute(), coco_loop(preds, targets[:5] + empty + targets[8:], COCO, md, class_metrics=True))


def test_update_batched_is_deterministic():
    res, gt_rows, S = _model_batch()
    gt = gt_rows.to(DEV)
    m = DeviceMeanAveragePrecision()
    m.update_batched(res, gt, S)
    m.update_batched(res, gt, S)
    assert torch.equal(m._dets[0], m._dets[1]) and torch.equal(m._gts[0], m._gts[1])


def test_gloo_world_size_2_device_map_sync(tmp_path):
    """Two ranks (fresh processes, one GPU) hold DIFFERENT images; compute() on each returns the value one process holding all
    images in rank order computes; the local records are untouched."""
    script = tmp_path / "w.py"
    script.write_text(
        "import sys, torch, torch.distributed as dist\n"
        f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.dirname(os.path.abspath(__file__))!r})\n"
        "from test_gpu_box_eval import _random_set, _t\n"
        "from multitask_bonetumor_yolo_amd.metrics import DeviceMeanAveragePrecision\n"
        "dist.init_process_group('gloo')\n"
        "r, w = dist.get_rank(), dist.get_world_size()\n"
        "def images(rank):\n"
        "    p, t = _random_set(20 + rank, n_img=6 + rank)\n"
        "    return _t(p), _t(t)\n"
        "m = DeviceMeanAveragePrecision(class_metrics=True); m.update(*images(r)); n_local = len(m._dets)\n"
        "got = m.compute()\n"
        "ref = DeviceMeanAveragePrecision(class_metrics=True, dist_sync=False)\n"
        "for k in range(w): ref.update(*images(k))\n"
        "want = ref.compute()\n"
        "assert got == want and len(m._dets) == n_local, (got, want)\n"
        "local = DeviceMeanAveragePrecision(class_metrics=True, dist_sync=False); local.update(*images(r))\n"
        "assert local.compute() != want\n"
        "print(f'RANK{r} ok {got[\"map\"]:.9f} {got[\"map_small\"]:.9f}', flush=True)\n"
        "dist.destroy_process_group()\n")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29563", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    rows = sorted(l.split() for o in outs for l in o.splitlines() if l.startswith("RANK"))
    assert len(rows) == 2 and rows[0][1:] == rows[1][1:]
