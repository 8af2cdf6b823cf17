"""Validation metric accumulators with the reference's definitions.

The reference trainer builds torchmetrics objects (`/root/reference/src/running_main_v3.py:198-217`) and feeds them in
`validation_step` (`:466-498` segmentation, `:535-575` boxes).  torchmetrics (and its pycocotools / faster-coco-eval
backend) is a third-party dependency that is absent here and unversioned in the reference: PARITY UNPINNED -- what is
restated is the published COCO evaluation (pycocotools `COCOeval.evaluateImg` / `accumulate` / `summarize`) and
torchmetrics' binary stat-score definitions.

  SegmentationMetrics     pixel counts on the device (`mtbt_seg_confusion`: one pass over logits + gt, no host sync in
                          `update`); F1 / precision / recall / accuracy / Dice / IoU and the single-instance mask mAP of
                          :480-497 from those counts in `compute`.
  MeanAveragePrecision    COCO box mAP over IoU thresholds with `max_detection_thresholds` (mAP@0.5 and @0.5:0.95 of :206-214):
                          host-side numpy matching -- at most 100 kept boxes per image after the device NMS, a few GT boxes.
  DeviceMeanAveragePrecision
                          torchmetrics' full bbox key set (the four COCO area ranges, per-class values with `class_metrics`): the
                          per-image matching on the device (`mtbt_box_eval`, straight from the NMS output and the collated GT rows,
                          no host sync per step).
  DeviceMaskMeanAveragePrecision
                          the same key set for INSTANCE MASKS (torchmetrics iou_type="segm"), from bit-packed masks: popcount tables
                          (`mtbt_mask_pair_counts`) and the same matching walk over them (`mtbt_mask_eval`), all on the device.
  ImageClassificationMetrics
                          image-class accuracy, normalised confusion matrix (:193-195, :458-459, :609-616) and the macro precision /
                          recall / F1 of evaluate_model.py:244-272 from a device-side confusion matrix (`mtbt_cls_confusion`).
  DetectionConfusionMatrix
                          the confusion matrix of the eval-mode loss's matched anchors (:218, :349-350, :710-722), counted on the
                          device by the loss's own decode and match (`mtbt_det_confusion`).

  SurfaceDistanceMetrics  boundary metrics of binary segmentation -- Hausdorff distance, HD95, average symmetric surface distance, normalised
                          surface Dice (MedPy's definitions; nothing in the reference computes them) -- from device-side records of
                          bit-packed masks (`mtbt_surface_distances`: edge sets, exact integer squared distances, order statistics).
  LesionMetrics           lesion-wise detection from the semantic mask -- ground-truth components found, predicted components that are
                          true, false-positive components per image (nothing in the reference computes them) -- from device-side
                          connected-component records of bit-packed masks (`mtbt_label_components`: areas and overlaps per component).

The two box classes and the segmentation mAP differ only in how they match; all three accumulate and summarise (pycocotools
`accumulate` / `summarize`) through one vectorised numpy function, `_accumulate`, once per epoch.

Data-parallel validation (configs[3]: one process per GPU, each rank sees its shard of the validation set): the reference's metric
objects are built with `dist_sync_on_step=True` (`running_main_v3.py:193-218`), i.e. torchmetrics gathers every rank's state before it
computes.  Here `compute()` does the same when a `torch.distributed` process group with more than one rank is alive (`dist_sync=True`,
the default): the per-image records (detections x ground-truth IoU matrices; pixel counts) of all ranks are all-gathered in rank order,
every rank computes the SAME global value, and the local state is left as it was (torchmetrics' sync / unsync around compute).
"""
import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .planes import filter_components, label_components, pack_masks, packed_planes, plane_pitch


def _world(group=None) -> int:
    import torch.distributed as dist
    return dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1


def _all_gather_records(local, group=None):
    """Every rank's list of per-image records, concatenated in rank order (a few KB per image: host objects; RCCL moves the pickled bytes
    through device tensors, gloo through the host).  All ranks must call it."""
    import torch.distributed as dist
    world = _world(group)
    if world == 1:
        return list(local)
    parts = [None] * world
    dist.all_gather_object(parts, list(local), group=group)
    return [rec for part in parts for rec in part]


def _sum_over_ranks(x: np.ndarray, group=None) -> np.ndarray:
    """`x` summed over the ranks of a live multi-rank process group, in rank order (a collective: all ranks must call it); without
    one, `x` itself."""
    return np.sum(_all_gather_records([x], group), axis=0) if _world(group) > 1 else x


COCO_IOU_THRESHOLDS = tuple(np.linspace(0.5, 0.95, 10))     # 0.50:0.05:0.95, the default of every mAP here (COCOeval.Params.iouThrs)


def _iou_limits(iou_thresholds) -> np.ndarray:
    """The IoU a match needs at each threshold: pycocotools evaluateImg caps the threshold just below 1."""
    return np.minimum(np.asarray(iou_thresholds, np.float64), 1 - 1e-10)


def box_iou_xyxy(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """COCO box IoU in float64 (pycocotools `bbIou` without crowd boxes): [D,4] x [G,4] -> [D,G]."""
    a, b = np.asarray(a, np.float64).reshape(-1, 4), np.asarray(b, np.float64).reshape(-1, 4)
    iw = np.clip(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0, None)
    inter = iw * ih
    union = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None] - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(union > 0, inter / union, 0.0)


class MeanAveragePrecision:
    """COCO mAP / mAR for one area range ("all"), up to 32 IoU thresholds, any max-detection thresholds.

    `update(preds, targets)` takes the torchmetrics layout the reference builds (`running_main_v3.py:553-575`): per image
    `dict(boxes [D,4] xyxy, scores [D], labels [D])` and `dict(boxes [G,4], labels [G])`."""

    def __init__(self, iou_thresholds: Optional[Sequence[float]] = None, max_detection_thresholds: Sequence[int] = (1, 10, 100),
                 dist_sync: bool = True, process_group=None):
        self.dist_sync, self.group = dist_sync, process_group
        self.iou_thresholds = np.asarray(iou_thresholds if iou_thresholds is not None else COCO_IOU_THRESHOLDS, np.float64)
        if self.iou_thresholds.size > 32:
            raise ValueError("MeanAveragePrecision: at most 32 IoU thresholds (one bit each in a match word)")
        self.max_dets = sorted(int(m) for m in max_detection_thresholds)
        self._images: List[tuple] = []

    def reset(self):
        self._images = []

    @staticmethod
    def _np(t, dtype):
        return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dtype)

    def update(self, preds: Sequence[Dict], targets: Sequence[Dict]):
        if len(preds) != len(targets):
            raise ValueError("MeanAveragePrecision.update: preds and targets differ in length")
        for p, t in zip(preds, targets):
            db, gb = self._np(p["boxes"], np.float64).reshape(-1, 4), self._np(t["boxes"], np.float64).reshape(-1, 4)
            self.add_image(self._np(p["scores"], np.float64), self._np(p["labels"], np.int64), self._np(t["labels"], np.int64), box_iou_xyxy(db, gb))

    def add_image(self, scores, labels, gt_labels, iou):
        """One image with a precomputed IoU matrix [D, G] (`update` computes it from the boxes)."""
        scores, labels, gt_labels = np.asarray(scores, np.float64).ravel(), np.asarray(labels, np.int64).ravel(), np.asarray(gt_labels, np.int64).ravel()
        iou = np.asarray(iou, np.float64).reshape(len(scores), len(gt_labels))
        self._images.append((scores, labels, gt_labels, iou))

    def _match(self, iou: np.ndarray) -> np.ndarray:
        """pycocotools evaluateImg without crowd / ignore flags: detections in score order, each takes the still unmatched GT
        of highest IoU >= threshold (of equal IoUs the later GT).  -> match words [D] uint32, bit t = matched at threshold t."""
        D, G = iou.shape
        word = np.zeros(D, np.uint32)
        if G == 0:
            return word
        for t, lim in enumerate(_iou_limits(self.iou_thresholds)):
            free = np.ones(G, bool)
            for d in range(D):
                v = np.where(free, iou[d], -1.0)
                m = G - 1 - int(np.argmax(v[::-1]))
                if v[m] >= lim:
                    free[m] = False
                    word[d] |= np.uint32(1 << t)
        return word

    def compute(self) -> Dict[str, float]:
        """With a live process group (and dist_sync): over the images of ALL ranks -- a collective, every rank must call it.

        The detections become `_accumulate` records of the area range "all" (no boxes reach `add_image`, so no other range is
        defined): rank = position in the stable score order of its (image, class), -1 past max_detection_thresholds[-1]; the match
        word of `_match` over those ranked detections (greedy in score order: every max-detection prefix matches as the whole list
        does); no ignore flags."""
        images = _all_gather_records(self._images, self.group) if self.dist_sync else self._images
        n = [len(im[0]) for im in images]
        cat = lambda k, dtype: np.concatenate([np.zeros(0, dtype)] + [im[k] for im in images])
        rank, match = np.full(sum(n), -1, np.int64), np.zeros((sum(n), len(AREA_RANGES)), np.uint32)
        for (scores, labels, gt_labels, iou), off in zip(images, np.cumsum([0] + n)):
            for c in np.unique(labels):
                di = np.nonzero(labels == c)[0]
                di = di[np.argsort(-scores[di], kind="mergesort")][: self.max_dets[-1]]
                rank[off + di] = np.arange(len(di))
                match[off + di, 0] = self._match(iou[np.ix_(di, np.nonzero(gt_labels == c)[0])])
        gt_label = cat(2, np.int64)
        rec = {"image": np.repeat(np.arange(len(images)), n), "rank": rank, "score": cat(0, np.float64), "label": cat(1, np.int64),
               "match": match, "ignore": np.zeros_like(match), "gt_label": gt_label, "gt_area": np.ones(len(gt_label), np.uint32)}
        out = _accumulate(rec, self.iou_thresholds, self.max_dets)
        return {k: out[k] for k in ("map", "map_50", "map_75", *(f"mar_{m}" for m in self.max_dets))}


AREA_RANGES = ("all", "small", "medium", "large")   # COCO: [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10], bounds inclusive
BOX_EVAL_CAP = 1024                                 # detections per image slot row (K) and GT boxes per image (csrc/box_eval.hip)


def _accumulate(records: Dict[str, np.ndarray], iou_thresholds: Sequence[float], max_dets: Sequence[int],
                class_metrics: bool = False) -> Dict[str, object]:
    """pycocotools `accumulate` + `summarize` over per-detection records, vectorised: the one implementation behind every mAP here
    (the records of the device matching `mtbt_box_eval`, of `MeanAveragePrecision._match` and of `_segm_map`).

    records: `image` [N] (update order), `rank` [N] (within (image, class); < 0 = not kept), `score` [N], `label` [N],
    `match` / `ignore` [N, 4] uint32 (word = area range, bit t = IoU threshold t), `gt_label` [G], `gt_area` [G] uint32
    (bit a = the GT box is not ignored in area range a)."""
    thr = np.asarray(iou_thresholds, np.float64)
    max_dets = sorted(int(m) for m in max_dets)
    T, A, Md = len(thr), len(AREA_RANGES), len(max_dets)
    rec_thr = np.linspace(0.0, 1.0, 101)
    R = len(rec_thr)
    rank = np.asarray(records["rank"], np.int64).ravel()
    ok = rank >= 0
    rank, image = rank[ok], np.asarray(records["image"], np.int64).ravel()[ok]
    score, label = np.asarray(records["score"], np.float64).ravel()[ok], np.asarray(records["label"], np.int64).ravel()[ok]
    match = np.asarray(records["match"], np.uint32).reshape(-1, A)[ok]
    ignore = np.asarray(records["ignore"], np.uint32).reshape(-1, A)[ok]
    gt_label, gt_area = np.asarray(records["gt_label"], np.int64).ravel(), np.asarray(records["gt_area"], np.uint32).ravel()
    classes = sorted(set(label.tolist()) | set(gt_label.tolist()))
    precision, recall = -np.ones((T, R, len(classes), A, Md)), -np.ones((T, len(classes), A, Md))
    bits = np.uint32(1) << np.arange(T, dtype=np.uint32)
    for k, c in enumerate(classes):
        sel = np.nonzero(label == c)[0]
        sel = sel[np.lexsort((rank[sel], image[sel]))]                      # images in update order, then score order within each
        g_area, r_sel, s_sel = gt_area[gt_label == c], rank[sel], score[sel]
        for a in range(A):
            npig = int(np.count_nonzero((g_area >> np.uint32(a)) & np.uint32(1)))
            if npig == 0:
                continue
            dtm = (match[sel, a][:, None] & bits) != 0                       # [n, T]
            dtig = (ignore[sel, a][:, None] & bits) != 0
            for m, maxdet in enumerate(max_dets):
                keep = np.nonzero(r_sel < maxdet)[0]
                keep = keep[np.argsort(-s_sel[keep], kind="mergesort")]
                tm, ti = dtm[keep].T, dtig[keep].T
                tps = np.cumsum(tm & ~ti, axis=1).astype(np.float64)
                fps = np.cumsum(~tm & ~ti, axis=1).astype(np.float64)
                nd = tps.shape[1]
                rc = tps / npig
                pr = tps / (fps + tps + np.spacing(1))
                recall[:, k, a, m] = rc[:, -1] if nd else 0.0
                pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]          # precision envelope
                for t in range(T):
                    inds = np.searchsorted(rc[t], rec_thr, side="left")
                    q = np.zeros(R)
                    hit = inds < nd
                    q[hit] = pr[t, inds[hit]]
                    precision[t, :, k, a, m] = q

    def mean(v):
        v = v[v > -1]
        return float(v.mean()) if v.size else -1.0

    out = {"map": mean(precision[:, :, :, 0, -1])}
    for name, t in (("map_50", 0.5), ("map_75", 0.75)):
        hit = np.nonzero(np.isclose(thr, t))[0]
        out[name] = mean(precision[hit[0], :, :, 0, -1]) if len(hit) else -1.0
    for a, name in enumerate(AREA_RANGES[1:], 1):
        out[f"map_{name}"] = mean(precision[:, :, :, a, -1])
    for m, maxdet in enumerate(max_dets):
        out[f"mar_{maxdet}"] = mean(recall[:, :, 0, m])
    for a, name in enumerate(AREA_RANGES[1:], 1):
        out[f"mar_{name}"] = mean(recall[:, :, a, -1])
    if class_metrics:
        out["classes"] = list(classes)
        out["map_per_class"] = [mean(precision[:, :, k, 0, -1]) for k in range(len(classes))]
        out[f"mar_{max_dets[-1]}_per_class"] = [mean(recall[:, k, 0, -1]) for k in range(len(classes))]
    return out


def _upload(parts: Sequence[np.ndarray], dev) -> List[torch.Tensor]:
    """Host arrays -> device tensors through ONE buffer of 16-byte aligned pieces: one host-to-device copy."""
    offs, off = [], 0
    for x in parts:
        offs.append(off)
        off += -(-x.nbytes // 16) * 16
    buf = np.zeros(max(off, 16), np.uint8)
    for x, o in zip(parts, offs):
        buf[o:o + x.nbytes] = np.ascontiguousarray(x).view(np.uint8).ravel()
    dbuf = torch.from_numpy(buf).to(dev)
    return [dbuf[o:o + x.nbytes].view(getattr(torch, x.dtype.name)).reshape(x.shape) for x, o in zip(parts, offs)]


class _DeviceCocoRecords:
    """What the device mAP classes share: the constructor's checks, the per-update device records a matching kernel (`mtbt_box_eval`,
    `mtbt_mask_eval`) writes, their one copy to the host, the cross-rank gather and the accumulation through `_accumulate`."""
    _what = "GT boxes"

    def __init__(self, iou_thresholds, max_detection_thresholds, class_metrics, dist_sync, process_group):
        name = type(self).__name__
        self.iou_thresholds = np.asarray(iou_thresholds if iou_thresholds is not None else COCO_IOU_THRESHOLDS, np.float64).ravel()
        if not 1 <= len(self.iou_thresholds) <= 32:
            raise ValueError(f"{name}: between 1 and 32 IoU thresholds")
        self.max_dets = sorted(int(m) for m in max_detection_thresholds)
        if not self.max_dets or self.max_dets[0] < 1:
            raise ValueError(f"{name}: max_detection_thresholds must be positive")
        self.class_metrics, self.dist_sync, self.group = bool(class_metrics), dist_sync, process_group
        self.reset()

    def reset(self):
        self._dets: List[torch.Tensor] = []     # per update: [B*K, 11] int32 = score bits, label, rank, match[4], ignore[4]
        self._gts: List[torch.Tensor] = []      # per update: [M, 3] int32 = image, class (as `_gt_fields` reads them), area-range set
        self._shapes: List[tuple] = []          # per update: (B, K, M)
        self._status: Optional[torch.Tensor] = None

    def _status_on(self, dev) -> torch.Tensor:
        if self._status is None:
            self._status = torch.zeros(4, dtype=torch.int32, device=dev)
        elif self._status.device != dev:
            raise ValueError(f"{type(self).__name__}: this metric keeps its records on {self._status.device}, the batch is on {dev}")
        return self._status

    def _keep(self, scores, labels, rank, mi, gt_cols, gt_area):
        """One update's records, kept on the device: scores [B,K] f32, labels [B,K], rank [B,K] i32, mi [2,B,K,4] (match, ignore),
        gt_cols [M,2] int32 (image, class), gt_area [M] int32."""
        B, K = scores.shape
        self._dets.append(torch.cat([scores.reshape(-1, 1).view(torch.int32), labels.reshape(-1, 1).to(torch.int32), rank.reshape(-1, 1),
                                     mi[0].reshape(-1, 4), mi[1].reshape(-1, 4)], 1))
        self._gts.append(torch.cat([gt_cols, gt_area.reshape(-1, 1)], 1))
        self._shapes.append((B, K, gt_cols.shape[0]))

    def _records(self):
        """-> (records dict over this process's images, number of images, status word) on the host."""
        if self._dets:
            dets = torch.cat(self._dets).cpu().numpy()
            gts = torch.cat(self._gts).cpu().numpy()
            status = int(self._status.cpu().numpy().max())
        else:
            dets, gts, status = np.zeros((0, 11), np.int32), np.zeros((0, 3), np.int32), 0
        image, gt_keep, gt_label, n_img = [], [], [], 0
        for B, K, M in self._shapes:
            image.append(np.repeat(np.arange(n_img, n_img + B), K))
            n_img += B
        for (B, K, M), lo in zip(self._shapes, np.cumsum([0] + [s[2] for s in self._shapes])):
            keep_u, label_u = self._gt_fields(gts[lo:lo + M], B)                   # rows of an image of their batch, their classes
            gt_keep.append(keep_u)
            gt_label.append(label_u)
        keep = np.concatenate(gt_keep) if gt_keep else np.zeros(0, bool)
        rec = {"image": np.concatenate(image) if image else np.zeros(0, np.int64), "score": dets[:, 0].view(np.float32).astype(np.float64),
               "label": dets[:, 1].astype(np.int64), "rank": dets[:, 2], "match": dets[:, 3:7].view(np.uint32),
               "ignore": dets[:, 7:11].view(np.uint32),
               "gt_label": (np.concatenate(gt_label) if gt_label else np.zeros(0, np.int64))[keep], "gt_area": gts[keep, 2].view(np.uint32)}
        kept = rec["rank"] >= 0
        for k in ("image", "score", "label", "rank", "match", "ignore"):
            rec[k] = rec[k][kept]
        return rec, n_img, status

    def compute(self) -> Dict[str, object]:
        """With a live process group (and dist_sync): over the images of ALL ranks -- a collective, every rank must call it."""
        rec, n_img, status = self._records()
        if self.dist_sync and _world(self.group) > 1:
            parts = _all_gather_records([(rec, n_img, status)], self.group)
            off, image = 0, []
            for r, n, _ in parts:
                image.append(r["image"] + off)
                off += n
            rec = {k: np.concatenate([p[0][k] for p in parts]) for k in rec}
            rec["image"] = np.concatenate(image)
            status = max(p[2] for p in parts)
        if status:
            raise RuntimeError(f"{type(self).__name__}.compute: an image holds more than {BOX_EVAL_CAP} {self._what} (the matching kernel's cap)")
        return _accumulate(rec, self.iou_thresholds, self.max_dets, self.class_metrics)

    @staticmethod
    def _gt_fields(gts: np.ndarray, B: int):
        """-> (rows of an image of their batch [M] bool, class [M] int64) from the first two int32 columns of one update's GT records."""
        raise NotImplementedError


class DeviceMeanAveragePrecision(_DeviceCocoRecords):
    """COCO box mAP / mAR with torchmetrics' bbox key set -- the four area ranges and, with `class_metrics`, per-class values --
    with the per-image matching on the device (`mtbt_box_eval`) and the once-per-epoch accumulation in vectorised numpy.

    `update_batched(det, gt_rows, img_size)`: `det` = the dict `postprocess.detect_and_segment` / `nms_batched` returns (boxes
    [B,K,4] xyxy, scores [B,K], labels [B,K], counts [B]), `gt_rows` = the collated [M,6] rows (batch_idx, cls, cx, cy, w, h)
    normalised (`preprocess.collate_boxes`), both on the device.  One launch, no host synchronisation.
    `update(preds, targets)`: the torchmetrics list-of-dicts layout the reference builds (running_main_v3.py:554-570), one
    host-to-device copy per call.  `compute()` copies the records to the host once; with a live process group (and
    `dist_sync`) it gathers every rank's records in rank order first (a collective: every rank must call it).
    Instance masks (`iou_type="segm"`) are `DeviceMaskMeanAveragePrecision`."""

    def __init__(self, iou_thresholds: Optional[Sequence[float]] = None, max_detection_thresholds: Sequence[int] = (1, 10, 100),
                 class_metrics: bool = False, dist_sync: bool = True, process_group=None, box_format: str = "xyxy", iou_type: str = "bbox"):
        if box_format != "xyxy":
            raise ValueError(f"DeviceMeanAveragePrecision: box_format {box_format!r} is not supported (only 'xyxy')")
        if iou_type != "bbox":
            raise ValueError(f"DeviceMeanAveragePrecision: iou_type {iou_type!r} is not supported (only 'bbox'; instance masks are "
                             "DeviceMaskMeanAveragePrecision)")
        super().__init__(iou_thresholds, max_detection_thresholds, class_metrics, dist_sync, process_group)

    @staticmethod
    def _gt_fields(gts, B):
        bidx = gts[:, 0].view(np.float32)                                        # the collated rows' (batch_idx, cls) float bits
        return (bidx >= 0) & (bidx < B) & (bidx == np.trunc(bidx)), np.trunc(gts[:, 1].view(np.float32)).astype(np.int64)

    def _launch(self, boxes, scores, labels, counts, gt, gt_format: int, img_size: float):
        lib = L.load()
        dev = boxes.device
        B, K = scores.shape
        M = gt.shape[0]
        if K > BOX_EVAL_CAP:
            raise ValueError(f"DeviceMeanAveragePrecision: {K} detection slots per image, at most {BOX_EVAL_CAP}")
        status = self._status_on(dev)
        rank = torch.empty((B, K), dtype=torch.int32, device=dev)
        mi = torch.empty((2, B, K, 4), dtype=torch.int32, device=dev)          # match, ignore (uint32 bit sets)
        gt_area = torch.empty((M,), dtype=torch.int32, device=dev)
        a = L.BoxEvalArgs()
        a.boxes, a.scores, a.labels = boxes.data_ptr(), scores.data_ptr(), labels.data_ptr()
        a.counts = counts.data_ptr() if counts is not None else None
        a.gt, a.gt_area = (gt.data_ptr(), gt_area.data_ptr()) if M else (None, None)
        a.rank, a.match, a.ignore, a.status = rank.data_ptr(), mi[0].data_ptr(), mi[1].data_ptr(), status.data_ptr()
        for t, v in enumerate(self.iou_thresholds):
            a.iou_thresholds[t] = float(v)
        a.B, a.K, a.M, a.T, a.max_det, a.gt_format, a.img_size = B, K, M, len(self.iou_thresholds), self.max_dets[-1], gt_format, float(img_size)
        with torch.cuda.device(dev):                                            # launch on the tensors' device, whatever is current
            L.check(lib.mtbt_box_eval(C.byref(a), L.stream(dev)), "mtbt_box_eval")
        self._keep(scores, labels, rank, mi, gt[:, :2].view(torch.int32), gt_area)

    def update_batched(self, det: Dict[str, torch.Tensor], gt_rows: torch.Tensor, img_size: float):
        """Asynchronous: launches on the current stream, keeps its records on the device, never synchronises with the host."""
        boxes, scores, labels, counts = det["boxes"], det["scores"], det["labels"], det.get("counts")
        if not all(t.is_cuda for t in (boxes, scores, labels, gt_rows)) or (counts is not None and not counts.is_cuda):
            raise RuntimeError("DeviceMeanAveragePrecision.update_batched: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        devs = {t.device for t in (boxes, scores, labels, gt_rows) + ((counts,) if counts is not None else ())}
        if len(devs) != 1:
            raise ValueError(f"DeviceMeanAveragePrecision.update_batched: detections and GT rows on different devices {sorted(map(str, devs))}")
        if boxes.dim() != 3 or boxes.shape[2] != 4 or scores.shape != boxes.shape[:2] or labels.shape != scores.shape:
            raise ValueError("DeviceMeanAveragePrecision.update_batched: boxes [B,K,4], scores [B,K], labels [B,K]")
        if gt_rows.dim() != 2 or gt_rows.shape[1] != 6:
            raise ValueError("DeviceMeanAveragePrecision.update_batched: gt_rows must be [M, 6] (batch_idx, cls, cx, cy, w, h)")
        if boxes.shape[0] == 0:
            return
        boxes = boxes.to(torch.float32).contiguous()
        if boxes.data_ptr() % 16:
            boxes = boxes.clone()
        counts = counts.to(torch.int32).contiguous() if counts is not None else None
        self._launch(boxes, scores.to(torch.float32).contiguous(), labels.to(torch.int64).contiguous(), counts,
                     gt_rows.to(torch.float32).contiguous(), 0, img_size)

    def update(self, preds: Sequence[Dict], targets: Sequence[Dict]):
        """torchmetrics layout: per image dict(boxes [D,4] xyxy, scores [D], labels [D]) and dict(boxes [G,4] xyxy pixels, labels [G])."""
        if len(preds) != len(targets):
            raise ValueError("DeviceMeanAveragePrecision.update: preds and targets differ in length")
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceMeanAveragePrecision.update: needs the MI355X (no CPU path)")
        if not preds:
            return
        np_ = MeanAveragePrecision._np
        B = len(preds)
        db = [np_(p["boxes"], np.float32).reshape(-1, 4) for p in preds]
        K = max(1, max(len(d) for d in db))
        if K > BOX_EVAL_CAP:
            raise ValueError(f"DeviceMeanAveragePrecision.update: {K} detections in one image, at most {BOX_EVAL_CAP}")
        boxes, scores = np.zeros((B, K, 4), np.float32), np.zeros((B, K), np.float32)
        labels, counts = np.zeros((B, K), np.int64), np.zeros(B, np.int32)
        rows = []
        for b, (p, t) in enumerate(zip(preds, targets)):
            n = len(db[b])
            boxes[b, :n], scores[b, :n], labels[b, :n], counts[b] = db[b], np_(p["scores"], np.float32).ravel(), np_(p["labels"], np.int64).ravel(), n
            gb, gl = np_(t["boxes"], np.float32).reshape(-1, 4), np_(t["labels"], np.float32).ravel()
            rows.append(np.concatenate([np.full((len(gb), 1), b, np.float32), gl[:, None], gb], 1))
        gt = np.concatenate(rows).astype(np.float32)
        views = _upload([boxes, scores, labels, counts, gt], self._status.device if self._status is not None else torch.device("cuda", torch.cuda.current_device()))
        self._launch(views[0], views[1], views[2], views[3], views[4], 1, 0.0)


MASK_EVAL_MAX_IMAGES = 32    # images per mtbt_mask_pair_counts launch (the image descriptors travel as kernel arguments)


def _mask_launch_layout(n_gt: Sequence[int], chunk: int = MASK_EVAL_MAX_IMAGES):
    """A list of images with n_gt[b] ground-truth planes each -> the launches of `mtbt_mask_pair_counts`, `chunk` images at a time:
    [(first image, one past the last image, g0 per image, gt_image int32 [M])].  The GT planes of a launch form one flat row list in
    image order; g0[i] is the flat row of image i's first plane (its own GT tensor is addressed from there) and gt_image[m] the image
    OF THE LAUNCH that row m belongs to."""
    out = []
    for c0 in range(0, len(n_gt), chunk):
        g = [int(v) for v in n_gt[c0:c0 + chunk]]
        if any(v < 0 for v in g):
            raise ValueError("_mask_launch_layout: a negative plane count")
        g0 = np.cumsum([0] + g)[:-1].astype(np.int64).tolist()
        out.append((c0, c0 + len(g), g0, np.repeat(np.arange(len(g), dtype=np.int32), g)))
    return out


def _pair_counts(images, K: int, counts, gt_image, M: int, dev, out=None):
    """One `mtbt_mask_pair_counts` launch.  images: [(H, W, det tensor, gt tensor, g0, gt_planes)], at most 32; counts int32 [B] or
    None; gt_image int32 [M] on the device.  -> (inter [M,K], det_area [B,K], gt_px [M]) int32 tensors holding the uint32 counts;
    `out=` takes the caller's three contiguous tensors of those shapes instead (every word is defined afterwards, whatever they held)."""
    lib = L.load()
    B = len(images)
    if out is None:
        out = (torch.empty((M, K), dtype=torch.int32, device=dev), torch.empty((B, K), dtype=torch.int32, device=dev),
               torch.empty((M,), dtype=torch.int32, device=dev))
    inter, det_area, gt_px = out
    for t, shape in zip(out, ((M, K), (B, K), (M,))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"_pair_counts: out must be contiguous int32 tensors [{M},{K}], [{B},{K}], [{M}] on the device")
    a = L.MaskPairArgs()
    a.counts = counts.data_ptr() if counts is not None else None
    a.gt_image, a.gt_area, a.inter = (gt_image.data_ptr(), gt_px.data_ptr(), inter.data_ptr()) if M else (None, None, None)
    a.det_area = det_area.data_ptr()
    a.B, a.K, a.M = B, K, M
    im = (L.MaskImage * B)()
    for i, (H, W, det, gt, g0, planes) in enumerate(images):
        im[i].det, im[i].gt_base = det.data_ptr(), gt.data_ptr()
        im[i].H, im[i].W, im[i].pitch, im[i].g0, im[i].gt_planes = H, W, plane_pitch(W), g0, planes
    with torch.cuda.device(dev):
        L.check(lib.mtbt_mask_pair_counts(C.byref(a), im, B, L.stream(dev)), "mtbt_mask_pair_counts")
    return inter, det_area, gt_px


class DeviceMaskMeanAveragePrecision(_DeviceCocoRecords):
    """COCO instance-mask mAP / mAR (torchmetrics `MeanAveragePrecision(iou_type="segm")`, no crowd annotations) with the key set of
    `DeviceMeanAveragePrecision`, from BIT-PACKED masks (`postprocess.masks_to_frames` / `pack_masks`: pitch = 8 * ceil(W / 64) bytes per
    row, pixel X = bit X & 7 of byte X >> 3) and entirely on the device: popcount tables of every (GT, detection) pair of an image
    (`mtbt_mask_pair_counts`), then pycocotools' matching walk with IoU = inter / (det + gt - inter) in fp64 from those exact integers
    (`mtbt_mask_eval`; 0 when the union is empty; areas are pixel counts).  Accumulated once per epoch like the box class.

    `update(preds, targets)`: torchmetrics' segm layout, per image dict(masks bool [D,H,W], scores [D], labels [D]) and
    dict(masks bool [G,H,W], labels [G]) on the device; a dict may instead hold packed uint8 masks [., H, pitch] with `"width": W`.
    Images keep their own sizes.  One host-to-device copy per 32 images.
    `update_batched(det, gt_masks, gt_labels)`: `det` = the dict `postprocess.detect_and_segment(..., frames=...)` returns
    (masks_frame, scores, labels, counts); gt_masks = a list of packed [G_b, H0_b, pitch_b]; gt_labels = a list of int tensors.
    `update_uniform(det_packed [B,K,S,pitch], scores, labels, counts, gt_packed [M,S,pitch], gt_rows [M,6])`: letterboxed batches;
    image and class of a GT plane come from the device-resident collated rows by `mtbt_box_eval`'s rule.  No host synchronisation,
    no host copy."""
    _what = "GT masks"

    def __init__(self, iou_thresholds: Optional[Sequence[float]] = None, max_detection_thresholds: Sequence[int] = (1, 10, 100),
                 class_metrics: bool = False, dist_sync: bool = True, process_group=None):
        super().__init__(iou_thresholds, max_detection_thresholds, class_metrics, dist_sync, process_group)

    @staticmethod
    def _gt_fields(gts, B):
        return (gts[:, 0] >= 0) & (gts[:, 0] < B), gts[:, 1].astype(np.int64)

    def _evaluate(self, tables, scores, labels, counts, gt_image, gt_label):
        """`mtbt_mask_eval` over the pair-count tables of B images, then the records are kept.  All device tensors."""
        lib = L.load()
        inter, det_area, gt_px = tables
        dev = scores.device
        B, K = scores.shape
        M = gt_image.shape[0]
        status = self._status_on(dev)
        rank = torch.empty((B, K), dtype=torch.int32, device=dev)
        mi = torch.empty((2, B, K, 4), dtype=torch.int32, device=dev)          # match, ignore (uint32 bit sets)
        gt_area = torch.empty((M,), dtype=torch.int32, device=dev)
        a = L.MaskEvalArgs()
        a.det_area, a.scores, a.labels = det_area.data_ptr(), scores.data_ptr(), labels.data_ptr()
        a.counts = counts.data_ptr() if counts is not None else None
        if M:
            a.inter, a.gt_px, a.gt_image, a.gt_label, a.gt_area = (t.data_ptr() for t in (inter, gt_px, gt_image, gt_label, gt_area))
        a.rank, a.match, a.ignore, a.status = rank.data_ptr(), mi[0].data_ptr(), mi[1].data_ptr(), status.data_ptr()
        for t, v in enumerate(self.iou_thresholds):
            a.iou_thresholds[t] = float(v)
        a.B, a.K, a.M, a.T, a.max_det = B, K, M, len(self.iou_thresholds), self.max_dets[-1]
        with torch.cuda.device(dev):
            L.check(lib.mtbt_mask_eval(C.byref(a), L.stream(dev)), "mtbt_mask_eval")
        self._keep(scores, labels, rank, mi, torch.stack([gt_image, gt_label], 1), gt_area)

    # ---- images with their own sizes -------------------------------------------------------------------------------------------
    @staticmethod
    def _packed_of(d: Dict, who: str):
        """-> (packed uint8 [n, H, pitch] on the device, H, W) of one image's dict."""
        m = d["masks"]
        if not isinstance(m, torch.Tensor) or not m.is_cuda or m.dim() != 3:
            raise RuntimeError(f"DeviceMaskMeanAveragePrecision.{who}: masks must be [n, H, W] CUDA/HIP tensors on an MI355X (no CPU path)")
        if "width" in d:
            W = int(d["width"])
            if m.dtype != torch.uint8 or m.shape[2] != plane_pitch(W):
                raise ValueError(f"DeviceMaskMeanAveragePrecision.{who}: packed masks of width {W} are uint8 [n, H, {plane_pitch(W)}]")
            m = m.contiguous()
            return (m if m.data_ptr() % 8 == 0 else m.clone()), int(m.shape[1]), W
        return pack_masks(m), int(m.shape[1]), int(m.shape[2])

    def _update_list(self, det_planes, sizes, n_det, scores, labels, gt_planes, gt_labels, dev):
        """det_planes / gt_planes: per image packed [>= n_det[b], H, pitch] / [G_b, H, pitch]; sizes (H, W); scores / labels: host arrays
        per image; gt_labels: host int arrays per image."""
        K = max(1, max(n_det))
        if K > BOX_EVAL_CAP:
            raise ValueError(f"DeviceMaskMeanAveragePrecision: {K} detections in one image, at most {BOX_EVAL_CAP}")
        for c0, c1, g0, gi in _mask_launch_layout([int(g.shape[0]) for g in gt_planes]):
            nb = c1 - c0
            sc, lb, cn = np.zeros((nb, K), np.float32), np.zeros((nb, K), np.int64), np.zeros(nb, np.int32)
            for i in range(nb):
                n = n_det[c0 + i]
                sc[i, :n], lb[i, :n], cn[i] = scores[c0 + i][:n], labels[c0 + i][:n], n
            gl = np.concatenate([np.zeros(0, np.int32)] + [np.asarray(g, np.int32).ravel() for g in gt_labels[c0:c1]])
            if len(gl) != len(gi):
                raise ValueError("DeviceMaskMeanAveragePrecision: one label per GT mask")
            d_sc, d_lb, d_cn, d_gi, d_gl = _upload([sc, lb, cn, gi, gl], dev)
            images = []
            for i in range(nb):
                H, W = sizes[c0 + i]
                det, gt = det_planes[c0 + i], gt_planes[c0 + i]
                images.append((H, W, det if det.numel() else d_sc, gt if gt.numel() else d_sc, g0[i], int(gt.shape[0])))
            tables = _pair_counts(images, K, d_cn, d_gi, len(gi), dev)
            self._evaluate(tables, d_sc, d_lb, d_cn, d_gi, d_gl)

    def update(self, preds: Sequence[Dict], targets: Sequence[Dict]):
        if len(preds) != len(targets):
            raise ValueError("DeviceMaskMeanAveragePrecision.update: preds and targets differ in length")
        if not preds:
            return
        np_ = MeanAveragePrecision._np
        det, gt, sizes = [], [], []
        for p, t in zip(preds, targets):
            dp, H, W = self._packed_of(p, "update")
            gp, Hg, Wg = self._packed_of(t, "update")
            if (H, W) != (Hg, Wg):
                raise ValueError(f"DeviceMaskMeanAveragePrecision.update: predicted masks are {H} x {W}, the image's GT masks {Hg} x {Wg}")
            det.append(dp)
            gt.append(gp)
            sizes.append((H, W))
        dev = det[0].device
        if any(t.device != dev for t in det + gt):
            raise ValueError("DeviceMaskMeanAveragePrecision.update: masks on different devices")
        scores, labels = [np_(p["scores"], np.float32).ravel() for p in preds], [np_(p["labels"], np.int64).ravel() for p in preds]
        n_det = [int(d.shape[0]) for d in det]
        if any(len(s) != n or len(l) != n for s, l, n in zip(scores, labels, n_det)):
            raise ValueError("DeviceMaskMeanAveragePrecision.update: one score and one label per predicted mask")
        self._update_list(det, sizes, n_det, scores, labels, gt, [np_(t["labels"], np.int32).ravel() for t in targets], dev)

    def update_batched(self, det: Dict, gt_masks: Sequence[torch.Tensor], gt_labels: Sequence[torch.Tensor]):
        """`det["masks_frame"]`: packed [K, H0_b, pitch_b] per image (only the first counts[b] planes are read).  The scores, labels and
        counts stay on the device; only the GT plane layout (a few integers per image) is uploaded."""
        planes, scores, labels, counts = det["masks_frame"], det["scores"], det["labels"], det.get("counts")
        B = len(planes)
        if len(gt_masks) != B or len(gt_labels) != B or scores.shape[0] != B:
            raise ValueError("DeviceMaskMeanAveragePrecision.update_batched: one GT mask stack and one label tensor per image")
        if not all(t.is_cuda for t in list(planes) + list(gt_masks) + [scores, labels]):
            raise RuntimeError("DeviceMaskMeanAveragePrecision.update_batched: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        if B == 0:
            return
        dev = scores.device
        K = scores.shape[1]
        if K > BOX_EVAL_CAP:
            raise ValueError(f"DeviceMaskMeanAveragePrecision.update_batched: {K} detection slots per image, at most {BOX_EVAL_CAP}")
        for d, g in zip(planes, gt_masks):
            if d.dtype != torch.uint8 or g.dtype != torch.uint8 or d.dim() != 3 or g.dim() != 3 or d.shape[0] != K or d.shape[1:] != g.shape[1:]:
                raise ValueError("DeviceMaskMeanAveragePrecision.update_batched: per image packed uint8 [K, H0, pitch] detections and "
                                 "[G, H0, pitch] GT planes of the same size")
        scores, labels = scores.to(torch.float32).contiguous(), labels.to(torch.int64).contiguous()
        counts = counts.to(torch.int32).contiguous() if counts is not None else None
        gl = torch.cat([torch.zeros(0, dtype=torch.int32, device=dev)] + [l.reshape(-1).to(device=dev, dtype=torch.int32) for l in gt_labels])
        if gl.numel() != sum(int(g.shape[0]) for g in gt_masks):
            raise ValueError("DeviceMaskMeanAveragePrecision.update_batched: one label per GT mask")
        m0 = 0
        for c0, c1, g0, gi in _mask_launch_layout([int(g.shape[0]) for g in gt_masks]):
            d_gi, = _upload([gi], dev)
            images = []
            for i, b in enumerate(range(c0, c1)):
                d, g = planes[b].contiguous(), gt_masks[b].contiguous()
                # the width is not needed beyond the pitch: the padding bits of both sides are zero
                images.append((int(d.shape[1]), int(d.shape[2]) * 8, d, g if g.numel() else d, g0[i], int(g.shape[0])))
            cn = counts[c0:c1] if counts is not None else None
            tables = _pair_counts(images, K, cn, d_gi, len(gi), dev)
            self._evaluate(tables, scores[c0:c1], labels[c0:c1], cn, d_gi, gl[m0:m0 + len(gi)])
            m0 += len(gi)

    # ---- letterboxed batches: everything stays on the device -------------------------------------------------------------------
    @staticmethod
    def gt_rows_fields(gt_rows: torch.Tensor, B: int):
        """The collated [M,6] rows -> (image int32 [M], -1 for a row of no image of the batch; class int32 [M]) by `mtbt_box_eval`'s rule
        (batch_idx an integer in [0, B); the class truncated), on the device."""
        bi = gt_rows[:, 0].to(torch.float32)
        ok = (bi >= 0) & (bi < B) & (bi == bi.trunc())
        return torch.where(ok, bi, torch.full_like(bi, -1.0)).to(torch.int32), gt_rows[:, 1].to(torch.float32).to(torch.int64).to(torch.int32)

    @staticmethod
    def pair_tables_uniform(det_packed: torch.Tensor, counts: Optional[torch.Tensor], gt_packed: torch.Tensor, gt_image: torch.Tensor):
        """The pixel-count tables of a uniform batch (all images S x pitch): (inter [M,K], det_area [B,K], gt_px [M]).  They do not depend
        on the IoU thresholds: several metric objects may share them (`update_uniform(..., tables=)`)."""
        B, K, S, pitch = det_packed.shape
        M = gt_packed.shape[0]
        dev = det_packed.device
        counts = counts.to(torch.int32).contiguous() if counts is not None else None
        parts = []
        for c0 in range(0, B, MASK_EVAL_MAX_IMAGES):
            nb = min(MASK_EVAL_MAX_IMAGES, B - c0)
            gi = gt_image if B <= MASK_EVAL_MAX_IMAGES else torch.where((gt_image >= c0) & (gt_image < c0 + nb), gt_image - c0, torch.full_like(gt_image, -1))
            images = [(S, pitch * 8, det_packed[b], gt_packed if M else det_packed, 0, M) for b in range(c0, c0 + nb)]
            parts.append(_pair_counts(images, K, counts[c0:] if counts is not None else None, gi, M, dev))
        if len(parts) == 1:
            return parts[0]
        # a GT row is counted by the launch that holds its image and is zero in every other one
        return sum(p[0] for p in parts), torch.cat([p[1] for p in parts]), sum(p[2] for p in parts)

    def update_uniform(self, det_packed: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, counts: Optional[torch.Tensor],
                       gt_packed: torch.Tensor, gt_rows: torch.Tensor, tables=None):
        """Asynchronous: launches on the current stream, keeps its records on the device, never synchronises with the host."""
        ts = (det_packed, scores, labels, gt_packed, gt_rows) + ((counts,) if counts is not None else ())
        if not all(t.is_cuda for t in ts):
            raise RuntimeError("DeviceMaskMeanAveragePrecision.update_uniform: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        if len({t.device for t in ts}) != 1:
            raise ValueError("DeviceMaskMeanAveragePrecision.update_uniform: tensors on different devices")
        if det_packed.dim() != 4 or det_packed.dtype != torch.uint8 or scores.shape != det_packed.shape[:2] or labels.shape != scores.shape:
            raise ValueError("DeviceMaskMeanAveragePrecision.update_uniform: det_packed uint8 [B,K,S,pitch], scores [B,K], labels [B,K]")
        if gt_packed.dim() != 3 or gt_packed.dtype != torch.uint8 or gt_packed.shape[1:] != det_packed.shape[2:] or det_packed.shape[3] % 8:
            raise ValueError("DeviceMaskMeanAveragePrecision.update_uniform: gt_packed uint8 [M,S,pitch] of the detections' plane size")
        if gt_rows.dim() != 2 or gt_rows.shape[1] != 6 or gt_rows.shape[0] != gt_packed.shape[0]:
            raise ValueError("DeviceMaskMeanAveragePrecision.update_uniform: gt_rows must be [M, 6] (batch_idx, cls, ...), one row per GT plane")
        B, K = scores.shape
        if B == 0:
            return
        if K > BOX_EVAL_CAP:
            raise ValueError(f"DeviceMaskMeanAveragePrecision.update_uniform: {K} detection slots per image, at most {BOX_EVAL_CAP}")
        counts = counts.to(torch.int32).contiguous() if counts is not None else None
        gt_image, gt_label = self.gt_rows_fields(gt_rows, B)
        if tables is None:
            tables = self.pair_tables_uniform(det_packed.contiguous(), counts, gt_packed.contiguous(), gt_image)
        self._evaluate(tables, scores.to(torch.float32).contiguous(), labels.to(torch.int64).contiguous(), counts, gt_image, gt_label)


class SegmentationMetrics:
    """Binary segmentation metrics of `validation_step` (`running_main_v3.py:466-498`) from device-side pixel counts."""

    def __init__(self, dist_sync: bool = True, process_group=None):
        self.dist_sync, self.group = dist_sync, process_group
        self._counts: List[torch.Tensor] = []
        self._psum: List[torch.Tensor] = []

    def reset(self):
        self._counts, self._psum = [], []

    def update(self, seg_logits: torch.Tensor, masks_gt: torch.Tensor):
        """seg_logits, masks_gt: [B,1,S,S] (or [B,S,S]) fp32 CUDA tensors.  Asynchronous: no host synchronisation."""
        if not (seg_logits.is_cuda and masks_gt.is_cuda):
            raise RuntimeError("SegmentationMetrics.update: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        if seg_logits.shape != masks_gt.shape:
            raise ValueError("SegmentationMetrics.update: logits and masks differ in shape")
        lib = L.load()
        x, t = seg_logits.float().contiguous(), masks_gt.float().contiguous()
        B, n = x.shape[0], x[0].numel()
        dev = x.device
        counts = torch.empty(B, 4, dtype=torch.int64, device=dev)
        psum = torch.empty(B, dtype=torch.float32, device=dev)
        ws, ws_bytes = L.workspace(lib.mtbt_seg_confusion_workspace_bytes, B, device=dev, what="mtbt_seg_confusion_workspace_bytes")
        L.check(lib.mtbt_seg_confusion(x.data_ptr(), t.data_ptr(), B, n, counts.data_ptr(), psum.data_ptr(), ws.data_ptr(), ws_bytes,
                                       L.stream(dev)), "mtbt_seg_confusion")
        self._counts.append(counts)
        self._psum.append(psum)

    def update_packed(self, pred_packed, gt_packed, W0):
        """The same counts from BIT-PACKED planes in the image frame (`postprocess.seg_to_frames`' "masks", `detect_sliced`'s
        `seg_frame`; ground truth from `pack_masks` / `fill_polygons`): TP / FP / FN / TN per image from popcounts
        (`mtbt_mask_pair_counts` with one plane per image).  pred_packed, gt_packed: uint8 [B, H, pitch] (or [B, 1, H, pitch], or
        [H, pitch]) tensors with one `W0`, or lists of per-image planes ([H_b, pitch_b] or [1, H_b, pitch_b]) with a list of widths.
        A packed plane carries no probabilities: the mask score's numerator is TP + FP, i.e. the score is 1.  Asynchronous."""
        if isinstance(pred_packed, torch.Tensor):
            p = pred_packed.reshape((-1,) + tuple(pred_packed.shape[-2:]))
            g = gt_packed.reshape((-1,) + tuple(gt_packed.shape[-2:]))
            pred, gt, widths = list(p), list(g), [int(W0)] * p.shape[0]
        else:
            pred, gt = [t.reshape(t.shape[-2:]) for t in pred_packed], [t.reshape(t.shape[-2:]) for t in gt_packed]
            widths = [int(w) for w in W0] if isinstance(W0, (list, tuple)) else [int(W0)] * len(pred)
        if len(pred) != len(gt) or len(widths) != len(pred):
            raise ValueError(f"SegmentationMetrics.update_packed: {len(pred)} predictions, {len(gt)} ground truths, {len(widths)} widths")
        for a, b, w in zip(pred, gt, widths):
            if not (a.is_cuda and b.is_cuda):
                raise RuntimeError("SegmentationMetrics.update_packed: expected CUDA/HIP tensors on an MI355X (no CPU path)")
            if a.dtype != torch.uint8 or b.dtype != torch.uint8 or a.shape != b.shape or a.shape[1] != plane_pitch(w):
                raise ValueError(f"SegmentationMetrics.update_packed: planes {tuple(a.shape)} / {tuple(b.shape)} for width {w}; expected uint8 "
                                 f"[H, {plane_pitch(w)}] both")
        if not pred:
            return
        dev = pred[0].device
        pred, gt = [t.contiguous() for t in pred], [t.contiguous() for t in gt]
        for c0 in range(0, len(pred), MASK_EVAL_MAX_IMAGES):
            nb = min(MASK_EVAL_MAX_IMAGES, len(pred) - c0)
            images = [(pred[b].shape[0], widths[b], pred[b], gt[b], b - c0, 1) for b in range(c0, c0 + nb)]
            inter, det_area, gt_px = _pair_counts(images, 1, None, torch.arange(nb, dtype=torch.int32, device=dev), nb, dev)
            u = lambda t: t.reshape(-1).to(torch.int64) & 0xFFFFFFFF            # the tables are uint32 counts in int32 words
            tp, d, g = u(inter), u(det_area), u(gt_px)
            px = torch.tensor([pred[b].shape[0] * widths[b] for b in range(c0, c0 + nb)], dtype=torch.int64).to(dev, non_blocking=True)
            self._counts.append(torch.stack([tp, d - tp, g - tp, px - d - g + tp], 1))
            self._psum.append(d.to(torch.float32))

    def per_image(self, sync: bool = False):
        """-> (counts [N,4] int64 = TP, FP, FN, TN; mask scores [N] = sum(prob * mask) / (sum(mask) + 1e-6), :483).
        `sync`: the images of all ranks in rank order (a collective)."""
        if self._counts:
            c = torch.cat(self._counts).cpu().numpy()
            p = torch.cat(self._psum).cpu().numpy()
        else:
            c, p = np.zeros((0, 4), np.int64), np.zeros(0, np.float32)
        if sync and _world(self.group) > 1:
            recs = _all_gather_records([(c, p)], self.group)
            c, p = np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])
        return c, (p / ((c[:, 0] + c[:, 1]).astype(np.float32) + np.float32(1e-6))).astype(np.float32)

    def compute(self) -> Dict[str, float]:
        """With a live process group (and dist_sync): from the pixel counts of ALL ranks -- a collective, every rank must call it.
        seg_map / seg_map_50 are the map / map_50 of `compute_map` (:478-497), -1.0 without images."""
        c, score = self.per_image(sync=self.dist_sync)
        tp, fp, fn, tn = (float(v) for v in c.sum(axis=0)) if len(c) else (0.0, 0.0, 0.0, 0.0)
        div = lambda a, b: a / b if b else 0.0                                    # torchmetrics _safe_divide
        out = {"f1": div(2 * tp, 2 * tp + fp + fn), "precision": div(tp, tp + fp), "recall": div(tp, tp + fn),
               "accuracy": div(tp + tn, tp + tn + fp + fn), "iou": div(tp, tp + fp + fn), "dice_global": div(2 * tp, 2 * tp + fp + fn)}
        den = (2 * c[:, 0] + c[:, 1] + c[:, 2]).astype(np.float64)
        dice = np.where(den > 0, 2 * c[:, 0] / np.maximum(den, 1), np.nan)         # per sample; empty-vs-empty samples are skipped
        out["dice"] = float(np.nanmean(dice)) if np.any(den > 0) else 0.0
        seg = _segm_map(c, score)
        out["seg_map"], out["seg_map_50"] = seg["map"], seg["map_50"]
        return out

    def compute_map(self) -> Dict[str, float]:
        """The segmentation mAP's standard COCO key set (torchmetrics `MeanAveragePrecision(iou_type="segm")` of :206, logged per scalar
        key at :624-633): map, map_50, map_75, map_small / medium / large, mar_1 / 10 / 100, mar_small / medium / large.

        From the per-image counts `update` keeps: each image holds one predicted and one GT instance, both class 0; the score is the
        mask score of `per_image`; mask IoU = TP / (TP + FP + FN), 0 when the union is empty (pycocotools' value for two empty masks);
        areas are pixel counts, detection TP + FP, GT TP + FN, ranges and inclusive bounds of `AREA_RANGES`.  Matching and ignore flags
        follow pycocotools `evaluateImg`: a detection matched to a GT outside the area range is ignored, so is an unmatched detection
        outside it.  Accumulated by `_accumulate` (IoU thresholds 0.50:0.05:0.95, max detections 1 / 10 / 100).  torchmetrics'
        version-dependent extras (`classes`, and the `map_per_class` / `mar_100_per_class` placeholders) are not reproduced.
        With a live process group (and dist_sync): over the images of ALL ranks -- a collective."""
        c, score = self.per_image(sync=self.dist_sync)
        return _segm_map(c, score)


def _segm_map(c: np.ndarray, score: np.ndarray) -> Dict[str, float]:
    """SegmentationMetrics.compute_map from per-image counts c [N,4] (TP, FP, FN, TN) and mask scores [N]."""
    c = np.asarray(c, np.int64).reshape(-1, 4)
    n = len(c)
    thr = COCO_IOU_THRESHOLDS
    union = (c[:, 0] + c[:, 1] + c[:, 2]).astype(np.float64)
    iou = np.where(union > 0, c[:, 0] / np.maximum(union, 1), 0.0)
    d_area, g_area = (c[:, 0] + c[:, 1]).astype(np.float64), (c[:, 0] + c[:, 2]).astype(np.float64)
    bounds = [(0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10)]     # AREA_RANGES, inclusive
    matched = iou[:, None] >= _iou_limits(thr)[None, :]                                     # [N, T]: the one GT of the image
    tbits = (np.uint32(1) << np.arange(len(thr), dtype=np.uint32))
    match, ignore, gt_bits = np.zeros((n, 4), np.uint32), np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32)
    for a, (lo, hi) in enumerate(bounds):
        g_in = (g_area >= lo) & (g_area <= hi)
        d_in = (d_area >= lo) & (d_area <= hi)
        gt_bits |= np.where(g_in, np.uint32(1 << a), np.uint32(0))
        ig = np.where(matched, ~g_in[:, None], ~d_in[:, None])                              # matched: the GT's flag; else the detection's
        match[:, a] = (matched * tbits).sum(1).astype(np.uint32)
        ignore[:, a] = (ig * tbits).sum(1).astype(np.uint32)
    rec = {"image": np.arange(n, dtype=np.int64), "rank": np.zeros(n, np.int64), "score": np.asarray(score, np.float64).ravel(),
           "label": np.zeros(n, np.int64), "match": match, "ignore": ignore, "gt_label": np.zeros(n, np.int64), "gt_area": gt_bits}
    return _accumulate(rec, thr, (1, 10, 100))


class _ConfusionCounts:
    """A [nc, nc] int64 confusion matrix (row = target, column = prediction) that a kernel adds to on the device, plus its status
    word, in ONE device buffer of nc * nc + 1 int64 (the status is the int32 low word of the last one): `compute()` copies it once."""

    def __init__(self, num_classes: int, dist_sync: bool, process_group):
        num_classes = int(num_classes)
        if not 1 <= num_classes <= L.CONFUSION_MAX_NC:
            raise ValueError(f"{type(self).__name__}: between 1 and {L.CONFUSION_MAX_NC} classes, got {num_classes}")
        self.num_classes, self.dist_sync, self.group = num_classes, dist_sync, process_group
        self.reset()

    def reset(self):
        self._state: Optional[torch.Tensor] = None

    def _buffers(self, dev):
        """-> (counts pointer, status pointer) on `dev`, zeroed at the first update after a reset."""
        nc = self.num_classes
        if self._state is None:
            self._state = torch.zeros(nc * nc + 1, dtype=torch.int64, device=dev)
        elif self._state.device != dev:
            raise ValueError(f"{type(self).__name__}: this metric keeps its counts on {self._state.device}, the batch is on {dev}")
        return self._state.data_ptr(), self._state[nc * nc:].view(torch.int32).data_ptr()

    def counts(self) -> np.ndarray:
        """[nc, nc] int64 over this process's updates -- or, with a live process group (and dist_sync), the sum over ALL ranks (a
        collective; the local state is left as it is).  Raises ValueError when a target class was outside [0, nc)."""
        nc = self.num_classes
        st = self._state.cpu().numpy() if self._state is not None else np.zeros(nc * nc + 1, np.int64)
        cm, status = st[:-1], int(st[-1])
        if self.dist_sync:
            cm, status = _sum_over_ranks(cm, self.group), max(_all_gather_records([status], self.group))
        if status:
            raise ValueError(f"{type(self).__name__}.compute: a target class outside [0, {nc}) was seen (those samples are not counted)")
        return cm.reshape(nc, nc).astype(np.int64)


def _normalize_rows(cm: np.ndarray) -> np.ndarray:
    """torchmetrics normalize="true": each row divided by its sum; a row without samples stays all zeros."""
    rows = cm.sum(axis=1, keepdims=True).astype(np.float64)
    return np.where(rows > 0, cm / np.maximum(rows, 1), 0.0)


class ImageClassificationMetrics(_ConfusionCounts):
    """Image-class metrics of the validation epoch: MulticlassAccuracy(average="micro") and MulticlassConfusionMatrix(normalize="true")
    of running_main_v3.py:193-195 (fed at :458-459, logged at :609-616), and the macro precision / recall / F1 of
    evaluate_model.py:244-272 -- all from one device-side confusion matrix (`mtbt_cls_confusion`).

    `update(logits [B, nc], target [B])` is asynchronous (no host synchronisation) and rejects CPU tensors.  `compute()` ->
    accuracy (micro: correct / N, 0.0 without samples), confusion_matrix (row-normalised, a row without samples is all zeros),
    confusion_counts, precision_macro / recall_macro / f1_macro (per class 0 where the denominator is 0; the mean runs over the
    classes with tp + fp + fn > 0, 0.0 if there are none).  A target outside [0, nc) makes `compute()` raise ValueError, as
    torchmetrics' target validation does."""

    def __init__(self, num_classes: int, dist_sync: bool = True, process_group=None):
        super().__init__(num_classes, dist_sync, process_group)

    def update(self, logits: torch.Tensor, target: torch.Tensor):
        if not (logits.is_cuda and target.is_cuda):
            raise RuntimeError("ImageClassificationMetrics.update: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        if logits.dim() != 2 or logits.shape[1] != self.num_classes or target.shape != logits.shape[:1]:
            raise ValueError(f"ImageClassificationMetrics.update: logits [B, {self.num_classes}] and target [B]")
        if logits.device != target.device:
            raise ValueError("ImageClassificationMetrics.update: logits and target on different devices")
        if logits.shape[0] == 0:
            return
        lib = L.load()
        dev = logits.device
        x, t = logits.float().contiguous(), target.long().contiguous()
        counts, status = self._buffers(dev)
        L.check(lib.mtbt_cls_confusion(x.data_ptr(), t.data_ptr(), x.shape[0], self.num_classes, counts, status,
                                       L.stream(dev)), "mtbt_cls_confusion")

    def compute(self) -> Dict[str, object]:
        cm = self.counts()
        tp = np.diag(cm).astype(np.float64)
        fp, fn = cm.sum(axis=0) - tp, cm.sum(axis=1) - tp
        n = float(cm.sum())
        div = lambda a, b: np.where(b > 0, a / np.where(b > 0, b, 1), 0.0)
        present = (tp + fp + fn) > 0
        macro = lambda v: float(v[present].mean()) if present.any() else 0.0
        return {"accuracy": float(tp.sum()) / n if n else 0.0, "confusion_matrix": _normalize_rows(cm), "confusion_counts": cm,
                "precision_macro": macro(div(tp, tp + fp)), "recall_macro": macro(div(tp, tp + fn)), "f1_macro": macro(div(2 * tp, 2 * tp + fp + fn))}


class DetectionConfusionMatrix(_ConfusionCounts):
    """The detection confusion matrix of the validation epoch (MulticlassConfusionMatrix(nc_det, normalize="true") of
    running_main_v3.py:218, fed at :710-722 with the (argmax of the class logits, GT class) pairs that the eval-mode `_multitask_loss`
    collects over its positive anchors at :349-350).

    `update(det_maps, gt_rows)`: the raw Detect maps of `forward(x, "train")` and the collated [M, 6] GT rows -- the inputs
    `multitask_loss` takes.  One `mtbt_det_confusion` launch decodes and matches every anchor exactly as the loss does (its argument
    block is built by the same helper, `loss.det_loss_args`), so the counted anchors are the loss's positives.  Asynchronous; rejects
    CPU tensors.  `compute()` -> confusion_matrix (row-normalised, empty rows all zeros) and confusion_counts; a GT class outside
    [0, nc_det) makes it raise ValueError."""

    def __init__(self, nc_det: int, img_size: int, iou_match_thresh: float = 0.5, reg_max: int = 16, dist_sync: bool = True, process_group=None):
        super().__init__(nc_det, dist_sync, process_group)
        self.img_size, self.iou_match_thresh, self.reg_max = img_size, float(iou_match_thresh), int(reg_max)

    def update(self, det_maps: Sequence[torch.Tensor], gt_rows: torch.Tensor):
        if not (all(m.is_cuda for m in det_maps) and gt_rows.is_cuda):
            raise RuntimeError("DetectionConfusionMatrix.update: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        if not 1 <= len(det_maps) <= 3 or any(m.dim() != 4 or m.shape[1] != 4 * self.reg_max + self.num_classes for m in det_maps):
            raise ValueError(f"DetectionConfusionMatrix.update: 1 to 3 Detect maps [B, {4 * self.reg_max + self.num_classes}, h, w]")
        if gt_rows.dim() != 2 or gt_rows.shape[1] != 6:
            raise ValueError("DetectionConfusionMatrix.update: gt_rows must be [M, 6] (batch_idx, cls, cx, cy, w, h)")
        if det_maps[0].shape[0] == 0:
            return
        from .loss import det_loss_args
        lib = L.load()
        dev = det_maps[0].device
        a, keep = det_loss_args(det_maps, gt_rows, img_size=self.img_size, nc_det=self.num_classes, reg_max=self.reg_max,
                                iou_match_thresh=self.iou_match_thresh)
        counts, status = self._buffers(dev)
        L.check(lib.mtbt_det_confusion(C.byref(a), counts, status, L.stream(dev)), "mtbt_det_confusion")
        del keep

    def compute(self) -> Dict[str, object]:
        cm = self.counts()
        return {"confusion_matrix": _normalize_rows(cm), "confusion_counts": cm}


# ---- surface distances ------------------------------------------------------------------------------------------------------------
SURFACE_MAX_DIM = 16384          # H and W of mtbt_surface_distances (squared distances stay below 2^29)
SURFACE_MAX_QUANTILES = 4


def surface_tol2(tolerance: float, spacing: float = 1.0) -> int:
    """The integer the device compares squared pixel distances with: d <= tolerance  <=>  d^2 <= floor((tolerance / spacing)^2)."""
    if not (spacing > 0) or not (tolerance >= 0):
        raise ValueError("surface_tol2: spacing must be > 0 and tolerance >= 0")
    return int(min(np.floor((float(tolerance) / float(spacing)) ** 2), 2.0 ** 32 - 1))


def surface_distances(a_packed: torch.Tensor, b_packed: torch.Tensor, W: int, *, quantiles: Sequence[float] = (0.95,), tol2: int = 0):
    """Surface-distance records of n pairs of bit-packed planes, on the device (`mtbt_surface_distances`; definitions in
    include/mtbt_hip.h: 4-neighbour edge sets, exact integer squared distances from every edge pixel of one plane to the other's edge set).

    a_packed, b_packed: uint8 [n, H, pitch] with pitch = 8 * ceil(W / 64) (`pack_masks`, `masks_to_frames`); bits X >= W never count.
    Returns a dict of device tensors -- n_edge, max_d2, n_within int32 [n, 2] (A->B, B->A; the values are below 2^31), sum_d float64
    [n, 2], rank_d2 int32 [n, Q, 3, 2] (A->B, B->A, pooled; the order statistics at floor(q (m - 1)) and the next) -- plus the host
    values `quantiles`, `tol2` and `shape` = (H, W) that `surface_metrics` needs.  Asynchronous: no host synchronisation."""
    W = int(W)
    same = "a_packed and b_packed must be uint8 [n, H, pitch] of the same shape"
    n, H, pitch, a_planes, b_planes = packed_planes("surface_distances", a_packed, W, b_packed, max_dim=SURFACE_MAX_DIM,
                                                    words=(same, same, "the two sides are on different devices"))
    q = tuple(float(v) for v in quantiles)
    if len(q) > SURFACE_MAX_QUANTILES or any(not 0.0 <= v <= 1.0 for v in q):
        raise ValueError(f"surface_distances: at most {SURFACE_MAX_QUANTILES} quantiles, each in [0, 1]")
    tol2 = int(tol2)
    if not 0 <= tol2 < 2 ** 32:
        raise ValueError("surface_distances: tol2 must fit an unsigned 32-bit integer")
    dev = a_packed.device
    Q = len(q)
    out = {"n_edge": torch.empty((n, 2), dtype=torch.int32, device=dev), "max_d2": torch.empty((n, 2), dtype=torch.int32, device=dev),
           "n_within": torch.empty((n, 2), dtype=torch.int32, device=dev), "sum_d": torch.empty((n, 2), dtype=torch.float64, device=dev),
           "rank_d2": torch.empty((n, Q, 3, 2), dtype=torch.int32, device=dev), "quantiles": q, "tol2": tol2, "shape": (H, W)}
    if n == 0:
        return out
    lib = L.load()
    ws, ws_bytes = L.workspace(lib.mtbt_surface_distances_workspace_bytes, n, H, W, device=dev, what="mtbt_surface_distances_workspace_bytes")
    a = L.SurfaceArgs()
    a.a, a.b, a.workspace, a.workspace_bytes = a_planes.data_ptr(), b_planes.data_ptr(), ws.data_ptr(), ws_bytes
    a.n_edge, a.max_d2, a.n_within, a.sum_d = (out[k].data_ptr() for k in ("n_edge", "max_d2", "n_within", "sum_d"))
    a.rank_d2 = out["rank_d2"].data_ptr() if Q else None
    for i, v in enumerate(q):
        a.q[i] = v
    a.n, a.H, a.W, a.pitch, a.tol2, a.Q = n, H, W, pitch, tol2, Q
    with torch.cuda.device(dev):
        L.check(lib.mtbt_surface_distances(C.byref(a), L.stream(dev)), "mtbt_surface_distances")
    return out


SURFACE_KEYS = ("hd", "hd95", "assd", "nsd")


def surface_metrics(records: Dict[str, object], *, spacing: float = 1.0, tolerance: float = 2.0, percentile_mode: str = "pooled",
                    undefined: str = "skip", quantile_index: int = 0) -> Dict[str, np.ndarray]:
    """Per-pair hd, hd95, assd, nsd and `defined` from the records of `surface_distances` (host arrays or tensors); pure host code.

    With d = spacing * sqrt(d2): hd = the largest d of both directed lists; hd95 = the `quantiles[quantile_index]` percentile with
    linear interpolation (numpy's default) of the pooled list (`percentile_mode="pooled"`, MedPy's hd95) or the larger of the two
    directed percentiles ("max", MONAI's); assd = (mean(A->B) + mean(B->A)) / 2; nsd = the share of both lists with
    d2 <= floor((tolerance / spacing)^2), which must be the `tol2` the records were made with.
    A pair with an empty edge set is undefined: `defined` is False and its four values are NaN (`undefined="skip"`); under
    `undefined="diagonal"` a pair with exactly ONE empty side gets spacing * sqrt(H^2 + W^2) for hd, hd95 and assd and 0 for nsd
    (`defined` stays False; a pair with both sides empty stays NaN)."""
    if percentile_mode not in ("pooled", "max"):
        raise ValueError(f"percentile_mode: 'pooled' (MedPy) or 'max' (MONAI), not {percentile_mode!r}")
    if undefined not in ("skip", "diagonal"):
        raise ValueError(f"undefined: 'skip' or 'diagonal', not {undefined!r}")
    if surface_tol2(tolerance, spacing) != int(records["tol2"]):
        raise ValueError(f"surface_metrics: tolerance {tolerance} at spacing {spacing} is tol2 = {surface_tol2(tolerance, spacing)}, "
                         f"the records were made with tol2 = {records['tol2']}")
    np_ = lambda k, dt: MeanAveragePrecision._np(records[k], dt)
    n_edge = np_("n_edge", np.int64).reshape(-1, 2)
    n = len(n_edge)
    max_d2, within, sum_d = np_("max_d2", np.int64).reshape(n, 2), np_("n_within", np.int64).reshape(n, 2), np_("sum_d", np.float64).reshape(n, 2)
    spacing = float(spacing)
    nA, nB = n_edge[:, 0], n_edge[:, 1]
    defined = (nA > 0) & (nB > 0)
    one = np.maximum(n_edge, 1).astype(np.float64)
    out = {"hd": spacing * np.sqrt(max_d2.max(axis=1).astype(np.float64)),
           "assd": spacing * 0.5 * (sum_d[:, 0] / one[:, 0] + sum_d[:, 1] / one[:, 1]),
           "nsd": within.sum(axis=1) / np.maximum(nA + nB, 1).astype(np.float64)}
    if len(records["quantiles"]):
        q = float(records["quantiles"][quantile_index])
        rank = spacing * np.sqrt(np_("rank_d2", np.float64).reshape(n, len(records["quantiles"]), 3, 2)[:, quantile_index])   # [n, 3, 2]
        m = np.stack([nA, nB, nA + nB], 1)
        pos = q * np.maximum(m - 1, 0).astype(np.float64)                        # the product the kernel formed
        t = pos - np.floor(pos)
        diff = rank[:, :, 1] - rank[:, :, 0]
        pct = np.where(t >= 0.5, rank[:, :, 1] - diff * (1 - t), rank[:, :, 0] + diff * t)        # numpy's _lerp
        out["hd95"] = pct[:, 2] if percentile_mode == "pooled" else pct[:, :2].max(axis=1)
    else:
        out["hd95"] = np.full(n, np.nan)
    H, W = records["shape"]
    diag = spacing * float(np.sqrt(float(H) ** 2 + float(W) ** 2))
    one_empty = (nA > 0) ^ (nB > 0)
    for k in SURFACE_KEYS:
        v = np.where(defined, out[k], np.nan)
        if undefined == "diagonal":
            v = np.where(one_empty, 0.0 if k == "nsd" else diag, v)
        out[k] = v
    out["defined"] = defined
    return out


class SurfaceDistanceMetrics:
    """Boundary metrics of binary segmentation -- Hausdorff distance, its `quantile` percentile (HD95), average symmetric surface
    distance and normalised surface Dice at `tolerance` -- with MedPy's definitions (`surface_metrics`) from device-side records
    (`surface_distances`: 4-neighbour edge sets, exact integer squared distances).  Isotropic `spacing` only.

    `update(seg_logits, masks_gt)`: [B,1,S,S] or [B,S,S] device tensors.  Prediction bit = logit > 0, target bit = masks_gt >= 1 (the
    rule of `mtbt_seg_confusion`); both sides are packed by `pack_masks`.  logit > 0 differs from sigmoid(logit) > 0.5 in fp32 only
    for 0 < logit <~ 6e-8, where the sigmoid rounds to exactly 0.5.  Asynchronous: the records stay on the device.
    `update_packed(a, b, W)`: pairs of packed planes uint8 [n, H, pitch], e.g. `masks_frame` against packed ground truth for pairs
    the caller has matched.
    `per_image(sync=False)` -> per-pair arrays hd, hd95, assd, nsd (NaN where a pair does not contribute) and `defined`.
    `compute()` -> the means of hd, hd95, assd, nsd over the contributing pairs (-1.0 when there is none), n_pairs and n_undefined
    (pairs with an empty edge set, whatever `undefined` does with them).  With a live process group (and `dist_sync`): over the
    pairs of ALL ranks in rank order -- a collective, every rank must call it."""

    def __init__(self, quantile: float = 0.95, tolerance: float = 2.0, spacing: float = 1.0, percentile_mode: str = "pooled",
                 undefined: str = "skip", dist_sync: bool = True, process_group=None):
        if not 0.0 <= float(quantile) <= 1.0:
            raise ValueError(f"SurfaceDistanceMetrics: quantile {quantile!r} is not in [0, 1]")
        if percentile_mode not in ("pooled", "max"):
            raise ValueError(f"SurfaceDistanceMetrics: percentile_mode 'pooled' (MedPy) or 'max' (MONAI), not {percentile_mode!r}")
        if undefined not in ("skip", "diagonal"):
            raise ValueError(f"SurfaceDistanceMetrics: undefined 'skip' or 'diagonal', not {undefined!r}")
        self.quantile, self.tolerance, self.spacing = float(quantile), float(tolerance), float(spacing)
        self.tol2 = surface_tol2(self.tolerance, self.spacing)
        self.percentile_mode, self.undefined = percentile_mode, undefined
        self.dist_sync, self.group = dist_sync, process_group
        self.reset()

    def reset(self):
        self._records: List[Dict[str, object]] = []

    def update_packed(self, a: torch.Tensor, b: torch.Tensor, W: int):
        """Asynchronous: launches on the current stream and keeps its records on the device."""
        rec = surface_distances(a, b, W, quantiles=(self.quantile,), tol2=self.tol2)
        if rec["n_edge"].shape[0]:
            self._records.append(rec)

    def update(self, seg_logits: torch.Tensor, masks_gt: torch.Tensor):
        if not (isinstance(seg_logits, torch.Tensor) and isinstance(masks_gt, torch.Tensor) and seg_logits.is_cuda and masks_gt.is_cuda):
            raise RuntimeError("SurfaceDistanceMetrics.update: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        if seg_logits.shape != masks_gt.shape:
            raise ValueError("SurfaceDistanceMetrics.update: logits and masks differ in shape")
        if seg_logits.dim() == 4 and seg_logits.shape[1] == 1:
            seg_logits, masks_gt = seg_logits[:, 0], masks_gt[:, 0]
        if seg_logits.dim() != 3:
            raise ValueError("SurfaceDistanceMetrics.update: logits and masks must be [B,1,S,S] or [B,S,S]")
        if seg_logits.shape[0] == 0:
            return
        self.update_packed(pack_masks(seg_logits.float()), pack_masks(masks_gt >= 1), seg_logits.shape[2])

    def per_image(self, sync: bool = False) -> Dict[str, np.ndarray]:
        parts = []
        for rec in self._records:
            host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in rec.items()}
            parts.append(surface_metrics(host, spacing=self.spacing, tolerance=self.tolerance, percentile_mode=self.percentile_mode,
                                         undefined=self.undefined))
        keys = SURFACE_KEYS + ("defined",)
        out = {k: np.concatenate([np.zeros(0, bool if k == "defined" else np.float64)] + [p[k] for p in parts]) for k in keys}
        if sync and _world(self.group) > 1:
            recs = _all_gather_records([out], self.group)
            out = {k: np.concatenate([r[k] for r in recs]) for k in keys}
        return out

    def compute(self) -> Dict[str, float]:
        per = self.per_image(sync=self.dist_sync)
        out: Dict[str, float] = {}
        for k in SURFACE_KEYS:
            v = per[k][~np.isnan(per[k])]
            out[k] = float(v.mean()) if v.size else -1.0
        out["n_pairs"], out["n_undefined"] = int(len(per["defined"])), int(np.count_nonzero(~per["defined"]))
        return out


# ---- lesion-wise detection from the semantic mask ------------------------------------------------------------------------------------
def lesion_hits(n_components, area, inter, overlap: float = 0.0):
    """Which components of `label_components(..., other=)` records are hit by the other side; pure host code.

    n_components [n], area and inter [n, C] (id i in row i - 1).  A component is hit when inter >= 1 and inter >= overlap * area, the
    product being one float64 multiplication.  Returns (hits int64 [n], truncated bool [n]): a plane with more than C components is
    truncated, and its components beyond the table count as not hit."""
    n_comp = np.asarray(n_components, np.int64).reshape(-1)
    area, inter = np.asarray(area, np.int64), np.asarray(inter, np.int64)
    n, C_ = len(n_comp), area.shape[1] if area.ndim == 2 else 0
    area, inter = area.reshape(n, C_), inter.reshape(n, C_)
    listed = np.arange(C_)[None, :] < np.minimum(n_comp, C_)[:, None]
    hit = listed & (inter >= 1) & (inter.astype(np.float64) >= np.float64(overlap) * area.astype(np.float64))
    return hit.sum(axis=1).astype(np.int64), n_comp > C_


class LesionMetrics:
    """Lesion-wise detection of binary segmentation: the connected components of the ground truth that the prediction finds and the
    components of the prediction that are true, from device-side records (`postprocess.label_components` with `other=`).

    A ground-truth component is FOUND when the prediction covers at least one of its pixels and at least `overlap` of its area
    (`lesion_hits`); a predicted component is TRUE by the same test against the ground truth.  With `min_area` > 0 predicted components
    below it are removed first (`filter_components`); the ground truth is never filtered.
    `update(seg_logits, masks_gt)`: [B,1,S,S] or [B,S,S] device tensors, prediction bit = logit > 0, target bit = masks_gt >= 1 (the
    rule of `SurfaceDistanceMetrics.update`).  `update_packed(pred, gt, W)`: packed uint8 [n, H, pitch] stacks.  Two labelling calls
    per batch; the records stay on the device until `compute()`.
    `compute()` -> lesion_recall = found / ground-truth components, lesion_precision = true / predicted components (pooled over the
    data set, each 0 when its denominator is 0), lesion_f1, fp_per_image (false predicted components per image), n_gt, n_pred,
    n_images, and n_truncated: the images with more than `max_components` components on a side, whose excess components count as not
    found / false.  With a live process group (and `dist_sync`): over ALL ranks -- a collective, every rank must call it."""

    def __init__(self, overlap: float = 0.0, min_area: int = 0, connectivity: int = 4, max_components: int = 1024,
                 dist_sync: bool = True, process_group=None):
        if not 0.0 <= float(overlap) <= 1.0:
            raise ValueError(f"LesionMetrics: overlap {overlap!r} is not in [0, 1]")
        if int(min_area) < 0 or int(min_area) != min_area:
            raise ValueError(f"LesionMetrics: min_area {min_area!r} is not an integer >= 0")
        if connectivity not in (4, 8):
            raise ValueError(f"LesionMetrics: connectivity 4 or 8, not {connectivity!r}")
        if not 1 <= int(max_components) <= 65536:
            raise ValueError(f"LesionMetrics: max_components {max_components!r} is outside [1, 65536]")
        self.overlap, self.min_area, self.connectivity, self.max_components = float(overlap), int(min_area), int(connectivity), int(max_components)
        self.dist_sync, self.group = dist_sync, process_group
        self.reset()

    def reset(self):
        self._records: List[Dict[str, torch.Tensor]] = []

    def update_packed(self, pred: torch.Tensor, gt: torch.Tensor, W: int):
        """Asynchronous: launches on the current stream and keeps its records on the device."""
        kw = dict(connectivity=self.connectivity, max_components=self.max_components, want_labels=False)
        if self.min_area > 0:
            pred =filter_components(pred, W, min_area=self.min_area, connectivity=self.connectivity)[0]
        p, g = label_components(pred, W, other=gt, **kw), label_components(gt, W, other=pred, **kw)
        if p["n_components"].shape[0]:
            self._records.append({f"{s}_{k}": r[k] for s, r in (("pred", p), ("gt", g)) for k in ("n_components", "area", "inter")})

    def update(self, seg_logits: torch.Tensor, masks_gt: torch.Tensor):
        if not (isinstance(seg_logits, torch.Tensor) and isinstance(masks_gt, torch.Tensor) and seg_logits.is_cuda and masks_gt.is_cuda):
            raise RuntimeError("LesionMetrics.update: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        if seg_logits.shape != masks_gt.shape:
            raise ValueError("LesionMetrics.update: logits and masks differ in shape")
        if seg_logits.dim() == 4 and seg_logits.shape[1] == 1:
            seg_logits, masks_gt = seg_logits[:, 0], masks_gt[:, 0]
        if seg_logits.dim() != 3:
            raise ValueError("LesionMetrics.update: logits and masks must be [B,1,S,S] or [B,S,S]")
        if seg_logits.shape[0] == 0:
            return
        self.update_packed(pack_masks(seg_logits.float()), pack_masks(masks_gt >= 1), seg_logits.shape[2])

    def counts(self, sync: bool = False) -> np.ndarray:
        """int64 [6]: ground-truth components, found ones, predicted components, true ones, images, truncated images."""
        tot = np.zeros(6, np.int64)
        for rec in self._records:
            h = {k: v.cpu().numpy() for k, v in rec.items()}
            found, cut_g = lesion_hits(h["gt_n_components"], h["gt_area"], h["gt_inter"], self.overlap)
            true, cut_p = lesion_hits(h["pred_n_components"], h["pred_area"], h["pred_inter"], self.overlap)
            tot += np.array([h["gt_n_components"].sum(), found.sum(), h["pred_n_components"].sum(), true.sum(), len(found),
                             np.count_nonzero(cut_g | cut_p)], np.int64)
        return _sum_over_ranks(tot, self.group) if sync else tot

    def compute(self) -> Dict[str, float]:
        n_gt, n_found, n_pred, n_true, n_images, n_cut = (int(v) for v in self.counts(sync=self.dist_sync))
        rec = n_found / n_gt if n_gt else 0.0
        prec = n_true / n_pred if n_pred else 0.0
        return {"lesion_recall": rec, "lesion_precision": prec, "lesion_f1": 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0,
                "fp_per_image": (n_pred - n_true) / n_images if n_images else 0.0, "n_gt": n_gt, "n_pred": n_pred, "n_images": n_images,
                "n_truncated": n_cut}
