"""The whole validation step as device work with no host synchronisation -- the counterpart of `trainstep.TrainStep`.

    vs = ValidationStep(model, projector=lit.seg_proto_projector, img_size=640)
    for ids, imgs, det_gt, masks_gt, cls_gt in val_loader:          # device tensors
        losses = vs.step(imgs, det_gt, masks_gt, cls_gt)            # 6 x 0-d device tensors
    logs = vs.compute()                                             # the reference's log keys; a collective under DDP
    vs.reset()

`step()` is `/root/reference/src/running_main_v3.py:447-599` (`validation_step`) per batch, every part fed from the SAME train-mode
maps: forward(x, "train") -> eval-mode `_multitask_loss` -> segmentation counts -> image and detection confusion matrices -> decode /
NMS -> the two box mAPs.  `compute()` is the epoch end (`:605-729`): the batch-size-weighted loss means and every metric under the
key the reference logs it with.
"""
from typing import Dict, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from .loss import instance_mask_loss, multitask_loss, task_aligned_det_loss
from .metrics import (DetectionConfusionMatrix, DeviceMaskMeanAveragePrecision, DeviceMeanAveragePrecision, ImageClassificationMetrics,
                      LesionMetrics, SegmentationMetrics, SurfaceDistanceMetrics, _sum_over_ranks)
from .postprocess import (CONF_TH, NMS_IOU, TOP_K, decode_boxes, fuse_detections, masks_to_frames, nms_batched, orient_batch, pack_masks,
                          proto_projector_logits, seg_to_frames, vote_masks)

LOSS_NAMES = ("total", "seg", "box_iou", "dfl", "det_cls", "img_cls")       # running_main_v3.py:578-582
MASK_LOSS_NAME = "mask"                                                      # appended with instance_mask_weight > 0


class BatchWeightedMeans:
    """Epoch means of per-batch 0-d device tensors weighted by the batch size: sum over every step of every rank of B * value, divided
    by the sum of B.  This is what Lightning's `log(..., on_epoch=True, sync_dist=True)` reduces to for a mean (the Lightning version is
    unpinned in the reference; this definition is the one implemented).  `update` adds on the device (fp64), without a host sync;
    `compute()` copies the sums once and, with a live process group (and dist_sync), adds every rank's sums and batch counts (a
    collective) and leaves the local state untouched."""

    def __init__(self, n: int, dist_sync: bool = True, process_group=None):
        self.n, self.dist_sync, self.group = int(n), dist_sync, process_group
        self.reset()

    def reset(self):
        self._sum: Optional[torch.Tensor] = None
        self._count = 0

    def update(self, values: Sequence[torch.Tensor], batch_size: int):
        v = torch.stack([t.reshape(()) for t in values[: self.n]]).to(torch.float64) * float(batch_size)
        self._sum = v if self._sum is None else self._sum.add_(v)
        self._count += int(batch_size)

    def compute(self) -> np.ndarray:
        s = np.append(self._sum.cpu().numpy() if self._sum is not None else np.zeros(self.n), self._count)   # the sums, then the count
        if self.dist_sync:
            s = _sum_over_ranks(s, self.group)
        return s[:-1] / s[-1] if s[-1] else np.zeros(self.n, np.float64)


class ValidationStep:
    def __init__(self, model, *, projector: Optional[nn.Conv2d] = None, img_size: int = 640, iou_match_thresh: float = 0.5,
                 label_smoothing: float = 0.1, loss_weights=(1.0, 2.0, 1.5, 0.5, 1.0), conf_th: float = CONF_TH, nms_iou: float = NMS_IOU,
                 top_k: int = TOP_K, map_max_detections: int = 100, dist_sync: bool = True, process_group=None,
                 instance_masks: bool = False, mask_crop: bool = True, det_loss: str = "reference", tal=None,
                 instance_mask_weight: float = 0.0, mask_assign: str = "iou", views: Optional[Sequence[int]] = None, wbf_iou: float = 0.55,
                 fused_masks: Optional[str] = None, surface=None, lesions=None, seg_views: bool = False):
        """`projector` = the trainer's `seg_proto_projector` (Conv2d(proto_ch, 1, 1), running_main_v3.py:186); created with torch's default
        init when not given.  The loss hyper-parameters default to the reference's (and TrainStep's); `label_smoothing` is accepted for
        symmetry with TrainStep but the eval-mode loss never smooths (:337).  conf_th / nms_iou / top_k: `:54-56`;
        `map_max_detections`: the trainer's hparam of :209-217.
        `instance_masks`: also score the Segment head's INSTANCE masks (COCO mask mAP next to the box mAP; nothing in the reference
        computes it): the kept boxes' masks at S x S, bit-packed (`masks_to_frames` with identity frames, cropped to their boxes with
        `mask_crop`), against per-box ground truth cut out of the image's one mask by its box rows (`pack_masks`).  Off: `step`
        launches nothing more and `compute()` returns the reference's keys only.
        `det_loss`, `tal`, `instance_mask_weight`, `mask_assign`: as in `TrainStep`, so that a run trained with them monitors the loss it
        optimises.  `det_loss="tal"`: the box / dfl / det_cls elements and the total hold the task-aligned terms, weighted by the same
        `loss_weights` slots; seg and img_cls still come from the eval-mode `multitask_loss` with detection weights 0.
        `instance_mask_weight` > 0: the total includes `weight * mask_loss`, the tuple gains mask_loss and its positive count (8 elements)
        and `compute()` gains `val_epoch/loss_mask`; `mask_assign="tal"` takes its positives from the task-aligned assignment.  No
        gradient is computed.  The detection confusion matrix keeps the reference's matching.  At the defaults nothing changes.
        `views` (orient codes 0..7 of `orient_batch`, at most 8): test-time augmentation of the BOX mAP only.  map_iou50 / map_iou50_95
        are updated from the weighted-boxes fusion (`fuse_detections`, IoU `wbf_iou`) of one detection list per view: view 0 is the
        step's own identity pass (the same maps the losses see), every other view one more forward of the oriented batch with the whole
        module in eval mode (`model(x, "infer")`), decoded and filtered like the identity pass.  The losses, the confusion matrices and
        the segmentation metrics stay on the identity pass (the last unless `seg_views`), and `compute()` keeps its keys.  `views=None`: not one launch changes.
        `fused_masks="vote"` (with `views` and `instance_masks`): the instance-mask mAP is fed from the fused list too -- every view's pass
        keeps its mask coefficients and prototypes, and the packed planes are voted over each cluster's members (`vote_masks`, as
        `detect_fused(masks="vote")`).  `views` with `instance_masks` needs it: there is no other fused mask to score.
        `seg_views=True` (with `views`): the SEMANTIC metrics take part in the test-time augmentation too -- `self.seg`, `surface` and
        `lesions` are fed the projector logits averaged over the views (`seg_to_frames` on every view's prototypes at identity
        frames, its `logits` output as [B,1,S,S]) instead of the identity pass's.  False: not one launch changes.
        `surface` (True, or a dict of `SurfaceDistanceMetrics`' options quantile / tolerance / spacing / percentile_mode / undefined):
        also the boundary metrics of the semantic mask -- one `SurfaceDistanceMetrics.update` on the projector logits `self.seg` sees;
        `compute()` gains seg_hd_epoch, seg_hd95_epoch, seg_assd_epoch, seg_nsd_epoch and seg_surface_undefined.  None: not one
        launch and not one key changes.
        `lesions` (True, or a dict of `LesionMetrics`' options overlap / min_area / connectivity / max_components): also lesion-wise
        detection from the semantic mask -- one `LesionMetrics.update` on the same logits; `compute()` gains seg_lesion_recall,
        seg_lesion_precision, seg_lesion_f1 and seg_lesion_fp_per_image.  None: not one launch and not one key changes."""
        self.surface_kw = self._surface_options(surface)
        self.lesion_kw = self._lesion_options(lesions)
        self.views = None if views is None else tuple(int(v) for v in views)
        self.wbf_iou = float(wbf_iou)
        if fused_masks not in (None, "vote"):
            raise ValueError(f"fused_masks: None or 'vote', not {fused_masks!r}")
        if fused_masks is not None and (self.views is None or not instance_masks):
            raise ValueError("fused_masks='vote' scores the voted masks of the fused list: it needs views and instance_masks=True")
        self.fused_masks = fused_masks
        self.seg_views = bool(seg_views)
        if self.seg_views and self.views is None:
            raise ValueError("seg_views=True averages the semantic logits over the views: it needs views")
        if self.views is not None:
            if instance_masks and fused_masks is None:
                raise NotImplementedError("ValidationStep: views with instance_masks=True needs fused_masks='vote' (the voted masks of "
                                          "detect_fused(masks='vote')); the leaders' masks are not scored")
            if not 1 <= len(self.views) <= 8 or any(not 0 <= v <= 7 for v in self.views):
                raise ValueError(f"views: 1..8 orient codes in 0..7, not {views!r}")
        if det_loss not in ("reference", "tal"):
            raise ValueError(f"det_loss: 'reference' (the reference trainer's _multitask_loss) or 'tal' (task-aligned), not {det_loss!r}")
        self.det_loss = det_loss
        self.tal_kw = dict(topk=10, alpha=0.5, beta=6.0)
        if tal is not None:
            if det_loss != "tal" or set(tal) - set(self.tal_kw):
                raise ValueError("tal: dict(topk=, alpha=, beta=), only with det_loss='tal'")
            self.tal_kw.update(tal)
        self.mask_w = float(instance_mask_weight)
        if self.mask_w < 0:
            raise ValueError("instance_mask_weight must be >= 0")
        if mask_assign not in ("iou", "tal"):
            raise ValueError(f"mask_assign: 'iou' (the mask loss's own IoU match) or 'tal' (the task-aligned assignment), not {mask_assign!r}")
        if mask_assign == "tal" and (det_loss != "tal" or not self.mask_w > 0):
            raise ValueError("mask_assign='tal' needs det_loss='tal' and instance_mask_weight > 0")
        self.mask_assign = mask_assign
        if not hasattr(model, "detect"):
            raise NotImplementedError("ValidationStep drives the canonical model (running_main_v3.py needs .detect, SURVEY F4)")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("ValidationStep: the model must live on an MI355X (no CPU path)")
        self.m, self.dev, self.S = model, dev, int(img_size)
        self.projector = (projector if projector is not None else nn.Conv2d(model.proto_ch, 1, 1)).to(dev)
        self.nc_det, self.reg_max = model.nc_det, model.detect.reg_max
        self.loss_kw = dict(img_size=self.S, nc_det=self.nc_det, reg_max=self.reg_max, iou_match_thresh=iou_match_thresh,
                            label_smoothing=label_smoothing, training=False, weights=loss_weights)
        if det_loss == "tal":        # the detection terms come from the task-aligned operator: the reference's get weight 0
            w = tuple(float(v) for v in loss_weights)
            self.tal_w = w[1:4]
            self.loss_kw["weights"] = (w[0], 0.0, 0.0, 0.0, w[4])
        self.nms_kw = dict(conf_th=conf_th, iou_th=nms_iou, top_k=top_k)
        sync = dict(dist_sync=dist_sync, process_group=process_group)
        self.loss_names = LOSS_NAMES + ((MASK_LOSS_NAME,) if self.mask_w > 0 else ())
        self.losses = BatchWeightedMeans(len(self.loss_names), **sync)
        self.seg = SegmentationMetrics(**sync)
        self.img = ImageClassificationMetrics(model.nc_img, **sync)
        self.det_cm = DetectionConfusionMatrix(self.nc_det, self.S, iou_match_thresh, self.reg_max, **sync)
        max_dets = (1, 10, int(map_max_detections))
        self.map50 = DeviceMeanAveragePrecision([0.5], max_dets, **sync)
        self.map50_95 = DeviceMeanAveragePrecision(None, max_dets, **sync)
        self.instance_masks, self.mask_crop = bool(instance_masks), bool(mask_crop)
        self.mask_map50 = DeviceMaskMeanAveragePrecision([0.5], max_dets, **sync) if self.instance_masks else None
        self.mask_map50_95 = DeviceMaskMeanAveragePrecision(None, max_dets, **sync) if self.instance_masks else None
        self.surface = SurfaceDistanceMetrics(**self.surface_kw, **sync) if self.surface_kw is not None else None
        self.lesions = LesionMetrics(**self.lesion_kw, **sync) if self.lesion_kw is not None else None

    @staticmethod
    def _surface_options(surface):
        """`surface=` of the constructor -> None (off) or the keyword arguments of `SurfaceDistanceMetrics`."""
        if surface is None or surface is False:
            return None
        if surface is True:
            return {}
        allowed = ("quantile", "tolerance", "spacing", "percentile_mode", "undefined")
        if not isinstance(surface, dict) or set(surface) - set(allowed):
            raise ValueError(f"surface: None, True or a dict with keys among {allowed}, not {surface!r}")
        SurfaceDistanceMetrics(**surface)          # its own checks of the values; needs no device
        return dict(surface)

    @staticmethod
    def _lesion_options(lesions):
        """`lesions=` of the constructor -> None (off) or the keyword arguments of `LesionMetrics`."""
        if lesions is None or lesions is False:
            return None
        if lesions is True:
            return {}
        allowed = ("overlap", "min_area", "connectivity", "max_components")
        if not isinstance(lesions, dict) or set(lesions) - set(allowed):
            raise ValueError(f"lesions: None, True or a dict with keys among {allowed}, not {lesions!r}")
        LesionMetrics(**lesions)                   # its own checks of the values; needs no device
        return dict(lesions)

    def reset(self):
        for m in (self.losses, self.seg, self.img, self.det_cm, self.map50, self.map50_95, self.mask_map50, self.mask_map50_95, self.surface,
                  self.lesions):
            if m is not None:
                m.reset()

    def forward(self, x: torch.Tensor):
        """forward(x, "train") under no_grad with the module in eval mode, as Lightning runs `validation_step`: the backbone and neck use
        their running statistics while the heads -- which forward(mode="train") switches to train mode -- run on batch statistics (the
        reference's flag quirk; kept).  Every module's `.training` flag is restored afterwards."""
        flags = [(mod, mod.training) for mod in self.m.modules()]
        self.m.eval()
        try:
            with torch.no_grad():
                return self.m(x, "train")
        finally:
            for mod, f in flags:
                mod.training = f

    def step(self, imgs: torch.Tensor, det_gt: torch.Tensor, masks_gt: torch.Tensor, cls_gt: torch.Tensor):
        """One validation batch: imgs [B,3,S,S], det_gt [M,6] collated rows, masks_gt [B,1,S,S], cls_gt [B], all on the model's device.
        Returns the eval-mode loss tuple (total, seg, box, dfl, cls_det, img_cls) as 0-d device tensors; no host synchronisation.
        With `instance_mask_weight` > 0 two elements follow: mask_loss and its positive count.
        With `instance_masks`, masks_gt must be bool, uint8 or float32 (what `pack_masks` takes; anything else raises ValueError)."""
        if not all(t.is_cuda for t in (imgs, det_gt, masks_gt, cls_gt)):
            raise RuntimeError("ValidationStep.step: expected CUDA/HIP tensors on an MI355X (no CPU path)")
        B = imgs.shape[0]
        det, seg_out, logits = self.forward(imgs)
        protos = seg_out[2]
        pj = self.projector
        losses = multitask_loss(det, protos, logits, det_gt, masks_gt, cls_gt, pj.weight, pj.bias, **self.loss_kw)
        assigned = None
        if self.det_loss == "tal":
            r = task_aligned_det_loss(det, det_gt, img_size=self.S, nc_det=self.nc_det, reg_max=self.reg_max, weights=self.tal_w,
                                      want_assignment=self.mask_assign == "tal", **self.tal_kw)
            tal = r[0] if self.mask_assign == "tal" else r
            if self.mask_assign == "tal":
                assigned = r[1]
            wb, wd, wc = self.tal_w
            losses = (losses[0] + (wb * tal[0] + wd * tal[1] + wc * tal[2]), losses[1], tal[0], tal[1], tal[2], losses[5])
        if self.mask_w > 0:
            mask = instance_mask_loss(det, seg_out[1], protos, det_gt, masks_gt, img_size=self.S, reg_max=self.reg_max,
                                      iou_match_thresh=self.loss_kw["iou_match_thresh"], weight=self.mask_w, mc_layout="bnA", assigned=assigned)
            losses = (losses[0] + self.mask_w * mask[0],) + tuple(losses[1:]) + (mask[0], mask[1])
        self.losses.update(losses, B)
        if not self.seg_views:
            self._seg_update(proto_projector_logits(protos, pj.weight, pj.bias, self.S), masks_gt)
        self.img.update(logits, cls_gt)
        self.det_cm.update(det, det_gt)
        d = decode_boxes(det, self.S, reg_max=self.reg_max, want_scores=False)
        k = nms_batched(d["boxes"], d["best_score"], d["best_label"], float(self.S), **self.nms_kw)
        per_view = None
        if self.views is not None:
            per_view = [(k, (seg_out[1], protos)) if v == 0 else self._view_detections(imgs, v) for v in self.views]
        if self.seg_views:
            self._seg_update(self._view_seg_logits([s[1] for _, s in per_view]), masks_gt)
        sources = None
        if self.views is not None:
            vote = self.fused_masks is not None
            k = fuse_detections([d for d, _ in per_view], img_size=self.S, orients=self.views, iou_thr=self.wbf_iou, top_k=self.nms_kw["top_k"],
                                want_members=vote)
            sources = [s for _, s in per_view] if vote else None
        self.map50.update_batched(k, det_gt, self.S)
        self.map50_95.update_batched(k, det_gt, self.S)
        if self.instance_masks:
            self._mask_update(seg_out[1], protos, k, det_gt, masks_gt, sources)
        return losses

    def _seg_update(self, seg_logits, masks_gt):
        """The semantic mask's metrics, all from the same logits [B,1,S,S]."""
        self.seg.update(seg_logits, masks_gt)
        if self.surface is not None:
            self.surface.update(seg_logits, masks_gt)
        if self.lesions is not None:
            self.lesions.update(seg_logits, masks_gt)

    def _view_seg_logits(self, protos_per_view):
        """The projector logits averaged over the views, upright, [B,1,S,S]: `seg_to_frames` at identity frames, its dense output (the
        images are back to back in its buffer since S * S is a multiple of 4)."""
        S, B = self.S, protos_per_view[0].shape[0]
        r = seg_to_frames(list(protos_per_view), self.projector, [(S, S, 1.0)] * B, orients=self.views, logits=True,
                          up=S / protos_per_view[0].shape[3])
        return r["logits_buffer"][:B * S * S].view(B, 1, S, S) if (S * S) % 4 == 0 else torch.stack(r["logits"])[:, None]

    def _view_detections(self, imgs, view: int):
        """The detection list of one more view: `model(orient_batch(imgs, view), "infer")` with every module in eval mode (flags restored
        afterwards), decoded and filtered like the identity pass.  Boxes in the view's frame: `fuse_detections` turns them back.  Returns
        (the list, (mc, protos) of that pass, in the view's frame: what `vote_masks` takes)."""
        flags = [(mod, mod.training) for mod in self.m.modules()]
        self.m.eval()
        try:
            with torch.no_grad():
                out = self.m(orient_batch(imgs, view), "infer")
        finally:
            for mod, f in flags:
                mod.training = f
        d = decode_boxes(out["detect_features"], self.S, reg_max=self.reg_max, want_scores=False)
        return nms_batched(d["boxes"], d["best_score"], d["best_label"], float(self.S), **self.nms_kw), tuple(out["segment_protos"][1:3])

    def _mask_update(self, mc, protos, k, det_gt, masks_gt, sources=None):
        """The instance-mask mAP's share of a step: detections' masks and per-box ground truth as packed S x S planes, one pair-count
        pass for both threshold sets.  Device work only.  With `sources` ((mc, protos) per view) `k` is the fused list and its planes
        are voted."""
        S, B, K = self.S, protos.shape[0], k["scores"].shape[1]
        frames = [(S, S, 1.0)] * B
        if sources is not None:
            r = vote_masks(k, sources, self.views, None, frames, crop=self.mask_crop, up=S / protos.shape[3])
        else:
            r = masks_to_frames(protos, mc.float(), k["keep_anchor"], k["counts"], k["boxes"], frames, up=S / protos.shape[3], crop=self.mask_crop)
        pitch = r["masks"][0].shape[2]
        plane = K * S * pitch
        # masks_to_frames starts every image on a 16-byte boundary (`_frame_layout`): the images are back to back, and the buffer is one
        # [B, K, S, pitch] tensor, exactly when an image's K planes are a multiple of 16 bytes; otherwise the views are gathered
        det = r["buffer"][:B * plane].view(B, K, S, pitch) if plane % 16 == 0 else torch.stack(r["masks"])
        rows = det_gt.to(torch.float32)
        gt_image, _ = DeviceMaskMeanAveragePrecision.gt_rows_fields(rows, B)
        cx, cy, w, h = rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5]      # mtbt_box_eval's gt_format 0, one fp32 operation at a time
        px = torch.stack([(cx - w / 2) * S, (cy - h / 2) * S, (cx + w / 2) * S, (cy + h / 2) * S], 1).clamp_(0, S)
        gt = pack_masks(masks_gt[:, 0], boxes=px, plane_of=gt_image)
        tables = DeviceMaskMeanAveragePrecision.pair_tables_uniform(det, k["counts"], gt, gt_image)
        for m in (self.mask_map50_95, self.mask_map50):
            m.update_uniform(det, k["scores"], k["labels"], k["counts"], gt, rows, tables=tables)

    def compute(self) -> Dict[str, object]:
        """The epoch's numbers under the reference's log keys (running_main_v3.py:578-582, :605-729; evaluate_model.py:244-272 for the
        macro image scores), plus the alias `val_epoch_map_iou50/map` that the checkpoint callback monitors (:803).  Confusion matrices
        are row-normalised numpy arrays.  With a live process group: over every rank's batches (a collective, every rank must call it)."""
        out: Dict[str, object] = {}
        for name, v in zip(self.loss_names, self.losses.compute()):
            out[f"val_epoch/loss_{name}"] = float(v)
        img = self.img.compute()
        out["val_epoch/img_accuracy_epoch"] = img["accuracy"]
        out["val_epoch/img_confusion_matrix_epoch"] = img["confusion_matrix"]
        for k in ("precision", "recall", "f1"):
            out[f"val_epoch/img_{k}_macro"] = img[f"{k}_macro"]
        out["val_epoch/det_confusion_matrix_epoch"] = self.det_cm.compute()["confusion_matrix"]
        seg = self.seg.compute()
        for k in ("f1", "precision", "recall", "accuracy", "dice"):
            out[f"val_epoch/seg_{k}_epoch"] = seg[k]
        for k, v in self.seg.compute_map().items():
            out[f"val_epoch/seg_map_{k}"] = v
        for prefix, m in (("val_epoch/map_iou50_95", self.map50_95), ("val_epoch/map_iou50", self.map50)):
            for k, v in m.compute().items():
                out[f"{prefix}_{k}"] = v
        out["val_epoch_map_iou50/map"] = out["val_epoch/map_iou50_map"]
        if self.instance_masks:
            for prefix, m in (("val_epoch/mask_map_iou50_95", self.mask_map50_95), ("val_epoch/mask_map_iou50", self.mask_map50)):
                for k, v in m.compute().items():
                    out[f"{prefix}_{k}"] = v
        if self.surface is not None:
            sd = self.surface.compute()
            for k in ("hd", "hd95", "assd", "nsd"):
                out[f"val_epoch/seg_{k}_epoch"] = sd[k]
            out["val_epoch/seg_surface_undefined"] = sd["n_undefined"]
        if self.lesions is not None:
            lm = self.lesions.compute()
            for k in ("recall", "precision", "f1"):
                out[f"val_epoch/seg_lesion_{k}"] = lm[f"lesion_{k}"]
            out["val_epoch/seg_lesion_fp_per_image"] = lm["fp_per_image"]
        return out
