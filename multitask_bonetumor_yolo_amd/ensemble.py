"""Test-time augmentation and model ensembles: several passes over the same batch, merged by weighted boxes fusion on the device.

    from multitask_bonetumor_yolo_amd import detect_fused
    out = detect_fused([model, ema_model], images, 640, views=(0, 1), weights=(1.0, 2.0))   # 4 sources: model-major, then view
    map50.update_batched(out, det_gt, 640)                                                  # boxes / scores / labels / counts

A source is a (model, view) pair; a view is one of the eight dihedral codes of `mtbt_augment_batch` (bit 0 flips x, bit 1 flips y, bit 2
transposes).  Every source is `orient_batch` -> `model(x, "infer")` -> `detect_and_segment`; one `fuse_detections` launch merges them
(`mtbt_fuse_detections`, include/mtbt_hip.h).  Instance masks of the fused list are its leaders' (`masks=True`) or voted over every
cluster's members (`masks="vote"`, `mtbt_vote_masks`).  No host synchronisation.
"""
from typing import Optional, Sequence

import torch

from .postprocess import (CONF_TH, NMS_IOU, TOP_K, FUSE_MAX_SOURCES, assemble_masks, detect_and_segment, fuse_detections, orient_batch,
                          seg_to_frames, unorient_batch, unpack_masks, vote_masks)


def _leader_masks(fused, outs, views, S: int) -> torch.Tensor:
    """uint8 [B, top_k, S, S]: each fused slot's mask is its leader's, assembled against the leader's own source and turned upright.
    One `assemble_masks` call per source over the slots that source leads (compacted to the front of the row by a stable argsort, the
    padded rows cost nothing), scattered back through the inverse permutation."""
    ls, la = fused["lead_source"], fused["lead_anchor"]
    B, top_k = ls.shape
    rows = torch.arange(B, device=ls.device)[:, None]
    masks = torch.zeros((B, top_k, S, S), dtype=torch.uint8, device=ls.device)
    for m, (out, view) in enumerate(zip(outs, views)):
        led = ls == m
        order = torch.argsort((~led).to(torch.uint8), dim=1, stable=True)      # the slots m leads first, in slot order
        anchors = torch.where(led.gather(1, order), la.gather(1, order), torch.zeros_like(la))
        _, mc, protos = out["segment_protos"]
        planes, _ = assemble_masks(protos, mc.float(), anchors, led.sum(1, dtype=torch.int32), (S, S))
        planes = unorient_batch(planes.view(torch.uint8), view)
        masks |= planes[rows, torch.argsort(order, dim=1)]                      # rows past the count are zero: only m's slots change
    return masks


@torch.no_grad()
def detect_fused(models, images: torch.Tensor, img_size: int, *, views: Sequence[int] = (0,), weights: Optional[Sequence[float]] = None,
                 conf_th: float = CONF_TH, iou_th: float = NMS_IOU, top_k: int = TOP_K, wbf_iou: float = 0.55, skip_thr: float = 0.0,
                 masks=False, frames=None, crop: bool = False, semantic=None, seg_threshold: float = 0.0):
    """Detections of `images` [B,3,S,S] (S = img_size) fused over models x views.

    `models`: one eval-mode model or a list of them (the k models of a k-fold run; the raw and the EMA weights of a `TrainStep`).
    `views`: orient codes 0..7, each model sees every view.  Sources are ordered model-major and at most 8; source (i, v) carries
    `weights[i]` (default 1).  conf_th / iou_th / top_k: each source's NMS; wbf_iou / skip_thr / top_k: the fusion
    (`postprocess.fuse_detections`).  Returns its dict: boxes [B,top_k,4] in the upright frame, scores, labels, counts, n_clusters,
    n_members, lead_source, lead_slot, lead_anchor.

    `masks=True` adds `masks`, uint8 [B,top_k,S,S] in the upright frame: each fused detection's mask is its LEADER's (the highest-scoring
    member): the leader's coefficients against its own source's prototypes, turned back by the inverse of that source's view.  Transient
    memory: B * top_k * S^2 bytes per source on top of the result.

    `masks="vote"` votes instead (`postprocess.vote_masks`): the sign of the score-weighted mean of the MEMBERS' prototype-resolution
    logits, every source turned upright, so that the mask belongs to the same members as the averaged box.  The result gains
    `member_slot`, `vote_coeff` and, without `frames`, `masks` uint8 [B,top_k,S,S] (identity frames (S, S, 1.0), unpacked); with `frames`
    ([(H0, W0, scale)] per image, `frames_of`) it gains `boxes_frame` [B,top_k,4] and the bit-packed `masks_frame` instead, as
    `detect_and_segment` returns them, cropped to the fused boxes with `crop`.  `frames` / `crop` need `masks="vote"`.

    `semantic` (the trainer's `seg_proto_projector`: an nn.Conv2d(32, 1, 1) or (weight, bias), or a list of one per model) adds the
    SEMANTIC mask averaged over models x views with the sources' weights (`postprocess.seg_to_frames`): `seg_frame`, the bit-packed
    planes uint8 [1, H0, pitch] per image (logit > `seg_threshold`), and `seg_logits`, fp32 [H0, W0] per image -- in `frames` when
    given, else in identity frames (S, S, 1.0).  None: not one launch changes."""
    if masks not in (False, True, "vote"):
        raise ValueError(f"detect_fused: masks is False, True (the leaders' masks) or 'vote', not {masks!r}")
    vote = isinstance(masks, str)
    if (frames is not None and not vote and semantic is None) or (crop and not vote):
        raise ValueError("detect_fused: frames / crop come with masks='vote' (frames also with semantic=)")
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    views = [int(v) for v in views]
    weights = [1.0] * len(models) if weights is None else [float(w) for w in weights]
    if not models or not views or len(models) * len(views) > FUSE_MAX_SOURCES:
        raise ValueError(f"detect_fused: {len(models)} models x {len(views)} views (1..{FUSE_MAX_SOURCES} sources)")
    if len(weights) != len(models):
        raise ValueError(f"detect_fused: {len(weights)} weights for {len(models)} models")
    if not images.is_cuda:
        raise RuntimeError("detect_fused: expected a CUDA/HIP tensor on an MI355X (no CPU path)")
    S = int(img_size)
    outs, dets, src_views, src_weights = [], [], [], []
    for model, w in zip(models, weights):
        for v in views:
            out = model(orient_batch(images, v), "infer")
            if "detect_features" not in out:
                raise NotImplementedError("detect_fused drives models with a Detect head")
            _, mc, protos = out["segment_protos"]
            dets.append(detect_and_segment(out["detect_features"], mc, protos, S, conf_th, iou_th, top_k, masks=False))
            outs.append(out)
            src_views.append(v)
            src_weights.append(w)
    fused = fuse_detections(dets, img_size=S, orients=src_views, weights=src_weights, iou_thr=wbf_iou, skip_thr=skip_thr, top_k=top_k,
                            want_members=vote)
    if vote:
        B = images.shape[0]
        r = vote_masks(fused, outs, src_views, src_weights, [(S, S, 1.0)] * B if frames is None else frames, crop=crop,
                       up=S / outs[0]["segment_protos"][2].shape[3])
        fused["vote_coeff"] = r["vote_coeff"]
        if frames is None:
            fused["masks"] = torch.stack([unpack_masks(p, S) for p in r["masks"]]).view(torch.uint8)
        else:
            fused["boxes_frame"], fused["masks_frame"] = r["boxes"], r["masks"]
    elif masks:
        fused["masks"] = _leader_masks(fused, outs, src_views, S)
    if semantic is not None:
        if isinstance(semantic, list):
            if len(semantic) != len(models):
                raise ValueError(f"detect_fused: {len(semantic)} projectors for {len(models)} models")
            semantic = [pj for pj in semantic for _ in views]
        protos = [out["segment_protos"][2] for out in outs]
        r = seg_to_frames(protos, semantic, [(S, S, 1.0)] * images.shape[0] if frames is None else frames, orients=src_views,
                          weights=src_weights, threshold=seg_threshold, logits=True, up=S / protos[0].shape[3])
        fused["seg_frame"], fused["seg_logits"], fused["_seg"] = r["masks"], r["logits"], r
    return fused
