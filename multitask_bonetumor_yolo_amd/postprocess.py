"""Device post-process over the HIP kernels: box decode, per-image NMS, mask assembly, proto projector.

Mirrors what the reference's trainer does on the model outputs
(`/root/reference/src/running_main_v3.py:510-552`, `:251-257`; `/root/reference/src/test_model.py:80-85`),
batched on the GPU with no per-image Python loop and no host synchronisation.  No CPU path.
"""
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .planes import _need_cuda, plane_pitch
# the operators on packed planes live in planes.py; they stay importable from here
from .planes import (COMPONENTS_MAX_DIM, COMPONENTS_MAX_TABLE, D2_NONE, POLYGON_MAX_COORD, coco_segm_results, components_to_instances,  # noqa: F401
                     contour_polygons, count_contour_vertices, distance_transform, fill_polygons, filter_components, label_components,
                     labelme_shapes, measure_components, measure_detections, measure_regions, pack_masks, region_properties, rle_encode,
                     rle_from_string, rle_to_string, signed_distance, trace_contours, unpack_masks, yolo_seg_planes, yolo_seg_polygons,
                     yolo_seg_rows)

CONF_TH, NMS_IOU, TOP_K = 0.05, 0.6, 100  # running_main_v3.py:54-56


def _nhwc_rows(t: torch.Tensor):
    """[N,C,H,W] logical tensor -> (fp32 tensor whose memory is NHWC rows, pixel stride).  Zero-copy for the
    channels-last tensors the model returns; NCHW-contiguous input is re-laid out once (a torch copy)."""
    assert t.dim() == 4
    t = t.float() if t.dtype != torch.float32 else t
    n, c, h, w = t.shape
    if not (t.stride(1) == 1 and t.stride(2) == w * t.stride(3) and t.stride(0) == h * w * t.stride(3)):
        t = t.contiguous(memory_format=torch.channels_last)
    return t, t.stride(3)


def _proto_rows(protos: torch.Tensor) -> torch.Tensor:
    """[N,nm,hp,wp] prototypes -> the fp32 tensor the mask kernels read: dense NHWC rows, a pixel's nm channels side by side
    (`_nhwc_rows`, and one more copy when the channels-last tensor is a view with a wider pixel stride)."""
    pr, ld = _nhwc_rows(protos)
    if ld != protos.shape[1]:
        pr = pr.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return pr


def decode_boxes(det_maps: Sequence[torch.Tensor], img_size: Optional[float] = None, reg_max: int = 16, xywh: bool = False,
                 strides: Optional[Sequence[float]] = None, preds_cat: Optional[torch.Tensor] = None, want_scores: bool = True):
    """Decode raw Detect maps (per level [B, 4*reg_max+nc, h, w]).

    Trainer semantics (running_main_v3.py:510-533) by default: xyxy pixels with stride = img_size / w.
    `xywh=True` + explicit `strides` gives ultralytics `Detect._inference` (stride may be 0).
    Returns dict(boxes [B,A,4], scores [B,A,nc] sigmoid, best_score [B,A], best_label [B,A] int32)."""
    lib = L.load()
    maps = []
    for m in det_maps:
        _need_cuda(m, "decode_boxes")
        maps.append(_nhwc_rows(m))
    B, no = det_maps[0].shape[0], det_maps[0].shape[1]
    nc = no - 4 * reg_max
    dev = det_maps[0].device
    A = sum(m.shape[2] * m.shape[3] for m in det_maps)
    a = L.DecodeArgs()
    for i, ((t, ld), m) in enumerate(zip(maps, det_maps)):
        a.map[i] = t.data_ptr()
        a.h[i], a.w[i], a.map_pixel_stride[i] = m.shape[2], m.shape[3], ld
        a.stride[i] = float(strides[i]) if strides is not None else float(img_size) / m.shape[3]
    a.n_levels, a.N, a.nc, a.reg_max, a.xywh = len(maps), B, nc, reg_max, int(xywh)
    out = {}
    if preds_cat is None:
        out["boxes"] = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
        out["best_score"] = torch.empty((B, A), dtype=torch.float32, device=dev)
        out["best_label"] = torch.empty((B, A), dtype=torch.int32, device=dev)
        a.boxes, a.best_score, a.best_label = out["boxes"].data_ptr(), out["best_score"].data_ptr(), out["best_label"].data_ptr()
        if want_scores:
            out["scores"] = torch.empty((B, A, nc), dtype=torch.float32, device=dev)
            a.scores = out["scores"].data_ptr()
    else:
        assert preds_cat.is_contiguous() and preds_cat.shape[:2] == (B, A)
        a.preds_cat, a.cat_stride = preds_cat.data_ptr(), preds_cat.shape[2]
    L.check(lib.mtbt_decode_boxes(C.byref(a), L.stream(dev)), "mtbt_decode_boxes")
    out["_keep"] = maps
    return out


def detect_inference(maps, head, mc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ultralytics `Detect._inference` / `Segment.forward` eval output: [B, 4+nc(+nm), A] =
    cat(dist2bbox(dfl(box), anchors, xywh) * head.stride, sigmoid(cls)(, mask coefficients)).
    `maps`: engine.Act list (plan-owned raw maps); `mc`: [B,A,nm] buffer.  Returned as a [B,4+nc+nm,A] view of
    a fresh [B,A,4+nc+nm] buffer."""
    B = maps[0].N
    A = sum(m.H * m.W for m in maps)
    width = 4 + head.nc + (mc.shape[2] if mc is not None else 0)
    cat = torch.empty((B, A, width), dtype=torch.float32, device=maps[0].buf.device)
    decode_boxes([m.nchw() for m in maps], reg_max=head.reg_max, xywh=True, strides=[float(s) for s in head.stride], preds_cat=cat)
    if mc is not None:
        cat[:, :, 4 + head.nc:].copy_(mc)
    return cat.permute(0, 2, 1)


def batch_bbox_iou(boxes1: torch.Tensor, boxes2: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """running_main_v3.py:71-97: pairwise IoU [N,M] of xyxy boxes; an empty side gives the reference's zero matrix."""
    lib = L.load()
    _need_cuda(boxes1, "batch_bbox_iou")
    n, m = boxes1.shape[0], boxes2.shape[0]
    out = torch.zeros((n, m), dtype=torch.float32, device=boxes1.device)
    if n and m:
        b1, b2 = boxes1.contiguous().float(), boxes2.to(boxes1.device).contiguous().float()
        L.check(lib.mtbt_bbox_iou_pairwise(b1.data_ptr(), n, b2.data_ptr(), m, C.c_float(eps), out.data_ptr(), L.stream(boxes1.device)),
                "mtbt_bbox_iou_pairwise")
    return out


def nms_batched(boxes: torch.Tensor, best_score: torch.Tensor, best_label: Optional[torch.Tensor], clamp_max: float,
                conf_th: float = CONF_TH, iou_th: float = NMS_IOU, top_k: int = TOP_K):
    """running_main_v3.py:535-552 for the whole batch: score > conf_th, clamp to [0, clamp_max], greedy NMS
    (torchvision.ops.nms arithmetic and ordering), first top_k.  boxes [B,A,4] xyxy, best_score [B,A].
    Returns dict(keep_idx int64 [B,top_k] (index into the confidence-filtered list, -1 padded), keep_anchor int32,
    boxes [B,top_k,4], scores, labels int64, counts int32 [B], n_cand int32 [B])."""
    lib = L.load()
    _need_cuda(boxes, "nms_batched")
    boxes = boxes.contiguous().float()
    best_score = best_score.contiguous().float()
    B, A = best_score.shape
    dev = boxes.device
    if best_label is not None:
        best_label = best_label.contiguous().to(torch.int32)
    o = {
        "keep_idx": torch.empty((B, top_k), dtype=torch.int64, device=dev),
        "keep_anchor": torch.empty((B, top_k), dtype=torch.int32, device=dev),
        "boxes": torch.empty((B, top_k, 4), dtype=torch.float32, device=dev),
        "scores": torch.empty((B, top_k), dtype=torch.float32, device=dev),
        "labels": torch.empty((B, top_k), dtype=torch.int64, device=dev),
        "counts": torch.empty((B,), dtype=torch.int32, device=dev),
        "n_cand": torch.empty((B,), dtype=torch.int32, device=dev),
    }
    wsb = lib.mtbt_nms_workspace_bytes(B, A)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    rc = lib.mtbt_nms_batched(boxes.data_ptr(), best_score.data_ptr(), best_label.data_ptr() if best_label is not None else None,
                              B, A, conf_th, iou_th, clamp_max, top_k, o["keep_idx"].data_ptr(), o["keep_anchor"].data_ptr(),
                              o["boxes"].data_ptr(), o["scores"].data_ptr(), o["labels"].data_ptr(), o["counts"].data_ptr(),
                              o["n_cand"].data_ptr(), ws.data_ptr(), wsb, L.stream(dev))
    L.check(rc, "mtbt_nms_batched")
    o["_keep"] = (boxes, best_score, best_label, ws)
    return o


def _mask_call(protos, coeff, cbs, cks, ccs, gather, counts, bias, K, out_hw, want_logits, want_masks):
    lib = L.load()
    _need_cuda(protos, "mask assembly")
    pr = _proto_rows(protos)
    B, nm, hp, wp = protos.shape
    dev = protos.device
    H, W = out_hw
    a = L.MaskArgs()
    a.protos, a.coeff = pr.data_ptr(), coeff.data_ptr()
    a.coeff_batch_stride, a.coeff_k_stride, a.coeff_c_stride = cbs, cks, ccs
    a.gather_idx = gather.data_ptr() if gather is not None else None
    a.counts = counts.data_ptr() if counts is not None else None
    a.bias = float(bias)
    a.N, a.K, a.nm, a.hp, a.wp, a.Hout, a.Wout = B, K, nm, hp, wp, H, W
    logits = torch.empty((B, K, H, W), dtype=torch.float32, device=dev) if want_logits else None
    masks = torch.empty((B, K, H, W), dtype=torch.bool, device=dev) if want_masks else None
    a.logits = logits.data_ptr() if logits is not None else None
    a.masks = masks.data_ptr() if masks is not None else None
    L.check(lib.mtbt_mask_assemble(C.byref(a), L.stream(dev)), "mtbt_mask_assemble")
    return logits, masks


def assemble_masks(protos: torch.Tensor, mc: torch.Tensor, keep_anchor: torch.Tensor, counts: Optional[torch.Tensor],
                   out_size, want_logits: bool = False):
    """Instance masks of the kept boxes (test_model.py:80-85 intended form): masks[b,k] =
    sigmoid(bilinear(sum_c mc[b,c,anchor(b,k)] * protos[b,c])) > 0.5.
    protos [B,nm,hp,wp]; mc [B,nm,A] (any strides, fp32); keep_anchor int32 [B,K]; counts int32 [B] or None.
    Rows k >= counts[b] are zero.  Returns (masks bool [B,K,H,W], logits or None)."""
    assert mc.dtype == torch.float32
    keep_anchor = keep_anchor.contiguous().to(torch.int32)
    if counts is not None:
        counts = counts.contiguous().to(torch.int32)
    logits, masks = _mask_call(protos, mc, mc.stride(0), mc.stride(2), mc.stride(1), keep_anchor, counts, 0.0,
                               keep_anchor.shape[1], tuple(out_size), want_logits, True)
    return masks, logits


def proto_projector_logits(protos: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, img_size: int) -> torch.Tensor:
    """Trainer's seg_proto_projector path (running_main_v3.py:186, :251-255): Conv2d(nm,1,1)(protos) then bilinear
    to img_size.  Returns logits [B,1,S,S] fp32."""
    w = weight.detach().reshape(-1).float().contiguous()
    logits, _ = _mask_call(protos, w, 0, 0, 1, None, None, 0.0, 1, (img_size, img_size), True, False)
    return logits.add_(bias.detach().reshape(1, 1, 1, 1).to(logits.dtype))      # device-side add: no host synchronisation (bilinear weights sum to 1)


MAX_FRAMES = 32   # images per mtbt_masks_to_frames launch (the frame descriptors travel as kernel arguments)


def frames_of(images: Sequence[torch.Tensor], scales: Sequence[float]):
    """The frames of the raw images `letterbox_batch` was given: [(H0, W0, scale)] with the scales it returned."""
    return [(int(im.shape[0]), int(im.shape[1]), float(s)) for im, s in zip(images, scales)]


def _frame_layout(frames, K: int, up: float):
    """Per image (H0, W0, step, scale, pitch, offset) and the byte size of the packed buffer."""
    rows, total = [], 0
    for H0, W0, scale in frames:
        H0, W0, scale = int(H0), int(W0), float(scale)
        step = C.c_float(scale / up).value if scale > 0 else 0.0
        if H0 < 1 or W0 < 1 or not 0.0 < step <= 1.0:
            raise ValueError(f"masks_to_frames: frame ({H0}, {W0}, scale {scale}) gives {step} prototype pixels per image pixel; the supported "
                             "range is 0 < scale / up <= 1, i.e. the image's long side is at least the prototype grid's (>= 160 px at S = 640)")
        pitch = plane_pitch(W0)
        rows.append((H0, W0, step, C.c_float(scale).value, pitch, total))
        total = (total + K * H0 * pitch + 15) // 16 * 16
    return rows, total


class _PackedFrames:
    """The packed buffer of one call of a frame operator `who` (K planes per image): its layout (`_frame_layout`), the checked or new
    `out`, the launches of at most MAX_FRAMES images with their `mtbt_frame` arrays, and the views that are returned."""

    def __init__(self, who: str, frames, K: int, up: float, out: Optional[torch.Tensor], dev):
        self.K = K
        self.rows, total = _frame_layout(frames, K, up)
        if out is None:
            out = torch.empty((total,), dtype=torch.uint8, device=dev)
        elif out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() < total or out.device != dev:
            raise ValueError(f"{who}: out must be a contiguous flat uint8 buffer of at least {total} bytes on {dev}")
        self.out = out

    def chunks(self):
        """(c0, nb, `mtbt_frame` array) of every launch: images c0 .. c0 + nb - 1."""
        for c0 in range(0, len(self.rows), MAX_FRAMES):
            rows = self.rows[c0:c0 + MAX_FRAMES]
            fr = (L.Frame * len(rows))()
            for i, (H0, W0, step, scale, pitch, off) in enumerate(rows):
                fr[i].height, fr[i].width, fr[i].step, fr[i].scale, fr[i].pitch, fr[i].offset = H0, W0, step, scale, pitch, off
            yield c0, len(rows), fr

    def views(self):
        return [self.out[off:off + self.K * H0 * pitch].view(self.K, H0, pitch) for H0, W0, step, scale, pitch, off in self.rows]


def masks_to_frames(protos: torch.Tensor, mc: torch.Tensor, keep_anchor: torch.Tensor, counts: Optional[torch.Tensor],
                    boxes: Optional[torch.Tensor], frames, up: Optional[float] = None, crop: bool = False, out: Optional[torch.Tensor] = None):
    """Kept boxes and their instance masks in the coordinates of the ORIGINAL images, masks one bit per pixel.

    `frames`: one (H0, W0, scale) per image, scale = S / max(H0, W0) as `letterbox_batch` returns it (see `frames_of`); images keep
    their own sizes.  `up` = letterboxed pixels per prototype pixel (S / wp; 4 when not given).  Supported range: 0 < scale / up <= 1
    (the image's long side is at least the prototype grid's, e.g. >= 160 px at S = 640); anything else raises ValueError.
    protos / mc / keep_anchor / counts as in `assemble_masks`; boxes [B,K,4] letterboxed xyxy (the NMS output).

      boxes[b,k]  = clamp(boxes[b,k] / float32(scale_b), 0, (W0, H0, W0, H0)); rows k >= counts[b] are zeros
      mask bit    = bilinear tap of the prototype-resolution logits at the original pixel (align_corners=False, one step, no S x S
                    plane) > 0; with `crop` also x1 <= X < x2 and y1 <= Y < y2 of the frame box (ultralytics crop_mask)

    Returns {"boxes": [B,K,4], "masks": list of uint8 [K, H0_b, pitch_b] views, "buffer": the flat uint8 buffer they view}.
    pitch_b = 8 * ceil(W0_b / 64) bytes; pixel X is bit X & 7 of byte X >> 3 (numpy.packbits(bitorder="little")); padding bits and
    planes k >= counts[b] are zero; every byte is written by the kernel.  Image b takes K * H0_b * pitch_b bytes (16-byte aligned
    starts): a 3000 x 3000 image at K = 100 is 113 MB, so lower `top_k` for large images.  `out=` takes a caller's flat uint8 buffer
    of at least that total.  `unpack_masks` gives bool planes."""
    lib = L.load()
    _need_cuda(protos, "masks_to_frames")
    assert mc.dtype == torch.float32
    pr = _proto_rows(protos)
    B, nm, hp, wp = protos.shape
    dev = protos.device
    keep_anchor = keep_anchor.contiguous().to(torch.int32)
    K = keep_anchor.shape[1]
    if len(frames) != B:
        raise ValueError(f"masks_to_frames: {len(frames)} frames for a batch of {B}")
    if crop and boxes is None:
        raise ValueError("masks_to_frames: crop=True needs the boxes")
    packed = _PackedFrames("masks_to_frames", frames, K, 4.0 if up is None else float(up), out, dev)
    out = packed.out
    if counts is not None:
        counts = counts.contiguous().to(torch.int32)
    boxes_frame = None
    if boxes is not None:
        boxes = boxes.contiguous().float()
        boxes_frame = torch.empty((B, K, 4), dtype=torch.float32, device=dev)
    for c0, nb, fr in packed.chunks():
        a = L.FrameMaskArgs()
        a.protos, a.coeff = pr[c0:].data_ptr(), mc[c0:].data_ptr()
        a.coeff_batch_stride, a.coeff_k_stride, a.coeff_c_stride = mc.stride(0), mc.stride(2), mc.stride(1)
        a.gather_idx = keep_anchor[c0:].data_ptr()
        a.counts = counts[c0:].data_ptr() if counts is not None else None
        a.boxes = boxes[c0:].data_ptr() if boxes is not None else None
        a.boxes_frame = boxes_frame[c0:].data_ptr() if boxes_frame is not None else None
        a.out, a.out_bytes = out.data_ptr(), out.numel()
        a.N, a.K, a.nm, a.hp, a.wp, a.crop = nb, K, nm, hp, wp, int(bool(crop))
        rc = lib.mtbt_masks_to_frames(C.byref(a), fr, nb, L.stream(dev))
        if rc == -1 and nm != 32:
            raise ValueError(f"masks_to_frames: {nm} prototype channels; the kernel supports 32")
        L.check(rc, "mtbt_masks_to_frames")
    return {"boxes": boxes_frame, "masks": packed.views(), "buffer": out}


def detect_and_segment(det_maps: List[torch.Tensor], mc: torch.Tensor, protos: torch.Tensor, img_size: int,
                       conf_th: float = CONF_TH, iou_th: float = NMS_IOU, top_k: int = TOP_K, masks: bool = True,
                       frames=None, crop: bool = False):
    """The whole validation post-process for a batch: decode -> filter/NMS/top-k -> instance masks.
    With `frames` ([(H0, W0, scale)] per image, see `frames_of`) the results come in the original images' coordinates instead of
    the dense letterboxed masks: `boxes_frame` [B,K,4] and `masks_frame` (bit-packed uint8 [K, H0_b, pitch_b] per image, cropped to
    the boxes with `crop`), as `masks_to_frames` documents them."""
    d = decode_boxes(det_maps, img_size, want_scores=False)
    k = nms_batched(d["boxes"], d["best_score"], d["best_label"], float(img_size), conf_th, iou_th, top_k)
    out = {"boxes": k["boxes"], "scores": k["scores"], "labels": k["labels"], "counts": k["counts"],
           "keep_idx": k["keep_idx"], "keep_anchor": k["keep_anchor"], "n_cand": k["n_cand"]}
    if frames is not None:
        r = masks_to_frames(protos, mc, k["keep_anchor"], k["counts"], k["boxes"], frames, up=img_size / protos.shape[3], crop=crop)
        out["boxes_frame"], out["masks_frame"] = r["boxes"], r["masks"]
    elif masks:
        out["masks"], _ = assemble_masks(protos, mc, k["keep_anchor"], k["counts"], (img_size, img_size))
    return out


FUSE_MAX_SOURCES, FUSE_MAX_CANDIDATES = 8, 4096   # include/mtbt_hip.h MTBT_FUSE_MAX_SOURCES / MTBT_FUSE_MAX_CANDIDATES


def _det_tensors(d: dict, with_anchor: bool):
    """[boxes, scores, labels, counts(, keep_anchor)] of a detection dict, typed and contiguous as the fusion and merge kernels read them."""
    src = [d["boxes"].contiguous().float(), d["scores"].contiguous().float(), d["labels"].contiguous().to(torch.int64),
           d["counts"].contiguous().to(torch.int32)]
    if with_anchor:
        src.append(d["keep_anchor"].contiguous().to(torch.int32))
    return src


def _row_tensors(a, N: int, top_k: int, dev, boxes: str, lead: str, with_anchor: bool) -> dict:
    """The padded output rows that the fusion and merge kernels write, [N, top_k] each, under the caller's names for the boxes and for
    the leader's list (`lead`: also the struct's field); their pointers go into the argument struct `a`."""
    i32 = {"dtype": torch.int32, "device": dev}
    o = {
        boxes: torch.empty((N, top_k, 4), dtype=torch.float32, device=dev),
        "scores": torch.empty((N, top_k), dtype=torch.float32, device=dev),
        "labels": torch.empty((N, top_k), dtype=torch.int64, device=dev),
        "counts": torch.empty((N,), **i32),
        "n_members": torch.empty((N, top_k), **i32),
        lead: torch.empty((N, top_k), **i32),
        "lead_slot": torch.empty((N, top_k), **i32),
    }
    if with_anchor:
        o["lead_anchor"] = torch.empty((N, top_k), **i32)
    field = {boxes: "out_boxes", "scores": "out_scores", "labels": "out_labels", "counts": "out_counts"}
    for key, t in o.items():
        setattr(a, field.get(key, key), t.data_ptr())
    return o


def _per_source(who: str, M: int, orients, weights, codes: Optional[range] = None):
    """`orients` / `weights` of M sources with their defaults (0 / 1), as lists of M.  With `codes` every orient must be one of them
    (without, the library refuses a bad one)."""
    orients = [0] * M if orients is None else [int(o) for o in orients]
    weights = [1.0] * M if weights is None else [float(w) for w in weights]
    if len(orients) != M or len(weights) != M or (codes is not None and any(o not in codes for o in orients)):
        note = "" if codes is None else f" ({codes[0]}..{codes[-1]})"
        raise ValueError(f"{who}: {len(orients)} orients{note} and {len(weights)} weights for {M} sources")
    return orients, weights


def _fuse_args(dets, img_size, orients, weights, iou_thr, skip_thr, top_k):
    """The checked `mtbt_box_fuse_args` of a `fuse_detections` call, its output dict (which keeps every tensor the struct points to
    alive under "_keep") and the device."""
    lib = L.load()
    dets = list(dets)
    M = len(dets)
    if not 1 <= M <= FUSE_MAX_SOURCES:
        raise ValueError(f"fuse_detections: {M} sources (1..{FUSE_MAX_SOURCES})")
    for d in dets:
        for key in ("boxes", "scores", "labels", "counts"):
            _need_cuda(d[key], "fuse_detections")
    B, K = dets[0]["scores"].shape
    dev = dets[0]["scores"].device
    for m, d in enumerate(dets):
        if tuple(d["scores"].shape) != (B, K) or tuple(d["boxes"].shape) != (B, K, 4) or tuple(d["labels"].shape) != (B, K) or tuple(d["counts"].shape) != (B,):
            raise ValueError(f"fuse_detections: source {m} has boxes {tuple(d['boxes'].shape)}, scores {tuple(d['scores'].shape)}, counts "
                             f"{tuple(d['counts'].shape)}; source 0 has B = {B}, K = {K}")
    if K < 1 or M * K > FUSE_MAX_CANDIDATES:
        raise ValueError(f"fuse_detections: {M} sources of K = {K} slots ({FUSE_MAX_CANDIDATES} slots at most, K >= 1)")
    orients, weights = _per_source("fuse_detections", M, orients, weights)
    top_k = K if top_k is None else int(top_k)
    with_anchor = all("keep_anchor" in d for d in dets)
    a = L.BoxFuseArgs()
    keep = []
    for m, d in enumerate(dets):
        src = _det_tensors(d, with_anchor)
        if with_anchor:
            a.anchors[m] = src[4].data_ptr()
        a.boxes[m], a.scores[m], a.labels[m], a.counts[m] = (t.data_ptr() for t in src[:4])
        a.orient[m], a.weight[m] = orients[m], weights[m]
        keep.append(src)
    o = _row_tensors(a, B, top_k, dev, "boxes", "lead_source", with_anchor)
    o["n_clusters"] = torch.empty((B,), dtype=torch.int32, device=dev)
    ws, wsb = L.workspace(lib.mtbt_fuse_workspace_bytes, M, B, K, device=dev, what="mtbt_fuse_workspace_bytes")
    a.n_sources, a.N, a.K, a.top_k = M, B, K, top_k
    a.img_size, a.iou_thr, a.skip_thr = float(img_size), float(iou_thr), float(skip_thr)
    a.n_clusters, a.workspace, a.workspace_bytes = o["n_clusters"].data_ptr(), ws.data_ptr(), wsb
    o["_keep"] = (keep, ws)
    return a, o, dev


def fuse_detections(dets: Sequence[dict], *, img_size: float, orients: Optional[Sequence[int]] = None,
                    weights: Optional[Sequence[float]] = None, iou_thr: float = 0.55, skip_thr: float = 0.0, top_k: Optional[int] = None,
                    want_members: bool = False):
    """Weighted boxes fusion (`mtbt_fuse_detections`) of several detection lists of the same batch: the views of test-time
    augmentation, the models of an ensemble.  One launch, no host synchronisation, deterministic.

    `dets`: 1..8 result dicts of `nms_batched` / `detect_and_segment` (boxes [B,K,4], scores, labels, counts; the same B and K, at most
    4096 slots together).  `orients[m]`: the dihedral code of the view source m saw (`orient_batch`; bit 0 flips x, bit 1 flips y, bit 2
    transposes; default 0), its boxes are turned back to the upright `img_size` frame.  `weights[m]` > 0 scales its scores (default 1).
    Candidates with score * weight <= skip_thr are dropped; a candidate joins the same-label cluster whose fused box it overlaps most when
    that IoU > iou_thr, else it opens a cluster; a cluster's box is the score-weighted mean of its members and its score
    mean(member scores) * min(members, sources) / sum(weights).  `top_k` defaults to K.

    Returns dict(boxes [B,top_k,4], scores, labels int64, counts int32 [B] -- what `update_batched` and the mask-mAP classes read --,
    n_clusters int32 [B] (before the cut), n_members int32 [B,top_k], lead_source / lead_slot int32 [B,top_k] (source and slot of each
    cluster's highest-scoring member, -1 padded) and, when every input has `keep_anchor`, lead_anchor int32 [B,top_k]).

    `want_members=True` (`mtbt_fuse_detections_members`: the same launch, every other entry bit-identical) adds `member_slot` int32
    [B, M*K]: for slot k of source m, at m * K + k, the output row of the cluster it opened or joined; -1 for a slot that was no candidate
    and for a member of a cluster that `top_k` cut.  `vote_masks` reads it."""
    a, o, dev = _fuse_args(dets, img_size, orients, weights, iou_thr, skip_thr, top_k)
    with torch.cuda.device(dev):
        if want_members:
            o["member_slot"] = torch.empty((a.N, a.n_sources * a.K), dtype=torch.int32, device=dev)
            L.check(L.load().mtbt_fuse_detections_members(C.byref(a), o["member_slot"].data_ptr(), L.stream(dev)), "mtbt_fuse_detections_members")
        else:
            L.check(L.load().mtbt_fuse_detections(C.byref(a), L.stream(dev)), "mtbt_fuse_detections")
    return o


def vote_masks(fused: dict, sources: Sequence, orients: Optional[Sequence[int]], weights: Optional[Sequence[float]], frames,
               crop: bool = False, out: Optional[torch.Tensor] = None, up: Optional[float] = None):
    """Instance masks of fused detections, voted over the members of each cluster (`mtbt_vote_masks`): the sign of the score-weighted
    mean of the members' prototype-resolution logits, every source turned upright first, sampled at the pixels of `frames`.

    `fused`: the result of `fuse_detections(dets, ..., want_members=True)` of detection lists that carry `keep_anchor`.  `sources[m]`:
    source m's model output (a dict with `segment_protos`) or its `(mc, protos)` pair -- mc [B,32,A] fp32, protos [B,32,G,G] in the frame
    of the view that source saw.  `orients` / `weights`: the ones the fusion was given (None: 0 / 1).  `frames`, `up`, `crop`, `out` and the
    packed layout: as in `masks_to_frames`, with the fused boxes and `top_k` planes per image.

      W[b,r,m,:] = sum over source m's members of row r of (score * weight_m) * coefficients, divided by the row's sum of score * weight
      mask bit   = bilinear tap of sum_m W[b,r,m,:] . upright protos_m at the frame pixel > 0 (and inside the fused frame box with `crop`)

    One coefficient row per (fused row, source) instead of one mask per member: the vote is linear up to the sign.  Returns what
    `masks_to_frames` returns ("boxes" [B,top_k,4] in the frames, "masks" views, "buffer") plus "vote_coeff" (W, float32 [B,top_k,M,32])
    and "vote_weight" (the rows' sums, float32 [B,top_k]).  No host synchronisation."""
    lib = L.load()
    if "member_slot" not in fused:
        raise ValueError("vote_masks: `fused` has no member_slot; call fuse_detections(..., want_members=True)")
    srcs = fused["_keep"][0]
    M = len(srcs)
    if len(sources) != M or any(len(s) < 5 for s in srcs):
        raise ValueError(f"vote_masks: {len(sources)} sources for a fusion of {M}, each of which must carry keep_anchor")
    orients, weights = _per_source("vote_masks", M, orients, weights, codes=range(8))
    member_slot, counts, boxes = fused["member_slot"], fused["counts"], fused["boxes"]
    _need_cuda(member_slot, "vote_masks")
    dev = member_slot.device
    B, top_k = fused["scores"].shape
    K = srcs[0][1].shape[1]
    if len(frames) != B:
        raise ValueError(f"vote_masks: {len(frames)} frames for a batch of {B}")
    keep = []
    for m, src in enumerate(sources):
        mc, protos = src["segment_protos"][1:3] if isinstance(src, dict) else src
        _need_cuda(protos, "vote_masks")
        pr = _proto_rows(protos)
        nm, hp, wp = protos.shape[1:]
        mc = mc.float()
        if protos.shape[0] != B or mc.shape[0] != B or mc.shape[1] != nm or nm != 32 or hp != wp or (keep and (hp, wp) != tuple(keep[0][0].shape[2:])):
            raise ValueError(f"vote_masks: source {m} has protos {tuple(protos.shape)} and mc {tuple(mc.shape)}; expected [{B}, 32, G, G] and "
                             f"[{B}, 32, A] with the same square G for every source")
        keep.append((pr, mc))
    G = keep[0][0].shape[2]
    packed = _PackedFrames("vote_masks", frames, top_k, 4.0 if up is None else float(up), out, dev)
    out = packed.out
    boxes = boxes.contiguous().float()
    boxes_frame = torch.empty((B, top_k, 4), dtype=torch.float32, device=dev)
    W = torch.empty((B, top_k, M, 32), dtype=torch.float32, device=dev)
    Ss = torch.empty((B, top_k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for c0, nb, fr in packed.chunks():
            a = L.VoteMaskArgs()
            for m, ((pr, mc), src) in enumerate(zip(keep, srcs)):
                a.protos[m], a.mc[m] = pr[c0:].data_ptr(), mc[c0:].data_ptr()
                a.mc_batch_stride[m], a.mc_k_stride[m], a.mc_c_stride[m] = mc.stride(0), mc.stride(2), mc.stride(1)
                a.scores[m], a.anchors[m] = src[1][c0:].data_ptr(), src[4][c0:].data_ptr()
                a.weight[m], a.orient[m] = weights[m], orients[m]
            a.member_slot, a.counts = member_slot[c0:].data_ptr(), counts[c0:].data_ptr()
            a.boxes, a.boxes_frame = boxes[c0:].data_ptr(), boxes_frame[c0:].data_ptr()
            a.W, a.Ss = W[c0:].data_ptr(), Ss[c0:].data_ptr()
            a.out, a.out_bytes = out.data_ptr(), out.numel()
            a.n_sources, a.N, a.K, a.top_k, a.nm, a.hp, a.wp, a.crop = M, nb, K, top_k, 32, G, G, int(bool(crop))
            L.check(lib.mtbt_vote_masks(C.byref(a), fr, nb, L.stream(dev)), "mtbt_vote_masks")
    return {"boxes": boxes_frame, "masks": packed.views(), "buffer": out, "vote_coeff": W, "vote_weight": Ss}


def _square(x: torch.Tensor, orient: int, what: str):
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError(f"{what}: expected [B, C, S, S] (square views only), got {tuple(x.shape)}")
    if not 0 <= int(orient) <= 7:
        raise ValueError(f"{what}: orient {orient} outside 0..7")


def orient_batch(x: torch.Tensor, orient: int) -> torch.Tensor:
    """The view Q of a [B, C, S, S] batch under one of the eight dihedral codes, by the pixel rule of `mtbt_augment_batch`:
    Q = flips(transpose(x)) -- the last two dimensions transposed if bit 2 is set, then x flipped if bit 0, then y flipped if bit 1.
    Plain torch indexing (not a hot path)."""
    _square(x, orient, "orient_batch")
    q = x.transpose(2, 3) if orient & 4 else x
    dims = [d for bit, d in ((1, 3), (2, 2)) if orient & bit]
    if dims:
        q = q.flip(dims)
    return q.contiguous()


def unorient_batch(q: torch.Tensor, orient: int) -> torch.Tensor:
    """The inverse of `orient_batch`, e.g. for dense [B, K, S, S] masks of a view: the flips undone, then the transpose."""
    _square(q, orient, "unorient_batch")
    dims = [d for bit, d in ((1, 3), (2, 2)) if orient & bit]
    x = q.flip(dims) if dims else q
    return (x.transpose(2, 3) if orient & 4 else x).contiguous()


# ---- sliced inference: merge the detection lists of an image's tiles, vote the masks across them (include/mtbt_hip.h `mtbt_tile`) ----
TILE_MAX_PER_IMAGE = 64
MERGE_METRICS = {"iou": 0, "ios": 1}
_TILE_FIELDS = ("image", "pox", "poy", "wx0", "wy0", "wx1", "wy1", "height", "width", "step", "scale", "fox", "foy")


def tile_table(tiles: Sequence[Sequence[dict]], dev=None):
    """`slice_geometry`'s per-image tile lists -> (host `mtbt_tile` array [NT], `first` int32 [N+1] (ctypes), device copy of the array
    (uint8 tensor, or None without `dev`))."""
    flat = [t for per in tiles for t in per]
    table = (L.Tile * max(len(flat), 1))()
    for d, t in zip(table, flat):
        for k in _TILE_FIELDS:
            setattr(d, k, t[k])
    first = (C.c_int32 * (len(tiles) + 1))()
    for n, per in enumerate(tiles):
        first[n + 1] = first[n] + len(per)
    dev_copy = None
    if dev is not None:
        dev_copy = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    return table, first, dev_copy


def merge_tiles(det: dict, tiles: Sequence[Sequence[dict]], frames, *, metric: str = "ios", thr: float = 0.5, skip_thr: float = 0.0,
                top_k: int = TOP_K, class_agnostic: bool = False):
    """The detection lists of an image's tiles merged in the image's own pixel frame (`mtbt_merge_tiles`): one launch, one workgroup per
    image, no host synchronisation, deterministic.

    `det`: the result of `nms_batched` / `detect_and_segment` over the NT tile canvases of `slice_batch` (boxes [NT,K,4] in each tile's
    canvas, scores, labels, counts and, for masks, keep_anchor).  `tiles`: `slice_geometry`'s lists.  `frames`: one (H0, W0, ...) per image.
    A candidate (score > skip_thr) is moved to the frame, clamp((v + tile offset) / tile scale, 0, (W0, H0)); in descending score a
    candidate that is still free opens a row and absorbs every later free candidate of its label (any label with `class_agnostic`) whose
    `metric` with the leader's own box exceeds `thr`: "ios" = intersection over the smaller area (a part cut by a tile border is absorbed
    by the whole), "iou" = the NMS overlap.  A row's box is the union of its members', its score and label the leader's; at most top_k rows.

    Returns dict(boxes_frame [N,top_k,4] (also under "boxes"), scores, labels int64, counts int32 [N], n_members, lead_tile (index into
    the flat tile table), lead_slot, lead_anchor (with keep_anchor), member_slot int32 [NT,K] (the row a slot opened or joined, else -1),
    n_left int32 [N] (candidates that were still free when top_k rows were full), tiles)."""
    lib = L.load()
    if metric not in MERGE_METRICS:
        raise ValueError(f"merge_tiles: metric {metric!r} (one of {sorted(MERGE_METRICS)})")
    for key in ("boxes", "scores", "labels", "counts"):
        _need_cuda(det[key], "merge_tiles")
    NT, K = det["scores"].shape
    N = len(tiles)
    dev = det["scores"].device
    if len(frames) != N or sum(len(per) for per in tiles) != NT:
        raise ValueError(f"merge_tiles: {len(frames)} frames and {sum(len(per) for per in tiles)} tiles for {N} images and {NT} detection lists")
    for n, (per, fr) in enumerate(zip(tiles, frames)):
        if len(per) > TILE_MAX_PER_IMAGE or len(per) * K > FUSE_MAX_CANDIDATES or any((t["height"], t["width"]) != (int(fr[0]), int(fr[1])) for t in per):
            raise ValueError(f"merge_tiles: image {n} has {len(per)} tiles of K = {K} slots ({TILE_MAX_PER_IMAGE} tiles and {FUSE_MAX_CANDIDATES} slots "
                             f"at most), all of them of its frame {tuple(fr[:2])}")
    top_k = int(top_k)
    table, first, table_dev = tile_table(tiles, dev)
    src = _det_tensors(det, "keep_anchor" in det)
    a = L.TileMergeArgs()
    o = _row_tensors(a, N, top_k, dev, "boxes_frame", "lead_tile", "keep_anchor" in det)
    o["member_slot"] = torch.empty((NT, K), dtype=torch.int32, device=dev)
    o["n_left"] = torch.empty((N,), dtype=torch.int32, device=dev)
    a.boxes, a.scores, a.labels, a.counts = (t.data_ptr() for t in src[:4])
    if "keep_anchor" in det:
        a.anchors = src[4].data_ptr()
    a.tiles, a.tiles_dev, a.first = table, table_dev.data_ptr(), first
    a.N, a.n_tiles, a.K, a.top_k = N, NT, K, top_k
    a.metric, a.class_agnostic, a.thr, a.skip_thr = MERGE_METRICS[metric], int(bool(class_agnostic)), float(thr), float(skip_thr)
    a.member_slot, a.n_left = o["member_slot"].data_ptr(), o["n_left"].data_ptr()
    with torch.cuda.device(dev):
        L.check(lib.mtbt_merge_tiles(C.byref(a), L.stream(dev)), "mtbt_merge_tiles")
    o["boxes"] = o["boxes_frame"]
    o["tiles"] = tiles
    o["_keep"] = (src, table, first, table_dev)
    return o


def vote_tile_masks(merged: dict, det: dict, mc: torch.Tensor, protos: torch.Tensor, tiles: Sequence[Sequence[dict]], frames,
                    crop: bool = False, out: Optional[torch.Tensor] = None):
    """Instance masks of merged rows, voted across the tiles of their members straight into the bit-packed frame planes
    (`mtbt_vote_tile_masks`).  `merged`: the result of `merge_tiles(det, tiles, frames)` of a `det` with keep_anchor; mc [NT,32,A] fp32
    and protos [NT,32,G,G] are the tiles' mask coefficients and prototypes, tile-major as `det`.

      W[n,r,t,:] = sum over row r's members in tile t of score * coefficients, divided by the row's sum of scores
      mask bit   = sum over the tiles with a window over the pixel, ascending, of the bilinear tap of W[n,r,t,:] . protos_t at the
                   pixel's place in that tile > 0 (and inside the merged box with `crop`); pixels no member tile sees are 0

    Returns what `masks_to_frames` returns ("boxes": the merged frame boxes, "masks": uint8 [top_k, H0_n, pitch_n] views, "buffer") plus
    "vote_coeff" (W, float32 [N,top_k,Tmax,32]) and "vote_weight" (float32 [N,top_k]).  No host synchronisation."""
    lib = L.load()
    if "keep_anchor" not in det:
        raise ValueError("vote_tile_masks: `det` has no keep_anchor")
    member_slot, counts, boxes = merged["member_slot"], merged["counts"], merged["boxes_frame"]
    _need_cuda(protos, "vote_tile_masks")
    dev = member_slot.device
    N, top_k = merged["scores"].shape
    NT, K = member_slot.shape
    pr = _proto_rows(protos)
    nm, hp, wp = protos.shape[1:]
    mc = mc.float()
    if protos.shape[0] != NT or mc.shape[0] != NT or mc.shape[1] != nm or nm != 32 or hp != wp:
        raise ValueError(f"vote_tile_masks: protos {tuple(protos.shape)} and mc {tuple(mc.shape)}; expected [{NT}, 32, G, G] and [{NT}, 32, A]")
    if len(frames) != N or len(tiles) != N or sum(len(per) for per in tiles) != NT:
        raise ValueError(f"vote_tile_masks: {len(frames)} frames and {len(tiles)} tile lists for {N} images, {NT} tiles")
    Tmax = max(1, max(len(per) for per in tiles))
    # the frame's own step and scale are not used (1 here): every tile carries its own
    packed = _PackedFrames("vote_tile_masks", [(fr[0], fr[1], 1.0) for fr in frames], top_k, 1.0, out, dev)
    out = packed.out
    if merged.get("tiles") is tiles and "_keep" in merged:
        table, first, table_dev = merged["_keep"][1:4]           # the table `merge_tiles` built and uploaded
    else:
        table, first, table_dev = tile_table(tiles, dev)
    scores, anchors = det["scores"].contiguous().float(), det["keep_anchor"].contiguous().to(torch.int32)
    boxes = boxes.contiguous().float()
    W = torch.empty((N, top_k, Tmax, 32), dtype=torch.float32, device=dev)
    Ss = torch.empty((N, top_k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for c0, nb, fr in packed.chunks():
            a = L.TileMaskArgs()
            a.protos, a.mc = pr.data_ptr(), mc.data_ptr()
            a.mc_batch_stride, a.mc_k_stride, a.mc_c_stride = mc.stride(0), mc.stride(2), mc.stride(1)
            a.anchors, a.scores, a.member_slot = anchors.data_ptr(), scores.data_ptr(), member_slot.data_ptr()
            a.counts, a.boxes = counts[c0:].data_ptr(), boxes[c0:].data_ptr()
            a.tiles, a.tiles_dev = table, table_dev.data_ptr()
            a.first = C.cast(C.byref(first, 4 * c0), C.POINTER(C.c_int32))
            a.W, a.Ss = W[c0:].data_ptr(), Ss[c0:].data_ptr()
            a.out, a.out_bytes = out.data_ptr(), out.numel()
            a.N, a.n_tiles, a.K, a.top_k, a.Tmax, a.nm, a.hp, a.wp, a.crop = nb, NT, K, top_k, Tmax, 32, hp, wp, int(bool(crop))
            L.check(lib.mtbt_vote_tile_masks(C.byref(a), fr, nb, L.stream(dev)), "mtbt_vote_tile_masks")
    return {"boxes": boxes, "masks": packed.views(), "buffer": out, "vote_coeff": W, "vote_weight": Ss, "_keep": (table, first, table_dev, pr, mc, scores, anchors)}


# ---- the semantic mask in the image frame: views averaged, tiles blended (include/mtbt_hip.h `mtbt_seg_to_frames`) ----------------
SEG_MAX_PASSES = 64
SEG_BLENDS = ("constant", "gaussian", "tent")


def seg_blend_table(blend, G: int) -> Optional[np.ndarray]:
    """The blend window along one axis of a tile's upright G-pixel prototype grid, float32 [G], or None for "constant".
    "gaussian": MONAI's sliding-window importance map along one axis, exp(-(i - (G-1)/2)^2 / (2 (0.125 G)^2)) in float64, rounded to
    float32 and floored at its smallest positive entry; "tent": min(i, G-1-i) + 1, normalised to a maximum of 1; an array [G] is used as
    given.  Every entry must be finite and > 0 (ValueError)."""
    G = int(G)
    if isinstance(blend, str):
        if blend not in SEG_BLENDS:
            raise ValueError(f"seg_to_frames: blend {blend!r} (one of {SEG_BLENDS}, or a float array [G])")
        if blend == "constant":
            return None
        i = np.arange(G, dtype=np.float64)
        if blend == "gaussian":
            tab = np.exp(-((i - (G - 1) / 2.0) ** 2) / (2.0 * (0.125 * G) ** 2)).astype(np.float32)
            tab = np.maximum(tab, tab[tab > 0].min())
        else:
            tab = np.minimum(i, G - 1 - i) + 1.0
            tab = (tab / tab.max()).astype(np.float32)
    else:
        tab = np.asarray(blend.detach().cpu() if isinstance(blend, torch.Tensor) else blend, dtype=np.float32)
    tab = np.ascontiguousarray(tab, dtype=np.float32)
    if tab.shape != (G,) or not np.all(np.isfinite(tab)) or not np.all(tab > 0):
        raise ValueError(f"seg_to_frames: the blend table must be [{G}] floats, every entry finite and > 0")
    return tab


def _seg_projectors(projector, M: int):
    """`projector` -> ([(weight [32], bias [1])] tensors, one per distinct projector, the index of each of the M passes into that list)."""
    def pair(p):
        w, b = (p.weight, p.bias) if hasattr(p, "weight") else p
        w = w.detach().reshape(-1).float()
        if w.numel() != 32:
            raise ValueError(f"seg_to_frames: a projector has {w.numel()} weights; the kernel supports 32 prototype channels")
        b = torch.zeros(1, device=w.device) if b is None else b.detach().reshape(-1).float()
        return w, b
    if isinstance(projector, list):
        if len(projector) != M:
            raise ValueError(f"seg_to_frames: {len(projector)} projectors for {M} passes")
        return [pair(p) for p in projector], list(range(M))
    return [pair(projector)], [0] * M


def _seg_plan(shapes, frames, orients, weights, tiles, blend, up, proj_of=None):
    """The host's share of `seg_to_frames`, without a device: the checks, and per image its sources (pass m ascending, then tile
    ascending) as `mtbt_seg_source` / `mtbt_tile` rows.  Returns (sources array, tile array, first int32 [N+1], blend table or None, G)."""
    M = len(shapes)
    if not 1 <= M <= SEG_MAX_PASSES:
        raise ValueError(f"seg_to_frames: {M} passes (1..{SEG_MAX_PASSES})")
    N = len(frames)
    NT = N if tiles is None else sum(len(per) for per in tiles)
    G = int(shapes[0][2])
    for m, sh in enumerate(shapes):
        if len(sh) != 4 or sh[1] != 32 or sh[2] != sh[3] or sh[2] != G or sh[0] != NT:
            raise ValueError(f"seg_to_frames: pass {m} has prototypes {tuple(sh)}; expected [{NT}, 32, {G}, {G}]")
    if tiles is not None and len(tiles) != N:
        raise ValueError(f"seg_to_frames: {len(tiles)} tile lists for {N} frames")
    orients = [int(o) for o in orients]
    if len(orients) == 1:
        orients = orients * M
    weights = [1.0] * M if weights is None else [float(w) for w in weights]
    if len(orients) != M or len(weights) != M or any(not 0 <= o <= 7 for o in orients):
        raise ValueError(f"seg_to_frames: {len(orients)} orients (0..7) and {len(weights)} weights for {M} passes")
    if any(not (w > 0 and np.isfinite(w)) for w in weights):
        raise ValueError(f"seg_to_frames: weights must be finite and > 0, not {weights}")
    tab = seg_blend_table(blend, G)
    per_image = []
    for n, fr in enumerate(frames):
        H0, W0 = int(fr[0]), int(fr[1])
        if tiles is None:
            scale = float(fr[2])
            own = [{"image": n, "pox": 0, "poy": 0, "wx0": 0, "wy0": 0, "wx1": W0, "wy1": H0, "height": H0, "width": W0,
                    "step": C.c_float(scale / up).value, "scale": C.c_float(scale).value, "fox": 0.0, "foy": 0.0, "_slot": n}]
        else:
            t0 = sum(len(per) for per in tiles[:n])
            own = [dict(t, _slot=t0 + i) for i, t in enumerate(tiles[n])]
            if any((t["height"], t["width"]) != (H0, W0) for t in own):
                raise ValueError(f"seg_to_frames: the tiles of image {n} are not of its frame ({H0}, {W0})")
        if M * len(own) > TILE_MAX_PER_IMAGE:
            raise ValueError(f"seg_to_frames: image {n} has {M} passes x {len(own)} tiles = {M * len(own)} sources ({TILE_MAX_PER_IMAGE} at most)")
        per_image.append(own)
    NS = sum(M * len(own) for own in per_image)
    src, table = (L.SegSource * max(NS, 1))(), (L.Tile * max(NS, 1))()
    first = (C.c_int32 * (N + 1))()
    s = 0
    for n, own in enumerate(per_image):
        rows = []
        for t in own:                                  # one descriptor per tile, copied whole for every pass
            d = L.Tile()
            for k in _TILE_FIELDS:
                setattr(d, k, t[k])
            whole = (t["wx0"], t["wy0"], t["wx1"], t["wy1"]) == (0, 0, t["width"], t["height"])   # a whole-image source: constant
            rows.append((d, t["_slot"], int(tab is not None and tiles is not None and not whole)))
        for m in range(M):
            for d, slot, bl in rows:
                table[s] = d
                src[s] = L.SegSource(m, slot, orients[m], proj_of[m] if proj_of else 0, bl, weights[m])
                s += 1
        first[n + 1] = s
    return src, table, first, tab, G


def seg_to_frames(protos, projector, frames, *, orients: Sequence[int] = (0,), weights: Optional[Sequence[float]] = None, tiles=None,
                  blend="constant", threshold: float = 0.0, logits: bool = False, out: Optional[torch.Tensor] = None,
                  up: Optional[float] = None, want_low: bool = False):
    """The SEMANTIC mask in the coordinates of the original images: the projector's logit (the trainer's `seg_proto_projector`, a 1x1
    conv over the prototypes) averaged over several forward passes and sampled at the image's own pixels, one bit per pixel
    (`mtbt_seg_to_frames`: one launch for the projector at prototype resolution, one for the blend).

    `protos`: one tensor or a list of M passes (TTA views, ensemble members), each [N,32,G,G] in the frame of the view that pass saw; with
    `tiles` (`slice_geometry`'s lists) each is [NT,32,G,G], tile-major as `detect_sliced` concatenates them.  Any memory format.
    `projector`: an nn.Conv2d(32, 1, 1), or (weight, bias), or a list of M of them (one per pass).  `orients` (codes 0..7, one per pass;
    a single one holds for all) and `weights` (> 0, default 1) per pass.  `frames`, `up`, `out` and the packed layout: as in
    `masks_to_frames`, one plane per image.  The sources of image n are its passes, m ascending, then its tiles ascending (at most 64):

      logit v   = sum_s w_s tap_s / sum_s w_s over the sources whose window holds the pixel, w_s = weight_s * blend window at the pixel's
                  place in the source's upright prototype grid, tap_s = the bilinear tap of the source's upright projector logits
      mask bit  = some source sees the pixel and v > threshold (a logit: 0.0 is sigmoid 0.5)

    `blend` ("constant", "gaussian", "tent" or a float array [G], `seg_blend_table`) weighs the tile sources down towards their borders,
    which removes the seams an equal-weight sum leaves where overlapping tiles disagree; sources that see the whole image (a TTA view,
    sliced inference's full view) are constant.

    Returns {"masks": [uint8 [1, H0, pitch] per image], "logits": [fp32 [H0, W0] per image] with `logits=True` (or a caller's flat fp32
    buffer; image b starts at a multiple of 4 floats, every element is written) else None, "buffer":
    the flat uint8 buffer, "logits_buffer": the flat fp32 one or None} (and "low", the projector logits [NS, G, G] per source, with
    `want_low`).  Nothing synchronises with the device."""
    passes = list(protos) if isinstance(protos, (list, tuple)) else [protos]
    up = 4.0 if up is None else float(up)
    src, table, first, tab, G = _seg_plan([tuple(p.shape) for p in passes], frames, orients, weights, tiles, blend, up,
                                          list(range(len(passes))) if isinstance(projector, list) else None)
    if float(threshold) != float(threshold):
        raise ValueError("seg_to_frames: threshold is NaN")
    lib = L.load()
    for p in passes:
        _need_cuda(p, "seg_to_frames")
    dev = passes[0].device
    M, N, NS = len(passes), len(frames), int(first[len(frames)])
    pairs, _ = _seg_projectors(projector, M)
    q = torch.stack([torch.cat([w.to(dev), b.to(dev)]) for w, b in pairs]).contiguous()
    rows = [_proto_rows(p) for p in passes]
    # with tiles the frame's own step and scale are not used (1 here): every tile carries its own
    packed = _PackedFrames("seg_to_frames", frames if tiles is None else [(fr[0], fr[1], 1.0) for fr in frames], 1, up if tiles is None else 1.0,
                           out, dev)
    offs, total = [], 0
    for H0, W0 in ((r[0], r[1]) for r in packed.rows):
        offs.append(total)
        total = (total + H0 * W0 + 3) // 4 * 4
    lbuf = None
    if isinstance(logits, torch.Tensor):        # the caller's flat fp32 buffer
        lbuf = logits
        if lbuf.dtype != torch.float32 or lbuf.dim() != 1 or not lbuf.is_contiguous() or lbuf.numel() < total or lbuf.device != dev:
            raise ValueError(f"seg_to_frames: logits must be True or a contiguous flat float32 buffer of at least {total} elements on {dev}")
        logits = True
    elif logits:
        lbuf = torch.empty((total,), dtype=torch.float32, device=dev)
    low = torch.empty((max(NS, 1) * G * G,), dtype=torch.float32, device=dev)
    src_dev = torch.frombuffer(bytearray(bytes(src)), dtype=torch.uint8).to(dev)
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    tab_dev = torch.from_numpy(tab).to(dev) if tab is not None else None
    with torch.cuda.device(dev):
        for c0, nb, fr in packed.chunks():
            a = L.SegFrameArgs()
            for m, pr in enumerate(rows):
                a.protos[m], a.pass_items[m] = pr.data_ptr(), pr.shape[0]
            a.proj, a.sources, a.sources_dev, a.tiles, a.tiles_dev = q.data_ptr(), src, src_dev.data_ptr(), table, table_dev.data_ptr()
            a.first = C.cast(C.byref(first, 4 * c0), C.POINTER(C.c_int32))
            if tab is not None:
                a.tab, a.tab_dev = tab.ctypes.data_as(C.POINTER(C.c_float)), tab_dev.data_ptr()
            a.workspace, a.workspace_bytes = low.data_ptr(), low.numel() * 4
            a.out, a.out_bytes = packed.out.data_ptr(), packed.out.numel()
            if logits:
                a.logits, a.logits_floats = lbuf.data_ptr(), total
                for i in range(nb):
                    a.logits_offset[i] = offs[c0 + i]
            a.threshold = float(threshold)
            a.N, a.n_sources, a.n_passes, a.n_proj, a.nm, a.hp, a.wp = nb, NS, M, len(pairs), 32, G, G
            L.check(lib.mtbt_seg_to_frames(C.byref(a), fr, nb, L.stream(dev)), "mtbt_seg_to_frames")
    r = {"masks": packed.views(), "buffer": packed.out, "logits_buffer": lbuf,
         "logits": [lbuf[o:o + H0 * W0].view(H0, W0) for o, (H0, W0) in zip(offs, ((r[0], r[1]) for r in packed.rows))] if logits else None,
         "_keep": (rows, q, src, table, first, tab, src_dev, table_dev, tab_dev, low)}
    if want_low:
        r["low"] = low[:NS * G * G].view(NS, G, G)
    return r
