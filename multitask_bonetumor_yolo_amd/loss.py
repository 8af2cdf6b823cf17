"""Multitask loss value on the GPU: the reference's `MultiTaskLitModel._multitask_loss`
(`/root/reference/src/running_main_v3.py:232-387`) as three kernel launches (csrc/loss.hip) instead of a per-image Python
loop with `.item()` synchronisations.  The returned 0-d tensors carry no autograd history; `with_grads=True` additionally
returns the gradient of the total with respect to the head outputs -- what `trainstep.TrainStep` feeds the backward launch plan
(`grad_out` writes it straight into that plan's input buffers).  (Under the drop-in autograd route the trainer's own torch loss is
used instead, on the tensors `forward(x, "train")` returns.)

No host synchronisation: the ground-truth boxes are grouped by image with device-side tensor ops, the positive count and
the mean matched IoU come back as tensors (the reference returns Python floats, `:385`)."""
import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib as L
from .planes import _need_cuda, distance_transform, pack_masks, plane_pitch
from .postprocess import _mask_call, _nhwc_rows


def group_gt_boxes(gt_boxes: torch.Tensor, n_images: int, img_size: float):
    """[G,6] = (batch_idx, cls, cx, cy, w, h) normalised  ->  (xyxy [G,4] pixels grouped by image, cls [G] int32, off [N+1] int32).

    The pixel boxes are laid out exactly as the reference builds them (`:303-308`): per image it concatenates the four
    coordinate COLUMNS end to end and views the result as [-1, 4], which for G > 1 boxes mixes coordinates of different
    boxes -- reproduced, not repaired (drop-in parity)."""
    dev = gt_boxes.device
    G = gt_boxes.shape[0]
    off = torch.zeros(n_images + 1, dtype=torch.int32, device=dev)
    if G == 0:
        return torch.zeros((1, 4), dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), off
    bidx = gt_boxes[:, 0].long()
    order = torch.argsort(bidx, stable=True)
    g, bidx = gt_boxes[order].float(), bidx[order]
    counts = torch.zeros(n_images, dtype=torch.long, device=dev).scatter_add_(0, bidx.clamp(0, n_images - 1), torch.ones_like(bidx))
    starts = torch.cumsum(counts, 0) - counts
    off[1:] = torch.cumsum(counts, 0).int()
    cols = torch.stack([(g[:, 2] - g[:, 4] / 2) * img_size, (g[:, 3] - g[:, 5] / 2) * img_size,
                        (g[:, 2] + g[:, 4] / 2) * img_size, (g[:, 3] + g[:, 5] / 2) * img_size], 0)      # [4, G]
    gi, o = counts[bidx], starts[bidx]
    local = torch.arange(G, device=dev) - o
    q = 4 * local[:, None] + torch.arange(4, device=dev)[None, :]                                       # position in cat(...)
    xyxy = cols[q // gi[:, None], o[:, None] + q % gi[:, None]]
    return xyxy.contiguous(), g[:, 1].int().contiguous(), off


def _fill_levels(a, maps: Sequence[torch.Tensor], *, reg_max: int, img_size: float, read_maps: bool = True):
    """The fields every loss argument block starts with (`L.LossArgs`, `L.MaskLossArgs`, `L.TalLossArgs`): map / h / w / map_pixel_stride
    from the raw Detect maps as NHWC rows, n_levels, N, reg_max, img_size.  -> (the tensors `a` points into: keep them alive until the
    launch is issued; the anchor count A).  `read_maps=False` fills the shapes only and leaves the map pointers null: what an entry
    point that reads no map takes."""
    keep = []
    for i, m in enumerate(maps):
        a.h[i], a.w[i] = m.shape[2], m.shape[3]
        if read_maps:
            t, ld = _nhwc_rows(m.detach())
            keep.append(t)
            a.map[i], a.map_pixel_stride[i] = t.data_ptr(), ld
    a.n_levels, a.N, a.reg_max, a.img_size = len(maps), maps[0].shape[0], reg_max, float(img_size)
    return keep, sum(m.shape[2] * m.shape[3] for m in maps)


def _map_grad_buffers(who: str, det_maps: Sequence[torch.Tensor], no: int, grad_out, zero: bool = False):
    """The gradient with respect to the Detect maps goes into one contiguous fp32 NHWC [B, h, w, no] buffer per map: `grad_out`'s
    (a training plan's input buffers, validated here) or fresh ones (zeroed with `zero`, for a launch that adds to them).
    -> (the buffers, their [B, no, h, w] views)."""
    B, dev = det_maps[0].shape[0], det_maps[0].device
    if grad_out is not None:
        bufs = list(grad_out)
        if len(bufs) != len(det_maps) or any(t.dtype != torch.float32 or t.numel() != B * m.shape[2] * m.shape[3] * no or not t.is_contiguous()
                                             for t, m in zip(bufs, det_maps)):
            raise ValueError(f"{who}: grad_out must hold one contiguous fp32 [B, h, w, no] buffer per map")
    else:
        bufs = [(torch.zeros if zero else torch.empty)(B, m.shape[2], m.shape[3], no, dtype=torch.float32, device=dev) for m in det_maps]
    return bufs, [t.view(B, m.shape[2], m.shape[3], no).permute(0, 3, 1, 2) for t, m in zip(bufs, det_maps)]


def det_loss_args(det_maps: Sequence[torch.Tensor], gt_boxes: torch.Tensor, *, img_size: float, nc_det: int, reg_max: int = 16,
                  iou_match_thresh: float = 0.5):
    """The detection fields of the loss's argument block (`L.LossArgs`): the raw Detect maps as NHWC rows, the GT rows grouped by
    image (`group_gt_boxes`), nc, reg_max, img_size and the match threshold.  -> (args, tensors the args point into: keep them alive
    until the launch is issued).  Shared by `multitask_loss` and `metrics.DetectionConfusionMatrix`, so that both decode and match the
    same anchors."""
    a = L.LossArgs()
    keep, _ = _fill_levels(a, det_maps, reg_max=reg_max, img_size=img_size)
    a.nc = nc_det
    xyxy, gcls, off = group_gt_boxes(gt_boxes.to(det_maps[0].device), a.N, float(img_size))
    keep += [xyxy, gcls, off]
    a.gt_xyxy, a.gt_cls, a.gt_off = xyxy.data_ptr(), gcls.data_ptr(), off.data_ptr()
    a.iou_thresh = float(iou_match_thresh)
    return a, keep


def multitask_loss(det_maps: Sequence[torch.Tensor], protos: torch.Tensor, img_logits: torch.Tensor, gt_boxes: torch.Tensor,
                   gt_masks: torch.Tensor, gt_cls: torch.Tensor, proj_weight: torch.Tensor, proj_bias: torch.Tensor, *, img_size: int,
                   nc_det: int, reg_max: int = 16, iou_match_thresh: float = 0.5, label_smoothing: float = 0.0, training: bool = True,
                   weights=(1.0, 2.0, 1.5, 0.5, 1.0), with_grads: bool = False, grad_out=None, want_seg_logits: bool = False):
    """det_maps: the raw Detect maps of `forward(x, "train")` (3 x [B, 4*reg_max+nc, h, w]); protos [B, nm, hp, wp];
    gt_masks [B,1,S,S] float; gt_cls [B] int64; proj_*: the trainer's `seg_proto_projector` (`:186`).
    Returns the reference's tuple as 0-d fp32 tensors: (total, seg, box, dfl, cls_det, img_cls[, n_pos, mean matched IoU]).
    `with_grads=True` returns `(that tuple, grads)` where grads = d total / d {det_maps (list, like det_maps), seg_logits [B,1,S,S]
    (the projector output after the bilinear resize, `:251-255`), img_logits}: the first operator of the backward pass.
    `want_seg_logits=True` appends one more element to what is returned: the fp32 [B, 1, S, S] segmentation logits this function builds
    anyway, WITHOUT the projector bias (the kernels add it), for `seg_region_loss(..., bias=proj_bias)`."""
    lib = L.load()
    _need_cuda(det_maps[0], "multitask_loss")
    dev = det_maps[0].device
    B = det_maps[0].shape[0]
    a, keep = det_loss_args(det_maps, gt_boxes, img_size=img_size, nc_det=nc_det, reg_max=reg_max, iou_match_thresh=iou_match_thresh)
    A = sum(m.shape[2] * m.shape[3] for m in det_maps)
    a.label_smoothing, a.training = float(label_smoothing), int(training)
    # segmentation logits: Conv1x1(protos) -> bilinear S x S (mtbt_mask_assemble's projector path), bias added in the kernel
    w = proj_weight.detach().reshape(-1).float().contiguous()
    seg_logits, _ = _mask_call(protos, w, 0, 0, 1, None, None, 0.0, 1, (img_size, img_size), True, False)
    tgt = gt_masks.to(dev).float().contiguous()
    bias = proj_bias.detach().reshape(-1).float().contiguous()
    a.seg_logits, a.seg_targets, a.seg_bias, a.seg_n = seg_logits.data_ptr(), tgt.data_ptr(), bias.data_ptr(), seg_logits.numel()
    il = img_logits.float().contiguous()
    ig = gt_cls.to(dev).long().contiguous()
    a.img_logits, a.img_gt, a.n_img_classes = il.data_ptr(), ig.data_ptr(), il.shape[1]
    a.w_seg, a.w_box, a.w_dfl, a.w_cls, a.w_img = (float(v) for v in weights)
    ws, nbytes = L.workspace(lib.mtbt_loss_workspace_bytes, B, A, seg_logits.numel(), device=dev, what="mtbt_loss_workspace_bytes")
    out = torch.empty(8, dtype=torch.float32, device=dev)
    a.workspace, a.workspace_bytes, a.out = ws.data_ptr(), nbytes, out.data_ptr()
    L.check(lib.mtbt_multitask_loss(C.byref(a), L.stream(dev)), "mtbt_multitask_loss")
    res = tuple(out[i] for i in range(8 if training else 6))
    if not with_grads:
        del keep
        return (res, seg_logits.view(B, 1, img_size, img_size)) if want_seg_logits else res
    # gradient of the total w.r.t. the head outputs (csrc/loss.hip: det_loss_grad_kernel, seg_img_grad_kernel)
    no = 4 * reg_max + nc_det
    # grad_out = {"det_maps": [NHWC fp32 buffers], "img_logits": [B, n] fp32}: write straight into a training plan's input buffers
    d_maps, d_views = _map_grad_buffers("multitask_loss", det_maps, no, grad_out["det_maps"] if grad_out is not None else None)
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in d_maps], *([None] * (3 - len(d_maps))))
    lds = (C.c_int32 * 3)(*([no] * len(d_maps)), *([0] * (3 - len(d_maps))))
    d_seg = torch.empty_like(seg_logits)
    d_img = grad_out["img_logits"] if grad_out is not None else torch.empty_like(il)
    L.check(lib.mtbt_multitask_loss_grad(C.byref(a), ptrs, lds, d_seg.data_ptr(), d_img.data_ptr(), L.stream(dev)), "mtbt_multitask_loss_grad")
    del keep
    grads = {"det_maps": d_views,                                      # [B, no, h, w] views of channels-last memory
             "seg_logits": d_seg.view(B, 1, img_size, img_size), "img_logits": d_img}
    return (res, grads, seg_logits.view(B, 1, img_size, img_size)) if want_seg_logits else (res, grads)


# ---- instance-mask loss (YOLOv8-seg single_mask_loss / crop_mask): csrc/mask_loss.hip ------------------------------------------
_CODE_OF = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}


def group_gt_rows(gt_boxes: torch.Tensor, n_images: int, img_size: float):
    """[G,6] = (batch_idx, cls, cx, cy, w, h) normalised  ->  (xyxy [G,4] pixels, off [N+1] int32): every GT row is its OWN box
    (x1 = (cx - w / 2) * S, ...), rows grouped by image in stable order.  Unlike `group_gt_boxes` this is not the reference's
    column-concatenated layout, which mixes coordinates of different boxes of an image: a mask target cropped to such a box means
    nothing.  Rows with a non-positive width or height (or an image index outside the batch) are moved behind `off[N]`: they belong
    to no image and are never matched.  Device-side tensor ops only, no host synchronisation.  It IS `group_gt_rows_cls` without the
    classes: one definition of the row order, which an assignment handed from the task-aligned loss to the mask loss relies on."""
    xyxy, _, off = group_gt_rows_cls(gt_boxes, n_images, img_size, want_cls=False)
    return xyxy, off


def instance_mask_loss(box_maps: Sequence[torch.Tensor], mc: torch.Tensor, protos: torch.Tensor, gt_boxes: torch.Tensor,
                       gt_masks: torch.Tensor, *, img_size: int, reg_max: int = 16, iou_match_thresh: float = 0.5, weight: float = 1.0,
                       with_grads: bool = False, grad_out=None, accumulate: bool = False, protos_grad_dtype=torch.float32,
                       mc_layout: Optional[str] = None, assigned: Optional[torch.Tensor] = None):
    """The YOLOv8-seg instance-mask loss on the device (definition: include/mtbt_hip.h, `mtbt_mask_loss_args`).  An extension beyond the
    reference's `_multitask_loss`, whose only use of the prototypes is the 1x1 projector.

    box_maps: the raw Detect maps (3 x [B, 4*reg_max+nc, h, w]); mc: the mask coefficients [B, A, nm] (`mc_layout="bAn"`) or the
    module's [B, nm, A] view ("bnA"), any strides -- with `mc_layout=None` the shape decides, and a shape that fits both (A == nm) is
    refused; protos [B, nm, hp, wp]; gt_boxes [G, 6]; gt_masks [B, 1, S, S] float.
    Returns (mask_loss, n_pos) as 0-d fp32 device tensors without autograd history.  `with_grads=True` returns
    `((mask_loss, n_pos), {"mc": [B, A, nm] fp32, "protos": [B, nm, hp, wp] view of channels-last memory in protos_grad_dtype})`,
    the gradient of `weight * mask_loss`.  `grad_out={"mc": [B, A, nm] fp32, "protos": NHWC buffer (fp32 / bf16 / fp16)}` writes them
    straight into a training plan's input buffers; `accumulate=True` adds to the buffers instead of overwriting them.
    `assigned` = int32 [B, A] on the device (`task_aligned_det_loss(want_assignment=True)`: a row of the grouped GT, or -1) takes the
    positives from that assignment instead of the IoU match (`mtbt_instance_mask_loss_assigned`): `box_maps` is then used for its
    shapes only, `reg_max` and `iou_match_thresh` are not read, and n_pos is the number of foreground anchors."""
    lib = L.load()
    _need_cuda(box_maps[0], "instance_mask_loss")
    _need_cuda(mc, "instance_mask_loss")
    _need_cuda(protos, "instance_mask_loss")
    dev = box_maps[0].device
    B, nm, hp, wp = protos.shape
    A = sum(m.shape[2] * m.shape[3] for m in box_maps)
    S = int(img_size)
    a = L.MaskLossArgs()
    keep = []
    if assigned is not None:
        _need_cuda(assigned, "instance_mask_loss")
        if assigned.dtype != torch.int32 or tuple(assigned.shape) != (B, A):
            raise ValueError(f"instance_mask_loss: assigned must be an int32 [B, A] = {(B, A)} tensor, not {assigned.dtype} {tuple(assigned.shape)}")
        assigned = assigned.contiguous()
        keep.append(assigned)
    keep += _fill_levels(a, box_maps, reg_max=reg_max, img_size=img_size, read_maps=assigned is None)[0]
    a.iou_thresh = float(iou_match_thresh)
    xyxy, off = group_gt_rows(gt_boxes.to(dev), B, float(img_size))
    a.n_gt, a.gt_xyxy, a.gt_off = int(gt_boxes.shape[0]), xyxy.data_ptr(), off.data_ptr()
    mcf = mc.detach()
    mcf = mcf if mcf.dtype == torch.float32 else mcf.float()
    if mc_layout is None:
        fits = [k for k, shp in (("bAn", (B, A, nm)), ("bnA", (B, nm, A))) if tuple(mcf.shape) == shp]
        if len(fits) != 1:
            raise ValueError(f"instance_mask_loss: mc {tuple(mc.shape)} fits {'both' if fits else 'neither'} of [B, A, nm] = {(B, A, nm)} and "
                             "[B, nm, A]: pass mc_layout")
        mc_layout = fits[0]
    if mc_layout not in ("bAn", "bnA") or tuple(mcf.shape) != ((B, A, nm) if mc_layout == "bAn" else (B, nm, A)):
        raise ValueError(f"instance_mask_loss: mc {tuple(mc.shape)} is not the {mc_layout!r} layout of B, A, nm = {(B, A, nm)}")
    a.mc_batch_stride = mcf.stride(0)
    a.mc_anchor_stride, a.mc_channel_stride = (mcf.stride(1), mcf.stride(2)) if mc_layout == "bAn" else (mcf.stride(2), mcf.stride(1))
    pt, pld = _nhwc_rows(protos.detach())
    if pld != nm:
        pt = pt.contiguous(memory_format=torch.channels_last)
    tgt = gt_masks.to(dev).float().contiguous()
    if tgt.numel() != B * S * S:
        raise ValueError(f"instance_mask_loss: gt_masks {tuple(gt_masks.shape)} is not [B, 1, {S}, {S}]")
    keep += [xyxy, off, mcf, pt, tgt]
    a.mc, a.protos, a.gt_masks = mcf.data_ptr(), pt.data_ptr(), tgt.data_ptr()
    a.hp, a.wp, a.nm, a.weight = hp, wp, nm, float(weight)
    grads = None
    if with_grads or grad_out is not None:
        if grad_out is not None:
            d_mc, d_pr = grad_out["mc"], grad_out["protos"]
            if d_mc.dtype != torch.float32 or d_mc.numel() != B * A * nm or not d_mc.is_contiguous():
                raise ValueError("instance_mask_loss: grad_out['mc'] must be a contiguous fp32 [B, A, nm] buffer")
            if d_pr.dtype not in _CODE_OF or d_pr.numel() != B * hp * wp * nm or not d_pr.is_contiguous():
                raise ValueError("instance_mask_loss: grad_out['protos'] must be a contiguous [B, hp, wp, nm] buffer (fp32 / bf16 / fp16)")
        else:
            mk = torch.zeros if accumulate else torch.empty
            d_mc = mk(B, A, nm, dtype=torch.float32, device=dev)
            d_pr = mk(B, hp, wp, nm, dtype=protos_grad_dtype, device=dev)
        a.d_mc, a.d_protos, a.dprotos_dtype = d_mc.data_ptr(), d_pr.data_ptr(), _CODE_OF[d_pr.dtype]
        a.accumulate_dmc = a.accumulate_dprotos = int(accumulate)
        grads = {"mc": d_mc.view(B, A, nm), "protos": d_pr.view(B, hp, wp, nm).permute(0, 3, 1, 2)}
    ws, nbytes = L.workspace(lib.mtbt_mask_loss_workspace_bytes, B, A, hp, wp, nm, device=dev, what="mtbt_mask_loss_workspace_bytes")
    out = torch.empty(2, dtype=torch.float32, device=dev)
    a.workspace, a.workspace_bytes, a.out = ws.data_ptr(), nbytes, out.data_ptr()
    if assigned is None:
        L.check(lib.mtbt_instance_mask_loss(C.byref(a), L.stream(dev)), "mtbt_instance_mask_loss")
    else:
        L.check(lib.mtbt_instance_mask_loss_assigned(C.byref(a), assigned.data_ptr(), L.stream(dev)), "mtbt_instance_mask_loss_assigned")
    del keep
    res = (out[0], out[1])
    return (res, grads) if grads is not None else res


class InstanceMaskLoss(torch.autograd.Function):
    """`weight * mask_loss` as an autograd node for the drop-in route: a trainer adds it to the loss it computes on the outputs of
    `model(x, "train")`.
        InstanceMaskLoss.apply(mc, protos, gt_boxes, gt_masks, img_size, reg_max, iou_match_thresh, weight, mc_layout, *box_maps)
    -> (weight * mask_loss, n_pos).  `mc_layout` names the layout of `mc`: "bnA" (the module's [B, nm, A]) or "bAn".  Forward runs the
    value and both gradients; backward scales them by the incoming gradient and hands them out in the inputs' dtypes.  The matching
    carries no gradient: the box maps get None."""

    @staticmethod
    def forward(ctx, mc, protos, gt_boxes, gt_masks, img_size, reg_max, iou_match_thresh, weight, mc_layout, *box_maps):
        (loss, n_pos), g = instance_mask_loss([m.detach() for m in box_maps], mc, protos, gt_boxes, gt_masks, img_size=img_size, reg_max=reg_max,
                                              iou_match_thresh=iou_match_thresh, weight=weight, with_grads=True, mc_layout=mc_layout)
        d_mc = g["mc"] if mc_layout == "bAn" else g["mc"].permute(0, 2, 1)
        ctx.save_for_backward(d_mc, g["protos"])
        ctx.dtypes, ctx.n_maps = (mc.dtype, protos.dtype), len(box_maps)
        ctx.mark_non_differentiable(n_pos)
        return loss * weight, n_pos

    @staticmethod
    def backward(ctx, g_loss, _g_npos):
        d_mc, d_pr = ctx.saved_tensors
        return ((d_mc * g_loss).to(ctx.dtypes[0]), (d_pr * g_loss).to(ctx.dtypes[1])) + (None,) * (7 + ctx.n_maps)


# ---- region terms of the segmentation loss (soft Dice, Kervadec's boundary loss): csrc/distance_transform.hip ------------------
def seg_region_loss(seg_logits: torch.Tensor, gt_masks: torch.Tensor, *, bias: Optional[torch.Tensor] = None, dice_weight: float = 1.0,
                    boundary_weight: float = 0.0, smooth: float = 1.0, with_grads: bool = False, grad_out: Optional[torch.Tensor] = None,
                    accumulate: bool = False, W: Optional[int] = None):
    """Soft Dice and the boundary loss of the semantic segmentation head on the device (definitions: include/mtbt_hip.h,
    `mtbt_seg_region_args`).  Extensions beyond the reference's `_multitask_loss`, whose segmentation term is BCE alone.

    seg_logits: [B, 1, H, W] or [B, H, W] fp32 logits; `bias` (one fp32 value on the device) is added in the kernel, so the bias-free
    tensor of `multitask_loss(want_seg_logits=True)` can be passed as it is.  gt_masks: [B, 1, H, W] or [B, H, W] float, bool or uint8,
    packed through `pack_masks` (bit = value > 0); with `W=` given, gt_masks is taken as already packed uint8 [B, H, pitch] planes of
    that width.  Returns (dice, boundary, dice_weight * dice + boundary_weight * boundary) as 0-d fp32 device tensors without autograd
    history.  The distance transform of the targets runs only when boundary_weight != 0 (boundary is 0 otherwise).
    `with_grads=True` returns `(that tuple, {"seg_logits": [B, 1, H, W] fp32})`, the gradient of the weighted sum.  `grad_out` = a
    contiguous fp32 buffer of B * H * W elements takes the gradient instead of a fresh tensor; `accumulate=True` ADDS it to what the
    buffer holds (`TrainStep` adds it to the BCE gradient that way).  Asynchronous: no host synchronisation."""
    if seg_logits.dim() == 4 and seg_logits.shape[1] == 1:
        seg_logits = seg_logits[:, 0]
    if seg_logits.dim() != 3 or seg_logits.dtype != torch.float32:
        raise ValueError(f"seg_region_loss: seg_logits must be fp32 [B, 1, H, W] or [B, H, W], not {seg_logits.dtype} {tuple(seg_logits.shape)}")
    B, H, Wd = (int(v) for v in seg_logits.shape)
    pitch = plane_pitch(Wd)
    dev = seg_logits.device
    if not float(dice_weight) >= 0 or not float(boundary_weight) >= 0 or not float(smooth) >= 0:
        raise ValueError("seg_region_loss: dice_weight, boundary_weight and smooth must be >= 0")
    if B < 1:
        raise ValueError("seg_region_loss: an empty batch")
    if W is not None:
        if int(W) != Wd or gt_masks.dtype != torch.uint8 or tuple(gt_masks.shape) != (B, H, pitch):
            raise ValueError(f"seg_region_loss: packed gt_masks of width {W} must be uint8 [{B}, {H}, {pitch}] for logits {tuple(seg_logits.shape)}")
    else:
        dense = gt_masks[:, 0] if gt_masks.dim() == 4 and gt_masks.shape[1] == 1 else gt_masks
        if tuple(dense.shape) != (B, H, Wd):
            raise ValueError(f"seg_region_loss: gt_masks {tuple(gt_masks.shape)} does not fit logits {tuple(seg_logits.shape)}")
    _need_cuda(seg_logits, "seg_region_loss")
    _need_cuda(gt_masks, "seg_region_loss")
    lib = L.load()
    if W is not None:
        planes = gt_masks.contiguous()
        planes = planes if planes.data_ptr() % 8 == 0 else planes.clone()
    else:
        planes = pack_masks(dense if dense.dtype in (torch.bool, torch.uint8, torch.float32) else dense.float())
    z = seg_logits.detach().contiguous()
    keep = [z, planes]
    a = L.SegRegionArgs()
    a.logits, a.targets = z.data_ptr(), planes.data_ptr()
    if bias is not None:
        _need_cuda(bias, "seg_region_loss")
        if bias.numel() != 1:
            raise ValueError("seg_region_loss: bias is one value")
        bias = bias.detach().reshape(-1).float().contiguous()
        keep.append(bias)
        a.bias = bias.data_ptr()
    if float(boundary_weight) != 0:
        keep += list(distance_transform(planes, Wd, to="both"))
        a.d2_set, a.d2_unset = keep[-2].data_ptr(), keep[-1].data_ptr()
    grads = None
    if with_grads or grad_out is not None:
        if grad_out is not None:
            if grad_out.dtype != torch.float32 or grad_out.numel() != B * H * Wd or not grad_out.is_contiguous() or grad_out.device != dev:
                raise ValueError(f"seg_region_loss: grad_out must be a contiguous fp32 buffer of {B} * {H} * {Wd} elements on {dev}")
            d = grad_out
        else:
            d = (torch.zeros if accumulate else torch.empty)((B, H, Wd), dtype=torch.float32, device=dev)
        a.d_logits, a.accumulate = d.data_ptr(), int(bool(accumulate))
        grads = {"seg_logits": d.view(B, 1, H, Wd)}
    ws, nbytes = L.workspace(lib.mtbt_seg_region_loss_workspace_bytes, B, H, Wd, device=dev, what="mtbt_seg_region_loss_workspace_bytes")
    out = torch.empty(3, dtype=torch.float32, device=dev)
    a.workspace, a.workspace_bytes, a.out = ws.data_ptr(), nbytes, out.data_ptr()
    a.B, a.H, a.W, a.pitch = B, H, Wd, pitch
    a.smooth, a.w_dice, a.w_boundary = float(smooth), float(dice_weight), float(boundary_weight)
    with torch.cuda.device(dev):
        L.check(lib.mtbt_seg_region_loss(C.byref(a), L.stream(dev)), "mtbt_seg_region_loss")
    del keep
    res = (out[0], out[1], out[2])
    return (res, grads) if grads is not None else res


class SegRegionLoss(torch.autograd.Function):
    """`dice_weight * dice + boundary_weight * boundary` as an autograd node for the drop-in route: a trainer adds element 0 to the loss
    it computes on its own segmentation logits (the full logits, bias included).
        SegRegionLoss.apply(seg_logits, gt_masks, dice_weight, boundary_weight, smooth) -> (weighted sum, dice, boundary)
    Forward runs the value and the gradient; backward scales it by the incoming gradient and hands it out in the logits' dtype."""

    @staticmethod
    def forward(ctx, seg_logits, gt_masks, dice_weight=1.0, boundary_weight=0.0, smooth=1.0):
        (dice, boundary, total), g = seg_region_loss(seg_logits.detach().float(), gt_masks, dice_weight=dice_weight, boundary_weight=boundary_weight,
                                                     smooth=smooth, with_grads=True)
        ctx.save_for_backward(g["seg_logits"])
        ctx.shape, ctx.dtype = seg_logits.shape, seg_logits.dtype
        ctx.mark_non_differentiable(dice, boundary)
        return total, dice, boundary

    @staticmethod
    def backward(ctx, g_total, _g_dice, _g_boundary):
        (d,) = ctx.saved_tensors
        return (d * g_total).view(ctx.shape).to(ctx.dtype), None, None, None, None


# ---- task-aligned detection loss (TaskAlignedAssigner + CIoU + DFL + BCE over all anchors): csrc/det_loss_tal.hip ---------------
def group_gt_rows_cls(gt_boxes: torch.Tensor, n_images: int, img_size: float, want_cls: bool = True):
    """`group_gt_rows` with the rows' classes: -> (xyxy [G,4] pixels, cls [G] int32, off [N+1] int32), every row its own box, rows grouped
    by image in stable order, rows with a non-positive side or an image index outside the batch behind `off[N]`.  Device-side tensor
    ops only.  `want_cls=False` (what `group_gt_rows` passes) returns None in place of the classes and launches nothing for them."""
    dev = gt_boxes.device
    G = gt_boxes.shape[0]
    off = torch.zeros(n_images + 1, dtype=torch.int32, device=dev)
    if G == 0:
        return torch.zeros((1, 4), dtype=torch.float32, device=dev), (torch.zeros(1, dtype=torch.int32, device=dev) if want_cls else None), off
    g = gt_boxes.float()
    bidx = g[:, 0].long()
    skip = (g[:, 4] <= 0) | (g[:, 5] <= 0) | (bidx < 0) | (bidx >= n_images)
    bidx = torch.where(skip, torch.full_like(bidx, n_images), bidx)
    order = torch.argsort(bidx, stable=True)
    g, bidx = g[order], bidx[order]
    counts = torch.zeros(n_images + 1, dtype=torch.long, device=dev).scatter_add_(0, bidx, torch.ones_like(bidx))
    off[1:] = torch.cumsum(counts[:n_images], 0).int()
    xyxy = torch.stack([(g[:, 2] - g[:, 4] / 2) * img_size, (g[:, 3] - g[:, 5] / 2) * img_size,
                        (g[:, 2] + g[:, 4] / 2) * img_size, (g[:, 3] + g[:, 5] / 2) * img_size], 1)
    return xyxy.contiguous(), (g[:, 1].int().contiguous() if want_cls else None), off


def task_aligned_det_loss(det_maps: Sequence[torch.Tensor], gt_boxes: torch.Tensor, *, img_size: int, nc_det: int, reg_max: int = 16,
                          topk: int = 10, alpha: float = 0.5, beta: float = 6.0, weights=(7.5, 1.5, 0.5), with_grads: bool = False,
                          grad_out=None, accumulate: bool = False, want_assignment: bool = False):
    """The task-aligned (YOLOv8) detection loss on the device (definition: include/mtbt_hip.h, `mtbt_tal_loss_args`).  An opt-in
    extension beyond the reference's `_multitask_loss`, whose positives need a predicted box that already overlaps a GT box.

    det_maps: the raw Detect maps (<= 3 x [B, 4*reg_max+nc, h, w]); gt_boxes [G, 6] = (batch_idx, cls, cx, cy, w, h) normalised, every
    row its own box (`group_gt_rows_cls`).  Returns (box, dfl, cls, n_fg, mean overlap of the foreground anchors) as 0-d fp32 device
    tensors without autograd history.  `with_grads=True` also returns the gradient of `weights . (box, dfl, cls)` with respect to the
    maps, a list of [B, no, h, w] views of NHWC fp32 memory; `grad_out=[NHWC fp32 buffers]` writes it straight into a training plan's
    input buffers, `accumulate=True` adds to the buffers.  `want_assignment=True` also returns `assigned` int32 [B, A] (the row of the
    grouped GT an anchor is assigned to, -1 = background) and `target_score` [B, A].  The extras follow the values in that order.  No
    host synchronisation."""
    lib = L.load()
    _need_cuda(det_maps[0], "task_aligned_det_loss")
    dev = det_maps[0].device
    B = det_maps[0].shape[0]
    no = 4 * reg_max + nc_det
    for i, m in enumerate(det_maps):
        if m.shape[1] != no:
            raise ValueError(f"task_aligned_det_loss: map {i} has {m.shape[1]} channels, expected 4 * reg_max + nc_det = {no}")
    a = L.TalLossArgs()
    keep, A = _fill_levels(a, det_maps, reg_max=reg_max, img_size=img_size)
    a.nc = nc_det
    xyxy, gcls, off = group_gt_rows_cls(gt_boxes.to(dev), B, float(img_size))
    keep += [xyxy, gcls, off]
    G = int(gt_boxes.shape[0])
    a.n_gt, a.gt_xyxy, a.gt_cls, a.gt_off = G, xyxy.data_ptr(), gcls.data_ptr(), off.data_ptr()
    a.topk, a.alpha, a.beta = int(topk), float(alpha), float(beta)
    a.w_box, a.w_dfl, a.w_cls = (float(v) for v in weights)
    d_views = None
    if with_grads or grad_out is not None:
        d_maps, d_views = _map_grad_buffers("task_aligned_det_loss", det_maps, no, grad_out, zero=accumulate)
        for i, t in enumerate(d_maps):
            a.d_map[i], a.d_map_pixel_stride[i] = t.data_ptr(), no
        a.accumulate = int(accumulate)
    assigned = tscore = None
    if want_assignment:
        assigned = torch.empty(B, A, dtype=torch.int32, device=dev)
        tscore = torch.empty(B, A, dtype=torch.float32, device=dev)
        a.assigned, a.target_score = assigned.data_ptr(), tscore.data_ptr()
    ws, nbytes = L.workspace(lib.mtbt_tal_loss_workspace_bytes, B, A, G, device=dev, what="mtbt_tal_loss_workspace_bytes")
    out = torch.empty(8, dtype=torch.float32, device=dev)
    a.workspace, a.workspace_bytes, a.out = ws.data_ptr(), nbytes, out.data_ptr()
    L.check(lib.mtbt_tal_det_loss(C.byref(a), L.stream(dev)), "mtbt_tal_det_loss")
    del keep
    res = [tuple(out[i] for i in range(5))]
    if d_views is not None:
        res.append(d_views)
    if want_assignment:
        res += [assigned, tscore]
    return res[0] if len(res) == 1 else tuple(res)


class TaskAlignedDetLoss(torch.autograd.Function):
    """`w_box * box + w_dfl * dfl + w_cls * cls` of the task-aligned detection loss as an autograd node for the drop-in route: a trainer
    uses it in place of the detection terms it computes on the maps of `model(x, "train")`.
        TaskAlignedDetLoss.apply(gt_boxes, img_size, reg_max, nc, topk, alpha, beta, w_box, w_dfl, w_cls, *det_maps)
    -> (weighted loss, n_fg).  Forward runs the value and the gradient; backward scales the gradient by the incoming one and hands it
    out in the maps' dtypes.  The assignment carries no gradient."""

    @staticmethod
    def forward(ctx, gt_boxes, img_size, reg_max, nc, topk, alpha, beta, w_box, w_dfl, w_cls, *det_maps):
        (box, dfl, cls, n_fg, _), g = task_aligned_det_loss([m.detach() for m in det_maps], gt_boxes, img_size=img_size, nc_det=nc, reg_max=reg_max,
                                                            topk=topk, alpha=alpha, beta=beta, weights=(w_box, w_dfl, w_cls), with_grads=True)
        ctx.save_for_backward(*g)
        ctx.dtypes = tuple(m.dtype for m in det_maps)
        ctx.mark_non_differentiable(n_fg)
        return w_box * box + w_dfl * dfl + w_cls * cls, n_fg

    @staticmethod
    def backward(ctx, g_loss, _g_nfg):
        return (None,) * 10 + tuple((g * g_loss).to(dt) for g, dt in zip(ctx.saved_tensors, ctx.dtypes))


class TaskAlignedSegLoss(torch.autograd.Function):
    """The detection and mask terms of ultralytics' `v8SegmentationLoss` in one autograd node for the drop-in route: the task-aligned
    detection loss, and the instance-mask loss on ITS foreground anchors and assigned GT rows.
        TaskAlignedSegLoss.apply(mc, protos, gt_boxes, gt_masks, img_size, reg_max, nc, topk, alpha, beta, w_box, w_dfl, w_cls, w_mask,
                                 mc_layout, *det_maps)
    -> (w_box * box + w_dfl * dfl + w_cls * cls + w_mask * mask, n_fg).  Forward runs `task_aligned_det_loss(want_assignment=True,
    with_grads=True)`, then `instance_mask_loss(assigned=...)`; backward scales the stored gradients by the incoming one and hands them
    out in the inputs' dtypes.  The assignment is a constant: the maps get the task-aligned loss's gradient only."""

    @staticmethod
    def forward(ctx, mc, protos, gt_boxes, gt_masks, img_size, reg_max, nc, topk, alpha, beta, w_box, w_dfl, w_cls, w_mask, mc_layout, *det_maps):
        maps = [m.detach() for m in det_maps]
        (box, dfl, cls, n_fg, _), g_maps, assigned, _ = task_aligned_det_loss(maps, gt_boxes, img_size=img_size, nc_det=nc, reg_max=reg_max, topk=topk,
                                                                             alpha=alpha, beta=beta, weights=(w_box, w_dfl, w_cls), with_grads=True,
                                                                             want_assignment=True)
        (mask, _), g = instance_mask_loss(maps, mc, protos, gt_boxes, gt_masks, img_size=img_size, reg_max=reg_max, weight=w_mask, with_grads=True,
                                          mc_layout=mc_layout, assigned=assigned)
        d_mc = g["mc"] if mc_layout == "bAn" else g["mc"].permute(0, 2, 1)
        ctx.save_for_backward(d_mc, g["protos"], *g_maps)
        ctx.dtypes = (mc.dtype, protos.dtype) + tuple(m.dtype for m in det_maps)
        ctx.mark_non_differentiable(n_fg)
        return w_box * box + w_dfl * dfl + w_cls * cls + w_mask * mask, n_fg

    @staticmethod
    def backward(ctx, g_loss, _g_nfg):
        grads = tuple((g * g_loss).to(dt) for g, dt in zip(ctx.saved_tensors, ctx.dtypes))
        return grads[:2] + (None,) * 13 + grads[2:]
