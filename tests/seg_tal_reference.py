"""CPU restatement of the instance-mask loss on a GIVEN assignment (include/mtbt_hip.h, `mtbt_instance_mask_loss_assigned`; the mask
term of ultralytics' `v8SegmentationLoss`, whose positives are the task-aligned assigner's foreground anchors with their assigned GT
rows).  TEST INFRASTRUCTURE: torch on the CPU, fp32, gradients from autograd.  It is the loop of `mask_loss_reference.mask_loss` with
the positives taken from the assignment instead of the IoU match; the cases are `tal_reference.case(1..5)`, which already carry `mc`,
`protos` and `masks`.  tests/test_cpu_seg_tal.py checks it against an independent per-anchor, per-pixel loop."""
import functools

import torch
import torch.nn.functional as F

import mask_loss_reference as M
import tal_reference as T


def mask_loss_from_assignment(mc, protos, gt_boxes, gt_masks, assigned, off, *, img_size):
    """mc [B, A, nm], protos [B, nm, hp, wp], gt_masks [B, 1, S, S], assigned [B, A] (row of the grouped GT or -1), off[b] = the first
    grouped row of image b  ->  (mask_loss, n_fg).  Differentiable in mc and protos; the assignment is a constant."""
    B, nm, hp, wp = protos.shape
    S = img_size
    assert S % hp == 0 and S % wp == 0
    tgt = F.interpolate(gt_masks.float(), size=(hp, wp), mode="nearest")[:, 0]
    scale = torch.tensor([wp / S, hp / S, wp / S, hp / S], dtype=torch.float32)
    xs, ys = torch.arange(wp, dtype=torch.float32)[None, None, :], torch.arange(hp, dtype=torch.float32)[None, :, None]
    total, n_fg = torch.zeros(()), 0
    for b in range(B):
        pos = torch.nonzero(assigned[b] >= 0).flatten()
        if pos.numel() == 0:
            continue
        gi = assigned[b][pos].long() - off[b]
        gx = M.gt_rows_of(gt_boxes, b, S)
        n_fg += pos.numel()
        q = gx[gi] * scale
        logits = torch.einsum("pc,chw->phw", mc[b][pos], protos[b])
        inside = (xs >= q[:, 0, None, None]) & (xs < q[:, 2, None, None]) & (ys >= q[:, 1, None, None]) & (ys < q[:, 3, None, None])
        bce = F.binary_cross_entropy_with_logits(logits, tgt[b].expand_as(logits), reduction="none")
        area = (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
        total = total + ((bce * inside).sum((1, 2)) / area).sum()
    norm = float(n_fg) if n_fg > 0 else float(B)
    return total / norm, n_fg


def mask_loss_assigned(case, assigned, off, weight=1.0):
    """(value, n_fg, d (weight * value) / d mc [B, A, nm], d / d protos [B, nm, hp, wp]) of a case on an assignment, by autograd."""
    mc, protos = case["mc"].clone().requires_grad_(), case["protos"].clone().requires_grad_()
    val, n_fg = mask_loss_from_assignment(mc, protos, case["gt"], case["masks"], assigned, off, img_size=case["kw"]["img_size"])
    if val.requires_grad:
        (weight * val).backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return val.detach(), n_fg, zero(mc), zero(protos)


@functools.lru_cache(maxsize=None)
def assignment(k: int, topk: int = 10):
    """`tal_reference.assign` of case k, once: dict(assigned [B, A] long, off, per, ...).  Cached: treat as read-only."""
    c = T.case(k)
    return T.assign(c["det"], c["gt"], topk=topk, **T.kw_of(c))


def margins(asg, topk):
    """(tightest relative gap between the topk-th and the next metric of a GT with more than topk positive metrics, tightest gap between
    the two largest overlaps at a contested anchor) of a `tal_reference.assign` result; inf where there is no such pair.  What decides
    whether an fp32 implementation in another summation order can be expected to reproduce the assignment exactly."""
    tight_m = tight_o = float("inf")
    for per in asg["per"]:
        if per is None:
            continue
        srt = torch.sort(per["metric"], dim=1, descending=True, stable=True).values
        for r in range(srt.shape[0]):
            if srt.shape[1] > topk and srt[r, topk] > 0:
                tight_m = min(tight_m, ((srt[r, topk - 1] - srt[r, topk]) / srt[r, topk - 1]).item())
        for a in torch.nonzero(per["sel"].sum(0) > 1).flatten().tolist():
            o = torch.sort(per["ov"][per["sel"][:, a], a], descending=True).values
            tight_o = min(tight_o, (o[0] - o[1]).item())
    return tight_m, tight_o


def offsets_of(case):
    """off[b] = the first grouped row of image b, for a hand-made assignment."""
    out, off = [], 0
    for b in range(case["protos"].shape[0]):
        out.append(off)
        off += M.gt_rows_of(case["gt"], b, case["kw"]["img_size"]).shape[0]
    return out


@functools.lru_cache(maxsize=None)
def reference(k: int, topk: int = 10, weight: float = 1.0):
    """(value, n_fg, d_mc, d_protos) of case k on its task-aligned assignment at `topk`, computed once."""
    asg = assignment(k, topk)
    return mask_loss_assigned(T.case(k), asg["assigned"], asg["off"], weight)
