"""CPU restatement of the instance-mask loss (include/mtbt_hip.h, `mtbt_mask_loss_args`; ultralytics `single_mask_loss` /
`crop_mask` with this project's matching rule) and the shared test cases.  TEST INFRASTRUCTURE: torch on the CPU, fp32, gradients
from autograd.  tests/test_cpu_mask_loss.py checks it against an independent per-positive, per-pixel loop."""
import functools

import torch
import torch.nn.functional as F

from oracle.postprocess import batch_bbox_iou

NM = 32


def decode_boxes(box_maps, img_size, reg_max=16):
    """[B, A, 4] xyxy pixels: softmax expectation of each side, anchors (x + .5, y + .5), stride = img_size / w (as oracle/loss.py)."""
    project = torch.arange(reg_max, dtype=torch.float32)
    boxes = []
    for fm in box_maps:
        b, ch, h, w = fm.shape
        stride = img_size / w
        flat = fm.permute(0, 2, 3, 1).reshape(b, h * w, ch)
        raw = flat[..., : 4 * reg_max].view(b, h * w, 4, reg_max)
        ltrb = torch.einsum("ijkl,l->ijk", F.softmax(raw, dim=-1), project)
        gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        anc = torch.stack((gx + 0.5, gy + 0.5), dim=-1).view(1, h * w, 2).repeat(b, 1, 1)
        d, a = ltrb * stride, anc * stride
        boxes.append(torch.cat((a - d[..., :2], a + d[..., 2:]), dim=-1))
    return torch.cat(boxes, 1)


def gt_rows_of(gt_boxes, b, img_size):
    """The image's GT rows as their own boxes, xyxy pixels [g, 4]; rows with a non-positive width or height are skipped."""
    c = gt_boxes[(gt_boxes[:, 0] == b) & (gt_boxes[:, 4] > 0) & (gt_boxes[:, 5] > 0)][:, 2:6].float()
    return torch.stack([(c[:, 0] - c[:, 2] / 2) * img_size, (c[:, 1] - c[:, 3] / 2) * img_size,
                        (c[:, 0] + c[:, 2] / 2) * img_size, (c[:, 1] + c[:, 3] / 2) * img_size], 1)


def match(box_maps, gt_boxes, img_size, reg_max=16, iou_match_thresh=0.5):
    """Per image (positive anchor indices ascending, matched row of the image's GT list, the image's GT boxes); no gradient."""
    with torch.no_grad():
        boxes = decode_boxes([m.detach() for m in box_maps], img_size, reg_max)
        out = []
        for b in range(boxes.shape[0]):
            gx = gt_rows_of(gt_boxes, b, img_size)
            if gx.shape[0] == 0:
                out.append((torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long), gx))
                continue
            best, gi = batch_bbox_iou(boxes[b], gx).max(dim=1)
            pos = torch.nonzero(best > iou_match_thresh).flatten()
            out.append((pos, gi[pos], gx))
    return out


def mask_loss(box_maps, mc, protos, gt_boxes, gt_masks, *, img_size, reg_max=16, iou_match_thresh=0.5):
    """mc [B, A, nm], protos [B, nm, hp, wp], gt_masks [B, 1, S, S] -> (mask_loss, n_pos).  Differentiable in mc and protos."""
    B, nm, hp, wp = protos.shape
    S = img_size
    assert S % hp == 0 and S % wp == 0
    tgt = F.interpolate(gt_masks.float(), size=(hp, wp), mode="nearest")[:, 0]
    scale = torch.tensor([wp / S, hp / S, wp / S, hp / S], dtype=torch.float32)
    xs, ys = torch.arange(wp, dtype=torch.float32)[None, None, :], torch.arange(hp, dtype=torch.float32)[None, :, None]
    total, n_pos = torch.zeros(()), 0
    for b, (pos, gi, gx) in enumerate(match(box_maps, gt_boxes, S, reg_max, iou_match_thresh)):
        if pos.numel() == 0:
            continue
        n_pos += pos.numel()
        q = gx[gi] * scale
        logits = torch.einsum("pc,chw->phw", mc[b][pos], protos[b])
        inside = (xs >= q[:, 0, None, None]) & (xs < q[:, 2, None, None]) & (ys >= q[:, 1, None, None]) & (ys < q[:, 3, None, None])
        bce = F.binary_cross_entropy_with_logits(logits, tgt[b].expand_as(logits), reduction="none")
        area = (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
        total = total + ((bce * inside).sum((1, 2)) / area).sum()
    norm = float(n_pos) if n_pos > 0 else float(B)
    return total / norm, n_pos


def mask_loss_and_grads(case, weight=1.0):
    """(value, n_pos, d (weight * value) / d mc [B, A, nm], d / d protos [B, nm, hp, wp]) by autograd."""
    mc, protos = case["mc"].clone().requires_grad_(), case["protos"].clone().requires_grad_()
    val, n_pos = mask_loss(case["det"], mc, protos, case["gt"], case["masks"], **case["kw"])
    if val.requires_grad:
        (weight * val).backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return val.detach(), n_pos, zero(mc), zero(protos)


GT_ROWS = {
    1: [(0, 1, .40, .45, .55, .50), (0, 0, .62, .58, .45, .60), (2, 1, .305, .71, .37, .29)],
    2: [(0, 1, .47, .52, .80, .76), (0, 0, .70, .30, .22, .26), (2, 1, .5, .5, 1.0, 1.0), (3, 0, .13, .85, .26, .30)],
    3: [(0, 1, 0.31, 0.36, 0.22, 0.30), (0, 0, 0.70, 0.70, 0.30, 0.25), (1, 0, 0.25, 0.60, 0.30, 0.30), (1, 1, 0.60, 0.30, 0.20, 0.40),
        (1, 1, 0.80, 0.80, 0.25, 0.25)],
}
SHAPES = {1: (64, 3, 5, True), 2: (128, 4, 3, False), 3: (640, 2, 17, True)}          # S, B, seed, steering onto the rows' own boxes


def _steer(det, gt, S, B, own_boxes):
    """tests/test_gpu_loss.py `_model_scale_case`: sharpen the side distributions of the 3 x 3 cells around each steering box so that
    some anchors decode onto it.  own_boxes: steer onto every row's own box (this loss's GT boxes); otherwise the literal code of that
    case, whose steering boxes are the column-concatenated layout of the image's rows -- in an image with two rows no anchor is then
    steered onto the smaller one, which is how case 2 gets a GT row without positives."""
    for lvl, fm in enumerate(det):
        h = fm.shape[2]
        stride = S / h
        for b in range(B):
            sel = gt[gt[:, 0] == b]
            if sel.numel() == 0:
                continue
            c = sel[:, 2:6]
            boxes = torch.cat([(c[:, 0] - c[:, 2] / 2) * S, (c[:, 1] - c[:, 3] / 2) * S, (c[:, 0] + c[:, 2] / 2) * S,
                               (c[:, 1] + c[:, 3] / 2) * S], dim=-1).view(-1, 4)
            if own_boxes:
                boxes = gt_rows_of(gt, b, S)
            for bx in boxes:
                if bx[2] <= bx[0] or bx[3] <= bx[1]:
                    continue
                cx, cy = int((bx[0] + bx[2]) / 2 / stride), int((bx[1] + bx[3]) / 2 / stride)
                for yy in range(max(cy - 1, 0), min(cy + 2, h)):
                    for xx in range(max(cx - 1, 0), min(cx + 2, h)):
                        ax, ay = (xx + 0.5) * stride, (yy + 0.5) * stride
                        ltrb = torch.tensor([ax - bx[0], ay - bx[1], bx[2] - ax, bx[3] - ay]) / stride
                        if ltrb.min() > 0.3 and ltrb.max() < 14.0:
                            for k in range(4):
                                fm[b, 16 * k:16 * k + 16, yy, xx] += 6.0 * torch.exp(-0.5 * (torch.arange(16.0) - ltrb[k]) ** 2 / 0.3)


@functools.lru_cache(maxsize=None)
def case(k: int):
    """Cases 1-3 of the instance-mask loss tests (nc = 2, nm = 32); case 4 is `empty(case(1))`.  Cached: treat as read-only."""
    S, B, seed, own = SHAPES[k]
    g = torch.Generator().manual_seed(seed)
    hs = (S // 8, S // 16, S // 32)
    det = [torch.randn(B, 64 + 2, h, h, generator=g) * 0.7 for h in hs]
    gt = torch.tensor(GT_ROWS[k], dtype=torch.float32)
    _steer(det, gt, S, B, own)
    A = sum(h * h for h in hs)
    mc = torch.randn(B, A, NM, generator=g) * 0.5
    protos = torch.randn(B, NM, S // 4, S // 4, generator=g)
    masks = (torch.rand(B, 1, S, S, generator=g) > 0.6).float()
    return dict(det=det, mc=mc, protos=protos, gt=gt, masks=masks, kw=dict(img_size=S, reg_max=16, iou_match_thresh=0.5), A=A)


def empty(c):
    return dict(c, gt=c["gt"][:0])


@functools.lru_cache(maxsize=None)
def reference(k: int, weight: float = 1.0):
    """(value, n_pos, d_mc, d_protos) of case k (4 = case 1 without GT), computed once."""
    return mask_loss_and_grads(empty(case(1)) if k == 4 else case(k), weight)


def positives_per_gt(c):
    """Per GT row of the case (in the rows' order within each image): number of positives."""
    out = []
    for pos, gi, gx in match(c["det"], c["gt"], c["kw"]["img_size"], c["kw"]["reg_max"], c["kw"]["iou_match_thresh"]):
        out += [int((gi == r).sum()) for r in range(gx.shape[0])]
    return out
