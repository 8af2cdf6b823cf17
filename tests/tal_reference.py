"""CPU restatement of the task-aligned detection loss (include/mtbt_hip.h, `mtbt_tal_loss_args`: TaskAlignedAssigner + CIoU + DFL +
BCE over all anchors) and the shared test cases.  TEST INFRASTRUCTURE: torch on the CPU, fp32, the top-k by a stable descending
`torch.sort`, gradients from autograd.  tests/test_cpu_tal.py checks it against an independent per-GT, per-anchor loop."""
import functools
import math

import torch
import torch.nn.functional as F

import mask_loss_reference as M

EPS = 1e-7
NC = 2
WEIGHTS = (7.5, 1.5, 0.5)


def anchors_of(det, img_size):
    """(anchor points [A, 2] in pixels, stride [A]) of the levels, in the maps' order."""
    pts, sts = [], []
    for fm in det:
        h, w = fm.shape[2], fm.shape[3]
        stride = img_size / w
        gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        pts.append(torch.stack((gx + 0.5, gy + 0.5), dim=-1).view(h * w, 2) * stride)
        sts.append(torch.full((h * w,), stride, dtype=torch.float32))
    return torch.cat(pts), torch.cat(sts)


def rows_of(det, reg_max):
    """([B, A, 4, reg_max] side logits, [B, A, nc] class logits)."""
    flat = torch.cat([fm.permute(0, 2, 3, 1).reshape(fm.shape[0], -1, fm.shape[1]) for fm in det], 1)
    return flat[..., : 4 * reg_max].reshape(flat.shape[0], flat.shape[1], 4, reg_max), flat[..., 4 * reg_max:]


def gt_of(gt, b, img_size):
    """The image's valid rows in order: (xyxy pixels [g, 4], class [g])."""
    keep = (gt[:, 0] == b) & (gt[:, 4] > 0) & (gt[:, 5] > 0)
    return M.gt_rows_of(gt, b, img_size), gt[keep][:, 1].long()


def ciou(p, g):
    """ciou(pred, gt) over the last dimension (xyxy), broadcasting."""
    px1, py1, px2, py2 = p.unbind(-1)
    gx1, gy1, gx2, gy2 = g.unbind(-1)
    wp, hp = px2 - px1, py2 - py1 + EPS
    wg, hg = gx2 - gx1, gy2 - gy1 + EPS
    inter = (torch.minimum(px2, gx2) - torch.maximum(px1, gx1)).clamp(min=0) * (torch.minimum(py2, gy2) - torch.maximum(py1, gy1)).clamp(min=0)
    union = wp * hp + wg * hg - inter + EPS
    iou = inter / union
    cw = torch.maximum(px2, gx2) - torch.minimum(px1, gx1)
    ch = torch.maximum(py2, gy2) - torch.minimum(py1, gy1)
    c2 = cw * cw + ch * ch + EPS
    rho2 = ((gx1 + gx2 - px1 - px2) ** 2 + (gy1 + gy2 - py1 - py2) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(wg / hg) - torch.atan(wp / hp)) ** 2
    with torch.no_grad():
        alpha = v / (v - iou + (1 + EPS))
    return iou - (rho2 / c2 + v * alpha)


def assign(det, gt, *, img_size, nc=NC, reg_max=16, topk=10, alpha=0.5, beta=6.0):
    """No gradient.  dict(assigned [B, A] long: row of the grouped GT or -1, t [B, A] target score, metric / ov / inside / sel: per
    image [g, A] tensors, rows: per image (xyxy, cls), off: first grouped row of each image)."""
    with torch.no_grad():
        det = [d.detach() for d in det]
        boxes = M.decode_boxes(det, img_size, reg_max)
        _, cls = rows_of(det, reg_max)
        pts, _ = anchors_of(det, img_size)
        B, A = boxes.shape[:2]
        assigned = torch.full((B, A), -1, dtype=torch.long)
        t = torch.zeros(B, A)
        per, rows, offs, off = [], [], [], 0
        for b in range(B):
            gx, gc = gt_of(gt, b, img_size)
            rows.append((gx, gc))
            offs.append(off)
            g = gx.shape[0]
            if g == 0:
                per.append(None)
                continue
            lt, rb = pts[None] - gx[:, None, :2], gx[:, None, 2:] - pts[None]
            inside = torch.cat((lt, rb), -1).amin(-1) > 1e-9                                   # [g, A]
            ov = ciou(boxes[b][None], gx[:, None]).clamp(min=0) * inside
            score = torch.sigmoid(cls[b])[:, gc].T                                             # [g, A]
            metric = score.pow(alpha) * ov.pow(beta)
            order = torch.sort(metric, dim=1, descending=True, stable=True).indices[:, :topk]
            sel = torch.zeros(g, A, dtype=torch.bool).scatter_(1, order, True) & inside
            fg = sel.any(0)
            best = torch.where(sel, ov, torch.full_like(ov, -1.0)).argmax(0)                   # first maximum in row order
            final = sel & (torch.arange(g)[:, None] == best[None])
            Mg, Og = (metric * final).amax(1), (ov * final).amax(1)
            ta = metric.gather(0, best[None])[0] * Og[best] / (Mg[best] + 1e-9)
            assigned[b] = torch.where(fg, best + off, torch.full_like(best, -1))
            t[b] = torch.where(fg, ta, torch.zeros_like(ta))
            per.append(dict(metric=metric, ov=ov, inside=inside, sel=sel, final=final, Mg=Mg, Og=Og))
            off += g
        return dict(assigned=assigned, t=t, per=per, rows=rows, off=offs)


def tal_loss(det, gt, *, img_size, nc=NC, reg_max=16, topk=10, alpha=0.5, beta=6.0, asg=None):
    """-> (box, dfl, cls, n_fg, mean ov over fg), differentiable in the maps; the assignment is a constant."""
    asg = assign(det, gt, img_size=img_size, nc=nc, reg_max=reg_max, topk=topk, alpha=alpha, beta=beta) if asg is None else asg
    boxes = M.decode_boxes(det, img_size, reg_max)
    raw, cls = rows_of(det, reg_max)
    pts, st = anchors_of(det, img_size)
    B, A = boxes.shape[:2]
    T = asg["t"].sum().clamp(min=1.0)
    target = torch.zeros(B, A, nc)
    box = dfl = torch.zeros(())
    n_fg, ov_sum = 0, 0.0
    for b in range(B):
        gx, gc = asg["rows"][b]
        fg = torch.nonzero(asg["assigned"][b] >= 0).flatten()
        if fg.numel() == 0:
            continue
        gi = asg["assigned"][b][fg] - asg["off"][b]
        ta = asg["t"][b][fg]
        target[b, fg, gc[gi]] = ta
        box = box + ((1.0 - ciou(boxes[b][fg], gx[gi])) * ta).sum()
        ltrb = (torch.cat((pts[fg] - gx[gi][:, :2], gx[gi][:, 2:] - pts[fg]), -1) / st[fg, None]).clamp(0, reg_max - 1 - 0.01)
        tl = ltrb.floor().long()
        wl = (tl + 1).float() - ltrb
        wr = 1 - wl
        logp = F.log_softmax(raw[b][fg], dim=-1)                                               # [n, 4, reg_max]
        ce = -(logp.gather(-1, tl[..., None])[..., 0] * wl + logp.gather(-1, (tl + 1)[..., None])[..., 0] * wr)
        dfl = dfl + (ce.mean(-1) * ta).sum()
        n_fg += fg.numel()
        ov_sum += float(asg["per"][b]["ov"][gi, fg].sum())
    cls_l = F.binary_cross_entropy_with_logits(cls, target, reduction="sum") / T
    return box / T, dfl / T, cls_l, n_fg, (ov_sum / n_fg if n_fg else 0.0)


def extra_rows(c, rows):
    return dict(c, gt=torch.cat([c["gt"], torch.tensor(rows, dtype=torch.float32)]))


@functools.lru_cache(maxsize=None)
def case(k: int):
    """Cases 1-3 = `mask_loss_reference.case(1..3)` as they are; 4 = case 1 without GT; 5 = case 1 plus a row whose box contains no
    anchor centre at any level and a row with a zero width (skipped).  Cached: treat as read-only."""
    if k == 4:
        return M.empty(M.case(1))
    if k == 5:
        return extra_rows(M.case(1), [(1, 0, .49, .49, .05, .05), (1, 1, .5, .5, 0, .3)])
    return M.case(k)


def kw_of(c):
    return dict(img_size=c["kw"]["img_size"], nc=NC, reg_max=c["kw"]["reg_max"])


@functools.lru_cache(maxsize=None)
def reference(k: int, weights=WEIGHTS):
    """dict(values (box, dfl, cls, n_fg, mean ov), grads: d (weights . (box, dfl, cls)) / d map per level, asg) of case k, once."""
    c = case(k)
    det = [d.clone().requires_grad_() for d in c["det"]]
    asg = assign(det, c["gt"], **kw_of(c))
    box, dfl, cls, n_fg, mov = tal_loss(det, c["gt"], asg=asg, **kw_of(c))
    (weights[0] * box + weights[1] * dfl + weights[2] * cls).backward()
    return dict(values=(float(box.detach()), float(dfl.detach()), float(cls.detach()), n_fg, mov), grads=[d.grad for d in det], asg=asg)
