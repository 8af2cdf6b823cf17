"""Timing probe of the instance-mask loss (GPU box), BASELINE configs[2] shape: batch 32, 640 x 640, 8400 anchors, 160 x 160 x 32
prototypes, 1 - 3 ground-truth boxes per image, Detect maps steered so that a few dozen anchors per box are positives.

  operator   `instance_mask_loss` (value + d_mc + d_protos, csrc/mask_loss.hip) beside a torch-on-device formulation of the same
             definition (decode, IoU, per-image positives, einsum, BCE, autograd) on the same inputs in the same process.  Device
             events around 20 calls per variant after warm-up, the variants alternating, 6 rounds.
  step       `TrainStep.step` with `instance_mask_weight` 0 and 1 (two models on one state), alternating, same scheme.  The match
             threshold of both is set so that the first batch has about 64 positives per image under the synthetic heads.

  python tools/mask_loss_probe.py [--batch 32] [--img 640] [--part operator|step|kernels]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/mask_loss_probe.py --part kernels      (per-kernel times, a run of its own)"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import instance_mask_loss

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--img", type=int, default=640)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--part", default="all", choices=["all", "operator", "step", "kernels"])
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, S, NM = args.batch, args.img, 32
hs = (S // 8, S // 16, S // 32)
A = sum(h * h for h in hs)

g = torch.Generator().manual_seed(0)
rows = []
for b in range(B):
    for _ in range(1 + b % 3):
        wh = torch.rand(2, generator=g) * 0.4 + 0.1
        cxy = torch.rand(2, generator=g) * (1 - wh) + wh / 2
        rows.append(torch.cat([torch.tensor([float(b), float(b % 2)]), cxy, wh]))
rows = torch.stack(rows)
xyxy = torch.stack([(rows[:, 2] - rows[:, 4] / 2) * S, (rows[:, 3] - rows[:, 5] / 2) * S, (rows[:, 2] + rows[:, 4] / 2) * S,
                    (rows[:, 3] + rows[:, 5] / 2) * S], 1)
masks = (torch.rand(B, 1, S // 16, S // 16, generator=g) > 0.4).float().repeat_interleave(16, 2).repeat_interleave(16, 3).to(dev)


def steered_maps():
    """Random Detect maps with the side distributions of the 5 x 5 cells around each box centre sharpened onto the box."""
    det = [torch.randn(B, 66, h, h, generator=g) * 0.7 for h in hs]
    for fm in det:
        h = fm.shape[2]
        stride = S / h
        for r, bx in zip(rows, xyxy):
            b = int(r[0])
            cx, cy = int((bx[0] + bx[2]) / 2 / stride), int((bx[1] + bx[3]) / 2 / stride)
            for yy in range(max(cy - 2, 0), min(cy + 3, h)):
                for xx in range(max(cx - 2, 0), min(cx + 3, h)):
                    ax, ay = (xx + 0.5) * stride, (yy + 0.5) * stride
                    ltrb = torch.tensor([ax - bx[0], ay - bx[1], bx[2] - ax, bx[3] - ay]) / stride
                    if ltrb.min() > 0.3 and ltrb.max() < 14.0:
                        for k in range(4):
                            fm[b, 16 * k:16 * k + 16, yy, xx] += 6.0 * torch.exp(-0.5 * (torch.arange(16.0) - ltrb[k]) ** 2 / 0.3)
    return [d.to(dev).contiguous(memory_format=torch.channels_last) for d in det]


def decode(det):
    project = torch.arange(16, dtype=torch.float32, device=dev)
    out = []
    for fm in det:
        b, ch, h, w = fm.shape
        stride = S / w
        flat = fm.permute(0, 2, 3, 1).reshape(b, h * w, ch)
        ltrb = torch.einsum("ijkl,l->ijk", F.softmax(flat[..., :64].view(b, h * w, 4, 16), dim=-1), project) * stride
        gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=dev), torch.arange(w, dtype=torch.float32, device=dev), indexing="ij")
        anc = torch.stack((gx + 0.5, gy + 0.5), dim=-1).view(1, h * w, 2) * stride
        out.append(torch.cat((anc - ltrb[..., :2], anc + ltrb[..., 2:]), dim=-1))
    return torch.cat(out, 1)


def iou(a, b):
    iw = (torch.min(a[:, None, 2], b[None, :, 2]) - torch.max(a[:, None, 0], b[None, :, 0])).clamp(min=0)
    ih = (torch.min(a[:, None, 3], b[None, :, 3]) - torch.max(a[:, None, 1], b[None, :, 1])).clamp(min=0)
    inter = iw * ih
    return inter / ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None].add((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).sub(inter).add(1e-7)


rows_d, xyxy_d = rows.to(dev), xyxy.to(dev)
per_image = [torch.nonzero(rows[:, 0] == b).flatten().to(dev) for b in range(B)]


def torch_formulation(det, mc, protos, thresh, weight=1.0):
    """The definition in torch on the device: value and both gradients (autograd)."""
    mc, protos = mc.detach().requires_grad_(), protos.detach().requires_grad_()
    hp, wp = protos.shape[2:]
    with torch.no_grad():
        boxes = decode(det)
        tgt = F.interpolate(masks, size=(hp, wp), mode="nearest")[:, 0]
        xs, ys = torch.arange(wp, dtype=torch.float32, device=dev)[None, None, :], torch.arange(hp, dtype=torch.float32, device=dev)[None, :, None]
    total, n_pos = torch.zeros((), device=dev), 0
    for b in range(B):
        gx = xyxy_d[per_image[b]]
        best, gi = iou(boxes[b], gx).max(dim=1)
        pos = torch.nonzero(best > thresh).flatten()
        if pos.numel() == 0:
            continue
        n_pos += pos.numel()
        q = gx[gi[pos]] * (wp / S)
        logits = torch.einsum("pc,chw->phw", mc[b][pos], protos[b])
        inside = (xs >= q[:, 0, None, None]) & (xs < q[:, 2, None, None]) & (ys >= q[:, 1, None, None]) & (ys < q[:, 3, None, None])
        bce = F.binary_cross_entropy_with_logits(logits, tgt[b].expand_as(logits), reduction="none")
        total = total + ((bce * inside).sum((1, 2)) / ((q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1]))).sum()
    val = total / max(n_pos, 1)
    (weight * val).backward()
    return val.detach(), n_pos, mc.grad, protos.grad


def timed(variants):
    for f in variants.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    for name, t in times.items():
        print(f"{name:44s} per call (us) rounds: " + " ".join(f"{v:9.1f}" for v in t) + f"   mean {sum(t) / len(t):9.1f}")
    return {k: sum(t) / len(t) for k, t in times.items()}


if args.part in ("all", "operator", "kernels"):
    det = steered_maps()
    mc = (torch.randn(B, A, NM, generator=g) * 0.5).to(dev)
    protos = torch.randn(B, NM, S // 4, S // 4, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
    d_mc = torch.empty(B, A, NM, device=dev)
    d_pr = torch.empty(B, S // 4, S // 4, NM, device=dev)
    kernel = lambda: instance_mask_loss(det, mc, protos, rows_d, masks, img_size=S, grad_out={"mc": d_mc, "protos": d_pr})
    (val, n_pos), _ = kernel()
    if args.part == "kernels":
        for _ in range(args.launches):
            kernel()
        torch.cuda.synchronize()
        print(f"{args.launches + 1} calls, {int(n_pos)} positives")
    else:
        tv, tn, tmc, tpr = torch_formulation(det, mc, protos, 0.5)
        print(f"B = {B}, {S} x {S}, A = {A}, {rows.shape[0]} GT rows, {int(n_pos)} positives (torch: {tn}); value {float(val):.6f} (torch {float(tv):.6f}); "
              f"max |d_mc - torch| {(d_mc - tmc).abs().max().item():.2e} of {tmc.abs().max().item():.2e}, "
              f"max |d_protos - torch| {(d_pr.permute(0, 3, 1, 2) - tpr).abs().max().item():.2e} of {tpr.abs().max().item():.2e}")
        m = timed({"instance_mask_loss (value + d_mc + d_protos)": kernel,
                   "torch formulation (value + autograd)": lambda: torch_formulation(det, mc, protos, 0.5)})
        k_us, t_us = m["instance_mask_loss (value + d_mc + d_protos)"], m["torch formulation (value + autograd)"]
        print(f"kernel / torch formulation: {k_us:.1f} us / {t_us:.1f} us = {k_us / t_us:.4f}")

if args.part in ("all", "step"):
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, init_synthetic_
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    torch.manual_seed(0)
    x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)).to(dev)
    gt_cls = (torch.arange(B) % 2).to(dev)
    models = [init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)).to(dev) for _ in range(2)]
    models[1].load_state_dict(models[0].state_dict())
    for m in models:
        m.set_compute_dtype(torch.bfloat16)
    steps = [TrainStep(m, (B, 3, S, S), optimizer="sgd", lr=1e-4, instance_mask_weight=w) for m, w in zip(models, (0.0, 1.0))]
    # a match threshold that gives about 64 positives per image on this batch (set once, from the first forward)
    tp = steps[1].tp
    tp.run_forward(x)
    boxes = decode([m.nchw().float() for m in tp.det_maps])
    best = torch.cat([iou(boxes[b], xyxy_d[per_image[b]]).max(dim=1)[0] for b in range(B)])
    thresh = float(torch.sort(best, descending=True)[0][min(64 * B, best.numel() - 1)])
    for ts in steps:
        ts.loss_kw["iou_match_thresh"] = thresh
    out = steps[1].step(x, rows_d, masks, gt_cls)
    print(f"TrainStep, B = {B}, {S} x {S}, bf16, match threshold {thresh:.4f}: mask loss {float(out[8]):.5f}, {int(out[9])} positives")
    m = timed({"TrainStep.step, instance_mask_weight = 0": lambda: steps[0].step(x, rows_d, masks, gt_cls),
               "TrainStep.step, instance_mask_weight = 1": lambda: steps[1].step(x, rows_d, masks, gt_cls)})
    a, b = m["TrainStep.step, instance_mask_weight = 0"], m["TrainStep.step, instance_mask_weight = 1"]
    print(f"mask term per step: {b - a:.1f} us ({(b / a - 1) * 100:.2f} % of the step)")
