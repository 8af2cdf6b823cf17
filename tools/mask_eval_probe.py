"""Timing probe of the instance-mask evaluation (GPU box): `mtbt_mask_pair_counts` on the bit-packed masks of one calibrated synthetic
step (batch 16, 640 x 640, K = 100, identity frames, 1 - 3 ground-truth masks per image) beside the only formulation there was before
it -- `unpack_masks`, boolean `&`, `.sum` in torch -- on the same inputs in the same process, plus `pack_masks` and `mtbt_mask_eval`.
Device events around 20 launches per variant after warm-up, the variants alternating, 6 rounds; prints the per-launch mean of every
round and the detection-plane bytes the pair counts read per second (all K planes: counts = None).

  python tools/mask_eval_probe.py [--batch 16] [--img 640]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, calibrate_synthetic_heads_, init_synthetic_, postprocess as pp
from multitask_bonetumor_yolo_amd.metrics import DeviceMaskMeanAveragePrecision as MaskMAP

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--img", type=int, default=640)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--rounds", type=int, default=6)
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, S = args.batch, args.img

torch.manual_seed(0)
model = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)).to(dev).eval()
model.set_compute_dtype(torch.bfloat16)
x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)).to(dev)
calibrate_synthetic_heads_(model, x[: min(B, 4)].contiguous())
with torch.no_grad():
    out = model(x, "infer")
    feats, mc, protos = out["segment_protos"]
    det = pp.detect_and_segment(out["detect_features"], mc, protos, S, masks=False)
mc, protos = mc.float(), protos.float().contiguous(memory_format=torch.channels_last)
counts, K = det["counts"], det["keep_anchor"].shape[1]
r = pp.masks_to_frames(protos, mc, det["keep_anchor"], None, det["boxes"], [(S, S, 1.0)] * B, up=S / protos.shape[3], crop=False)
planes = torch.stack(r["masks"])                                         # [B, K, S, pitch]: every slot holds a mask (counts = None)
pitch = planes.shape[3]

# ground truth: 1 - 3 boxes per image cut out of one random-blob mask per image, as ValidationStep builds it
g = torch.Generator().manual_seed(1)
rows = []
for b in range(B):
    for _ in range(1 + b % 3):
        wh = torch.rand(2, generator=g) * 0.4 + 0.1
        cxy = torch.rand(2, generator=g) * (1 - wh) + wh / 2
        rows.append(torch.cat([torch.tensor([float(b), float(b % 2)]), cxy, wh]))
rows = torch.stack(rows).to(dev)
dense_gt = (torch.rand(B, S // 16, S // 16, generator=g) > 0.4).float().to(dev).repeat_interleave(16, 1).repeat_interleave(16, 2)
gt_image, gt_label = MaskMAP.gt_rows_fields(rows, B)
px = torch.stack([(rows[:, 2] - rows[:, 4] / 2) * S, (rows[:, 3] - rows[:, 5] / 2) * S, (rows[:, 2] + rows[:, 4] / 2) * S,
                  (rows[:, 3] + rows[:, 5] / 2) * S], 1).clamp_(0, S)
gt = pp.pack_masks(dense_gt, boxes=px, plane_of=gt_image)
M = gt.shape[0]
per_image = [torch.nonzero(gt_image == b).flatten() for b in range(B)]
print(f"B = {B}, K = {K}, {S} x {S}, pitch {pitch}: {planes.numel() / 1e6:.1f} MB of detection planes, {M} GT planes ({gt.numel() / 1e6:.2f} MB); "
      f"kept boxes per image {counts.tolist()}")


def torch_pair_counts():
    """The formulation available without the kernel: one byte per pixel, then boolean algebra."""
    inter = torch.zeros((M, K), dtype=torch.int64, device=dev)
    for b in range(B):
        d = pp.unpack_masks(planes[b], S)                                # [K, S, S] bool
        gb = pp.unpack_masks(gt[per_image[b]], S)                        # [G, S, S]
        inter[per_image[b]] = (gb[:, None] & d[None]).sum((2, 3))
    return inter


tables = MaskMAP.pair_tables_uniform(planes, None, gt, gt_image)
same = torch.equal(tables[0].to(torch.int64), torch_pair_counts())
print(f"kernel table == torch table: {same}")
metric = MaskMAP()
scores, labels = det["scores"].float().contiguous(), det["labels"].long().contiguous()


def eval_only():
    metric.reset()
    metric._evaluate(tables, scores, labels, None, gt_image, gt_label)


variants = {
    "mtbt_mask_pair_counts": lambda: MaskMAP.pair_tables_uniform(planes, None, gt, gt_image),
    "torch unpack, &, sum": torch_pair_counts,
    "mtbt_mask_eval (T = 10)": eval_only,
    "mtbt_pack_masks (GT)": lambda: pp.pack_masks(dense_gt, boxes=px, plane_of=gt_image),
}
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
    mean = sum(t) / len(t)
    line = f"{name:26s} per launch (us) rounds: " + " ".join(f"{v:9.1f}" for v in t) + f"   mean {mean:9.1f}"
    if name == "mtbt_mask_pair_counts":
        line += f"  -> {planes.numel() / mean / 1e6:.2f} TB/s of detection planes (copy rate 6.29 TB/s)"
    print(line)
k_us, t_us = (sum(times[n]) / len(times[n]) for n in ("mtbt_mask_pair_counts", "torch unpack, &, sum"))
print(f"kernel / torch formulation: {k_us:.1f} us / {t_us:.1f} us = {k_us / t_us:.4f}")
