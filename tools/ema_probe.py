"""Cost probe of the weight EMA (GPU box), BASELINE configs[2] size: batch 32, 640 x 640, bf16.

Two `TrainStep`s on two models of one state, `ema=None` and `ema=True`, in one process.  Each takes a few whole steps (warm-up: plans, first
launches, gradients in the buckets); then device events around the clip + update phase alone (`TrainStep._clip_and_update`: the sum of
squares per bucket, the clip coefficient, one optimiser launch per stepped bucket and the projector's -- with the EMA riding on those
launches -- plus, with EMA on, one `mtbt_ema_update` over all BatchNorm statistics and the counter copy), `--calls` calls per sample, the
two variants alternating, `--rounds` samples each.  Median and spread (min .. max) per call, and the same for the whole step.

  python tools/ema_probe.py [--batch 32] [--img 640] [--optimizer sgd|adamw] [--calls 20] [--rounds 9]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, TrainStep, init_synthetic_

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--img", type=int, default=640)
ap.add_argument("--optimizer", default="sgd", choices=["sgd", "adamw"])
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--step-calls", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, S = args.batch, args.img

torch.manual_seed(0)
g = torch.Generator().manual_seed(0)
x = torch.rand(B, 3, S, S, generator=g).to(dev)
rows = torch.tensor([[float(b), float(b % 2), 0.3 + 0.4 * ((b * 7) % 10) / 10, 0.5, 0.3, 0.35] for b in range(B)]).to(dev)
masks = (torch.rand(B, 1, S // 16, S // 16, generator=g) > 0.4).float().repeat_interleave(16, 2).repeat_interleave(16, 3).to(dev)
gt_cls = (torch.arange(B) % 2).to(dev)

models = [init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)).to(dev) for _ in range(2)]
models[1].load_state_dict(models[0].state_dict())
for m in models:
    m.set_compute_dtype(torch.bfloat16)
steps = {"ema off": TrainStep(models[0], (B, 3, S, S), optimizer=args.optimizer, lr=1e-6, iou_match_thresh=0.05),
         "ema on": TrainStep(models[1], (B, 3, S, S), optimizer=args.optimizer, lr=1e-6, iou_match_thresh=0.05, ema=True)}
n_param = sum(b.numel() for ts in [steps["ema on"]] for b in ts.params.buckets[ts.n_skip:])
print(f"B = {B}, {S} x {S}, bf16, {args.optimizer}: {n_param / 1e6:.2f} M stepped parameters in {len(steps['ema on'].params.buckets) - steps['ema on'].n_skip} "
      f"buckets, {steps['ema on'].bufs.buckets[0].numel()} buffer values; {args.calls} calls per sample, {args.rounds} samples, variants alternating")


def sample(f, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def report(title, variants, calls):
    for f in variants.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            times[name].append(sample(f, calls))
    med = {}
    for name, t in times.items():
        med[name] = statistics.median(t)
        print(f"{title:24s} {name:8s} per call (us): median {med[name]:9.1f}   min {min(t):9.1f}   max {max(t):9.1f}   samples " + " ".join(f"{v:.1f}" for v in t))
    print(f"{title:24s} on - off: {med['ema on'] - med['ema off']:+.1f} us ({(med['ema on'] / med['ema off'] - 1) * 100:+.2f} %)")


for ts in steps.values():                         # warm-up: whole steps, so that the buckets hold real gradients
    for _ in range(3):
        ts.step(x, rows, masks, gt_cls)
torch.cuda.synchronize()
report("clip + update phase", {k: ts._clip_and_update for k, ts in steps.items()}, args.calls)
report("whole step", {k: (lambda ts=ts: ts.step(x, rows, masks, gt_cls)) for k, ts in steps.items()}, args.step_calls)
