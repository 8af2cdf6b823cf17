"""Timing probe of the surface-distance operator (GPU box): `metrics.surface_distances` beside the path a user had before it -- copy the
planes to the host, then scipy erosion, Euclidean distance transform and numpy percentile per pair (MedPy's recipe) -- on the same
masks in the same process, at two workloads:

  (a) 16 semantic pairs at 640 x 640 (one validation batch of the projector mask);
  (b) 100 instance pairs at 1536 x 2048 (packed frame-resolution instance planes against matched ground truth).

Device: HIP events around one call after warm-up, median of `--repeats`.  Host: wall clock around copy + scipy on the first
`--host-pairs` pairs of the workload (all of (a); the EDT of a 3 Mpixel plane takes a good fraction of a second), median of
`--host-repeats`, scaled to the workload's pair count.  The two paths' hd / hd95 / assd are compared on those pairs.
Then `ValidationStep.step` at batch 16, 640 x 640 with `surface=None` and `surface=True`, the variants alternating.
The whole probe ends itself after `--time-limit` seconds.

  python tools/surface_probe.py [--repeats 10] [--skip-step]"""
import argparse
import os
import signal
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, ValidationStep, init_synthetic_, synthetic_images
from multitask_bonetumor_yolo_amd.metrics import surface_distances, surface_metrics
from multitask_bonetumor_yolo_amd.postprocess import pack_masks

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--host-repeats", type=int, default=3)
ap.add_argument("--host-pairs", type=int, default=8)
ap.add_argument("--time-limit", type=int, default=420)
ap.add_argument("--skip-step", action="store_true")
args = ap.parse_args()
signal.alarm(args.time_limit)
dev = torch.device("cuda", 0)
CROSS = ndimage.generate_binary_structure(2, 1)


def blob_pairs(n, H, W, seed):
    """n pairs of lesion-like masks, made on the device: a union of two or three ellipses with a wavy outline, and the same shifted and
    rescaled a little.  -> two bool tensors [n, H, W]."""
    rng = np.random.default_rng(seed)
    yy = torch.arange(H, device=dev, dtype=torch.float32)[:, None].expand(H, W)
    xx = torch.arange(W, device=dev, dtype=torch.float32)[None, :].expand(H, W)
    a, b = torch.zeros((n, H, W), dtype=torch.bool, device=dev), torch.zeros((n, H, W), dtype=torch.bool, device=dev)
    for i in range(n):
        for _ in range(int(rng.integers(2, 4))):
            cy, cx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W
            ry, rx = rng.uniform(0.05, 0.2) * H, rng.uniform(0.05, 0.2) * W
            wav = 1 + 0.08 * torch.sin(int(rng.integers(3, 9)) * torch.atan2(yy - cy, xx - cx) + float(rng.uniform(0, 6.28)))
            a[i] |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < wav
            dy, dx, s = rng.uniform(-0.02, 0.02) * H, rng.uniform(-0.02, 0.02) * W, rng.uniform(0.9, 1.1)
            b[i] |= ((yy - cy - dy) / (ry * s)) ** 2 + ((xx - cx - dx) / (rx * s)) ** 2 < wav
    return a, b


def host_path(pa, pb, W, q=0.95):
    """What a user does without the operator: D2H of the packed planes, unpack, then MedPy's recipe with scipy."""
    a = np.unpackbits(pa.cpu().numpy(), axis=-1, bitorder="little")[:, :, :W].astype(bool)
    b = np.unpackbits(pb.cpu().numpy(), axis=-1, bitorder="little")[:, :, :W].astype(bool)
    out = []
    for x, y in zip(a, b):
        ex, ey = x ^ ndimage.binary_erosion(x, CROSS, border_value=0), y ^ ndimage.binary_erosion(y, CROSS, border_value=0)
        xy, yx = ndimage.distance_transform_edt(~ey)[ex], ndimage.distance_transform_edt(~ex)[ey]
        out.append((max(xy.max(), yx.max()), np.percentile(np.hstack((xy, yx)), 100 * q), 0.5 * (xy.mean() + yx.mean())))
    return np.array(out)


def workload(name, n, H, W, seed, host_pairs):
    a, b = blob_pairs(n, H, W, seed)
    pa, pb = pack_masks(a), pack_masks(b)
    del a, b
    for _ in range(2):
        rec = surface_distances(pa, pb, W, quantiles=(0.95,), tol2=4)
    torch.cuda.synchronize()
    t_dev = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rec = surface_distances(pa, pb, W, quantiles=(0.95,), tol2=4)
        e1.record()
        e1.synchronize()
        t_dev.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in rec.items()}
    got = surface_metrics(host, tolerance=2.0)
    t_final = (time.perf_counter() - t0) * 1e3
    hp = min(host_pairs, n)
    t_host = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        want = host_path(pa[:hp], pb[:hp], W)
        t_host.append((time.perf_counter() - t0) * 1e3 * n / hp)
    err = max(np.abs(got[k][:hp] - want[:, i]).max() for i, k in enumerate(("hd", "hd95", "assd")))
    d, h = float(np.median(t_dev)), float(np.median(t_host))
    edges = host["n_edge"].sum(axis=1)
    print(f"({name}) {n} pairs {H} x {W}: edge pixels per pair median {int(np.median(edges))}, max {int(edges.max())}; undefined {int((~got['defined']).sum())}")
    print(f"({name}) device  surface_distances  ms: median {d:9.3f}  min {min(t_dev):9.3f}  max {max(t_dev):9.3f}  ({args.repeats} repeats; "
          f"+ {t_final:.2f} ms D2H of the records and host finalisation)")
    print(f"({name}) host    D2H + scipy        ms: median {h:9.1f}  min {min(t_host):9.1f}  max {max(t_host):9.1f}  ({args.host_repeats} repeats on "
          f"{hp} of {n} pairs, scaled to {n})")
    print(f"({name}) host / device = {h / d:.1f}x; max |device - host| over hd, hd95, assd on those pairs = {err:.3e}")


workload("a", 16, 640, 640, 0, 16)
workload("b", 100, 1536, 2048, 1, args.host_pairs)

if not args.skip_step:
    B, S = 16, 640
    torch.manual_seed(0)
    model = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), seed=0).to(dev)
    proj = torch.nn.Conv2d(model.proto_ch, 1, 1).to(dev)
    imgs = synthetic_images(B, S, seed=0).to(dev)
    gt = torch.tensor([[float(b), float(b % 2), 0.5, 0.5, 0.3, 0.3] for b in range(B)], device=dev)
    masks = blob_pairs(B, S, S, 2)[0][:, None].float()
    cls = torch.arange(B, device=dev) % 2
    steps = {"surface=None": ValidationStep(model, projector=proj, img_size=S), "surface=True": ValidationStep(model, projector=proj, img_size=S, surface=True)}
    for vs in steps.values():
        for _ in range(2):
            vs.step(imgs, gt, masks, cls)
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(args.repeats):
        for name, vs in steps.items():
            vs.reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            vs.step(imgs, gt, masks, cls)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    for name, t in times.items():
        print(f"ValidationStep.step batch {B}, {S} x {S}, {name:13s} ms: median {np.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}")
    sd = steps["surface=True"].surface.compute()
    print(f"surface share of the step: {np.median(times['surface=True']) - np.median(times['surface=None']):.3f} ms; its pairs: {sd}")
