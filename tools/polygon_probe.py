"""Timing probe of the polygon rasteriser (GPU box): `postprocess.fill_polygons` beside the path a user had before it -- draw the
polygons on the host with PIL `ImageDraw.polygon`, pack the bits and upload the planes -- on the same polygons in the same process:

  (a) 16 canvases of 640 x 640, each the union of 3 wavy polygons of 200 vertices (one training batch's canvas masks);
  (b) 100 planes of 2048 x 1536 (H x W), one such polygon each (the instance ground truth of a large image).

Device: the whole call (host quantisation and packing, one upload, the launch) under a host clock that ends in a synchronise, and the
kernel part alone under HIP events with the upload already queued; every shape warmed up, medians of `--repeats`, the two workloads
alternating.  Host: wall clock around PIL + packbits + H2D of all planes, median of `--host-repeats`.  PIL's fill rule is not this
project's (it paints boundary pixels): the two results are compared only by the share of pixels that differ, which is printed.
The whole probe ends itself after `--time-limit` seconds.

  python tools/polygon_probe.py [--repeats 20]"""
import argparse
import os
import signal
import sys
import time

import numpy as np
import torch
from PIL import Image, ImageDraw

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multitask_bonetumor_yolo_amd.postprocess as pp
from multitask_bonetumor_yolo_amd.postprocess import fill_polygons, unpack_masks

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--host-repeats", type=int, default=3)
ap.add_argument("--time-limit", type=int, default=300)
args = ap.parse_args()
signal.alarm(args.time_limit)
dev = torch.device("cuda", 0)


def wavy(rng, H, W, n=200):
    t = 2 * np.pi * np.arange(n) / n
    r = rng.uniform(0.08, 0.3) * min(H, W) * (1 + 0.15 * np.sin(int(rng.integers(3, 9)) * t + rng.uniform(0, 6.28)))
    return np.stack([rng.uniform(0.2, 0.8) * W + r * np.cos(t), rng.uniform(0.2, 0.8) * H + r * np.sin(t)], axis=1)


def host_path(planes, H, W):
    """What a user does without the operator: PIL per plane, pack the bits, upload."""
    pitch = 8 * ((W + 63) // 64)
    out = np.zeros((len(planes), H, pitch), dtype=np.uint8)
    for k, polys in enumerate(planes):
        im = Image.new("1", (W, H), 0)
        d = ImageDraw.Draw(im)
        for p in polys:
            d.polygon([tuple(v) for v in p.tolist()], fill=1)
        bits = np.packbits(np.asarray(im, dtype=bool), axis=-1, bitorder="little")
        out[k, :, :bits.shape[1]] = bits
    t = torch.from_numpy(out).to(dev)
    torch.cuda.synchronize()
    return t


def whole_call(planes, H, W):
    t0 = time.perf_counter()
    r = fill_polygons(planes, H, W, records=True, device=dev)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


class _Timed:
    """The loaded library with HIP events recorded right around mtbt_fill_polygons: what the stream does for one call after the upload
    (the two clears, the fill kernel, the box kernel), the host packing left out."""

    def __init__(self, lib):
        self.lib, self.e0, self.e1 = lib, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def mtbt_fill_polygons(self, *a):
        self.e0.record()
        rc = self.lib.mtbt_fill_polygons(*a)
        self.e1.record()
        return rc


def device_part(planes, H, W):
    timed, load = _Timed(pp.L.load()), pp.L.load
    pp.L.load = lambda: timed
    try:
        fill_polygons(planes, H, W, records=True, device=dev)
    finally:
        pp.L.load = load
    timed.e1.synchronize()
    return timed.e0.elapsed_time(timed.e1)


rng = np.random.default_rng(0)
work = {"a": ([[wavy(rng, 640, 640) for _ in range(3)] for _ in range(16)], 640, 640),
        "b": ([[wavy(rng, 2048, 1536)] for _ in range(100)], 2048, 1536)}
for planes, H, W in work.values():
    for _ in range(3):
        whole_call(planes, H, W)
        device_part(planes, H, W)
calls, kern = {k: [] for k in work}, {k: [] for k in work}
for _ in range(args.repeats):                                      # the workloads alternate
    for k, (planes, H, W) in work.items():
        calls[k].append(whole_call(planes, H, W)[0])
        kern[k].append(device_part(planes, H, W))
for k, (planes, H, W) in work.items():
    t_host = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        ref = host_path(planes, H, W)
        t_host.append((time.perf_counter() - t0) * 1e3)
    got, area, _ = fill_polygons(planes, H, W, records=True, device=dev)
    differ = (unpack_masks(got, W) != unpack_masks(ref, W)).float().mean().item()
    print(f"({k}) {len(planes)} planes {H} x {W}, {sum(len(p) for p in planes)} polygons of 200 vertices: set pixels "
          f"{area.sum().item() / (len(planes) * H * W):.3f}; pixels that differ from PIL's rule {differ:.5f}")
    for name, t in (("fill_polygons, whole call (host packing + upload + kernels)", calls[k]), ("fill_polygons, kernels (HIP events around the entry point)", kern[k])):
        print(f"({k}) device  {name:62s} ms: median {np.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}  ({args.repeats} repeats)")
    h, d = float(np.median(t_host)), float(np.median(calls[k]))
    print(f"({k}) host    PIL ImageDraw.polygon + packbits + upload                    ms: median {h:8.1f}  min {min(t_host):8.1f}  max {max(t_host):8.1f}  "
          f"({args.host_repeats} repeats); host / whole call = {h / d:.1f}x")
