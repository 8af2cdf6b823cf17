"""Timing probe of the connected-component operator (GPU box): `postprocess.label_components` (labels + records) beside the path a user
had before it -- copy the planes to the host, then `scipy.ndimage.label` and `find_objects` per plane -- on the same masks in the same
process: 16 planes of 640 x 640 (one validation batch of the projector mask), with two contents:

  (a) lesion-like: two or three wavy ellipses per plane plus specks at p = 0.002 (a few hundred components a plane);
  (b) noise at p = 0.5 (tens of thousands of components a plane, far over the table cap: the worst case of the union phase).

Device: HIP events around one call after warm-up (workspace and output allocation included), median of `--repeats`.  Host: wall clock
around D2H + unpack + scipy on all 16 planes, median of `--host-repeats`.  The label maps of the two paths are compared.
The whole probe ends itself after `--time-limit` seconds.

  python tools/components_probe.py [--repeats 20]"""
import argparse
import os
import signal
import sys
import time

import numpy as np
import torch
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd.postprocess import filter_components, label_components, pack_masks

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--host-repeats", type=int, default=3)
ap.add_argument("--time-limit", type=int, default=300)
args = ap.parse_args()
signal.alarm(args.time_limit)
dev = torch.device("cuda", 0)
N, S = 16, 640


def lesion_planes(seed):
    rng = np.random.default_rng(seed)
    yy = torch.arange(S, device=dev, dtype=torch.float32)[:, None].expand(S, S)
    xx = torch.arange(S, device=dev, dtype=torch.float32)[None, :].expand(S, S)
    a = torch.zeros((N, S, S), dtype=torch.bool, device=dev)
    for i in range(N):
        for _ in range(int(rng.integers(2, 4))):
            cy, cx = rng.uniform(0.2, 0.8) * S, rng.uniform(0.2, 0.8) * S
            ry, rx = rng.uniform(0.04, 0.15) * S, rng.uniform(0.04, 0.15) * S
            wav = 1 + 0.08 * torch.sin(int(rng.integers(3, 9)) * torch.atan2(yy - cy, xx - cx) + float(rng.uniform(0, 6.28)))
            a[i] |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < wav
    return a | torch.from_numpy(rng.uniform(size=(N, S, S)) < 0.002).to(dev)


def host_path(packed):
    """What a user does without the operator: D2H of the packed planes, unpack, then scipy per plane."""
    dense = np.unpackbits(packed.cpu().numpy(), axis=-1, bitorder="little")[:, :, :S].astype(bool)
    out = []
    for m in dense:
        lab, n = ndimage.label(m)
        out.append((lab, n, ndimage.find_objects(lab)))
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def workload(name, planes):
    packed = pack_masks(planes)
    calls = {"label_components (labels + records)": lambda: label_components(packed, S, max_components=1024),
             "label_components (records only)": lambda: label_components(packed, S, max_components=1024, want_labels=False),
             "filter_components (min_area=16)": lambda: filter_components(packed, S, min_area=16)}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(args.repeats):                              # the variants alternate
        for k, fn in calls.items():
            t, r = timed(fn)
            times[k].append(t)
            if k.endswith("(labels + records)"):
                rec = r
    t_host = []
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        want = host_path(packed)
        t_host.append((time.perf_counter() - t0) * 1e3)
    labels, n_comp = rec["labels"].cpu().numpy(), rec["n_components"].cpu().numpy()
    same = all(np.array_equal(labels[i], w[0]) and n_comp[i] == w[1] for i, w in enumerate(want))
    print(f"({name}) {N} planes {S} x {S}: components per plane median {int(np.median(n_comp))}, max {int(n_comp.max())}; "
          f"set pixels {float(planes.float().mean()):.3f}; label maps equal scipy's: {same}")
    for k, t in times.items():
        print(f"({name}) device  {k:38s} ms: median {np.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}  ({args.repeats} repeats)")
    h, d = float(np.median(t_host)), float(np.median(times["label_components (labels + records)"]))
    print(f"({name}) host    D2H + scipy label + find_objects         ms: median {h:8.1f}  min {min(t_host):8.1f}  max {max(t_host):8.1f}  "
          f"({args.host_repeats} repeats); host / device = {h / d:.1f}x")


workload("a", lesion_planes(0))
workload("b", torch.from_numpy(np.random.default_rng(1).uniform(size=(N, S, S)) < 0.5).to(dev))
