"""Timing probe of the device CLAHE (GPU box): `mtbt_clahe_batch` on radiograph-like images (tests/clahe_reference.py `radiograph`:
a black background around a bright noisy body) at 8 x 8 tiles and clip limit 2.0, three workloads:

  (a) 16 images of 1536 x 2048 x 3     (b) 1 image of 3000 x 3000 x 3     (c) 16 images of 640 x 640 x 3

Device time per call: HIP events around `--calls` back-to-back calls of the entry point on prepared descriptors and one workspace (the
clear of the histograms and the three launches; no host work in the window), every workload warmed up, the workloads alternating, median
and min .. max of `--rounds` readings.  Each time is set against the copy bound: the source read twice (histograms, apply) plus the
destination written once, at the 6.29 TB/s copy rate DESIGN.md uses.  The output of every workload is compared with the numpy reference
on its first image before anything is timed.  `--alt LIB` times a second build of the library beside the first in the same process,
alternating (a build with -DMTBT_CLAHE_SEG_PIXELS=1073741824 is the one-workgroup-per-tile form of the histogram pass).
If cv2 can be imported, the host time of cv2's CLAHE on the same images and the count of values that differ from it by 0, 1 and more
than 1 are printed as well; if not, the probe says so and runs without it.  The whole probe ends itself after `--time-limit` seconds.

  python tools/clahe_probe.py [--rounds 7] [--calls 20] [--alt other/libmtbt_hip.so]"""
import argparse
import ctypes as C
import os
import signal
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clahe_reference as R  # noqa: E402
from multitask_bonetumor_yolo_amd import _lib as L  # noqa: E402
from multitask_bonetumor_yolo_amd.preprocess import clahe_clip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--alt", default=None)
ap.add_argument("--time-limit", type=int, default=300)
args = ap.parse_args()
signal.alarm(args.time_limit)
dev = torch.device("cuda", 0)
GRID, LIMIT, COPY_RATE = (8, 8), 2.0, 6.29e12


def bind(path):
    lib = C.CDLL(path)
    for name in ("mtbt_clahe_batch", "mtbt_clahe_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SYMBOLS[name]
    return lib


libs = {"library": L.load()}
if args.alt:
    libs["alt"] = bind(args.alt)

rng = np.random.default_rng(0)
work = {}
for key, (n, H, W) in {"a": (16, 1536, 2048), "b": (1, 3000, 3000), "c": (16, 640, 640)}.items():
    host = [R.radiograph(rng, H, W, 3) for _ in range(min(n, 2))]                     # two distinct images, repeated: the timing sees n buffers
    src = [torch.from_numpy(host[i % len(host)]).to(dev) for i in range(n)]
    dst = [torch.empty_like(t) for t in src]
    descs = (L.ClaheImage * n)()
    for d, s, o in zip(descs, src, dst):
        d.src, d.dst, d.height, d.width, d.channels, d.clip = s.data_ptr(), o.data_ptr(), H, W, 3, clahe_clip(LIMIT, H, W, GRID)
        d.src_row_stride = d.dst_row_stride = 3 * W
    nbytes = libs["library"].mtbt_clahe_workspace_bytes(descs, n, *GRID)
    work[key] = dict(n=n, H=H, W=W, host=host, src=src, dst=dst, descs=descs, nbytes=nbytes, ws=torch.empty(nbytes, dtype=torch.uint8, device=dev))


def call(lib, w):
    rc = lib.mtbt_clahe_batch(w["descs"], w["n"], *GRID, w["ws"].data_ptr(), w["nbytes"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise RuntimeError(f"mtbt_clahe_batch: {rc}")


def timed(lib, w):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.calls):
        call(lib, w)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / args.calls                                      # microseconds per call


for name, lib in libs.items():                                                         # right before fast: the first image of every workload
    for key, w in work.items():
        w["dst"][0].zero_()
        call(lib, w)
        torch.cuda.synchronize()
        ref = R.clahe(w["host"][0], GRID, clahe_clip(LIMIT, w["H"], w["W"], GRID))
        if not np.array_equal(w["dst"][0].cpu().numpy(), ref):
            raise SystemExit(f"({key}) {name}: the output differs from tests/clahe_reference.py")
        for _ in range(3):
            timed(lib, w)
print("outputs equal the numpy reference on the first image of every workload")

times = {(name, key): [] for name in libs for key in work}
for _ in range(args.rounds):
    for key, w in work.items():
        for name, lib in libs.items():
            times[name, key].append(timed(lib, w))
for key, w in work.items():
    moved = 3 * w["n"] * w["H"] * w["W"] * 3                                            # source twice, destination once
    bound = moved / COPY_RATE * 1e6
    for name in libs:
        t = times[name, key]
        med = float(np.median(t))
        print(f"({key}) {w['n']:2d} x {w['H']} x {w['W']} x 3  {name:8s} us per call: median {med:8.1f}  min {min(t):8.1f}  max {max(t):8.1f}  "
              f"({args.rounds} readings of {args.calls} calls); copy bound {bound:7.1f} us ({moved / 1e6:.1f} MB at 6.29 TB/s): {med / bound:.2f}x the bound")

try:
    import cv2
except ImportError:
    cv2 = None
    print("cv2 is not installed here: no host time and no pixel comparison with cv2's CLAHE")
if cv2 is not None:
    for key, w in work.items():
        op = cv2.createCLAHE(clipLimit=LIMIT, tileGridSize=GRID)
        img = w["host"][0]
        t0 = time.perf_counter()
        theirs = op.apply(np.ascontiguousarray(R.keys(img).astype(np.uint8)))
        ms = (time.perf_counter() - t0) * 1e3
        ours = R.clahe(np.ascontiguousarray(R.keys(img).astype(np.uint8)), GRID, clahe_clip(LIMIT, w["H"], w["W"], GRID))
        diff = np.abs(ours.astype(int) - theirs.astype(int))
        print(f"({key}) cv2 on the key plane of one image, host: {ms:.1f} ms; values that differ from cv2 by 0 / 1 / more: "
              f"{int((diff == 0).sum())} / {int((diff == 1).sum())} / {int((diff > 1).sum())}")
