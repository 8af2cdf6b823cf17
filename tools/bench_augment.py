#!/usr/bin/env python3
"""Time `preprocess.augment_batch` beside `preprocess.letterbox_batch` on one batch of BTXRD-sized radiographs (default 16 images of
about 2048 x 1536 -> 640 x 640), all in one process on the same device buffers: the letterbox, the augmentation at the identity
geometry (same output, same source bytes), the identity geometry with an intensity table, and orient = 4 (transposed: each output
row gathers down a column of the source), and `preprocess.mosaic_batch` on B canvases of four of the same sources each: once with random
centres in the middle half of the canvas (corner placement, the resized sizes of the identity geometry) and once with the degenerate
centre (S, S), where a canvas is the identity augmentation of its first tile.  Device events around 20 calls per variant after warm-up,
the variants alternating, 5 rounds; the median and the rounds per variant, the ratio to the letterbox and, for the mosaic, the ratio to the augmentation
at the identity geometry are printed, after a sha256 of each variant's output (image and mask tensors), so that two builds can be compared at
the size that is timed.  usage: python tools/bench_augment.py [B] [H0] [W0] [S]"""
import hashlib, os, sys, statistics
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import preprocess as P
B, H0, W0, S = (int(v) for v in (sys.argv[1:5] + ["16", "2048", "1536", "640"][len(sys.argv) - 1:]))
rng = np.random.default_rng(0)
imgs = [rng.integers(0, 256, size=(H0 - 8 * i, W0 + 4 * i, 3), dtype=np.uint8) for i in range(B)]
masks = [rng.integers(0, 256, size=a.shape[:2], dtype=np.uint8) for a in imgs]
di, dm = [torch.from_numpy(a).cuda() for a in imgs], [torch.from_numpy(a).cuda() for a in masks]
ident = P.letterbox_geometry([a.shape[:2] for a in imgs], S)
transposed = ident.copy()
transposed[:, 4] = 4
lut = torch.from_numpy(P.sample_photometric(B, rng)).cuda()
index = np.stack([(np.arange(B) + 5 * t) % B for t in range(4)], axis=1)          # tile 0 of canvas i is image i
mgeom = ident[index]                                                              # [B, 4, 8]
centres = np.stack([4 * np.floor(rng.uniform(0.25, 0.75, B) * S / 4), np.floor(rng.uniform(0.25, 0.75, B) * S)], axis=1).astype(np.int32)
for t in range(4):                                                                # the corner facing the centre touches it
    mgeom[:, t, 2] = centres[:, 0] - (0 if t & 1 else mgeom[:, t, 0])
    mgeom[:, t, 3] = centres[:, 1] - (0 if t & 2 else mgeom[:, t, 1])
degenerate = np.full((B, 2), S, dtype=np.int32)
variants = {
    "letterbox_batch": lambda: P.letterbox_batch(di, dm, S),
    "augment identity": lambda: P.augment_batch(di, dm, ident, None, S),
    "augment identity + table": lambda: P.augment_batch(di, dm, ident, lut, S),
    "augment orient=4": lambda: P.augment_batch(di, dm, transposed, None, S),
    "mosaic random centres": lambda: P.mosaic_batch(di, dm, index, mgeom, centres, None, S),
    "mosaic centre (S, S)": lambda: P.mosaic_batch(di, dm, index, ident[index], degenerate, None, S),
}
assert torch.equal(variants["letterbox_batch"]()[0], variants["augment identity"]()[0])
assert torch.equal(variants["mosaic centre (S, S)"]()[0], variants["augment identity"]()[0])
for k, f in variants.items():
    print(f"{k:26s} sha256 {hashlib.sha256(b''.join(t.cpu().numpy().tobytes() for t in f()[:2])).hexdigest()}")
for f in variants.values():
    for _ in range(5):
        f()
torch.cuda.synchronize()
times = {k: [] for k in variants}
for _ in range(5):
    for k, f in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            f()
        b.record(); torch.cuda.synchronize()
        times[k].append(a.elapsed_time(b) / 20 * 1e3)
base, aug = statistics.median(times["letterbox_batch"]), statistics.median(times["augment identity"])
out_bytes = B * 4 * S * S * 4
for k, t in times.items():
    us = statistics.median(t)
    print(f"{k:26s} {us:8.1f} us / batch of {B} (min {min(t):.1f}, max {max(t):.1f}, rounds {' '.join(f'{v:.1f}' for v in t)}; {out_bytes / us / 1e3:.0f} GB/s of output)  x{us / base:.3f} of letterbox_batch"
          + (f", x{us / aug:.3f} of augment identity" if k.startswith("mosaic") else ""))
