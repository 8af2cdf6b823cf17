#!/usr/bin/env python3
"""Time the affine warp (mtbt_warp_batch) at the identity and at 33 degrees beside mtbt_augment_batch with the letterbox geometry on the
same sources, in one process, alternating the three.  Both write 16 B per canvas pixel; a 33-degree time above the identity time is the
cost of the source gather.  usage: python tests/bench_warp_vs_augment.py [H0] [W0] [S] [repeats]"""
import math, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import preprocess as P
H0, W0, S, REP = (int(v) for v in (sys.argv[1:5] + ["768", "1024", "640", "5"][len(sys.argv) - 1:]))


def forward(angle):
    s, t = S / max(H0, W0), math.radians(angle)
    lin = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]]) * s
    return np.concatenate([lin, (np.array([S / 2, S / 2]) - lin @ np.array([W0 / 2, H0 / 2]))[:, None]], axis=1)


def timed(fn, iters=50):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


rng = np.random.default_rng(0)
for B in (16, 32):
    di = [torch.from_numpy(rng.integers(0, 256, size=(H0, W0, 3), dtype=np.uint8)).cuda() for _ in range(B)]
    dm = [torch.from_numpy(rng.integers(0, 256, size=(H0, W0), dtype=np.uint8)).cuda() for _ in range(B)]
    geom = P.letterbox_geometry([(H0, W0)] * B, S)
    ident = P.affine_coefficients(np.stack([forward(0.0)] * B))       # the letterbox scale about the centre, no turn
    turned = P.affine_coefficients(np.stack([forward(33.0)] * B))
    runs = {"augment_batch letterbox": lambda: P.augment_batch(di, dm, geom, None, S), "warp_batch 0 deg": lambda: P.warp_batch(di, dm, ident, None, S),
            "warp_batch 33 deg": lambda: P.warp_batch(di, dm, turned, None, S)}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(REP):                                                # alternate, so that drift hits the three alike
        for k, fn in runs.items():
            us[k].append(timed(fn))
    out_mb = B * 4 * S * S * 4 / 1e6
    base = min(us["augment_batch letterbox"])
    for k, v in us.items():
        print(f"B={B} {k:24s} best {min(v):8.1f} us  median {sorted(v)[len(v) // 2]:8.1f} us  spread {max(v) - min(v):6.1f} us  "
              f"{out_mb / min(v) * 1e3:6.0f} GB/s of output  x{min(v) / base:.2f} of augment_batch", flush=True)
