"""Timing probe of the weighted boxes fusion (GPU box): `mtbt_fuse_detections` on the detection lists of the benchmark's calibrated
synthetic model (batch 16, 640 x 640, bf16, K = 100), one list per dihedral view, for M = 2 and M = 4 sources.  One process, warm;
device events around `--launches` back-to-back launches of the same argument struct, the variants alternating, `--rounds` rounds; prints
every reading, the median per launch and what the fusion found (candidates and clusters per image).

  python tools/box_fuse_probe.py [--batch 16] [--img 640]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, _lib as L, calibrate_synthetic_heads_, init_synthetic_, postprocess as pp

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--img", type=int, default=640)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()
dev = torch.device("cuda", 0)
B, S = args.batch, args.img

torch.manual_seed(0)
model = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)).to(dev).eval()
model.set_compute_dtype(torch.bfloat16)
x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)).to(dev)
calibrate_synthetic_heads_(model, x[: min(B, 4)].contiguous())
views = (0, 1, 2, 3)
dets = []
with torch.no_grad():
    for v in views:
        out = model(pp.orient_batch(x, v), "infer")
        _, mc, protos = out["segment_protos"]
        dets.append(pp.detect_and_segment(out["detect_features"], mc, protos, S, masks=False))
print(f"B = {B}, {S} x {S}, K = {dets[0]['scores'].shape[1]}; kept boxes per image and view: {[d['counts'].tolist() for d in dets]}")

lib = L.load()
stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
variants = {}
for M in (2, 4):
    a, o, _ = pp._fuse_args(dets[:M], S, list(views[:M]), None, 0.55, 0.0, None)
    L.check(lib.mtbt_fuse_detections(C.byref(a), stream), "mtbt_fuse_detections")
    torch.cuda.synchronize()
    print(f"M = {M}: clusters per image {o['n_clusters'].tolist()}, kept {o['counts'].tolist()}, "
          f"clusters with >= 2 members {int((o['n_members'] >= 2).sum())}, largest {int(o['n_members'].max())}")
    variants[M] = (a, o)

readings = {M: [] for M in variants}
for r in range(args.rounds + 1):                                           # round 0 is the warm-up
    for M, (a, _) in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            lib.mtbt_fuse_detections(C.byref(a), stream)
        e1.record()
        e1.synchronize()
        if r:
            readings[M].append(e0.elapsed_time(e1) * 1000.0 / args.launches)
for M, v in readings.items():
    print(f"M = {M}: us per launch, {args.launches} launches per reading: {' '.join(f'{t:.1f}' for t in v)}; median {statistics.median(v):.1f}")
