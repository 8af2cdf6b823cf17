"""Timing probe of the mask vote over fused detections (GPU box) on the benchmark's calibrated synthetic model (batch 16, 640 x 640, bf16,
top_k = 100), M = 2 (views 0, 1) and M = 8 (views 0 - 7) sources.  One process, warm; device events around `--reps` back-to-back calls, the
variants alternating, `--rounds` rounds; prints every reading and the median per call and, before the `launch` timings, a sha256 of each of
their results (planes, boxes, vote_coeff, vote_weight), so that two builds can be compared byte for byte at the size that is timed.

  whole    detect_fused(masks="vote") against detect_fused(masks=True) (the leaders' masks): M forwards + NMS + fusion + masks
  masks    the mask half alone on kept forward results: ensemble._leader_masks against vote_masks + unpack (identity frames, dense uint8)
  launch   vote_masks (mtbt_vote_masks: coefficient launch + mask launch, packed planes) against M calls of masks_to_frames
           (mtbt_masks_to_frames), one per source on its own kept list: the same frames, the same number of planes per call

  python tools/mask_vote_probe.py [--batch 16] [--img 640]"""
import argparse
import hashlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, calibrate_synthetic_heads_, detect_fused, ensemble, init_synthetic_, postprocess as pp

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--img", type=int, default=640)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()


def digest(r):
    """sha256 of a frame operator's result: the packed planes, the boxes and, where they exist, vote_coeff and vote_weight."""
    h = hashlib.sha256()
    for t in list(r["masks"]) + [r.get(k) for k in ("boxes", "vote_coeff", "vote_weight")]:
        if t is not None:
            h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


dev = torch.device("cuda", 0)
B, S = args.batch, args.img

torch.manual_seed(0)
model = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)).to(dev).eval()
model.set_compute_dtype(torch.bfloat16)
x = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(0)).to(dev)
calibrate_synthetic_heads_(model, x[: min(B, 4)].contiguous())
frames = [(S, S, 1.0)] * B


def timed(variants):
    """variants: name -> callable.  Median ms per call and the readings."""
    readings = {k: [] for k in variants}
    for r in range(args.rounds + 1):                                       # round 0 is the warm-up
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            e1.synchronize()
            if r:
                readings[name].append(e0.elapsed_time(e1) / args.reps)
    for name, v in readings.items():
        print(f"  {name}: ms per call, {args.reps} calls per reading: {' '.join(f'{t:.3f}' for t in v)}; median {statistics.median(v):.3f}", flush=True)


for M in (2, 8):
    views = tuple(range(M))
    with torch.no_grad():
        outs = [model(pp.orient_batch(x, v), "infer") for v in views]
        dets = [pp.detect_and_segment(o["detect_features"], o["segment_protos"][1], o["segment_protos"][2], S, masks=False) for o in outs]
    fused = pp.fuse_detections(dets, img_size=S, orients=views, want_members=True)
    up = S / outs[0]["segment_protos"][2].shape[3]
    torch.cuda.synchronize()
    print(f"M = {M}: B = {B}, {S} x {S}, top_k = {fused['scores'].shape[1]}; fused rows per image {fused['counts'].tolist()}, rows with >= 2 members "
          f"{int((fused['n_members'] >= 2).sum())}, largest cluster {int(fused['n_members'].max())}", flush=True)
    timed({"whole, masks=True  ": lambda: detect_fused(model, x, S, views=views, masks=True),
           "whole, masks='vote'": lambda: detect_fused(model, x, S, views=views, masks="vote")})
    timed({"masks, leaders     ": lambda: ensemble._leader_masks(fused, outs, views, S),
           "masks, vote        ": lambda: torch.stack([pp.unpack_masks(p, S) for p in pp.vote_masks(fused, outs, views, None, frames, up=up)["masks"]])})
    buf = torch.empty((pp._frame_layout(frames, fused["scores"].shape[1], up)[1],), dtype=torch.uint8, device=dev)
    srcs = [(o["segment_protos"][2].float(), o["segment_protos"][1].float()) for o in outs]      # fp32 once: neither side converts per call
    pairs = [(mc, protos) for protos, mc in srcs]

    def per_source(crop):
        for (protos, mc), d in zip(srcs, dets):
            pp.masks_to_frames(protos, mc, d["keep_anchor"], d["counts"], d["boxes"], frames, up=up, crop=crop, out=buf)

    for crop in (False, True):
        print(f"  vote_masks M={M} crop={crop!s:5} sha256 {digest(pp.vote_masks(fused, pairs, views, None, frames, crop=crop, out=buf, up=up))}", flush=True)
        for m, ((protos, mc), d) in enumerate(zip(srcs, dets)):
            r = pp.masks_to_frames(protos, mc, d["keep_anchor"], d["counts"], d["boxes"], frames, up=up, crop=crop, out=buf)
            print(f"  masks_to_frames source {m} of {M} crop={crop!s:5} sha256 {digest(r)}", flush=True)
        timed({f"launch, vote_masks crop={crop!s:5}           ": lambda: pp.vote_masks(fused, pairs, views, None, frames, crop=crop, out=buf, up=up),
               f"launch, {M} x masks_to_frames crop={crop!s:5}": lambda: per_source(crop)})
