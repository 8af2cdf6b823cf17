"""Timing probe of sliced inference's merge and mask launches (GPU box) on one 2048 x 1536 image at S = 640: 12 tiles plus the full view,
K = 100 slots per tile, top_k = 100 merged rows, on the planted detection lists of tests/slice_reference.py (no model).  One process,
warm; device events around `--reps` back-to-back calls of the Python wrappers (so the host's share -- the tile table, its upload, the
frame tile choice -- is inside every reading), the variants alternating, `--rounds` rounds; prints every reading and the median per call
and, before the mask timings, a sha256 of each of their results (planes, boxes, vote_coeff, vote_weight), so that two builds can be
compared byte for byte at the size that is timed.

  merge    postprocess.merge_tiles (mtbt_merge_tiles: one workgroup for the image's 1300 slots)
  vote     postprocess.vote_tile_masks (mtbt_vote_tile_masks: coefficient launch + mask launch, 100 packed planes of 1536 x 2048)
  frame    postprocess.masks_to_frames of the full view's own list on the same frame (mtbt_masks_to_frames: one source, the same number of
           plane bytes), for scale: the only yardstick there is

  python tools/slice_probe.py [--height 1536] [--width 2048]"""
import argparse
import hashlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slice_reference as SR  # noqa: E402
from multitask_bonetumor_yolo_amd import postprocess as pp, preprocess as pre  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--height", type=int, default=1536)
ap.add_argument("--width", type=int, default=2048)
ap.add_argument("--img", type=int, default=640)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--objects", type=int, default=150)
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
S, K, H0, W0 = args.img, args.k, args.height, args.width

tiles = pre.slice_geometry([(H0, W0)], S)
det_np, mc, protos = SR.tile_lists(tiles, K, 3, S, A=8400, n_obj=args.objects)
det = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in det_np.items()}
mc, protos = mc.to(dev), protos.to(dev).contiguous(memory_format=torch.channels_last)
frames = [(H0, W0, S / max(H0, W0))]
merged = pp.merge_tiles(det, tiles, frames, top_k=K)
torch.cuda.synchronize()
print(f"{H0} x {W0} at S = {S}: {len(tiles[0])} tiles, K = {K}; slots in use per tile {det_np['counts'].tolist()}; merged rows {int(merged['counts'][0])}, "
      f"rows with >= 2 members {int((merged['n_members'] >= 2).sum())}, largest row {int(merged['n_members'].max())}, n_left {int(merged['n_left'][0])}",
      flush=True)
pitch = 8 * ((W0 + 63) // 64)
buf = torch.empty((K * H0 * pitch + 16,), dtype=torch.uint8, device=dev)
print(f"plane bytes per mask call: {K * H0 * pitch}", flush=True)
full = len(tiles[0]) - 1                                                   # the full view's own list and prototypes


def timed(variants):
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


timed({"merge, merge_tiles (ios 0.5)      ": lambda: pp.merge_tiles(det, tiles, frames, top_k=K),
       "merge, merge_tiles (iou 0.5)      ": lambda: pp.merge_tiles(det, tiles, frames, metric="iou", top_k=K)})
for crop in (False, True):
    print(f"  vote_tile_masks crop={crop!s:5} sha256 {digest(pp.vote_tile_masks(merged, det, mc, protos, tiles, frames, crop=crop, out=buf))}", flush=True)
    r = pp.masks_to_frames(protos[full:], mc[full:], det["keep_anchor"][full:], det["counts"][full:], det["boxes"][full:], frames, up=4.0, crop=crop, out=buf)
    print(f"  masks_to_frames crop={crop!s:5} sha256 {digest(r)}", flush=True)
    timed({f"vote,  vote_tile_masks crop={crop!s:5} ": lambda: pp.vote_tile_masks(merged, det, mc, protos, tiles, frames, crop=crop, out=buf),
           f"frame, masks_to_frames crop={crop!s:5} ": lambda: pp.masks_to_frames(protos[full:], mc[full:], det["keep_anchor"][full:], det["counts"][full:],
                                                                             det["boxes"][full:], frames, up=4.0, crop=crop, out=buf)})
