"""Timing probe of the frame operator (GPU box): `postprocess.masks_to_frames` (bit-packed masks in the original image frame, crop off
and crop on) beside the dense `assemble_masks`, in one process, on the kept boxes of one calibrated synthetic step
(batch 16, 640 x 640, K = 100, identity frames).  Device events around 20 launches per variant after warm-up, the variants
alternating, 6 rounds; prints a sha256 of each frame variant's planes and boxes (so that two builds can be compared byte for byte at the
size that is timed), then the per-launch mean of every round and the bytes each variant writes.

  python tools/frame_mask_probe.py [--batch 16] [--img 640]"""
import argparse
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, calibrate_synthetic_heads_, init_synthetic_, postprocess as pp

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--img", type=int, default=640)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--rounds", type=int, default=6)
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
with torch.no_grad():
    out = model(x, "infer")
    feats, mc, protos = out["segment_protos"]
    det = pp.detect_and_segment(out["detect_features"], mc, protos, S, masks=False)
mc, protos = mc.float(), protos.float().contiguous(memory_format=torch.channels_last)
keep, counts, boxes = det["keep_anchor"], det["counts"], det["boxes"]
K = keep.shape[1]
frames = [(S, S, 1.0)] * B
buf = torch.empty(pp._frame_layout(frames, K, S / protos.shape[3])[1], dtype=torch.uint8, device=dev)
live = torch.arange(K, device=dev)[None, :] < counts[:, None]
area = ((boxes[..., 2] - boxes[..., 0]) * (boxes[..., 3] - boxes[..., 1]))[live].mean() / (S * S)
print(f"kept boxes per image: {counts.tolist()}; mean box area {float(area):.3f} of the image")

variants = {
    "frames crop=off": lambda: pp.masks_to_frames(protos, mc, keep, counts, boxes, frames, up=S / protos.shape[3], crop=False, out=buf),
    "frames crop=on": lambda: pp.masks_to_frames(protos, mc, keep, counts, boxes, frames, up=S / protos.shape[3], crop=True, out=buf),
    "dense assemble_masks": lambda: pp.assemble_masks(protos, mc, keep, counts, (S, S)),
}
bytes_written = {"frames crop=off": buf.numel(), "frames crop=on": buf.numel(), "dense assemble_masks": B * K * S * S}
for name in ("frames crop=off", "frames crop=on"):
    print(f"{name:22s} sha256 {digest(variants[name]())}", flush=True)
for f in variants.values():
    for _ in range(5):
        f()
torch.cuda.synchronize()
# same bits at identity frames (outside the sign-ambiguous band the tests allow)
dense, logits = pp.assemble_masks(protos, mc, keep, counts, (S, S), want_logits=True)
r = pp.masks_to_frames(protos, mc, keep, counts, boxes, frames, up=S / protos.shape[3], crop=False, out=buf)
diff = sum(int(((pp.unpack_masks(r["masks"][b], S) != dense[b]) & (logits[b].abs() >= 1e-4)).sum()) for b in range(B))
print(f"bits differing from the dense kernel outside |logit| < 1e-4: {diff}")
del dense, logits
times = {k: [] for k in variants}
for _ in range(args.rounds):
    for name, f in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            f()
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / args.launches)
for name, t in times.items():
    mean = sum(t) / len(t)
    print(f"{name:22s} {bytes_written[name] / 1e6:8.1f} MB written  per launch (us) rounds: " + " ".join(f"{v:7.1f}" for v in t)
          + f"   mean {mean:7.1f}  -> {bytes_written[name] / mean / 1e6:.2f} TB/s of output")
