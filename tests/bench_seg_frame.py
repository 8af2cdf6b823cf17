#!/usr/bin/env python3
"""Time the semantic mask in the image frame (postprocess.seg_to_frames, mtbt_seg_to_frames) on an MI355X.

(i)  16 frames of 640 x 640 from 8 views at G = 160 (test-time augmentation), packed planes plus logits;
(ii) one 2048 x 1536 frame from 12 tiles plus the full view under the gaussian window (sliced inference), with and without logits.
Each is timed as the whole call on one stream, beside
  - `out.copy_()` of a buffer whose read + write traffic is the operator's own input + output bytes (prototypes in, planes and logits
    out; the [NS, G, G] workspace between the two launches is not counted), alternating with the operator in one process: the floor,
    since both launches are HBM-class;
  - for (i) the torch composition a user would otherwise write: `proto_projector_logits` per view, `unorient_batch`, weighted mean, > 0.
The two launches of a call are timed separately from a kernel trace, taken in runs of their own (tracing slows the host):
    rocprofv3 --kernel-trace --stats -d DIR/<case> -- python tests/bench_seg_frame.py --kernel <case>      case = i | ii | ii_bits
and `--stats DIR` reads the *_kernel_stats.csv files found there.  Prints the table and writes it to profiles/seg_frame_probe.txt.
usage: python tests/bench_seg_frame.py [--repeats R] [--stats DIR] [--out PATH] | --kernel CASE"""
import argparse, csv, glob, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multitask_bonetumor_yolo_amd import postprocess as pp
from multitask_bonetumor_yolo_amd import preprocess as pre

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--stats", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_frame_probe.txt"))
ap.add_argument("--kernel", default=None, choices=("i", "ii", "ii_bits"))
args = ap.parse_args()
S, G = 640, 160
DEV = "cuda"


def timed(fn, iters=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


g = torch.Generator().manual_seed(0)
w, b = torch.randn(32, generator=g).to(DEV), torch.randn(1, generator=g).to(DEV)
pitch = lambda W0: 8 * ((W0 + 63) // 64)

# (i) 16 frames, 8 views
N, V = 16, 8
views = [torch.randn(N, 32, G, G, generator=g).to(DEV).contiguous(memory_format=torch.channels_last) for _ in range(V)]
weights = [float(v + 1) for v in range(V)]
frames_i = [(S, S, 1.0)] * N
out_i = torch.empty(N * S * pitch(S), dtype=torch.uint8, device=DEV)
lg_i = torch.empty(N * S * S, dtype=torch.float32, device=DEV)
# (ii) one 2048 x 1536 frame, 12 tiles plus the full view
H0, W0 = 1536, 2048
tiles = pre.slice_geometry([(H0, W0)], S)
NT = len(tiles[0])
assert NT == 13
protos_ii = torch.randn(NT, 32, G, G, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
frames_ii = [(H0, W0, S / W0)]
out_ii = torch.empty(H0 * pitch(W0), dtype=torch.uint8, device=DEV)
lg_ii = torch.empty(H0 * W0, dtype=torch.float32, device=DEV)

cases = {
    "i": (lambda: pp.seg_to_frames(views, (w, b), frames_i, orients=range(V), weights=weights, logits=lg_i, out=out_i),
          N * V, N * (S * pitch(S) + S * S * 4)),
    "ii": (lambda: pp.seg_to_frames(protos_ii, (w, b), frames_ii, tiles=tiles, blend="gaussian", logits=lg_ii, out=out_ii),
           NT, H0 * pitch(W0) + H0 * W0 * 4),
    "ii_bits": (lambda: pp.seg_to_frames(protos_ii, (w, b), frames_ii, tiles=tiles, blend="gaussian", out=out_ii), NT, H0 * pitch(W0)),
}
names = {"i": f"(i)  {N} x {S}^2 from {V} views, bits + logits", "ii": f"(ii) {W0} x {H0} from {NT} sources, bits + logits",
         "ii_bits": f"(ii) {W0} x {H0} from {NT} sources, bits only"}

if args.kernel:
    fn = cases[args.kernel][0]
    for _ in range(25):
        fn()
    torch.cuda.synchronize()
    sys.exit(0)


def composition():
    acc = None
    for v, (p, wt) in enumerate(zip(views, weights)):
        up = pp.unorient_batch(pp.proto_projector_logits(p, w, b, S), v)
        acc = up * wt if acc is None else acc.add_(up, alpha=wt)
    return (acc / sum(weights)) > 0


def kernel_times(case):
    """Average ns of the two kernels from the trace of `--kernel case`, or None."""
    if not args.stats:
        return None
    found = glob.glob(os.path.join(args.stats, case, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        return None
    t = {}
    for row in csv.DictReader(open(found[0])):
        for k in ("seg_project_kernel", "seg_blend_kernel"):
            if k in row["Name"]:
                t[k] = (float(row["AverageNs"]) / 1e3, int(row["Calls"]))
    return t if len(t) == 2 else None


lines = ["Semantic mask in the image frame (mtbt_seg_to_frames, csrc/seg_frame.hip) on an MI355X, G = 160, fp32 prototypes [., 160, 160, 32].",
         f"Whole call (both launches, host work included) beside a copy with the same read + write traffic on the same stream, alternating,",
         f"{args.repeats} rounds of 20 calls, median (min .. max).  Kernel lines: averages of a rocprofv3 kernel trace taken in a run of its own.", ""]
for key, (fn, ns, out_bytes) in cases.items():
    in_bytes = ns * G * G * 32 * 4
    half = torch.empty((in_bytes + out_bytes) // 2, dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(half)
    copy = lambda: dst.copy_(half)
    fn(); copy(); torch.cuda.synchronize()
    tk, tc = [], []
    for _ in range(args.repeats):
        tk.append(timed(fn)); tc.append(timed(copy))
    mk, mc = float(np.median(tk)), float(np.median(tc))
    lines.append(f"{names[key]}: {in_bytes / 1e6:.1f} MB in, {out_bytes / 1e6:.1f} MB out")
    lines.append(f"    call {mk:8.1f} us ({min(tk):.1f} .. {max(tk):.1f})   copy {mc:7.1f} us ({min(tc):.1f} .. {max(tc):.1f})   ratio {mk / mc:5.2f}   "
                 f"{(in_bytes + out_bytes) / mk / 1e6:5.2f} TB/s of in + out")
    kt = kernel_times(key)
    if kt is None:
        lines.append("    per launch: not measured")
    else:
        p_us, b_us = kt["seg_project_kernel"][0], kt["seg_blend_kernel"][0]
        ws = ns * G * G * 4
        lines.append(f"    launch 1 (projector) {p_us:7.1f} us: {(in_bytes + ws) / p_us / 1e6:5.2f} TB/s of {(in_bytes + ws) / 1e6:.1f} MB   "
                     f"launch 2 (blend) {b_us:7.1f} us: {(ws + out_bytes) / b_us / 1e6:5.2f} TB/s of {(ws + out_bytes) / 1e6:.1f} MB   "
                     f"sum / copy {(p_us + b_us) / mc:5.2f}   ({kt['seg_blend_kernel'][1]} traced calls)")
    if key == "i":
        composition(); torch.cuda.synchronize()
        t_op, t_co = [], []
        for _ in range(args.repeats):
            t_op.append(timed(fn, 10)); t_co.append(timed(composition, 10))
        got = torch.stack([pp.unpack_masks(m, S)[0] for m in fn()["masks"]])
        want = composition()[:, 0]
        lines.append(f"    torch composition (proto_projector_logits per view, unorient_batch, weighted mean, > 0) {float(np.median(t_co)):8.1f} us "
                     f"({min(t_co):.1f} .. {max(t_co):.1f}): {float(np.median(t_co)) / float(np.median(t_op)):.1f} x the call; "
                     f"bits that differ {int((got != want).sum())} of {got.numel()} (another summation order)")
    del half, dst

text = "\n".join(lines) + "\n"
print(text)
open(args.out, "w").write(text)
