#!/usr/bin/env python3
"""Time the region measurements of bit-packed planes and label maps (mtbt_measure_regions) on an MI355X.

Two inputs: N planes of S^2 of lesion-like blobs with specks (`components_reference.big_plane`) in LABEL mode after `label_components`
(C = 2048 regions per plane: the blob comes after some 1200 specks in id order), and K instance planes of 2048 x 1536 (one ellipse each)
in PLANE mode.  For each, alternating in one process:
  measure           `measure_regions` through the Python wrapper (allocations included, no host synchronisation)
  label + measure   `measure_components` (label mode only)
  copy              `out.copy_()` of the same input bytes (the label map, or the packed planes) on the same stream
and the host route both replace: `unpack_masks(...).cpu()` (the dense masks over the bus), then per region on this host
scipy.spatial.ConvexHull of the pixel corners and pdist over the hull's vertices (two planes timed, scaled).
Prints the table and writes it to profiles/measure_probe.txt (or the path given last).
usage: python tests/bench_measure.py [N] [S] [K] [repeats] [out.txt]"""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import components_reference as CR
import measure_reference as R
from multitask_bonetumor_yolo_amd import label_components, measure_components, measure_regions
from multitask_bonetumor_yolo_amd.postprocess import unpack_masks
from scipy import ndimage
from scipy.spatial import ConvexHull
from scipy.spatial.distance import pdist
N, S, K, REP = (int(v) for v in (sys.argv[1:5] + ["32", "640", "100", "5"][len(sys.argv) - 1:]))
C_ = 2048                                        # the blob of `big_plane` comes after some 1200 specks in id order


def timed(fn, iters=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def host_region(ys, xs):
    """What a host library does for one region: the hull of the pixel corners, then the farthest pair of its vertices."""
    pts = np.unique(np.concatenate([np.stack([xs + dx, ys + dy], axis=1) for dx in (0, 1) for dy in (0, 1)]), axis=0).astype(np.float64)
    v = pts[ConvexHull(pts).vertices]
    return float(pdist(v, "sqeuclidean").max())


def instance_planes(rng, K, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((K, H, W), bool)
    for k in range(K):
        cy, cx, ry, rx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, rng.uniform(0.05, 0.25) * H, rng.uniform(0.05, 0.25) * W
        out[k] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0
    return out


rng = np.random.default_rng(0)
lines = ["Region measurements (mtbt_measure_regions; csrc/measure.hip) on an MI355X, through the Python wrappers (allocations included), beside a",
         f"plain copy of the same input bytes on the same stream.  Alternating, {REP} rounds of 10 calls, median (min .. max), microseconds per call.", ""]
for name, dense, labelled in ((f"label mode, {N} x {S} x {S} blobs with specks, C = {C_}", np.stack([CR.big_plane(np.random.default_rng(100 + i), S) for i in range(N)]), True),
                              (f"plane mode, {K} instance planes of 2048 x 1536", instance_planes(rng, K, 2048, 1536), False)):
    n, H, W = dense.shape
    packed = torch.from_numpy(CR.pack_bits(dense)).cuda()
    if labelled:
        labels = label_components(packed, W, max_components=C_)["labels"]
        src = labels
        variants = {"measure": lambda: measure_regions(None, W, labels=labels, max_regions=C_),
                    "label + measure": lambda: measure_components(packed, W, max_components=C_)}
    else:
        src = packed
        variants = {"measure": lambda: measure_regions(packed, W)}
    mirror = torch.empty_like(src)
    variants["copy"] = lambda: mirror.copy_(src)
    res = variants["measure"]()
    want = R.measure_labels(labels[0].cpu().numpy(), 8) if labelled else [R.measure_plane(dense[0])]
    ok = all(res["caliper"][0, r].tolist() == w["caliper"] and res["sums"][0, r].tolist() == w["sums"] for r, w in enumerate(want))
    for f in variants.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(REP):
        for k, f in variants.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    # the host route: dense masks over the bus, then scipy per region
    unpack_masks(packed[:1], W).cpu()                            # the first call loads torch's kernels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = unpack_masks(packed, W).cpu().numpy()
    t_bus = (time.perf_counter() - t0) * 1e6
    k = min(n, 2)
    n_regions = 0
    t0 = time.perf_counter()
    for i in range(k):
        if labelled:
            lab, nl = ndimage.label(host[i])
            for sl, j in zip(ndimage.find_objects(lab), range(1, min(nl, C_) + 1)):
                ys, xs = np.nonzero(lab[sl] == j)
                host_region(ys + sl[0].start, xs + sl[1].start)
                n_regions += 1
        else:
            host_region(*np.nonzero(host[i]))
            n_regions += 1
    t_sp = (time.perf_counter() - t0) / k * n * 1e6
    lines.append(f"{name}: {src.numel() * src.element_size() / 1e6:.2f} MB of input, {int((res['n_hull'] > 0).sum())} non-empty regions, "
                 f"largest hull {int(res['n_hull'].max())} vertices; the first regions equal the restatement: {ok}")
    for k_, v in med.items():
        lines.append(f"  {k_:16s} {v:10.1f} us ({min(t[k_]):.1f} .. {max(t[k_]):.1f})   {v / med['copy']:8.1f} x the copy")
    lines.append(f"  host route: unpack + .cpu() {t_bus / 1e3:.1f} ms ({host.nbytes / 1e6:.1f} MB dense), then scipy ConvexHull + pdist per region "
                 f"{t_sp / 1e3:.0f} ms (scaled from {k} planes, {n_regions} regions); measure is {(t_bus + t_sp) / med['measure']:.0f} x faster")
    lines.append("")

text = "\n".join(lines)
print(text)
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "measure_probe.txt")
open(out_path, "w").write(text)
