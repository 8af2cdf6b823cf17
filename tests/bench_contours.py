#!/usr/bin/env python3
"""Time contour tracing and run-length encoding of bit-packed planes (mtbt_trace_contours, mtbt_rle_encode) on an MI355X.

Three inputs: N planes of S^2 of lesion-like blobs with specks (`components_reference.big_plane`), N planes of noise at p = 0.5 (the most
vertices a random plane has: 3 for every 4 lattice points), one plane of 2048 x 1536.  For each, alternating in one process:
  trace V,C given   `trace_contours` with explicit capacities (no host synchronisation)
  trace counted     `trace_contours(max_vertices=None)`: the counting pass, one read-back, exact allocation
  count only        `count_contour_vertices`
  rle               `rle_encode` with an explicit capacity
  copy              `out.copy_()` of the same packed input bytes on the same stream (the floor of any pass over the planes)
and the host route these replace: `unpack_masks(...).cpu()` (the dense masks over the bus) followed by a host tracer -- the numpy
restatement of the rule (one plane timed, scaled to N) and, as the quicker host baseline, scipy.ndimage.label + find_objects, which
finds the components' boxes but no polygon (four planes timed, scaled).
Prints the table and writes it to profiles/contours_probe.txt (or the path given last).
usage: python tests/bench_contours.py [N] [S] [repeats] [out.txt]"""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import components_reference as CR
import contour_reference as R
from multitask_bonetumor_yolo_amd import count_contour_vertices, rle_encode, trace_contours
from multitask_bonetumor_yolo_amd.postprocess import unpack_masks
from scipy import ndimage
N, S, REP = (int(v) for v in (sys.argv[1:4] + ["32", "640", "5"][len(sys.argv) - 1:]))
CAP = 8192


def timed(fn, iters=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def large_plane(rng, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    m = ((yy - 0.45 * H) / (0.3 * H)) ** 2 + ((xx - 0.5 * W) / (0.3 * W)) ** 2 < 1.0
    m &= ~(((yy - 0.4 * H) / (0.08 * H)) ** 2 + ((xx - 0.55 * W) / (0.08 * W)) ** 2 < 1.0)
    return m | (rng.uniform(size=(H, W)) < 0.02)


rng = np.random.default_rng(0)
kinds = {"blobs": np.stack([CR.big_plane(np.random.default_rng(100 + i), S) for i in range(N)]),
         "noise p=0.5": rng.uniform(size=(N, S, S)) < 0.5,
         "one 2048x1536": large_plane(rng, 2048, 1536)[None]}
lines = [f"Contours and run lengths of bit-packed planes (mtbt_trace_contours, mtbt_rle_encode; csrc/contours.hip) on an MI355X: {N} planes of",
         f"{S} x {S} (blobs with specks; noise) and one plane of 2048 x 1536, through the Python wrappers (allocations included), beside a plain",
         f"copy of the same packed bytes on the same stream.  Alternating, {REP} rounds of 10 calls, median (min .. max), microseconds per call.", ""]

for name, dense in kinds.items():
    n, H, W = dense.shape
    packed = torch.from_numpy(CR.pack_bits(dense)).cuda()
    mirror = torch.empty_like(packed)
    nv = count_contour_vertices(packed, W)
    V, total = int(nv.max()), int(nv.sum())
    res = trace_contours(packed, W, max_contours=CAP, max_vertices=V)
    runs, n_runs = rle_encode(packed, W)
    Rcap = int(n_runs.max())
    assert torch.equal(res["n_vertices"], nv) and int(res["n_contours"].min()) >= 0
    variants = {"trace V,C given": lambda: trace_contours(packed, W, max_contours=CAP, max_vertices=V),
                "trace counted": lambda: trace_contours(packed, W, max_contours=CAP),
                "count only": lambda: count_contour_vertices(packed, W),
                "rle": lambda: rle_encode(packed, W, max_runs=Rcap),
                "copy": lambda: mirror.copy_(packed)}
    for f in variants.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(REP):
        for k, f in variants.items():
            t[k].append(timed(f))
    med = {k: float(np.median(v)) for k, v in t.items()}
    # the host route: dense masks over the bus, then a host tracer
    unpack_masks(packed[:1], W).cpu()                            # the first call loads torch's kernels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = unpack_masks(packed, W).cpu().numpy()
    t_bus = (time.perf_counter() - t0) * 1e6
    t0 = time.perf_counter()
    ref = R.records(host[0], 4, CAP)
    t_ref = (time.perf_counter() - t0) * n * 1e6
    k = min(n, 4)
    t0 = time.perf_counter()
    for i in range(k):
        ndimage.find_objects(ndimage.label(host[i])[0])
    t_sp = (time.perf_counter() - t0) / k * n * 1e6
    nv0 = int(nv[0])
    ok = ref["n_contours"] == int(res["n_contours"][0]) and np.array_equal(res["vertices"][0, :nv0].cpu().numpy(), ref["vertices"])
    lines.append(f"{name}: {n} x {H} x {W}, {packed.numel() / 1e6:.2f} MB packed, {total} vertices ({V} in the largest plane), "
                 f"{int(res['n_contours'].sum())} contours, {int(n_runs.sum())} runs; plane 0 equals the restatement: {ok}")
    for k_, v in med.items():
        lines.append(f"  {k_:16s} {v:10.1f} us ({min(t[k_]):.1f} .. {max(t[k_]):.1f})   {v / med['copy']:8.1f} x the copy")
    lines.append(f"  host route: unpack + .cpu() {t_bus / 1e3:.1f} ms ({host.nbytes / 1e6:.1f} MB dense), then the numpy restatement {t_ref / 1e3:.0f} ms "
                 f"(scaled from one plane) or scipy label + find_objects {t_sp / 1e3:.1f} ms (no polygons);")
    lines.append(f"  trace V,C given is {(t_bus + t_sp) / med['trace V,C given']:.0f} x faster than copy-out + scipy, {(t_bus + t_ref) / med['trace V,C given']:.0f} x "
                 "faster than copy-out + the restatement")
    lines.append("")

text = "\n".join(lines)
print(text)
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "contours_probe.txt")
open(out_path, "w").write(text)
