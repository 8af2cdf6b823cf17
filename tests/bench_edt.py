#!/usr/bin/env python3
"""Time the distance transform (mtbt_distance_transform) and what the region terms add to a training step, on an MI355X.

(a) Both maps of N planes at S^2, for three kinds of plane (lesion-like blobs, noise at p = 0.5, a single pixel), beside two baselines:
    `out.copy_()` of the same output bytes on the same stream, alternating with the kernel in one process (the floor: the transform
    writes those bytes once), and scipy's distance_transform_edt on this host, two calls per plane (what a host path would run; a few
    planes are timed and scaled).
(b) The training step of `bench.py --mode train` (same model, batch and targets) with the region terms off and on, alternating: the
    added time per step.
Prints the table and writes it to profiles/edt_probe.txt (or the path given last).
usage: python tests/bench_edt.py [N] [S] [repeats] [train_batch] [out.txt]   (train_batch 0 skips (b))"""
import ctypes as C, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multitask_bonetumor_yolo_amd import _lib as L
N, S, REP, TB = (int(v) for v in (sys.argv[1:5] + ["32", "640", "5", "32"][len(sys.argv) - 1:]))


def timed(fn, iters=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


rng = np.random.default_rng(0)
pitch = 8 * ((S + 63) // 64)
yy, xx = np.mgrid[0:S, 0:S]
kinds = {}
m = np.zeros((N, S, S), bool)
for i in range(N):                                                    # one or two lesions of about S / 8 .. S / 5 across
    for _ in range(int(rng.integers(1, 3))):
        cx, cy, rx, ry = rng.integers(S // 4, 3 * S // 4), rng.integers(S // 4, 3 * S // 4), rng.integers(S // 16, S // 10), rng.integers(S // 16, S // 10)
        m[i] |= ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0
kinds["blobs"] = m
kinds["noise p=0.5"] = rng.uniform(size=(N, S, S)) < 0.5
m = np.zeros((N, S, S), bool)
m[np.arange(N), rng.integers(0, S, N), rng.integers(0, S, N)] = True
kinds["single pixel"] = m

lib, stream = L.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
d_set, d_unset = (torch.empty(N, S, S, dtype=torch.int32, device="cuda") for _ in range(2))
c_set, c_unset = torch.empty_like(d_set), torch.empty_like(d_unset)
nb = lib.mtbt_distance_transform_workspace_bytes(N, S, S)
ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
out_bytes = 2 * d_set.numel() * 4
lines = [f"Distance transform (mtbt_distance_transform, csrc/distance_transform.hip) on an MI355X: both maps of {N} planes of {S} x {S}",
         f"({out_bytes / 1e6:.1f} MB of output, {nb / 1e6:.1f} MB of workspace), beside a plain copy of the same output bytes on the same stream",
         f"(alternating, {REP} rounds of 20 calls, median) and scipy.ndimage.distance_transform_edt on this host (two calls per plane).", ""]


def plain_copy():
    c_set.copy_(d_set)
    c_unset.copy_(d_unset)


for name, dense in kinds.items():
    full = np.zeros((N, S, 8 * pitch), bool)
    full[:, :, :S] = dense
    packed = torch.from_numpy(np.packbits(full, axis=2, bitorder="little")).cuda()
    a = L.DistanceTransformArgs()
    a.packed, a.workspace, a.workspace_bytes, a.d2_set, a.d2_unset = packed.data_ptr(), ws.data_ptr(), nb, d_set.data_ptr(), d_unset.data_ptr()
    a.n, a.H, a.W, a.pitch = N, S, S, pitch

    def edt():
        L.check(lib.mtbt_distance_transform(C.byref(a), stream), "mtbt_distance_transform")

    edt(); plain_copy(); torch.cuda.synchronize()
    t_k, t_c = [], []
    for _ in range(REP):
        t_k.append(timed(edt)); t_c.append(timed(plain_copy))
    from scipy.ndimage import distance_transform_edt
    k = min(N, 4)
    t0 = time.perf_counter()
    for i in range(k):
        host = (distance_transform_edt(~dense[i]), distance_transform_edt(dense[i]))
    t_host = (time.perf_counter() - t0) / k * N * 1e6
    got = d_set[k - 1].cpu().numpy().view(np.uint32).astype(np.int64)
    ok = bool(np.array_equal(got, np.rint(host[0] ** 2).astype(np.int64))) if dense[k - 1].any() else None
    tk, tc = float(np.median(t_k)), float(np.median(t_c))
    lines.append(f"{name:13s} transform {tk:9.1f} us (min {min(t_k):.1f}, max {max(t_k):.1f})   copy {tc:7.1f} us   ratio {tk / tc:6.2f}   "
                 f"{out_bytes / tk / 1e6:6.2f} TB/s of output   scipy {t_host / 1e3:8.1f} ms ({t_host / tk:7.0f} x)   d2_set equals scipy: {ok}")

if TB > 0:
    import bench
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, init_synthetic_
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    torch.manual_seed(0)
    model = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)).cuda()
    model.set_compute_dtype(torch.bfloat16)
    x = torch.rand(TB, 3, S, S, generator=torch.Generator().manual_seed(0)).cuda()
    boxes, masks, cls = bench.synthetic_targets(TB, S, 0, "cuda")
    ts = TrainStep(model, (TB, 3, S, S), optimizer="sgd", lr=1e-4)

    def step_with(wd, wb):
        def f():
            ts.seg_dice_weight, ts.seg_boundary_weight = wd, wb
            ts.step(x, boxes, masks, cls)
        return f

    conf = {"off": step_with(0.0, 0.0), "dice": step_with(1.0, 0.0), "dice + boundary": step_with(1.0, 0.01)}
    for f in conf.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in conf}
    for _ in range(REP):
        for k, f in conf.items():
            t[k].append(timed(f, iters=10))
    med = {k: float(np.median(v)) for k, v in t.items()}
    lines += ["", f"Training step (the model, batch {TB} x {S}^2 and targets of bench.py --mode train, bf16, SGD), region terms off and on, alternating,",
              f"{REP} rounds of 10 steps, median (min .. max):"]
    for k in conf:
        lines.append(f"{k:16s} {med[k] / 1e3:8.3f} ms ({min(t[k]) / 1e3:.3f} .. {max(t[k]) / 1e3:.3f})   added {(med[k] - med['off']) / 1e3:+7.3f} ms")

text = "\n".join(lines) + "\n"
print(text)
out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, "profiles", "edt_probe.txt")
open(out_path, "w").write(text)
