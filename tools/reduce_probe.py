"""Bit-identity and timing probe of the training step's fixed-order reductions (csrc/rowreduce.h and its users; GPU box): fixed-seed
inputs, one sha256 line per output of a first call, then device events around `--launches` back-to-back calls of every entry point, the
entry points alternating, `--rounds` readings each; prints the readings and their median.  Two builds of the library agree when all
their sha256 lines agree:

  bash tools/lib_ab_cmd.sh python3 tools/reduce_probe.py

Covered: mtbt_bn_forward_nhwc, mtbt_bn_forward_partials_nhwc and mtbt_bn_backward_nhwc at (C 64, P 204 800) bf16 -- the fixed path --,
(C 96, P 51 200) bf16 -- the general path -- and (C 2048, P 300) f32 -- 256 pieces per pixel; mtbt_channel_sum at C 64 and C 2056 (257
pieces: the serial branch of rows_reduce); mtbt_sumsq at n = 5 000 000; mtbt_bifpn_fuse_backward with dwgt; mtbt_conv_wgrad at a shape
with >= 8 slices (wgrad_reduce4_kernel); mtbt_scale_grad mode 1; mtbt_projector_backward at 32 and 248 prototypes.
Digests only, small shapes: the BatchNorm entry points for every activation instantiation (none, silu, elu, run-time) in both dtypes, and the
remaining dtype / path combinations of mtbt_channel_sum."""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--only", default="", help="time only the entry points whose name contains this (all digests are still printed)")
args = ap.parse_args()
DEV = torch.device("cuda", 0)
lib = L.load()
S = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
F32, BF16 = torch.float32, torch.bfloat16
CODE = {F32: 0, BF16: 1}
ACTS = {"none": 0, "silu": 1, "elu": 2, "gelu": 3}     # _lib.ACT_*: gelu takes the run-time-activation instantiations
gen = torch.Generator().manual_seed(20)
entries = {}          # name -> callable that launches once


def entry(name, fn, timed=True):
    if timed:
        entries[name] = fn


def rand(*shape, dtype=F32, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=gen) * scale + shift).to(DEV, dtype)


def digest(name, *tensors):
    torch.cuda.synchronize()
    for i, t in enumerate(tensors):
        print(f"sha256 {name}[{i}] {hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()}")


def ws_for(nbytes):
    return torch.empty(max(nbytes // 4, 1) + 16, device=DEV), nbytes


def bn_case(Cc, P, dtype, act="silu", timed=True):
    tag = f"C{Cc}-P{P}-{'bf16' if dtype == BF16 else 'f32'}" + ("" if act == "silu" else "-" + act)
    ACT = ACTS[act]
    eps, mom, LD = 1e-3, 0.03, Cc + 24
    x, dy = rand(P, Cc, dtype=dtype, scale=1.5, shift=0.2), rand(P, LD, dtype=dtype)
    gamma, beta = rand(Cc, scale=0.3, shift=1.0), rand(Cc, scale=0.2)
    rm0, rv0 = rand(Cc, scale=0.1, shift=0.2), rand(Cc, scale=0.1, shift=2.0).abs()
    y = torch.zeros(P, LD, dtype=dtype, device=DEV)
    stats = torch.zeros(2 * Cc, device=DEV)
    ws, nb = ws_for(lib.mtbt_bn_train_workspace_bytes(P, Cc))

    def forward(rm, rv):
        L.check(lib.mtbt_bn_forward_nhwc(x.data_ptr(), y.data_ptr(), LD, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), C.c_float(mom),
                                         C.c_float(eps), ACT, P, Cc, CODE[dtype], 0, stats.data_ptr(), ws.data_ptr(), nb, S), "bn_forward")
    rm, rv = rm0.clone(), rv0.clone()
    forward(rm, rv)
    digest(f"bn_forward {tag}", y, stats, rm, rv)
    entry(f"bn_forward {tag}", lambda: forward(rm, rv), timed)

    # the partial rows a conv epilogue would have written: per 256 pixels, sum (x - shift) and sum (x - shift)^2, pitch 2C + 8
    rows, pitch = (P + 255) // 256, 2 * Cc + 8
    xs = x.float() - rm0
    pad = torch.zeros(rows * 256 - P, Cc, device=DEV)
    part0 = torch.zeros(rows, pitch, device=DEV)
    part0[:, :Cc] = torch.cat([xs, pad]).view(rows, 256, Cc).double().sum(1).float()
    part0[:, Cc:2 * Cc] = torch.cat([xs * xs, pad]).view(rows, 256, Cc).double().sum(1).float()
    part0 = part0.cpu().to(DEV)
    stats2 = torch.zeros(2 * Cc, device=DEV)

    def partials(part, rm, rv):
        L.check(lib.mtbt_bn_forward_partials_nhwc(x.data_ptr(), y.data_ptr(), LD, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), C.c_float(mom),
                                                  C.c_float(eps), ACT, P, Cc, CODE[dtype], part.data_ptr(), rows, pitch, rm.data_ptr(), stats2.data_ptr(), S),
                "bn_forward_partials")
    rm2, rv2, part = rm0.clone(), rv0.clone(), part0.clone()
    partials(part, rm2, rv2)                                # shift aliases running_mean, as the training plan passes it
    digest(f"bn_forward_partials {tag}", y, stats2, rm2, rv2)
    entry(f"bn_forward_partials {tag}", lambda: partials(part, rm2, rv2), timed)     # (a tall `part` is folded in place again: the time is the same)

    dx = torch.zeros(P, Cc, dtype=dtype, device=DEV)
    dg, db = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    ws2, nb2 = ws_for(lib.mtbt_bn_backward_workspace_bytes(P, Cc))

    def backward():
        L.check(lib.mtbt_bn_backward_nhwc(dy.data_ptr(), LD, x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), C.c_float(eps), ACT, 0,
                                          dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, P, Cc, CODE[dtype], ws2.data_ptr(), nb2, S), "bn_backward")
    backward()
    digest(f"bn_backward {tag}", dx, dg, db)
    entry(f"bn_backward {tag}", backward, timed)


def channel_sum_case(Cc, P, dtype, timed=True):
    tag = f"C{Cc}-P{P}" + ("" if timed else "-bf16" if dtype == BF16 else "-f32")
    LD = Cc + 16
    a, b = rand(P, LD, dtype=dtype), rand(P, LD, dtype=dtype)
    ws, nb = ws_for(lib.mtbt_channel_sum_workspace_bytes(P, Cc))
    out1, out2 = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)

    def run(out, second):
        L.check(lib.mtbt_channel_sum(a.data_ptr(), b.data_ptr() if second else None, P, Cc, LD, LD, CODE[dtype], out.data_ptr(), 0, ws.data_ptr(), nb, S), "channel_sum")
    run(out1, False)
    run(out2, True)
    digest(f"channel_sum {tag}", out1, out2)
    entry(f"channel_sum {tag}", lambda: run(out2, True), timed)


def sumsq_case(n):
    v = rand(n)
    ws, nb = ws_for(lib.mtbt_sumsq_workspace_bytes())
    out = torch.zeros(1, device=DEV)

    def run():
        L.check(lib.mtbt_sumsq(v.data_ptr(), n, out.data_ptr(), 0, ws.data_ptr(), nb, S), "sumsq")
    run()
    digest(f"sumsq n{n}", out)
    entries[f"sumsq n{n}"] = run


def fuse_case(N, H, W, Cc, mode):
    x, dy = rand(N, H // 2, W // 2, Cc, dtype=BF16), rand(N, H, W, Cc, dtype=BF16)      # mode 1: bilinear x2 up of a half-size input
    wgt = torch.tensor([0.37], device=DEV)
    dx, dw = torch.zeros_like(x), torch.zeros(1, device=DEV)
    ws, nb = ws_for(lib.mtbt_bifpn_fuse_backward_workspace_bytes())

    def run():
        L.check(lib.mtbt_bifpn_fuse_backward(dy.data_ptr(), x.data_ptr(), mode, wgt.data_ptr(), dx.data_ptr(), 0, dw.data_ptr(), 0, N, H, W, Cc, CODE[BF16],
                                             ws.data_ptr(), nb, S), "bifpn_fuse_backward")
    run()
    digest("bifpn_fuse_backward", dx, dw)
    entries["bifpn_fuse_backward"] = run


def wgrad_case(N, H, W, Cc, K):
    x, dy = rand(N, H, W, Cc, dtype=BF16), rand(N, H, W, K, dtype=BF16)
    dw = torch.zeros(K, Cc, device=DEV)
    ws, nb = ws_for(lib.mtbt_conv_wgrad_workspace_bytes(N, H, W, Cc, K, 1, 1))

    def run():
        L.check(lib.mtbt_conv_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), N, H, W, Cc, K, 1, 1, 0, 1, H * W * Cc, Cc, H * W * K, K, CODE[BF16], 0,
                                    ws.data_ptr(), nb, S), "conv_wgrad")
    run()
    digest("conv_wgrad", dw)
    entries["conv_wgrad"] = run


def scale_grad_case(K, Cc):
    G, Wt, vec = rand(K, Cc), rand(K, Cc), rand(Cc)
    dW, dvec = torch.zeros(K, Cc, device=DEV), torch.zeros(Cc, device=DEV)

    def run():
        L.check(lib.mtbt_scale_grad(1, G.data_ptr(), Wt.data_ptr(), vec.data_ptr(), None, None, dW.data_ptr(), dvec.data_ptr(), None, K, Cc, 0, S), "scale_grad")
    run()
    digest("scale_grad mode1", dW, dvec)
    entries["scale_grad mode1"] = run


def projector_case(N, nm, hp, wp, Ho, Wo):
    protos, w, dseg = rand(N, hp, wp, nm), rand(nm, scale=0.3), rand(N, Ho, Wo)
    dp, dw, db = torch.zeros_like(protos), torch.zeros(nm, device=DEV), torch.zeros(1, device=DEV)
    ws, nb = ws_for(lib.mtbt_projector_backward_workspace_bytes(N, hp, wp, nm))

    def run():
        L.check(lib.mtbt_projector_backward(dseg.data_ptr(), protos.data_ptr(), w.data_ptr(), dp.data_ptr(), CODE[F32], 0, dw.data_ptr(), db.data_ptr(), 0, N, hp, wp, nm,
                                            Ho, Wo, ws.data_ptr(), nb, S), "projector_backward")
    run()
    digest(f"projector_backward nm{nm}", dp, dw, db)
    entries[f"projector_backward nm{nm}"] = run


bn_case(64, 204800, BF16)
bn_case(96, 51200, BF16)
bn_case(2048, 300, F32)
channel_sum_case(64, 51200, BF16)
channel_sum_case(2056, 300, F32)
sumsq_case(5_000_000)
fuse_case(2, 64, 66, 256, 1)
wgrad_case(8, 80, 80, 64, 64)          # 51 200 pixels over one 64 x 64 tile: far more than 8 slices
scale_grad_case(256, 96)
projector_case(4, 32, 160, 160, 640, 640)      # 102 400 rows of 5 pieces: 51 row groups per workgroup
projector_case(2, 248, 48, 48, 192, 192)       # the documented maximum, 32 pieces: 8 row groups
# digests only: every ACT x dtype instantiation of the BatchNorm kernels on the fixed path, both dtypes of the general path, and the
# dtype / path combinations of mtbt_channel_sum the timed cases leave out
for dt in (F32, BF16):
    for a in ("none", "silu", "elu", "gelu"):
        bn_case(64, 5000, dt, a, timed=False)
    bn_case(96, 1100, dt, "elu", timed=False)
    bn_case(2048, 300, dt, "elu", timed=False)
channel_sum_case(64, 5000, F32, timed=False)
channel_sum_case(2056, 300, BF16, timed=False)

entries = {k: f for k, f in entries.items() if args.only in k}
readings = {k: [] for k in entries}
for r in range(args.rounds + 1):                                           # round 0 is the warm-up
    for name, fn in entries.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        e1.synchronize()
        if r:
            readings[name].append(e0.elapsed_time(e1) * 1000.0 / args.launches)
for name, v in readings.items():
    print(f"us per call {name}: {' '.join(f'{t:.1f}' for t in v)}; median {statistics.median(v):.1f} (range {min(v):.1f} - {max(v):.1f})")
