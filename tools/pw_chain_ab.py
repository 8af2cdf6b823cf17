#!/usr/bin/env python3
"""Per-site A/B of plan option PW_CHAIN: the two 1x1 launches of a site against the one `mtbt_pw_chain_nhwc` launch that replaces them, timed
the way the step runs them (tools/chain_tune.py): a captured HIP graph of 16 sites on one stream, operands rotating through a ring of
buffers larger than the L2s, no host in the loop.  The two forms alternate; every reading is printed, the verdict compares the difference
of the means with the spread of the repeated pair readings.
    python tools/pw_chain_ab.py [--batch 16] [--img 640] [--rounds 5]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import _lib as L  # noqa: E402
from multitask_bonetumor_yolo_amd.engine import Act, Plan  # noqa: E402

DEV = torch.device("cuda:0")
SITES, RING = 16, 6
CH = 256


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def graph_of(plan):
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        plan.run()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.run()
        for _ in range(2):
            g.replay()
        torch.cuda.synchronize()
    return g, s


def time_graph(g, s, reps=8):
    with torch.cuda.stream(s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(reps):
            g.replay()
        e1.record(s)
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps / SITES * 1e3


def site(N, H, W, head, rounds):
    """(pair readings, fused readings) in us per site.  Neck: ELU then SiLU into the first 256 channels of a 512-channel buffer; head: SiLU
    then the bias-only 256 -> 2 conv into channels 64 .. 65 of a 68-float map."""
    dt = torch.bfloat16
    K, ld, c0, odt = (2, 68, 64, torch.float32) if head else (256, 512, 0, dt)
    act1, act2 = (L.ACT_SILU, L.ACT_NONE) if head else (L.ACT_ELU, L.ACT_SILU)
    xs = [Act.of(torch.randn(N, H, W, CH, device=DEV).to(dt)) for _ in range(RING)]
    ts = [Act.of(torch.empty(N, H, W, CH, device=DEV, dtype=dt)) for _ in range(RING)]
    ys = [Act(torch.empty(N, H, W, ld, device=DEV, dtype=odt), c0, N, H, W, K, ld, H * W * ld) for _ in range(RING)]
    w1 = (torch.randn(CH, CH, device=DEV) / 16).to(dt)
    w2 = (torch.randn(K, CH, device=DEV) / 16).to(dt)
    s1, s2 = torch.zeros(CH, device=DEV), torch.zeros(K, device=DEV)
    pair, fused = Plan(DEV), Plan(DEV)
    for i in range(SITES):
        x, t, y = xs[i % RING], ts[i % RING], ys[i % RING]
        pair.conv(x, w1, t, shift=s1, act=act1)
        pair.conv(t, w2, y, shift=s2, act=act2)
        a = fused.pw_chain_args(x, w1, s1, act1, w2, s2, act2, y, any_size=True)
        if a is None:
            return None
        fused.pw_chain(a, x, w1, s1, w2, s2, y)
    gp, sp = graph_of(pair)
    gf, sf = graph_of(fused)
    tp, tf = [], []
    for _ in range(rounds):
        tp.append(time_graph(gp, sp))
        tf.append(time_graph(gf, sf))
    return tp, tf


def main():
    batch, img, rounds = arg("--batch", 16), arg("--img", 640), arg("--rounds", 5)
    print(f"# per site in a {SITES}-site graph chain, batch {batch} x {img}^2, bf16; pair = two mtbt_conv2d_nhwc launches, fused = mtbt_pw_chain_nhwc", flush=True)
    for head in (False, True):
        for stride in (8, 16, 32):
            h = img // stride
            r = site(batch, h, h, head, rounds)
            label = f"{'head 256->256->2 f32' if head else 'neck 256->256->256  '} @{h}x{h} ({batch * h * h} px)"
            if r is None:
                print(f"{label}: the library declines the shape (two launches)", flush=True)
                continue
            tp, tf = r
            mp, mf = sum(tp) / len(tp), sum(tf) / len(tf)
            spread = max(tp) - min(tp)
            verdict = "fused faster" if mp - mf > spread and max(tf) < min(tp) else "not resolved"
            print(f"{label}: pair {' '.join(f'{t:.1f}' for t in tp)} | fused {' '.join(f'{t:.1f}' for t in tf)} us | means {mp:.1f} -> {mf:.1f}, "
                  f"pair spread {spread:.1f}: {verdict}", flush=True)


if __name__ == "__main__":
    main()
