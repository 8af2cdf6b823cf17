#!/usr/bin/env python3
"""Print the lane schedule of the batch-16 640x640 plan (built on CPU tensors, nothing is launched).
usage: MTBT_LANES=3 MTBT_LANE_WIDE_US=60 python tools/dump_schedule.py [B S]
MTBT_HEADS_MERGED=1 prints the merged-heads plan: a shared launch carries its members' names joined by " + " (batched launches as `batch[n]`)."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, init_synthetic_
from multitask_bonetumor_yolo_amd.model import _Lowering, plan_option
from multitask_bonetumor_yolo_amd.engine import code_of

B, S = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (16, 640)
m = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False)).eval()
xs = torch.empty(B, 3, S, S)
with torch.no_grad():
    lo = _Lowering(m, xs, code_of(torch.bfloat16))
    c3, c4, c5 = lo.backbone()
    feats = list(lo.neck(c3, c4, c5))
    lo.p.pool.reuse = os.environ.get("MTBT_HEAD_REUSE", "0") == "1"
    if plan_option(m, "HEADS_MERGED") == "1":
        heads = [(m.detect, "detect"), (m.segment, "segment")]
        mc, offs, A = lo.mc_buffer([(f.N, f.H, f.W) for f in feats], m.segment)
        lo.proto(feats[0], m.segment)
        for i, f in enumerate(feats):
            assert lo.heads_mergeable(i, heads, f)
            lo.heads_level_merged(i, f, heads, [lo.head_map(f, h) for h, _ in heads], mc, offs[i], A)
    else:
        lo.det_branch(feats, m.detect, "detect")
        lo.det_branch(feats, m.segment, "segment")
        lo.seg_extras(feats, m.segment)
    lo.cls_head(feats[2])
s = lo.p.schedule()
for i, l in enumerate(lo.p.launches):
    est = max(l.flops / 4e14, l.bytes / 2e12) * 1e6
    kind = f"batch[{l.args[1]}] " if l.fn is lo.p.lib.mtbt_conv2d_nhwc_batch else ""
    print(f"{i:3d} lane {s.lane[i]} est {est:6.1f}us deps {s.deps[i]} waits {s.waits[i]} rec {s.records[i]:3d}  {kind}{l.name}")
print("lanes used", sorted(set(s.lane)), "events", s.n_events, "est makespan %.2f ms" % (s.est_makespan * 1e3))
