"""Timing probe of the device box mAP (GPU box).  Synthetic 16-image batches: 100 kept detections per image, 3 GT boxes, 2 classes,
COCO IoU thresholds 0.5:0.95 (T = 10), max-dets [1, 10, 100].

  rocprofv3 --kernel-trace --stats -d OUT -o box --output-format csv -- python tools/box_eval_probe.py --kernel
      130 launches of mtbt_box_eval (30 warm-up + 100 timed); the per-launch kernel time is coco_match_kernel<BoxPairs>'s AverageNs in
      OUT/.../box_kernel_stats.csv
  python tools/box_eval_probe.py --host
      host time of compute() over ~5000 images: DeviceMeanAveragePrecision (records from update_batched) against the
      host-matching MeanAveragePrecision fed the same detections and GT boxes (the shared keys agree)"""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multitask_bonetumor_yolo_amd.metrics import DeviceMeanAveragePrecision, MeanAveragePrecision

DEV = "cuda:0"


def batch(rng, B=16, K=100, G=3, S=640):
    c = rng.uniform(60, 580, (B, G, 2)); wh = rng.uniform(20, 200, (B, G, 2))
    gt = np.concatenate([c - wh / 2, c + wh / 2], -1)
    src = rng.integers(0, G, (B, K))
    db = np.take_along_axis(gt, src[..., None], 1) + rng.normal(0, 8, (B, K, 4))
    db = np.sort(db.reshape(B, K, 2, 2), axis=2).reshape(B, K, 4).clip(0, S).astype(np.float32)
    sc = rng.uniform(0.05, 1, (B, K)).astype(np.float32)
    dl = rng.integers(0, 2, (B, K)); gl = rng.integers(0, 2, (B, G))
    rows = np.concatenate([np.repeat(np.arange(B), G)[:, None], gl.reshape(-1, 1), (c / S).reshape(-1, 2), (wh / S).reshape(-1, 2)], 1).astype(np.float32)
    return db, sc, dl, rows


def dev_det(db, sc, dl):
    B, K = sc.shape
    return dict(boxes=torch.from_numpy(db).to(DEV), scores=torch.from_numpy(sc).to(DEV), labels=torch.from_numpy(dl).to(DEV),
                counts=torch.full((B,), K, dtype=torch.int32, device=DEV))


if "--kernel" in sys.argv:
    rng = np.random.default_rng(0)
    db, sc, dl, rows = batch(rng)
    det, gt = dev_det(db, sc, dl), torch.from_numpy(rows).to(DEV)
    m = DeviceMeanAveragePrecision()
    for _ in range(30):
        m.update_batched(det, gt, 640)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(100):
        m.update_batched(det, gt, 640)
    torch.cuda.synchronize()
    print(f"update_batched wall: {(time.perf_counter() - t) / 100 * 1e6:.1f} us per 16-image batch (incl. host launch + record copies)")
    print("map", m.compute()["map"])

if "--host" in sys.argv:
    rng = np.random.default_rng(1)
    dm, hm = DeviceMeanAveragePrecision(), MeanAveragePrecision()
    n = 0
    while n < 5000:
        db, sc, dl, rows = batch(rng)
        dm.update_batched(dev_det(db, sc, dl), torch.from_numpy(rows).to(DEV), 640)
        B = sc.shape[0]
        for b in range(B):
            r = rows[rows[:, 0] == b]
            cx, cy, w, h = r[:, 2:6].T                                     # the kernel's fp32 per-box conversion
            s = np.float32(640)
            g = np.stack([(cx - w / 2) * s, (cy - h / 2) * s, (cx + w / 2) * s, (cy + h / 2) * s], 1).clip(0, s)
            hm.update([dict(boxes=db[b], scores=sc[b], labels=dl[b])], [dict(boxes=g, labels=r[:, 1].astype(np.int64))])
        n += B
    torch.cuda.synchronize()
    t = time.perf_counter(); rd = dm.compute(); td = time.perf_counter() - t
    t = time.perf_counter(); rh = hm.compute(); th = time.perf_counter() - t
    print(f"{n} images x 100 detections: compute() device class {td:.3f} s (keys {len(rd)}), host class {th:.3f} s (keys {len(rh)})")
    print("map", rd["map"], rh["map"], "map_small/medium/large", rd["map_small"], rd["map_medium"], rd["map_large"])
    assert all(rd[k] == rh[k] for k in rh), (rd, rh)
