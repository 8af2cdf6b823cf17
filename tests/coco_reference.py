"""Plain-loop restatement of pycocotools COCOeval (evaluateImg / accumulate / summarize; no crowd) with the four area ranges and
per-class output, and the random box sets the mAP tests feed it.

A plain module (no fixtures), written out here because oracle/ is frozen.  It shares no code with the product's vectorised
accumulation (`metrics._accumulate`): tests/test_gpu_box_eval.py checks the device box mAP against it, tests/test_cpu_metrics.py the
host MeanAveragePrecision, tests/test_cpu_validation_metrics.py the segmentation mAP."""
import numpy as np

AREAS = [(0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10)]
COCO = np.linspace(0.5, 0.95, 10).tolist()


def _iou(d, g):
    iw = max(min(d[2], g[2]) - max(d[0], g[0]), 0.0)
    ih = max(min(d[3], g[3]) - max(d[1], g[1]), 0.0)
    inter = iw * ih
    union = (d[2] - d[0]) * (d[3] - d[1]) + (g[2] - g[0]) * (g[3] - g[1]) - inter
    return inter / union if union > 0 else 0.0


def _area(b):
    return (b[2] - b[0]) * (b[3] - b[1])


def coco_loop(preds, targets, thr, max_dets, class_metrics=False):
    """bbox: per image preds dict(boxes [D,4] xyxy, scores [D], labels [D]) and targets dict(boxes [G,4] xyxy, labels [G])."""
    images = []
    for p, t in zip(preds, targets):
        dt, gt = [[float(v) for v in b] for b in p["boxes"]], [[float(v) for v in b] for b in t["boxes"]]
        images.append(([float(s) for s in p["scores"]], [int(l) for l in p["labels"]], [_area(d) for d in dt],
                       [int(l) for l in t["labels"]], [_area(g) for g in gt], [[_iou(d, g) for g in gt] for d in dt]))
    return coco_loop_iou(images, thr, max_dets, class_metrics)


def coco_loop_iou(images, thr, max_dets, class_metrics=False):
    """The same restatement from per-image IoU matrices instead of boxes (a segmentation mAP has only pixel counts):
    images = [(det scores [D], det labels [D], det areas [D], GT labels [G], GT areas [G], IoU [D][G])]."""
    thr, max_dets = list(thr), sorted(max_dets)
    T, A, Md, R = len(thr), len(AREAS), len(max_dets), 101
    rec_thr = np.linspace(0.0, 1.0, R)
    classes = sorted({int(l) for im in images for l in im[1]} | {int(l) for im in images for l in im[3]})
    ev = {}
    for i, (scores, labels, d_area, gt_labels, g_area, iou) in enumerate(images):                # evaluateImg
        for k, c in enumerate(classes):
            gt = [j for j, l in enumerate(gt_labels) if int(l) == c]
            dt = [j for j, l in enumerate(labels) if int(l) == c]
            for a, (lo, hi) in enumerate(AREAS):
                if not gt and not dt:
                    continue
                gig = [1 if (g_area[j] < lo or g_area[j] > hi) else 0 for j in gt]
                gind = sorted(range(len(gt)), key=lambda j: gig[j])
                gs, gigs = [gt[j] for j in gind], [gig[j] for j in gind]
                ds = [dt[j] for j in sorted(range(len(dt)), key=lambda j: -scores[dt[j]])][: max_dets[-1]]
                dtm, dtig = np.zeros((T, len(ds)), bool), np.zeros((T, len(ds)), bool)
                for ti, tv in enumerate(thr):
                    gtm = [0] * len(gs)
                    for di, d in enumerate(ds):
                        best, m = min(tv, 1 - 1e-10), -1
                        for gi, g in enumerate(gs):
                            if gtm[gi]:
                                continue
                            if m > -1 and gigs[m] == 0 and gigs[gi] == 1:
                                break
                            v = iou[d][g]
                            if v < best:
                                continue
                            best, m = v, gi
                        if m == -1:
                            continue
                        dtig[ti, di], dtm[ti, di], gtm[m] = bool(gigs[m]), True, 1
                    for di, d in enumerate(ds):
                        if not dtm[ti, di] and (d_area[d] < lo or d_area[d] > hi):
                            dtig[ti, di] = True
                ev[k, a, i] = ([scores[d] for d in ds], dtm, dtig, gigs)
    precision, recall = -np.ones((T, R, len(classes), A, Md)), -np.ones((T, len(classes), A, Md))
    for k in range(len(classes)):                                                               # accumulate
        for a in range(A):
            es = [ev[k, a, i] for i in range(len(images)) if (k, a, i) in ev]
            npig = sum(1 for e in es for g in e[3] if g == 0)
            if npig == 0:
                continue
            for m, md in enumerate(max_dets):
                sc = np.array([s for e in es for s in e[0][:md]])
                inds = np.argsort(-sc, kind="mergesort")
                dtm = np.concatenate([e[1][:, :md] for e in es], 1)[:, inds]
                dtig = np.concatenate([e[2][:, :md] for e in es], 1)[:, inds]
                tp_sum = np.cumsum(dtm & ~dtig, axis=1).astype(np.float64)
                fp_sum = np.cumsum(~dtm & ~dtig, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = (tp / (fp + tp + np.spacing(1))).tolist()
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(R)
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thr, side="left")):
                        if pi >= nd:
                            break
                        q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q

    def mean(s):                                                                                # summarize
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    out = {"map": mean(precision[:, :, :, 0, -1])}
    for name, tv in (("map_50", 0.5), ("map_75", 0.75)):
        hit = [j for j, v in enumerate(thr) if np.isclose(v, tv)]
        out[name] = mean(precision[hit[0], :, :, 0, -1]) if hit else -1.0
    for a, name in ((1, "small"), (2, "medium"), (3, "large")):
        out[f"map_{name}"] = mean(precision[:, :, :, a, -1])
    for m, md in enumerate(max_dets):
        out[f"mar_{md}"] = mean(recall[:, :, 0, m])
    for a, name in ((1, "small"), (2, "medium"), (3, "large")):
        out[f"mar_{name}"] = mean(recall[:, :, a, -1])
    if class_metrics:
        out["classes"] = classes
        out["map_per_class"] = [mean(precision[:, :, k, 0, -1]) for k in range(len(classes))]
        out[f"mar_{max_dets[-1]}_per_class"] = [mean(recall[:, k, 0, -1]) for k in range(len(classes))]
    return out


def _random_set(seed, n_img=40):
    """Boxes on integer pixels (areas exact, incl. 32^2 and 96^2), scores rounded to 0.1 (ties), 3 classes of which class 2
    has detections but no GT, images without GT and images without detections, duplicated GT boxes (equal-IoU ties)."""
    rng = np.random.default_rng(seed)
    sides = np.array([6, 16, 30, 32, 33, 50, 80, 96, 97, 150])
    preds, targets = [], []
    for i in range(n_img):
        G = 0 if i % 9 == 4 else int(rng.integers(1, 7))
        wh = np.where(rng.uniform(size=(G, 1)) < 0.4, rng.choice(sides, (G, 1)), rng.choice(sides, (G, 2)))
        wh = np.broadcast_to(wh, (G, 2))
        xy = rng.integers(0, 400, (G, 2))
        gb = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        gl = rng.integers(0, 2, G)
        if G > 1 and rng.uniform() < 0.3:
            gb[-1], gl[-1] = gb[0], gl[0]
        D = 0 if i % 9 == 7 else int(rng.integers(1, 30))
        if G:
            src = rng.integers(0, G, D)
            db = gb[src] + np.round(rng.normal(0, 3.0, (D, 4)) * (rng.uniform(size=(D, 1)) < 0.7))
            dl = np.where(rng.uniform(size=D) < 0.8, gl[src], rng.integers(0, 3, D))
        else:
            db, dl = np.zeros((D, 4)), rng.integers(0, 3, D)
        far = rng.uniform(size=D) < 0.2
        db[far] = np.concatenate([rng.integers(0, 400, (int(far.sum()), 2)), rng.integers(420, 600, (int(far.sum()), 2))], 1)
        db = np.sort(db.reshape(D, 2, 2), axis=1).reshape(D, 4)                                   # x1 <= x2, y1 <= y2
        preds.append(dict(boxes=db.astype(np.float32), scores=np.round(rng.uniform(0, 1, D), 1).astype(np.float32), labels=dl.astype(np.int64)))
        targets.append(dict(boxes=gb, labels=gl.astype(np.int64)))
    return preds, targets
