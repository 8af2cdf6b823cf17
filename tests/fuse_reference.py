"""numpy float32 restatement of `mtbt_fuse_detections` (include/mtbt_hip.h): weighted boxes fusion of M detection lists.

The arithmetic is the project's own definition, one correctly rounded fp32 operation at a time in the order the header writes it, so the
kernel is compared with `torch.equal`.  The greedy pass is vectorised over the clusters (one numpy expression per candidate): an image of
4096 candidates takes a few seconds."""
import numpy as np

F = np.float32


def orderable(x):
    """The NMS key of an fp32 value: unsigned integers in the order of the floats."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def descending_order(values, index):
    """Ascending 64-bit keys ~orderable(value) << 32 | index: stable descending value, ties to ascending index."""
    keys = ((~orderable(values)).astype(np.uint64) << np.uint64(32)) | np.asarray(index, dtype=np.uint64)
    return np.argsort(keys, kind="stable")


def unorient(boxes, orient, S):
    """[n, 4] xyxy of a view -> the upright frame: two corner points through the inverse of the augmentation's pixel rule."""
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4)
    S = F(S)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    if orient & 1:
        x1, x2 = S - x1, S - x2
    if orient & 2:
        y1, y2 = S - y1, S - y2
    if orient & 4:
        x1, y1, x2, y2 = y1, x1, y2, x2
    return np.stack([np.fmin(x1, x2), np.fmin(y1, y2), np.fmax(x1, x2), np.fmax(y1, y2)], axis=1).astype(np.float32)


def overlaps(fused, box):
    """ovr of every cluster's fused box (i) with one candidate box (j): the NMS arithmetic."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        iarea = (fused[:, 2] - fused[:, 0]) * (fused[:, 3] - fused[:, 1])
        jarea = (box[2] - box[0]) * (box[3] - box[1])
        xx1, yy1 = np.fmax(fused[:, 0], box[0]), np.fmax(fused[:, 1], box[1])
        xx2, yy2 = np.fmin(fused[:, 2], box[2]), np.fmin(fused[:, 3], box[3])
        w, h = np.fmax(F(0), xx2 - xx1), np.fmax(F(0), yy2 - yy1)
        inter = w * h
        return inter / ((iarea + jarea) - inter)


def fuse_image(sources, orients, weights, S, iou_thr, skip_thr, top_k, K):
    """One image.  sources: per source (boxes [K,4] f32, scores [K] f32, labels [K] i64, count, anchors [K] i32 or None)."""
    M = len(sources)
    iou_thr, skip_thr = F(iou_thr), F(skip_thr)
    cb, cs, cl, cc = [], [], [], []
    for m, (boxes, scores, labels, count, _) in enumerate(sources):
        cnt = max(0, min(int(count), K))
        s = np.asarray(scores, dtype=np.float32)[:cnt] * F(weights[m])
        keep = s > skip_thr
        cb.append(unorient(np.asarray(boxes, dtype=np.float32)[:cnt], orients[m], S)[keep])
        cs.append(s[keep])
        cl.append(np.asarray(labels, dtype=np.int64)[:cnt][keep])
        cc.append((m * K + np.arange(cnt, dtype=np.int64))[keep])
    cb, cs, cl, cc = np.concatenate(cb), np.concatenate(cs), np.concatenate(cl), np.concatenate(cc)
    order = descending_order(cs, cc)
    cb, cs, cl, cc = cb[order], cs[order], cl[order], cc[order]

    nc = len(cs)
    fused = np.zeros((nc, 4), np.float32)
    sums = np.zeros((nc, 4), np.float32)
    ss = np.zeros(nc, np.float32)
    label = np.zeros(nc, np.int64)
    members = np.zeros(nc, np.int32)
    lead = np.zeros(nc, np.int64)
    ncl = 0
    for j in range(nc):
        best, bi = F(-np.inf), -1
        if ncl:
            ovr = overlaps(fused[:ncl], cb[j])
            ovr = np.where((label[:ncl] == cl[j]) & ~np.isnan(ovr), ovr, F(-np.inf))
            k = int(np.argmax(ovr))                     # first of the largest: the lowest cluster index
            if ovr[k] > best:
                best, bi = ovr[k], k
        if best > iou_thr:
            ss[bi] = ss[bi] + cs[j]
            sums[bi] = sums[bi] + cs[j] * cb[j]
            members[bi] += 1
            fused[bi] = sums[bi] / ss[bi]
        else:
            ss[ncl], sums[ncl], members[ncl], fused[ncl], label[ncl], lead[ncl] = cs[j], cs[j] * cb[j], 1, cb[j], cl[j], cc[j]
            ncl += 1

    W = F(weights[0])
    for m in range(1, M):
        W = W + F(weights[m])
    score = ((ss[:ncl] / members[:ncl].astype(np.float32)) * np.minimum(members[:ncl], M).astype(np.float32)) / W
    order = descending_order(score, np.arange(ncl))[:top_k]
    n = len(order)
    out = {
        "boxes": np.zeros((top_k, 4), np.float32), "scores": np.zeros(top_k, np.float32), "labels": np.full(top_k, -1, np.int64),
        "n_members": np.zeros(top_k, np.int32), "lead_source": np.full(top_k, -1, np.int32), "lead_slot": np.full(top_k, -1, np.int32),
        "counts": np.int32(n), "n_clusters": np.int32(ncl),
    }
    out["boxes"][:n], out["scores"][:n], out["labels"][:n], out["n_members"][:n] = fused[order], score[order], label[order], members[order]
    out["lead_source"][:n], out["lead_slot"][:n] = lead[order] // K, lead[order] % K
    if all(src[4] is not None for src in sources):
        out["lead_anchor"] = np.full(top_k, -1, np.int32)
        for r in range(n):
            out["lead_anchor"][r] = sources[out["lead_source"][r]][4][out["lead_slot"][r]]
    return out


def fuse_detections(dets, img_size, orients=None, weights=None, iou_thr=0.55, skip_thr=0.0, top_k=None):
    """Batched: `dets` is a list of dicts of numpy arrays boxes [N,K,4], scores [N,K], labels [N,K], counts [N] and optionally
    keep_anchor [N,K].  Returns the dict of arrays `postprocess.fuse_detections` returns (lead_anchor only with every keep_anchor)."""
    M = len(dets)
    N, K = dets[0]["scores"].shape
    orients = [0] * M if orients is None else list(orients)
    weights = [1.0] * M if weights is None else list(weights)
    top_k = K if top_k is None else top_k
    rows = []
    for n in range(N):
        srcs = [(d["boxes"][n], d["scores"][n], d["labels"][n], d["counts"][n], d["keep_anchor"][n] if "keep_anchor" in d else None) for d in dets]
        rows.append(fuse_image(srcs, orients, weights, img_size, iou_thr, skip_thr, top_k, K))
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


# ---- inputs for the tests --------------------------------------------------------------------------------------------------------
def orient_boxes(boxes, orient, S):
    """Upright [.., 4] xyxy -> the frame of view `orient` (the inverse of `unorient`; exact for coordinates that are multiples of 1/8)."""
    b = np.array(boxes, dtype=np.float32)
    S = F(S)
    x1, y1, x2, y2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    if orient & 4:
        x1, y1, x2, y2 = y1, x1, y2, x2
    if orient & 1:
        x1, x2 = S - x1, S - x2
    if orient & 2:
        y1, y2 = S - y1, S - y2
    return np.stack([np.fmin(x1, x2), np.fmin(y1, y2), np.fmax(x1, x2), np.fmax(y1, y2)], axis=-1).astype(np.float32)


def clustered_lists(M, N, K, counts, seed, S=640.0, nc=2, n_centres=6, jitter=5.0, score_levels=None, orients=None):
    """M detection lists of N images in the manner of the NMS stress set (boxes around a few centres), source m > 0 a jittered copy of
    source 0's objects: most clusters get one member per source.  Coordinates are multiples of 1/8 px.  counts: [M][N].  Each list
    is sorted by descending score over its first counts[m][n] slots, padded as the NMS pads; `keep_anchor` is a made-up anchor index.
    With `orients` the boxes of source m are given in that view's frame."""
    rng = np.random.default_rng(seed)
    base = np.zeros((N, K, 4), np.float32)
    base_label = rng.integers(0, nc, size=(N, K)).astype(np.int64)
    for n in range(N):
        centres = rng.random((n_centres, 2)) * S * 0.6 + S * 0.2
        c = centres[rng.integers(0, n_centres, K)] + rng.normal(size=(K, 2)) * 12
        wh = rng.random((K, 2)) * 60 + 30
        base[n] = np.concatenate([c - wh / 2, c + wh / 2], 1)
    dets = []
    for m in range(M):
        boxes = np.clip(np.round((base + (rng.uniform(-jitter, jitter, size=base.shape) if m else 0.0)) * 8) / 8, 0, S).astype(np.float32)
        if score_levels:
            scores = rng.integers(1, score_levels + 1, size=(N, K)).astype(np.float32) / F(score_levels + 1)
        else:
            scores = (rng.random((N, K)) * 0.9 + 0.05).astype(np.float32)
        labels, anchors = base_label.copy(), rng.integers(0, 8400, size=(N, K)).astype(np.int32)
        cnt = np.asarray(counts[m], dtype=np.int32)
        for n in range(N):
            order = np.argsort(-scores[n, :cnt[n]], kind="stable")
            for arr in (boxes, scores, labels, anchors):
                arr[n, :cnt[n]] = arr[n, :cnt[n]][order]
            boxes[n, cnt[n]:], scores[n, cnt[n]:], labels[n, cnt[n]:], anchors[n, cnt[n]:] = 0, 0, -1, -1
        if orients is not None:
            boxes = orient_boxes(boxes, orients[m], S)
            boxes[np.arange(K)[None, :] >= cnt[:, None]] = 0
        dets.append({"boxes": boxes, "scores": scores, "labels": labels, "counts": cnt, "keep_anchor": anchors})
    return dets
