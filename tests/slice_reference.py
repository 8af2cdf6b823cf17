"""CPU restatement of sliced inference (`mtbt_merge_tiles`, `mtbt_vote_tile_masks`, include/mtbt_hip.h).  TEST INFRASTRUCTURE.

  frame box    clamp((v + off) / scale, 0, hi) per component, fp32: one add, one division (`frame_reference.frame_boxes` with the tile's
               offset added first)
  order        `fuse_reference.descending_order` of the candidates' scores and their index c = (tile within the image) K + k
  merging      greedy in that order: a free candidate opens a row and absorbs every later free candidate of its label whose metric with
               the LEADER's own box exceeds thr; IoU is `fuse_reference.overlaps`, IoS the same intersection over the smaller area
  Ss, W        fp32, one correctly rounded operation at a time: members in ascending c; multiply, then add from 0; one division
  masks        per tile, `frame_reference`'s bilinear form at sx = max((X + 0.5) * step - 0.5 - pox, 0); the taps of the tiles whose window
               holds the pixel are added in ascending tile order from 0; its crop / pack rules
"""
import numpy as np
import torch

import frame_reference as FR
import fuse_reference as FU

F = np.float32
METRICS = {"iou": 0, "ios": 1}


def frame_boxes(boxes, tile):
    """[n,4] canvas xyxy of one tile -> the image's frame."""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    off = np.array([tile["fox"], tile["foy"], tile["fox"], tile["foy"]], np.float32)
    hi = np.array([tile["width"], tile["height"], tile["width"], tile["height"]], np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = (b + off) / F(tile["scale"])
    return np.fmin(np.fmax(q, F(0)), hi).astype(np.float32)


def metric_of(box, others, metric):
    """metric(box_i, box_j) of one leader box against [n,4] others: the NMS intersection and areas."""
    if metric == "iou":
        return FU.overlaps(others, box)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        iarea = (box[2] - box[0]) * (box[3] - box[1])
        jarea = (others[:, 2] - others[:, 0]) * (others[:, 3] - others[:, 1])
        xx1, yy1 = np.fmax(others[:, 0], box[0]), np.fmax(others[:, 1], box[1])
        xx2, yy2 = np.fmin(others[:, 2], box[2]), np.fmin(others[:, 3], box[3])
        w, h = np.fmax(F(0), xx2 - xx1), np.fmax(F(0), yy2 - yy1)
        return (w * h) / np.fmin(iarea, jarea)


def merge_image(det, t0, tiles, K, metric, thr, skip_thr, top_k, class_agnostic):
    """One image whose tiles are det rows [t0, t0 + len(tiles))."""
    thr, skip_thr = F(thr), F(skip_thr)
    cb, cs, cl, cc = [np.zeros((0, 4), np.float32)], [np.zeros(0, np.float32)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for tl, tile in enumerate(tiles):
        t = t0 + tl
        cnt = max(0, min(int(det["counts"][t]), K))
        s = np.asarray(det["scores"][t], dtype=np.float32)[:cnt]
        keep = s > skip_thr
        cb.append(frame_boxes(det["boxes"][t][:cnt], tile)[keep])
        cs.append(s[keep])
        cl.append(np.asarray(det["labels"][t], dtype=np.int64)[:cnt][keep])
        cc.append((tl * K + np.arange(cnt, dtype=np.int64))[keep])
    cb, cs, cl, cc = np.concatenate(cb), np.concatenate(cs), np.concatenate(cl), np.concatenate(cc)
    order = FU.descending_order(cs, cc)
    cb, cs, cl, cc = cb[order], cs[order], cl[order], cc[order]
    nc = len(cs)
    state = np.full(nc, -1, np.int64)
    rows = 0
    for i in range(nc):
        if state[i] != -1:
            continue
        if rows == top_k:
            break
        state[i] = rows
        later = np.arange(i + 1, nc)
        if len(later):
            m = metric_of(cb[i], cb[later], metric)
            hit = (state[later] == -1) & (m > thr)              # (a NaN never matches)
            if not class_agnostic:
                hit &= cl[later] == cl[i]
            state[later[hit]] = rows
        rows += 1
    out = {
        "boxes_frame": np.zeros((top_k, 4), np.float32), "scores": np.zeros(top_k, np.float32), "labels": np.full(top_k, -1, np.int64),
        "n_members": np.zeros(top_k, np.int32), "lead_tile": np.full(top_k, -1, np.int32), "lead_slot": np.full(top_k, -1, np.int32),
        "lead_anchor": np.full(top_k, -1, np.int32), "counts": np.int32(rows), "n_left": np.int32((state == -1).sum()),
    }
    member_slot = np.full(len(tiles) * K, -1, np.int32)
    member_slot[cc] = state
    for r in range(rows):
        mem = np.nonzero(state == r)[0]
        lead = mem[0]
        out["boxes_frame"][r] = np.concatenate([cb[mem, :2].min(0), cb[mem, 2:].max(0)])
        out["scores"][r], out["labels"][r], out["n_members"][r] = cs[lead], cl[lead], len(mem)
        out["lead_tile"][r], out["lead_slot"][r] = t0 + cc[lead] // K, cc[lead] % K
        if "keep_anchor" in det:
            out["lead_anchor"][r] = det["keep_anchor"][out["lead_tile"][r], out["lead_slot"][r]]
    return out, member_slot.reshape(len(tiles), K)


def merge_tiles(det, tiles, metric="ios", thr=0.5, skip_thr=0.0, top_k=None, class_agnostic=False):
    """Batched: det = dict of numpy arrays over the NT tiles (boxes [NT,K,4], scores, labels, counts [NT], keep_anchor); tiles = the
    per-image lists of `preprocess.slice_geometry`.  Returns the arrays `postprocess.merge_tiles` returns."""
    NT, K = det["scores"].shape
    top_k = K if top_k is None else top_k
    rows, slots, t0 = [], [], 0
    for per in tiles:
        o, ms = merge_image(det, t0, per, K, metric, thr, skip_thr, top_k, class_agnostic)
        rows.append(o)
        slots.append(ms)
        t0 += len(per)
    out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    out["member_slot"] = np.concatenate(slots) if slots else np.zeros((0, K), np.int32)
    return out


def vote_coefficients(det, mc, merged, tiles, top_k):
    """W float32 [N, top_k, Tmax, nm] and Ss float32 [N, top_k].  mc: [NT, nm, A] float32."""
    N, K = len(tiles), det["scores"].shape[1]
    Tmax, nm = max(1, max(len(per) for per in tiles)), mc.shape[1]
    W, Ss = np.zeros((N, top_k, Tmax, nm), np.float32), np.zeros((N, top_k), np.float32)
    t0 = 0
    for n, per in enumerate(tiles):
        ms = merged["member_slot"][t0:t0 + len(per)]
        for r in range(min(int(merged["counts"][n]), top_k)):
            ss = F(0)
            for tl, k in zip(*np.nonzero(ms == r)):                            # ascending c = tile ascending, then k ascending
                ss = ss + F(det["scores"][t0 + tl, k])
            Ss[n, r] = ss
            for tl in range(len(per)):
                ks = np.nonzero(ms[tl] == r)[0]
                if not len(ks):
                    continue
                acc = np.zeros(nm, np.float32)
                for k in ks:
                    acc = acc + F(det["scores"][t0 + tl, k]) * np.asarray(mc[t0 + tl, :, int(det["keep_anchor"][t0 + tl, k])], dtype=np.float32)
                W[n, r, tl] = acc / ss
        t0 += len(per)
    return W, Ss


def _taps(lo, hi, size, step, po):
    d = torch.arange(lo, hi, dtype=torch.float32)
    s = torch.clamp((d + 0.5) * torch.tensor(step, dtype=torch.float32) - 0.5 - torch.tensor(float(po), dtype=torch.float32), min=0)
    i0 = torch.clamp(s.to(torch.int64), max=size - 1)
    i1 = torch.clamp(i0 + 1, max=size - 1)
    l1 = torch.clamp(s - i0.to(torch.float32), 0, 1)
    return i0, i1, 1 - l1, l1


def tile_logits(coeffs, protos, tile):
    """coeffs [R,nm], protos [nm,G,G] of one tile -> its taps [R, wy1-wy0, wx1-wx0] at the pixels of its window."""
    G = protos.shape[-1]
    low = torch.einsum("kc,chw->khw", coeffs.float(), protos.float())
    y0, y1, b0, b1 = _taps(tile["wy0"], tile["wy1"], G, tile["step"], tile["poy"])
    x0, x1, a0, a1 = _taps(tile["wx0"], tile["wx1"], G, tile["step"], tile["pox"])
    top = a0 * low[:, y0][:, :, x0] + a1 * low[:, y0][:, :, x1]
    bot = a0 * low[:, y1][:, :, x0] + a1 * low[:, y1][:, :, x1]
    return b0[:, None] * top + b1[:, None] * bot


def vote_reference(W, merged, protos, tiles, crop=False, only_tile=None):
    """The mask half.  W [N,top_k,Tmax,nm] numpy, protos float32 torch [NT,nm,G,G].  Per image dict(logits [top_k,H0,W0] (the summed taps),
    contrib int [top_k,H0,W0] (tiles added at the pixel), bits, region, packed).  only_tile[n][r] = the one tile (within the image)
    allowed to vote for row r (the leader-only plane of the tests)."""
    out, t0 = [], 0
    top_k = W.shape[1]
    for n, per in enumerate(tiles):
        H0, W0 = per[0]["height"], per[0]["width"]
        cnt = min(int(merged["counts"][n]), top_k)
        ms = merged["member_slot"][t0:t0 + len(per)]
        logits = torch.zeros(top_k, H0, W0)
        contrib = torch.zeros(top_k, H0, W0, dtype=torch.int32)
        for tl, tile in enumerate(per):
            has = torch.tensor([r < cnt and bool((ms[tl] == r).any()) and (only_tile is None or only_tile[n][r] == tl) for r in range(top_k)])
            if not has.any():
                continue
            v = tile_logits(torch.from_numpy(np.ascontiguousarray(W[n, :, tl])), protos[t0 + tl], tile)
            win = (slice(None), slice(tile["wy0"], tile["wy1"]), slice(tile["wx0"], tile["wx1"]))
            logits[win] = torch.where(has[:, None, None], logits[win] + v, logits[win])
            contrib[win] += has[:, None, None].to(torch.int32)
        bits = logits > 0
        region = None
        if crop:
            region = FR.crop_region(torch.from_numpy(np.ascontiguousarray(merged["boxes_frame"][n])), H0, W0)
            region[cnt:] = False
            bits = bits & region
        out.append({"logits": logits, "contrib": contrib, "bits": bits, "region": region, "packed": FR.pack_bits(bits)})
        t0 += len(per)
    return out


# ---- inputs for the tests --------------------------------------------------------------------------------------------------------
def tile_lists(tiles, K, seed, S, A=300, nm=32, n_obj=20, empty=(), cells=17):
    """Detection lists of the tiles of `tiles`: every image has n_obj objects (boxes around a few centres, two labels), and a tile lists
    the objects it sees -- the box moved to its canvas, jittered by up to 1.5 px, clipped at the canvas border, dropped when less than 6 px
    of it is left -- by descending score, at most K, padded as the NMS pads.  Coordinates are multiples of 1/8 px.  keep_anchor is the
    cell of a cells x cells grid over the image the object's centre falls in (mod A): the members of a row mostly carry the same
    coefficients.  Images in `empty` get no detections.  Returns (det dict of numpy arrays, mc [NT,nm,A] strided like the model's,
    protos [NT,nm,G,G])."""
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    NT = sum(len(per) for per in tiles)
    det = {"boxes": np.zeros((NT, K, 4), np.float32), "scores": np.zeros((NT, K), np.float32), "labels": np.full((NT, K), -1, np.int64),
           "counts": np.zeros(NT, np.int32), "keep_anchor": np.full((NT, K), -1, np.int32)}
    G = S // 4
    mcs, t = [], 0
    for n, per in enumerate(tiles):
        H0, W0 = per[0]["height"], per[0]["width"]
        m = min(H0, W0)
        centres = rng.random((6, 2)) * [W0 * 0.8, H0 * 0.8] + [W0 * 0.1, H0 * 0.1]
        c = centres[rng.integers(0, 6, n_obj)] + rng.normal(size=(n_obj, 2)) * m * 0.05
        wh = rng.random((n_obj, 2)) * m * 0.2 + m * 0.1
        obj = np.concatenate([c - wh / 2, c + wh / 2], 1)
        label = rng.integers(0, 2, n_obj)
        score = rng.random(n_obj) * 0.85 + 0.1
        cell = np.clip((c[:, 0] / W0 * cells).astype(np.int64), 0, cells - 1) * cells + np.clip((c[:, 1] / H0 * cells).astype(np.int64), 0, cells - 1)
        base_c = torch.randn(A, nm, generator=g)
        for tile in per:
            z, off = tile["zoom"], np.array([tile["ox"], tile["oy"], tile["ox"], tile["oy"]], np.float64)
            b = np.clip(np.round((obj * z - off + rng.uniform(-1.5, 1.5, size=obj.shape)) * 8) / 8, 0, S)
            s = (score + rng.uniform(-0.04, 0.04, n_obj)).astype(np.float32)
            seen = ((b[:, 2] - b[:, 0]) >= 6) & ((b[:, 3] - b[:, 1]) >= 6) & (n not in empty)
            idx = np.nonzero(seen)[0]
            idx = idx[np.argsort(-s[idx], kind="stable")][:K]
            k = len(idx)
            det["boxes"][t, :k], det["scores"][t, :k], det["labels"][t, :k] = b[idx], s[idx], label[idx]
            det["keep_anchor"][t, :k], det["counts"][t] = cell[idx] % A, k
            mcs.append(base_c + 0.1 * torch.randn(A, nm, generator=g))
            t += 1
    mc = torch.stack(mcs).permute(0, 2, 1)
    protos = torch.randn(NT, nm, G, G, generator=g)
    return det, mc, protos
