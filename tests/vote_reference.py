"""CPU restatement of the mask vote over fused detections (`mtbt_fuse_detections_members` + `mtbt_vote_masks`, include/mtbt_hip.h).
TEST INFRASTRUCTURE.

  membership   the greedy pass of `fuse_reference.fuse_image`, re-derived with its own helpers and keeping, for every candidate
               c = m K + k, the cluster it opened or joined; after the output order, the cluster's row (-1 past the top_k cut and for
               slots that were no candidates).  Boxes, scores and member counts must equal `fuse_reference.fuse_image` bit for bit
               (`fuse_members` asserts it).
  Ss, W        fp32, one correctly rounded operation at a time in the header's order: members in ascending c; multiply, then add; one
               division at the end.
  low, bits    `frame_reference.frame_logits` on the 32 M coefficients of a row against the 32 M upright prototype channels
               (m ascending, c ascending), then its crop / pack rules.
"""
import numpy as np
import torch

import frame_reference as FR
import fuse_reference as FU

F = np.float32


def members_image(sources, orients, weights, S, iou_thr, skip_thr, top_k, K):
    """One image: (member_slot int32 [M K], boxes [top_k,4], scores [top_k], n_members [top_k], count) -- `fuse_reference.fuse_image`'s
    candidates, order, greedy pass and output order, with the membership kept."""
    M = len(sources)
    iou_thr, skip_thr = F(iou_thr), F(skip_thr)
    cb, cs, cl, cc = [], [], [], []
    for m, (boxes, scores, labels, count, _) in enumerate(sources):
        cnt = max(0, min(int(count), K))
        s = np.asarray(scores, dtype=np.float32)[:cnt] * F(weights[m])
        keep = s > skip_thr
        cb.append(FU.unorient(np.asarray(boxes, dtype=np.float32)[:cnt], orients[m], S)[keep])
        cs.append(s[keep])
        cl.append(np.asarray(labels, dtype=np.int64)[:cnt][keep])
        cc.append((m * K + np.arange(cnt, dtype=np.int64))[keep])
    cb, cs, cl, cc = np.concatenate(cb), np.concatenate(cs), np.concatenate(cl), np.concatenate(cc)
    order = FU.descending_order(cs, cc)
    cb, cs, cl, cc = cb[order], cs[order], cl[order], cc[order]
    nc = len(cs)
    fused, sums = np.zeros((nc, 4), np.float32), np.zeros((nc, 4), np.float32)
    ss, label, members = np.zeros(nc, np.float32), np.zeros(nc, np.int64), np.zeros(nc, np.int32)
    cluster_of = np.zeros(nc, np.int64)
    ncl = 0
    for j in range(nc):
        best, bi = F(-np.inf), -1
        if ncl:
            ovr = FU.overlaps(fused[:ncl], cb[j])
            ovr = np.where((label[:ncl] == cl[j]) & ~np.isnan(ovr), ovr, F(-np.inf))
            k = int(np.argmax(ovr))
            if ovr[k] > best:
                best, bi = ovr[k], k
        if best > iou_thr:
            ss[bi] = ss[bi] + cs[j]
            sums[bi] = sums[bi] + cs[j] * cb[j]
            members[bi] += 1
            fused[bi] = sums[bi] / ss[bi]
            cluster_of[j] = bi
        else:
            ss[ncl], sums[ncl], members[ncl], fused[ncl], label[ncl] = cs[j], cs[j] * cb[j], 1, cb[j], cl[j]
            cluster_of[j] = ncl
            ncl += 1
    W = F(weights[0])
    for m in range(1, M):
        W = W + F(weights[m])
    score = ((ss[:ncl] / members[:ncl].astype(np.float32)) * np.minimum(members[:ncl], M).astype(np.float32)) / W
    out_order = FU.descending_order(score, np.arange(ncl))[:top_k]
    n = len(out_order)
    row_of = np.full(ncl, -1, np.int32)
    row_of[out_order] = np.arange(n, dtype=np.int32)
    member_slot = np.full(M * K, -1, np.int32)
    if nc:
        member_slot[cc] = row_of[cluster_of]
    boxes, scores, n_members = np.zeros((top_k, 4), np.float32), np.zeros(top_k, np.float32), np.zeros(top_k, np.int32)
    boxes[:n], scores[:n], n_members[:n] = fused[out_order], score[out_order], members[out_order]
    return member_slot, boxes, scores, n_members, n


def fuse_members(dets, img_size, orients=None, weights=None, iou_thr=0.55, skip_thr=0.0, top_k=None):
    """`fuse_reference.fuse_detections` plus `member_slot` int32 [N, M K].  The re-derived boxes, scores and member counts are asserted
    bit-equal to `fuse_reference.fuse_image`'s."""
    M = len(dets)
    N, K = dets[0]["scores"].shape
    orients = [0] * M if orients is None else list(orients)
    weights = [1.0] * M if weights is None else list(weights)
    top_k = K if top_k is None else top_k
    out = FU.fuse_detections(dets, img_size, orients, weights, iou_thr, skip_thr, top_k)
    slots = []
    for n in range(N):
        srcs = [(d["boxes"][n], d["scores"][n], d["labels"][n], d["counts"][n], None) for d in dets]
        ms, boxes, scores, n_members, cnt = members_image(srcs, orients, weights, img_size, iou_thr, skip_thr, top_k, K)
        assert cnt == out["counts"][n]
        assert np.array_equal(boxes.view(np.uint32), out["boxes"][n].view(np.uint32))
        assert np.array_equal(scores.view(np.uint32), out["scores"][n].view(np.uint32))
        assert np.array_equal(n_members, out["n_members"][n])
        slots.append(ms)
    out["member_slot"] = np.stack(slots)
    return out


def vote_coefficients(dets, mcs, member_slot, counts, weights, top_k):
    """W float32 [N, top_k, M, nm] and Ss float32 [N, top_k].  dets[m]: scores [N,K], keep_anchor [N,K]; mcs[m]: [N, nm, A] float32."""
    M = len(dets)
    N, K = dets[0]["scores"].shape
    nm = mcs[0].shape[1]
    W, Ss = np.zeros((N, top_k, M, nm), np.float32), np.zeros((N, top_k), np.float32)
    for n in range(N):
        for r in range(min(int(counts[n]), top_k)):
            ss = F(0)
            for c in np.nonzero(member_slot[n] == r)[0]:                       # ascending c = m ascending, then k ascending
                ss = ss + F(dets[c // K]["scores"][n, c % K]) * F(weights[c // K])
            Ss[n, r] = ss
            for m in range(M):
                ks = np.nonzero(member_slot[n, m * K:(m + 1) * K] == r)[0]
                if not len(ks):
                    continue
                acc = np.zeros(nm, np.float32)
                for k in ks:
                    s = F(dets[m]["scores"][n, k]) * F(weights[m])
                    acc = acc + s * np.asarray(mcs[m][n, :, int(dets[m]["keep_anchor"][n, k])], dtype=np.float32)
                W[n, r, m] = acc / ss
    return W, Ss


def unorient_protos(protos: torch.Tensor, orient: int) -> torch.Tensor:
    """[.., G, G] of a view -> upright (`postprocess.unorient_batch`): the flips undone, then the transpose."""
    dims = [d for bit, d in ((1, -1), (2, -2)) if orient & bit]
    x = protos.flip(dims) if dims else protos
    return (x.transpose(-1, -2) if orient & 4 else x).contiguous()


def orient_protos(protos: torch.Tensor, orient: int) -> torch.Tensor:
    """Upright [.., G, G] -> the view (`postprocess.orient_batch`)."""
    q = protos.transpose(-1, -2) if orient & 4 else protos
    dims = [d for bit, d in ((1, -1), (2, -2)) if orient & bit]
    return (q.flip(dims) if dims else q).contiguous()


def vote_reference(W, counts, boxes, protos, orients, frames, up, crop=False):
    """The mask half for a batch.  W [N,top_k,M,nm] (numpy), counts [N], boxes [N,top_k,4] fused (numpy), protos: per source a float32
    torch tensor [N,nm,G,G] in its view's frame.  Returns per image dict(logits [top_k,H0,W0], bits, region, boxes, packed) as
    `frame_reference.frame_reference` does."""
    N, top_k, M, nm = W.shape
    out = []
    for b, (H0, W0, scale) in enumerate(frames):
        n = min(int(counts[b]), top_k)
        upright = torch.cat([unorient_protos(protos[m][b].float(), orients[m]) for m in range(M)], 0)      # [M nm, G, G]: m, then c
        coeffs = torch.from_numpy(np.ascontiguousarray(W[b])).reshape(top_k, M * nm).clone()
        coeffs[n:] = 0
        logits = FR.frame_logits(coeffs, upright, H0, W0, scale, up)
        logits[n:] = 0
        fb = FR.frame_boxes(torch.from_numpy(np.ascontiguousarray(boxes[b])), n, H0, W0, scale)
        bits = logits > 0
        region = None
        if crop:
            region = FR.crop_region(fb, H0, W0)
            bits = bits & region
        out.append({"logits": logits, "bits": bits, "region": region, "boxes": fb, "packed": FR.pack_bits(bits)})
    return out


def vote_inputs(dets, N, G, seed, orients, S=640.0, A=300, nm=32, cells=17):
    """Mask inputs for `fuse_reference.clustered_lists` detections.  The sources share one UPRIGHT prototype stack and one coefficient
    table up to a small per-source perturbation, and a live slot's `keep_anchor` is re-drawn as the cell of a cells x cells grid its
    upright box centre falls in (mod A): the members of a cluster mostly carry the same coefficients, as the views of one model do, so
    the voted logits keep a single source's magnitude.  Source m's prototypes are given in its view's frame.
    Returns (mcs [M] of [N,nm,A] strided like the model's, protos [M] of [N,nm,G,G])."""
    g = torch.Generator().manual_seed(seed)
    base_p = torch.randn(N, nm, G, G, generator=g)
    base_c = torch.randn(N, A, nm, generator=g)
    mcs, protos = [], []
    for m, d in enumerate(dets):
        K = d["scores"].shape[1]
        live = np.arange(K)[None, :] < d["counts"][:, None]
        up = FU.unorient(d["boxes"].reshape(-1, 4), orients[m], S).reshape(N, K, 4)
        cx, cy = (up[..., 0] + up[..., 2]) / 2, (up[..., 1] + up[..., 3]) / 2
        cell = np.clip((cx / S * cells).astype(np.int64), 0, cells - 1) * cells + np.clip((cy / S * cells).astype(np.int64), 0, cells - 1)
        d["keep_anchor"] = np.where(live, cell % A, -1).astype(np.int32)
        mcs.append((base_c + 0.1 * torch.randn(N, A, nm, generator=g)).permute(0, 2, 1))
        protos.append(orient_protos(base_p + 0.05 * torch.randn(N, nm, G, G, generator=g), orients[m]))
    return mcs, protos
