"""GPU parity of the mask vote over fused detections (`fuse_detections(want_members=True)`, `vote_masks`, `detect_fused(masks="vote")`,
`ValidationStep(fused_masks="vote")`) against its CPU restatement (tests/vote_reference.py) at S = 160, G = 40, A = 300, K = 21, counts
[21, 3, 0], on the clustered lists of tests/fuse_reference.py (clusters really have several members).

Membership, W and Ss are compared bit for bit.  Mask bits may differ from the reference only where the reference's |logit| < BAND_M =
1e-4 * M: the 32-channel band of the frame tests, grown linearly with the 32 M-term sum (the fp32 summation bound grows with the number of
terms; the terms keep a single source's magnitude because W is a weighted MEAN).  The share of such pixels among the live planes is capped
per case at SHARE = 8e-4.  The reference alone (computed on the CPU for this seed, `reference_shares()` below) gives, per case of BIT_CASES
in order, 1.2e-5, 5.1e-5, 2.1e-4, 2.2e-4, 7.7e-5 and 0 (the cropped 1 x 70 frame lies outside every box, the other two planes sets are
small): the cap is 3.5 x the largest, the ratio of the frame test (2e-4 over 5.6e-5), and no case's share exceeds 1e-3."""
import functools

import numpy as np
import pytest
import torch

import frame_reference as FR
import fuse_reference as FU
import vote_reference as VR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import (ConvNeXtBiFPNYOLO, DeviceMaskMeanAveragePrecision, ValidationStep, calibrate_synthetic_heads_,
                                              detect_fused, init_synthetic_, synthetic_images)
    from multitask_bonetumor_yolo_amd import postprocess as pp

DEV = "cuda:0"
S, G, A, K, N, UP = 160.0, 40, 300, 21, 3, 4.0
COUNTS = [21, 3, 0]
BAND, SHARE = 1e-4, 8e-4            # BAND per source
ORIENTS = {1: (0,), 3: (5, 2, 7), 8: (0, 1, 2, 3, 4, 5, 6, 7)}
WEIGHTS = {1: (1.0,), 3: (1.0, 2.0, 0.5), 8: (1.0,) * 8}
SIZES_A = [(97, 211), (211, 97), (1, 70)]
SIZES_B = [(1, 70), (160, 160), (97, 211)]        # the sizes that sat in the empty slot come to the front
SIZES_I = [(160, 160)] * 3
FUSE_KEYS = ("boxes", "scores", "labels", "counts", "n_clusters", "n_members", "lead_source", "lead_slot", "lead_anchor")
# (M, top_k, skip_thr)
FUSE_CASES = [(1, 21, 0.0), (1, 16, 0.0), (3, 21, 0.2), (3, 16, 0.0), (8, 21, 0.0), (8, 16, 0.2)]
# (M, top_k, skip_thr, sizes, crop): all eight orients (M = 8), ragged and cut row groups, every frame size with live planes
BIT_CASES = [(1, 21, 0.0, SIZES_A, False), (3, 21, 0.2, SIZES_A, True), (8, 21, 0.0, SIZES_A, False), (8, 16, 0.2, SIZES_I, True),
             (3, 16, 0.0, SIZES_B, False), (1, 16, 0.0, SIZES_B, True)]


def _frames(sizes):
    return [(H0, W0, S / max(H0, W0)) for H0, W0 in sizes]


@functools.lru_cache(maxsize=None)
def _reference(M, top_k, skip_thr, seed=3):
    """The CPU side of a case, computed once: inputs, fused list with membership, W, Ss."""
    orients, weights = ORIENTS[M], WEIGHTS[M]
    dets = FU.clustered_lists(M, N, K, [COUNTS] * M, seed, S=S, orients=orients)
    mcs, protos = VR.vote_inputs(dets, N, G, seed, orients, S=S, A=A)
    fused = VR.fuse_members(dets, S, orients, weights, skip_thr=skip_thr, top_k=top_k)
    W, Ss = VR.vote_coefficients(dets, mcs, fused["member_slot"], fused["counts"], weights, top_k)
    return dets, mcs, protos, fused, W, Ss


@functools.lru_cache(maxsize=None)
def _reference_bits(M, top_k, skip_thr, sizes, crop):
    dets, mcs, protos, fused, W, Ss = _reference(M, top_k, skip_thr)
    return VR.vote_reference(W, fused["counts"], fused["boxes"], protos, ORIENTS[M], _frames(sizes), UP, crop)


def reference_shares():
    """The reference's own share of in-band pixels per case of BIT_CASES (CPU only; the figures of the module docstring)."""
    out = []
    for M, top_k, skip, sizes, crop in BIT_CASES:
        ref, cnt = _reference_bits(M, top_k, skip, tuple(sizes), crop), _reference(M, top_k, skip)[3]["counts"]
        amb = sum(int((ref[b]["logits"][:int(cnt[b])].abs() < BAND * M).sum()) for b in range(N))
        tot = sum(ref[b]["logits"][:int(cnt[b])].numel() for b in range(N))
        out.append(amb / max(tot, 1))
    return out


def _device_dets(dets):
    return [{k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in d.items()} for d in dets]


def _device_sources(mcs, protos):
    return [(mc.to(DEV), p.to(DEV).contiguous(memory_format=torch.channels_last)) for mc, p in zip(mcs, protos)]


def _fuse(M, top_k, skip_thr, want_members=True):
    dets = _reference(M, top_k, skip_thr)[0]
    return pp.fuse_detections(_device_dets(dets), img_size=S, orients=ORIENTS[M], weights=WEIGHTS[M], skip_thr=skip_thr, top_k=top_k,
                              want_members=want_members)


def _total_bytes(frames, planes):
    return sum((planes * H0 * FR.pitch_of(W0) + 15) // 16 * 16 for H0, W0, _ in frames)


@pytest.mark.parametrize("M,top_k,skip_thr", FUSE_CASES)
def test_membership_is_the_references_and_changes_nothing_else(M, top_k, skip_thr):
    want = _reference(M, top_k, skip_thr)[3]
    got, plain = _fuse(M, top_k, skip_thr), _fuse(M, top_k, skip_thr, want_members=False)
    torch.cuda.synchronize()
    assert "member_slot" not in plain and sorted(k for k in got if k != "member_slot") == sorted(plain)
    for k in FUSE_KEYS:
        w = torch.from_numpy(np.asarray(want[k]))
        assert got[k].dtype == w.dtype and torch.equal(got[k].cpu(), w), k
        assert torch.equal(got[k], plain[k]), k
    ms = got["member_slot"].cpu()
    assert ms.dtype == torch.int32 and tuple(ms.shape) == (N, M * K)
    assert torch.equal(ms, torch.from_numpy(want["member_slot"]))
    if top_k == 16:
        assert (want["n_clusters"] > want["counts"]).any(), "the case must cut clusters"
    if skip_thr > 0:
        assert any(((d["scores"] * np.float32(w) <= np.float32(skip_thr)) & (d["scores"] > 0)).any() for d, w in zip(_reference(M, top_k, skip_thr)[0], WEIGHTS[M]))
    assert M == 1 or (want["n_members"] >= 2).any()


@pytest.mark.parametrize("M,top_k,skip_thr", FUSE_CASES)
def test_vote_coefficients_are_bit_equal(M, top_k, skip_thr):
    dets, mcs, protos, fused, W, Ss = _reference(M, top_k, skip_thr)
    r = pp.vote_masks(_fuse(M, top_k, skip_thr), _device_sources(mcs, protos), ORIENTS[M], WEIGHTS[M], _frames(SIZES_I), up=UP)
    torch.cuda.synchronize()
    assert r["vote_coeff"].dtype == torch.float32 and tuple(r["vote_coeff"].shape) == (N, top_k, M, 32)
    assert torch.equal(r["vote_weight"].cpu(), torch.from_numpy(Ss))
    assert torch.equal(r["vote_coeff"].cpu().view(torch.int32), torch.from_numpy(W).view(torch.int32))
    assert (W != 0).any() and all(not W[n, int(fused["counts"][n]):].any() for n in range(N))


@pytest.mark.parametrize("case", range(len(BIT_CASES)))
def test_bits_against_the_cpu_reference(case):
    M, top_k, skip_thr, sizes, crop = BIT_CASES[case]
    dets, mcs, protos, fused, W, Ss = _reference(M, top_k, skip_thr)
    ref = _reference_bits(M, top_k, skip_thr, tuple(sizes), crop)
    frames = _frames(sizes)
    buf = torch.full((_total_bytes(frames, top_k),), 0xFF, dtype=torch.uint8, device=DEV)       # the kernel must write every byte
    r = pp.vote_masks(_fuse(M, top_k, skip_thr), _device_sources(mcs, protos), ORIENTS[M], WEIGHTS[M], frames, crop=crop, out=buf, up=UP)
    torch.cuda.synchronize()
    assert r["buffer"].data_ptr() == buf.data_ptr()
    amb = tot = bits = 0
    for b, (H0, W0, _) in enumerate(frames):
        n = int(fused["counts"][b])
        packed = r["masks"][b]
        assert packed.dtype == torch.uint8 and tuple(packed.shape) == (top_k, H0, FR.pitch_of(W0))
        allbits = FR.unpack_bits(packed, W0)
        got = allbits[:, :, :W0]
        assert not allbits[:, :, W0:].any(), "padding bits"
        assert not got[n:].any(), "planes r >= counts"
        near = ref[b]["logits"].abs() < BAND * M
        diff = got != ref[b]["bits"]
        print(f"case {case} image {b} {H0}x{W0} M={M} crop={crop}: differing bits {int(diff.sum())}, in-band pixels {int(near[:n].sum())} of {near[:n].numel()}")
        assert not (diff & ~near).any(), "bits differ outside the sign-ambiguous band"
        if crop:
            assert not (got & ~ref[b]["region"]).any(), "bit set outside the fused box"
        amb += int(near[:n].sum())
        tot += near[:n].numel()
        assert torch.equal(r["boxes"][b].cpu(), ref[b]["boxes"]), "boxes_frame is not bit-equal"
        bits += int(got.sum())
    assert bits > 1000 and amb <= SHARE * max(tot, 1), (bits, amb, tot)


@pytest.mark.parametrize("crop", [False, True])
def test_one_source_equals_masks_to_frames(crop):
    """M = 1, orient 0, weight 1 on the GPU: the rows with one member against the frame operator on the leader's coefficients."""
    dets, mcs, protos, fused, W, Ss = _reference(1, 21, 0.0)
    f = _fuse(1, 21, 0.0)
    (mc, pr), = _device_sources(mcs, protos)
    frames = _frames(SIZES_A)
    vote = pp.vote_masks(f, [(mc, pr)], (0,), (1.0,), frames, crop=crop, up=UP)
    one = pp.masks_to_frames(pr, mc, f["lead_anchor"].clamp(min=0), f["counts"], f["boxes"], frames, up=UP, crop=crop)
    lead = torch.from_numpy(fused["lead_anchor"]).clamp(min=0)
    ref = FR.frame_reference(protos[0], mcs[0], lead, fused["counts"], torch.from_numpy(fused["boxes"]), frames, UP, crop)
    assert torch.equal(vote["boxes"], one["boxes"])
    single = torch.from_numpy(fused["n_members"] == 1)
    assert single.any()
    for b, (H0, W0, _) in enumerate(frames):
        diff = (pp.unpack_masks(vote["masks"][b], W0) != pp.unpack_masks(one["masks"][b], W0)).cpu()[single[b]]
        assert not (diff & ~(ref[b]["logits"][single[b]].abs() < BAND)).any()


# ---- more images than one launch takes (32 frames): the chunks of `vote_masks` ------------------------------------------------------
CH_B, CH_G, CH_S, CH_K, CH_ORIENTS = 33, 16, 64.0, 5, (0, 5)
CH_FRAMES = [(H0, W0, CH_S / max(H0, W0)) for H0, W0 in [(20, 30), (30, 20)] * 17][:CH_B]


@functools.lru_cache(maxsize=None)
def _chunk_inputs(seed=7):
    counts = np.random.default_rng(seed).integers(0, CH_K + 1, size=(2, CH_B))
    counts[:, 5], counts[:, CH_B - 1] = 0, (CH_K, 3)                 # an image without detections; the last image has fused rows
    dets = FU.clustered_lists(2, CH_B, CH_K, counts.tolist(), seed, S=CH_S, orients=CH_ORIENTS)
    mcs, protos = VR.vote_inputs(dets, CH_B, CH_G, seed, CH_ORIENTS, S=CH_S, A=A)
    return dets, mcs, protos


def _chunk_call(lo, hi, crop):
    """The public calls on images lo .. hi - 1 alone: fusion with membership, then the vote into a buffer pre-filled with 0xFF."""
    dets, mcs, protos = _chunk_inputs()
    fused = pp.fuse_detections(_device_dets([{k: v[lo:hi] for k, v in d.items()} for d in dets]), img_size=CH_S, orients=CH_ORIENTS,
                               want_members=True)
    frames = CH_FRAMES[lo:hi]
    buf = torch.full((_total_bytes(frames, CH_K),), 0xFF, dtype=torch.uint8, device=DEV)
    r = pp.vote_masks(fused, _device_sources([mc[lo:hi] for mc in mcs], [p[lo:hi] for p in protos]), CH_ORIENTS, None, frames, crop=crop,
                      out=buf, up=CH_S / CH_G)
    assert r["buffer"].data_ptr() == buf.data_ptr()
    return r


@pytest.mark.parametrize("crop", [False, True])
def test_more_than_32_images_are_chunked(crop):
    """33 images, M = 2 (orients 0 and 5), G = 16, S = 64, K = 5, frames 20 x 30 and 30 x 20 in turn: the second launch (image 32 alone)
    writes what a call on that image alone writes, byte for byte, and its planes are the CPU restatement's outside BAND * M."""
    last = CH_B - 1
    whole, head, tail = _chunk_call(0, CH_B, crop), _chunk_call(0, last, crop), _chunk_call(last, CH_B, crop)
    torch.cuda.synchronize()
    at = head["buffer"].numel()                                      # image 32's planes start where 32 images end (16-byte aligned)
    assert whole["buffer"].numel() == at + tail["buffer"].numel()
    assert torch.equal(whole["buffer"][:at], head["buffer"]) and torch.equal(whole["buffer"][at:], tail["buffer"])
    for k in ("boxes", "vote_coeff", "vote_weight"):
        assert torch.equal(whole[k][:last].view(torch.int32), head[k].view(torch.int32)), k
        assert torch.equal(whole[k][last:].view(torch.int32), tail[k].view(torch.int32)), k
    # image 32 against the CPU
    dets, mcs, protos = _chunk_inputs()
    d1 = [{k: v[last:] for k, v in d.items()} for d in dets]
    fused = VR.fuse_members(d1, CH_S, CH_ORIENTS, None, top_k=CH_K)
    W, Ss = VR.vote_coefficients(d1, [mc[last:] for mc in mcs], fused["member_slot"], fused["counts"], (1.0, 1.0), CH_K)
    ref = VR.vote_reference(W, fused["counts"], fused["boxes"], [p[last:] for p in protos], CH_ORIENTS, CH_FRAMES[last:], CH_S / CH_G, crop)[0]
    H0, W0, _ = CH_FRAMES[last]
    n = int(fused["counts"][0])
    packed = whole["masks"][last]
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (CH_K, H0, FR.pitch_of(W0))
    allbits = FR.unpack_bits(packed, W0)
    got = allbits[:, :, :W0]
    assert not allbits[:, :, W0:].any(), "padding bits"
    assert 0 < n and not got[n:].any(), "planes r >= counts"
    near = ref["logits"].abs() < BAND * 2
    diff = got != ref["bits"]
    print(f"crop={crop} image {last} {H0}x{W0}: differing bits {int(diff.sum())}, in-band pixels {int(near[:n].sum())} of {near[:n].numel()}")
    assert not (diff & ~near).any(), "bits differ outside the sign-ambiguous band"
    assert got.any() and torch.equal(whole["boxes"][last].cpu(), ref["boxes"])
    assert not whole["masks"][5].any(), "an image without detections has zero planes"


# ---- the public routes on the synthetic model of test_gpu_ensemble.py ----------------------------------------------------------------
MS, MB, TOP_K = 128, 3, 50
NMS = dict(conf_th=0.05, iou_th=0.6, top_k=TOP_K)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), seed=0).to(DEV).eval()
    return calibrate_synthetic_heads_(m, synthetic_images(MB, MS, seed=5).to(DEV))


@pytest.fixture(scope="module")
def x():
    return synthetic_images(MB, MS, seed=5).to(DEV)


def test_detect_fused_vote(model, x):
    views = (0, 5)
    lead = detect_fused(model, x, MS, views=views, masks=True, **NMS)
    vote = detect_fused(model, x, MS, views=views, masks="vote", **NMS)
    plain = detect_fused(model, x, MS, views=views, **NMS)
    assert sorted(lead) == sorted(list(plain) + ["masks"]) and sorted(vote) == sorted(list(lead) + ["member_slot", "vote_coeff"])
    for k in FUSE_KEYS:
        assert torch.equal(vote[k], plain[k]) and torch.equal(lead[k], plain[k]), k
    assert vote["masks"].dtype == torch.uint8 and tuple(vote["masks"].shape) == (MB, TOP_K, MS, MS) and int(vote["masks"].max()) == 1
    assert vote["member_slot"].dtype == torch.int32 and tuple(vote["member_slot"].shape) == (MB, 2 * TOP_K)
    assert vote["vote_coeff"].dtype == torch.float32 and tuple(vote["vote_coeff"].shape) == (MB, TOP_K, 2, 32)
    assert (vote["n_members"] >= 2).any()
    # masks=True is still the leaders' planes: the leader's coefficients against its own source, turned back
    planes = []
    for v in views:
        with torch.no_grad():
            out = model(pp.orient_batch(x, v), "infer")
        _, mc, protos = out["segment_protos"]
        d = pp.detect_and_segment(out["detect_features"], mc, protos, MS, masks=False, **NMS)
        m, _ = pp.assemble_masks(protos, mc.float(), d["keep_anchor"], d["counts"], (MS, MS))
        planes.append(pp.unorient_batch(m.view(torch.uint8), v))
    ls, lk, cnt = lead["lead_source"].cpu(), lead["lead_slot"].cpu(), lead["counts"].cpu()
    for b in range(MB):
        for r in range(TOP_K):
            want = planes[ls[b, r]][b, lk[b, r]] if r < cnt[b] else torch.zeros_like(lead["masks"][b, r])
            assert torch.equal(lead["masks"][b, r], want), (b, r)
    # frames: packed planes and boxes in the images' own coordinates
    frames = [(100, 128, 1.0), (128, 90, 1.0), (128, 128, 1.0)]
    fr = detect_fused(model, x, MS, views=views, masks="vote", frames=frames, crop=True, **NMS)
    assert "masks" not in fr and fr["boxes_frame"].dtype == torch.float32 and tuple(fr["boxes_frame"].shape) == (MB, TOP_K, 4)
    for b, (H0, W0, _) in enumerate(frames):
        assert fr["masks_frame"][b].dtype == torch.uint8 and tuple(fr["masks_frame"][b].shape) == (TOP_K, H0, FR.pitch_of(W0))
    assert torch.equal(pp.unpack_masks(fr["masks_frame"][2], MS), (vote["masks"][2] > 0) & FR.crop_region(fr["boxes_frame"][2].cpu(), MS, MS).to(DEV))
    with pytest.raises(ValueError):
        detect_fused(model, x, MS, views=views, masks=True, frames=frames, **NMS)
    with pytest.raises(ValueError):
        detect_fused(model, x, MS, views=views, masks="mean", **NMS)


def test_detect_fused_vote_of_one_source_is_the_leader(model, x):
    """One source, view 0, no joins (wbf_iou = 1): every row's vote is its only member, i.e. the leader's mask outside the band."""
    kw = dict(views=(0,), wbf_iou=1.0, **NMS)
    lead, vote = detect_fused(model, x, MS, masks=True, **kw), detect_fused(model, x, MS, masks="vote", **kw)
    with torch.no_grad():
        out = model(x, "infer")
    _, mc, protos = out["segment_protos"]
    _, logits = pp.assemble_masks(protos, mc.float(), lead["lead_anchor"].clamp(min=0), lead["counts"], (MS, MS), want_logits=True)
    assert int(lead["counts"].min()) > 0 and int(lead["n_members"].max()) == 1 and lead["masks"].any()
    diff = vote["masks"] != lead["masks"]
    print(f"differing bits {int(diff.sum())} of {diff.numel()}")
    assert not (diff & ~(logits.abs() < BAND)).any()


def _batch(seed):
    g = torch.Generator().manual_seed(100 + seed)
    rows = []
    for b in range(MB):
        for _ in range(1 + b % 2):
            wh = torch.rand(2, generator=g) * 0.3 + 0.1
            cxy = torch.rand(2, generator=g) * (1 - wh) + wh / 2
            rows.append(torch.cat([torch.tensor([float(b), float(torch.randint(0, 2, (1,), generator=g))]), cxy, wh]))
    masks = (torch.rand(MB, 1, MS, MS, generator=g) > 0.7).float()
    return synthetic_images(MB, MS, seed=seed).to(DEV), torch.stack(rows).to(DEV), masks.to(DEV), torch.randint(0, 2, (MB,), generator=g).to(DEV)


def test_validation_step_scores_the_voted_masks(model):
    proj = torch.nn.Conv2d(model.proto_ch, 1, 1).to(DEV)
    imgs, det_gt, masks_gt, cls_gt = batch = _batch(5)
    views = (0, 1)
    plain = ValidationStep(model, projector=proj, img_size=MS, instance_masks=True)
    tta = ValidationStep(model, projector=proj, img_size=MS, views=views, instance_masks=True, fused_masks="vote")
    lp, lt = plain.step(*batch), tta.step(*batch)
    assert all(torch.equal(a, b) for a, b in zip(lp, lt))                                  # the losses stay on the identity pass
    cp, ct = plain.compute(), tta.compute()
    assert sorted(cp) == sorted(ct) and any(k.startswith("val_epoch/mask_map_iou50_95_") for k in ct)
    # by hand: the two passes, the fusion with membership, the vote, the packed ground truth, the metric
    det, seg_out, _ = tta.forward(imgs)
    d = pp.decode_boxes(det, MS, reg_max=tta.reg_max, want_scores=False)
    k0 = pp.nms_batched(d["boxes"], d["best_score"], d["best_label"], float(MS), **tta.nms_kw)
    with torch.no_grad():
        out1 = model(pp.orient_batch(imgs, 1), "infer")
    d1 = pp.decode_boxes(out1["detect_features"], MS, reg_max=tta.reg_max, want_scores=False)
    k1 = pp.nms_batched(d1["boxes"], d1["best_score"], d1["best_label"], float(MS), **tta.nms_kw)
    fused = pp.fuse_detections([k0, k1], img_size=MS, orients=views, iou_thr=0.55, top_k=tta.nms_kw["top_k"], want_members=True)
    r = pp.vote_masks(fused, [(seg_out[1], seg_out[2]), tuple(out1["segment_protos"][1:3])], views, None, [(MS, MS, 1.0)] * MB, crop=True,
                      up=MS / seg_out[2].shape[3])
    rows = det_gt.to(torch.float32)
    gt_image = rows[:, 0].to(torch.int32)
    cx, cy, w, h = rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5]
    px = torch.stack([(cx - w / 2) * MS, (cy - h / 2) * MS, (cx + w / 2) * MS, (cy + h / 2) * MS], 1).clamp_(0, MS)
    gt = pp.pack_masks(masks_gt[:, 0], boxes=px, plane_of=gt_image)
    for prefix, thr in (("val_epoch/mask_map_iou50", [0.5]), ("val_epoch/mask_map_iou50_95", None)):
        m = DeviceMaskMeanAveragePrecision(thr, (1, 10, 100))
        m.update_batched({"masks_frame": r["masks"], "scores": fused["scores"], "labels": fused["labels"], "counts": fused["counts"]},
                         [gt[gt_image == b] for b in range(MB)], [rows[gt_image == b, 1] for b in range(MB)])
        for key, v in m.compute().items():
            got = ct[f"{prefix}_{key}"]
            assert np.array_equal(np.asarray(got), np.asarray(v), equal_nan=True), (prefix, key, got, v)
    with pytest.raises(NotImplementedError, match="detect_fused"):
        ValidationStep(model, projector=proj, img_size=MS, views=views, instance_masks=True)
    with pytest.raises(ValueError):
        ValidationStep(model, projector=proj, img_size=MS, instance_masks=True, fused_masks="vote")
    with pytest.raises(ValueError):
        ValidationStep(model, projector=proj, img_size=MS, views=views, instance_masks=True, fused_masks="leader")
