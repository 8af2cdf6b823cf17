"""GPU parity of sliced inference (`preprocess.slice_batch`, `postprocess.merge_tiles`, `postprocess.vote_tile_masks`, `detect_sliced`)
against its CPU restatement (tests/slice_reference.py) on the shapes of tests/test_cpu_slice.py: S = 160, G = 40, K = 21, images of
300 x 410, 410 x 300 (3 x 3 tiles plus the full view), 97 x 120 (one tile) and 170 x 260 (five tiles, all empty).

The merge outputs, W and Ss are compared bit for bit.  Mask bits may differ from the reference only where the reference's |summed logit|
< 1e-4 * (tiles added at the pixel): the per-source band of test_gpu_mask_vote.py, one fp32 MFMA-versus-einsum rounding difference per
added tap.  The share of such pixels among the voted pixels of the live planes is capped per case at SHARE = 8e-4, that file's cap; the
reference alone (tests/test_cpu_slice.py::test_reference_share_of_in_band_pixels prints them) gives 1.2e-4, 7.2e-5, 1.4e-4 and 1.2e-4 for
the four BIT_CASES at this seed."""
import functools

import numpy as np
import pytest
import torch

import augment_reference as AR
import frame_reference as FR
import slice_reference as SR
from test_cpu_slice import A, BAND, BIT_CASES, EMPTY, K, MERGE_CASES, S, SEED, SHARE, SIZES, UP, inputs, merged_case, tiles_of

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import (ConvNeXtBiFPNYOLO, DeviceMaskMeanAveragePrecision, calibrate_synthetic_heads_, detect_sliced,
                                              init_synthetic_, synthetic_images)
    from multitask_bonetumor_yolo_amd import postprocess as pp
    from multitask_bonetumor_yolo_amd import preprocess as pre

DEV = "cuda:0"
MERGE_KEYS = ("boxes_frame", "scores", "labels", "counts", "n_members", "lead_tile", "lead_slot", "lead_anchor", "member_slot", "n_left")


@functools.lru_cache(maxsize=None)
def _reference(case):
    tiles, det, mc, protos, merged = merged_case(case)
    W, Ss = SR.vote_coefficients(det, mc, merged, tiles, MERGE_CASES[case][3])
    return tiles, det, mc, protos, merged, W, Ss


@functools.lru_cache(maxsize=None)
def _reference_bits(case, crop):
    tiles, det, mc, protos, merged, W, Ss = _reference(case)
    return SR.vote_reference(W, merged, protos, tiles, crop)


def _dev(det):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in det.items()}


def _frames(sizes):
    return [(H0, W0, S / max(H0, W0)) for H0, W0 in sizes]


def _merge(case, det=None, tiles=None, sizes=SIZES):
    metric, thr, skip, top_k, agnostic = MERGE_CASES[case]
    if det is None:
        tiles, det = _reference(case)[:2]
    return pp.merge_tiles(_dev(det), tiles, _frames(sizes), metric=metric, thr=thr, skip_thr=skip, top_k=top_k, class_agnostic=agnostic)


def _assert_merge_equal(got, want):
    for k in MERGE_KEYS:
        w = torch.from_numpy(np.asarray(want[k]))
        assert got[k].dtype == w.dtype and tuple(got[k].shape) == tuple(w.shape), k
        g = got[k].cpu()
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w), k


def _total_bytes(sizes, planes):
    return sum((planes * H0 * FR.pitch_of(W0) + 15) // 16 * 16 for H0, W0 in sizes)


def test_slice_batch_is_the_augmentation_of_each_tiles_row():
    rng = np.random.default_rng(1)
    sizes = [(230, 310), (97, 120)]
    imgs = [rng.integers(0, 256, size=(H0, W0, 3), dtype=np.uint8) for H0, W0 in sizes]
    tiles = pre.slice_geometry(sizes, S, zoom=0.9)
    assert [len(per) for per in tiles] == [5, 1]
    x = pre.slice_batch([torch.from_numpy(im).to(DEV) for im in imgs], tiles, S)
    torch.cuda.synchronize()
    assert x.dtype == torch.float32 and tuple(x.shape) == (6, 3, S, S)
    for i, t in enumerate(t for per in tiles for t in per):
        want, _ = AR.augment(imgs[t["image"]], None, t["geom"], S)
        assert torch.equal(x[i].cpu(), torch.from_numpy(want)), i


@pytest.mark.parametrize("case", range(len(MERGE_CASES)))
def test_merge_is_bit_equal(case):
    want = _reference(case)[4]
    got = _merge(case)
    torch.cuda.synchronize()
    _assert_merge_equal(got, want)
    assert got["boxes"] is got["boxes_frame"] and (want["n_members"] >= 2).any() and int(want["counts"][3]) == 0
    if case in (1, 3, 4):
        assert (want["n_left"] > 0).any()


def test_merge_with_more_candidates_than_threads():
    """10 tiles of K = 128: 1280 slots and 2048 keys against the kernel's 256 threads, so its strided loops, its sort above 512 keys
    and its LDS layout at a large Cmax run (the cases above have 210 slots).  400 objects per image; once uncut, once cut at 16 rows."""
    tiles = tiles_of()
    det = SR.tile_lists(tiles, 128, SEED, S, A=A, n_obj=400, empty=EMPTY)[0]
    listed = [int((det["scores"][t0:t0 + 10] > 0).sum()) for t0 in (0, 10)]
    assert max(listed) > 1024, listed
    d = _dev(det)
    for top_k in (100, 16):
        want = SR.merge_tiles(det, tiles, "ios", 0.5, 0.0, top_k, False)
        got = pp.merge_tiles(d, tiles, _frames(SIZES), metric="ios", thr=0.5, skip_thr=0.0, top_k=top_k, class_agnostic=False)
        torch.cuda.synchronize()
        _assert_merge_equal(got, want)
        assert (want["n_left"] > 0).any() == (top_k == 16), (top_k, want["n_left"])


@pytest.mark.parametrize("case", range(len(MERGE_CASES)))
def test_vote_coefficients_are_bit_equal(case):
    tiles, det, mc, protos, merged, W, Ss = _reference(case)
    d = _dev(det)
    r = pp.vote_tile_masks(_merge(case), d, mc.to(DEV), protos.to(DEV), tiles, _frames(SIZES))
    torch.cuda.synchronize()
    assert r["vote_coeff"].dtype == torch.float32 and tuple(r["vote_coeff"].shape) == tuple(W.shape) and W.shape[2] == 10
    assert torch.equal(r["vote_weight"].cpu().view(torch.int32), torch.from_numpy(Ss).view(torch.int32))
    assert torch.equal(r["vote_coeff"].cpu().view(torch.int32), torch.from_numpy(W).view(torch.int32))
    assert (W != 0).any() and all(not W[n, int(merged["counts"][n]):].any() for n in range(len(tiles)))


@pytest.mark.parametrize("which", range(len(BIT_CASES)))
def test_bits_against_the_cpu_reference(which):
    case, crop = BIT_CASES[which]
    top_k = MERGE_CASES[case][3]
    tiles, det, mc, protos, merged, W, Ss = _reference(case)
    ref = _reference_bits(case, crop)
    buf = torch.full((_total_bytes(SIZES, top_k),), 0xAA, dtype=torch.uint8, device=DEV)       # the kernel must write every byte
    r = pp.vote_tile_masks(_merge(case), _dev(det), mc.to(DEV), protos.to(DEV).contiguous(memory_format=torch.channels_last), tiles,
                           _frames(SIZES), crop=crop, out=buf)
    torch.cuda.synchronize()
    assert r["buffer"].data_ptr() == buf.data_ptr()
    assert torch.equal(r["boxes"].cpu().view(torch.int32), torch.from_numpy(merged["boxes_frame"]).view(torch.int32))
    amb = tot = bits = 0
    for n, (H0, W0) in enumerate(SIZES):
        cnt = int(merged["counts"][n])
        packed = r["masks"][n]
        assert packed.dtype == torch.uint8 and tuple(packed.shape) == (top_k, H0, FR.pitch_of(W0))
        allbits = FR.unpack_bits(packed, W0)
        got = allbits[:, :, :W0]
        assert not allbits[:, :, W0:].any(), "padding bits"
        assert not got[cnt:].any(), "planes r >= counts"
        voted = ref[n]["contrib"] > 0
        near = (ref[n]["logits"].abs() < BAND * ref[n]["contrib"]) & voted
        diff = got != ref[n]["bits"]
        print(f"case {case} crop={crop} image {n} {H0}x{W0}: differing bits {int(diff.sum())}, in-band pixels {int(near.sum())} of {int(voted.sum())}")
        assert not (diff & ~near).any(), "bits differ outside the sign-ambiguous band"
        assert not (got & ~voted).any(), "a bit where no member tile sees the pixel"
        if crop:
            assert not (got & ~ref[n]["region"]).any(), "bit set outside the merged box"
        amb += int(near.sum())
        tot += int(voted.sum())
        bits += int(got.sum())
    assert bits > 1000 and amb <= SHARE * max(tot, 1), (bits, amb, tot)
    assert int(ref[0]["contrib"].max()) >= 3, "some pixel is voted by two windows and the full view"


def test_single_full_view_tile_is_masks_to_frames():
    """One tile per image at S / max(H0, W0), no matches (thr = +inf): the frame operator, boxes bit for bit, planes outside the band."""
    sizes = SIZES[:3]
    tiles = [pre.slice_geometry([sz], S, zoom=S / max(sz), full_view=False)[0] for sz in sizes]
    for n, per in enumerate(tiles):
        per[0]["image"] = n
    det, mc, protos = SR.tile_lists(tiles, K, SEED, S, A=A)
    d, frames = _dev(det), _frames(sizes)
    mcd, prd = mc.to(DEV), protos.to(DEV).contiguous(memory_format=torch.channels_last)
    merged = pp.merge_tiles(d, tiles, frames, thr=float("inf"), top_k=K)
    one = pp.masks_to_frames(prd, mcd, d["keep_anchor"].clamp(min=0), d["counts"], d["boxes"], frames, up=float(UP), crop=True)
    assert torch.equal(merged["boxes_frame"].view(torch.int32), one["boxes"].view(torch.int32))
    assert torch.equal(merged["counts"], d["counts"]) and int(merged["n_members"].max()) == 1 and int(merged["n_left"].max()) == 0
    outs = []
    for fill in (0xAA, 0x55):
        buf = torch.full((_total_bytes(sizes, K),), fill, dtype=torch.uint8, device=DEV)
        outs.append(pp.vote_tile_masks(merged, d, mcd, prd, tiles, frames, crop=True, out=buf))
    torch.cuda.synchronize()
    assert torch.equal(outs[0]["buffer"], outs[1]["buffer"]), "a byte of the output was not written"
    ref = FR.frame_reference(protos, mc, torch.from_numpy(det["keep_anchor"]).clamp(min=0), det["counts"], torch.from_numpy(det["boxes"]), frames,
                             float(UP), crop=True)
    for n, (H0, W0) in enumerate(sizes):
        allbits = FR.unpack_bits(outs[0]["masks"][n], W0)
        assert not allbits[:, :, W0:].any(), "padding bits"
        diff = (pp.unpack_masks(outs[0]["masks"][n], W0) != pp.unpack_masks(one["masks"][n], W0)).cpu()
        print(f"image {n}: {int(diff.sum())} bits differ from masks_to_frames")
        assert not (diff & ~(ref[n]["logits"].abs() < BAND)).any()
        assert allbits.any()


# ---- more images than one launch takes (32 frames): the chunks of `vote_tile_masks` -------------------------------------------------
CH_N, CH_S, CH_K = 33, 64, 5                                          # G = 16
CH_SIZES = ([(40, 50), (70, 100)] * 17)[:CH_N]                        # one tile; 2 x 2 tiles plus the full view


@functools.lru_cache(maxsize=None)
def _chunk_inputs():
    tiles = pre.slice_geometry(CH_SIZES, CH_S)
    assert [len(per) for per in tiles[:2]] == [1, 5]
    return (tiles,) + SR.tile_lists(tiles, CH_K, SEED, CH_S, A=A, empty=(4,))


def _chunk_call(lo, hi, crop):
    """The public calls on images lo .. hi - 1 alone: their tiles renumbered from image 0, the merge, then the vote into a buffer
    pre-filled with 0xFF."""
    tiles, det, mc, protos = _chunk_inputs()
    t0, t1 = sum(len(per) for per in tiles[:lo]), sum(len(per) for per in tiles[:hi])
    sub = [[dict(t, image=n) for t in per] for n, per in enumerate(tiles[lo:hi])]
    d = _dev({k: v[t0:t1] for k, v in det.items()})
    sizes = CH_SIZES[lo:hi]
    frames = [(H0, W0, CH_S / max(H0, W0)) for H0, W0 in sizes]
    merged = pp.merge_tiles(d, sub, frames, top_k=CH_K)
    buf = torch.full((_total_bytes(sizes, CH_K),), 0xFF, dtype=torch.uint8, device=DEV)
    r = pp.vote_tile_masks(merged, d, mc[t0:t1].to(DEV), protos[t0:t1].to(DEV).contiguous(memory_format=torch.channels_last), sub, frames,
                           crop=crop, out=buf)
    assert r["buffer"].data_ptr() == buf.data_ptr()
    return r


@pytest.mark.parametrize("crop", [False, True])
def test_more_than_32_images_are_chunked(crop):
    """33 images of 40 x 50 (one tile) and 70 x 100 (five) in turn at S = 64, K = 5: the second launch (image 32 alone, whose tile is
    number 96 of the table) writes what a call on that image alone writes, byte for byte, and its planes are the CPU restatement's
    outside BAND * (tiles added)."""
    last = CH_N - 1
    whole, head, tail = _chunk_call(0, CH_N, crop), _chunk_call(0, last, crop), _chunk_call(last, CH_N, crop)
    torch.cuda.synchronize()
    at = head["buffer"].numel()                                      # image 32's planes start where 32 images end (16-byte aligned)
    assert whole["buffer"].numel() == at + tail["buffer"].numel()
    assert torch.equal(whole["buffer"][:at], head["buffer"]) and torch.equal(whole["buffer"][at:], tail["buffer"])
    for k in ("boxes", "vote_weight"):
        assert torch.equal(whole[k][:last].view(torch.int32), head[k].view(torch.int32)), k
        assert torch.equal(whole[k][last:].view(torch.int32), tail[k].view(torch.int32)), k
    W, tmax = whole["vote_coeff"].view(torch.int32), tail["vote_coeff"].shape[2]   # W's third dimension is the batch's largest tile count
    assert tuple(W.shape) == (CH_N, CH_K, 5, 32) and tmax == 1
    assert torch.equal(W[:last], head["vote_coeff"].view(torch.int32))
    assert torch.equal(W[last:, :, :tmax], tail["vote_coeff"].view(torch.int32)) and not W[last:, :, tmax:].any()
    # image 32 against the CPU
    tiles, det, mc, protos = _chunk_inputs()
    t0 = sum(len(per) for per in tiles[:last])
    assert t0 == 96 and len(tiles[last]) == 1
    d1, per = {k: v[t0:] for k, v in det.items()}, [tiles[last]]
    merged = SR.merge_tiles(d1, per, top_k=CH_K)
    Wr, _ = SR.vote_coefficients(d1, mc[t0:], merged, per, CH_K)
    ref = SR.vote_reference(Wr, merged, protos[t0:], per, crop)[0]
    H0, W0 = CH_SIZES[last]
    cnt = int(merged["counts"][0])
    packed = whole["masks"][last]
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (CH_K, H0, FR.pitch_of(W0))
    allbits = FR.unpack_bits(packed, W0)
    got = allbits[:, :, :W0]
    assert not allbits[:, :, W0:].any(), "padding bits"
    assert 0 < cnt and not got[cnt:].any(), "planes r >= counts"
    voted = ref["contrib"] > 0
    near = (ref["logits"].abs() < BAND * ref["contrib"]) & voted
    diff = got != ref["bits"]
    print(f"crop={crop} image {last} {H0}x{W0}: differing bits {int(diff.sum())}, in-band pixels {int(near.sum())} of {int(voted.sum())}")
    assert not (diff & ~near).any(), "bits differ outside the sign-ambiguous band"
    assert got.any() and not (got & ~voted).any()
    assert torch.equal(whole["boxes"][last].cpu().view(torch.int32), torch.from_numpy(merged["boxes_frame"][0]).view(torch.int32))
    assert not whole["masks"][4].any(), "an image without detections has zero planes"


# ---- the public route on the synthetic model of the vote tests ---------------------------------------------------------------------
MS, TILE_K, TOP = 128, 50, 60


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), seed=0).to(DEV).eval()
    return calibrate_synthetic_heads_(m, synthetic_images(3, MS, seed=5).to(DEV))


def _raw_images():
    x = synthetic_images(2, 260, seed=7)
    crops = [x[0, :, :200, :260], x[1, :, :260, :190]]
    return [(c.flip(0).permute(1, 2, 0) * 255).to(torch.uint8).contiguous().to(DEV) for c in crops]          # BGR uint8 [H0, W0, 3]


def test_detect_sliced_is_the_composition(model):
    raw = _raw_images()
    kw = dict(batch=8, tile_top_k=TILE_K, top_k=TOP)
    plain = detect_sliced(model, raw, MS, **kw)
    vote = detect_sliced(model, raw, MS, masks="vote", crop=True, **kw)
    # by hand
    sizes = [(200, 260), (260, 190)]
    tiles = pre.slice_geometry(sizes, MS)
    assert [len(per) for per in tiles] == [7, 7]
    x = pre.slice_batch(raw, tiles, MS)
    dets, mcs, prs = [], [], []
    with torch.no_grad():
        for c0 in range(0, 14, 8):
            out = model(x[c0:c0 + 8], "infer")
            _, mc, pr = out["segment_protos"]
            dets.append(pp.detect_and_segment(out["detect_features"], mc, pr, MS, top_k=TILE_K, masks=False))
            mcs.append(mc.float())
            prs.append(pr.float())
    det = {k: torch.cat([d[k] for d in dets]) for k in ("boxes", "scores", "labels", "counts", "keep_anchor")}
    frames = [(H0, W0, MS / max(H0, W0)) for H0, W0 in sizes]
    merged = pp.merge_tiles(det, tiles, frames, top_k=TOP)
    r = pp.vote_tile_masks(merged, det, torch.cat(mcs), torch.cat(prs), tiles, frames, crop=True)
    torch.cuda.synchronize()
    assert sorted(k for k in vote if k != "_keep") == sorted([k for k in plain if k != "_keep"] + ["masks_frame", "vote_coeff"])
    for k in MERGE_KEYS + ("boxes",):
        assert torch.equal(plain[k], merged[k]) and torch.equal(vote[k], merged[k]), k
    assert vote["tiles"] == tiles and torch.equal(vote["vote_coeff"], r["vote_coeff"])
    for n, (H0, W0) in enumerate(sizes):
        assert vote["masks_frame"][n].dtype == torch.uint8 and tuple(vote["masks_frame"][n].shape) == (TOP, H0, FR.pitch_of(W0))
        assert torch.equal(vote["masks_frame"][n], r["masks"][n])
    assert int(vote["counts"].max()) > 0 and int(vote["n_members"].max()) >= 2 and any(m.any() for m in vote["masks_frame"])
    # the result feeds the mask mAP as it is
    g = torch.Generator().manual_seed(0)
    gt = [pp.pack_masks((torch.rand(2, H0, W0, generator=g) > 0.6).to(DEV)) for H0, W0 in sizes]
    metric = DeviceMaskMeanAveragePrecision([0.5], (1, 10, 100))
    metric.update_batched(vote, gt, [torch.tensor([0, 1], device=DEV)] * 2)
    res = metric.compute()
    assert len(res) > 0
    with pytest.raises(ValueError):
        detect_sliced(model, raw, MS, masks=True)
    with pytest.raises(ValueError):
        detect_sliced(model, raw, MS, crop=True)


def test_detect_sliced_full_view_alone_is_detect_and_segment(model):
    """zoom = S / max(H0, W0) on one image and no matches: the plain letterbox pass, boxes bit for bit."""
    raw = _raw_images()[:1]
    sl = detect_sliced(model, raw, MS, zoom=MS / 260, thr=float("inf"), tile_top_k=TILE_K, top_k=TILE_K)
    imgs, _, scales = pre.letterbox_batch(raw, None, MS)
    with torch.no_grad():
        out = model(imgs, "infer")
    _, mc, pr = out["segment_protos"]
    want = pp.detect_and_segment(out["detect_features"], mc, pr, MS, top_k=TILE_K, frames=pp.frames_of(raw, scales), crop=True)
    torch.cuda.synchronize()
    assert len(sl["tiles"][0]) == 1 and int(want["counts"][0]) > 0
    assert torch.equal(sl["boxes_frame"].view(torch.int32), want["boxes_frame"].view(torch.int32))
    assert torch.equal(sl["scores"], want["scores"]) and torch.equal(sl["labels"], want["labels"]) and torch.equal(sl["counts"], want["counts"])
