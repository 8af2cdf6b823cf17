"""GPU parity of the frame operator (`postprocess.masks_to_frames`: instance masks and boxes in the original image frame, masks one
bit per pixel) against its CPU restatement (tests/frame_reference.py), against the dense mask kernel at identity frames, across the
32-frames-per-launch boundary, and through `detect_and_segment(frames=...)`.

Mask bits may differ from a reference only where that reference's |logit| < 1e-4 (the band `test_mask_assembly_and_projector` uses:
the kernel sums the 32 channels in another order than einsum).  The share of such pixels is capped at 2e-4 per case; the reference
alone gives 1.4e-5 .. 5.6e-5 for these shapes and this seed."""
import pytest
import torch

import frame_reference as FR

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import postprocess as pp

DEV = "cuda:0"
SIZES = [(97, 211), (211, 97), (300, 65), (33, 130), (160, 160), (480, 333), (1, 70)]
# three per call, every size used; counts are [21, 3, 0] by position, so the last two groups bring the sizes that sat in the empty slot to the front
GROUPS = [SIZES[0:3], SIZES[3:6], [SIZES[6], SIZES[0], SIZES[4]], [SIZES[2], SIZES[5], SIZES[1]], [SIZES[5], SIZES[2], SIZES[3]]]
BAND, SHARE = 1e-4, 2e-4


def _inputs(B, hp, wp, K, counts, seed=11, A=300):
    g = torch.Generator().manual_seed(seed)
    protos = torch.randn(B, 32, hp, wp, generator=g)
    mc = torch.randn(B, A, 32, generator=g).permute(0, 2, 1)  # logical [B,nm,A], strided like the model's
    keep_anchor = torch.randint(0, A, (B, K), generator=g, dtype=torch.int32)
    return protos, mc, keep_anchor, torch.tensor(counts, dtype=torch.int32), g


def _boxes(frames, K, g):
    """Letterboxed xyxy boxes inside each image's content: box 0 is the whole content (touches every border), box 1 has zero width,
    box 2 zero height at the bottom border, the rest are random."""
    out = torch.zeros(len(frames), K, 4)
    for b, (H0, W0, scale) in enumerate(frames):
        cw, ch = W0 * scale, H0 * scale
        xy = torch.rand(K, 2, generator=g) * torch.tensor([cw, ch]) * 0.8
        wh = torch.rand(K, 2, generator=g) * torch.tensor([cw, ch]) * 0.6
        bx = torch.cat([xy, torch.minimum(xy + wh, torch.tensor([cw, ch]))], 1)
        bx[0] = torch.tensor([0.0, 0.0, cw, ch])
        if K > 2:
            bx[1, 2] = bx[1, 0]
            bx[2, 1] = bx[2, 3] = ch
        out[b] = bx
    return out


def _total_bytes(frames, K):
    return sum((K * H0 * FR.pitch_of(W0) + 15) // 16 * 16 for H0, W0, _ in frames)


def _run(protos, mc, keep_anchor, counts, boxes, frames, up, crop):
    K = keep_anchor.shape[1]
    buf = torch.full((_total_bytes(frames, K),), 0xFF, dtype=torch.uint8, device=DEV)   # the kernel must write every byte
    r = pp.masks_to_frames(protos.to(DEV).contiguous(memory_format=torch.channels_last), mc.to(DEV), keep_anchor.to(DEV), counts.to(DEV),
                           boxes.to(DEV), frames, up=up, crop=crop, out=buf)
    torch.cuda.synchronize()
    assert r["buffer"].data_ptr() == buf.data_ptr()
    return r


def _check_against_reference(r, ref, frames, counts, crop):
    amb = tot = 0
    for b, (H0, W0, _) in enumerate(frames):
        n = int(counts[b])
        packed = r["masks"][b]
        assert packed.dtype == torch.uint8 and tuple(packed.shape) == (len(ref[b]["bits"]), H0, FR.pitch_of(W0))
        allbits = FR.unpack_bits(packed, W0)
        got = allbits[:, :, :W0]
        assert torch.equal(pp.unpack_masks(packed, W0).cpu(), got)
        assert not allbits[:, :, W0:].any(), "padding bits"
        assert not got[n:].any(), "planes k >= counts"
        near = ref[b]["logits"].abs() < BAND
        diff = got != ref[b]["bits"]
        print(f"image {b} {H0}x{W0} crop={crop}: differing bits {int(diff.sum())}, in-band pixels {int(near[:n].sum())} of {near[:n].numel()}")
        assert not (diff & ~near).any(), "bits differ outside the sign-ambiguous band"
        if crop:
            assert not (got & ~ref[b]["region"]).any(), "bit set outside the box"
        amb += int(near[:n].sum())
        tot += near[:n].numel()
        assert torch.equal(r["boxes"][b].cpu(), ref[b]["boxes"]), "boxes_frame is not bit-equal"
    assert amb <= SHARE * max(tot, 1), (amb, tot)


@pytest.mark.parametrize("crop", [False, True])
@pytest.mark.parametrize("group", range(len(GROUPS)))
def test_parity_with_the_cpu_reference(group, crop):
    S, up, K = 160, 4.0, 21
    counts = [21, 3, 0]
    protos, mc, keep_anchor, cnt, g = _inputs(3, 40, 40, K, counts)
    frames = [(H0, W0, S / max(H0, W0)) for H0, W0 in GROUPS[group]]
    boxes = _boxes(frames, K, g)
    r = _run(protos, mc, keep_anchor, cnt, boxes, frames, up, crop)
    ref = FR.frame_reference(protos, mc, keep_anchor, cnt, boxes, frames, up, crop)
    _check_against_reference(r, ref, frames, cnt, crop)


@pytest.mark.parametrize("hw", [40, 64])
def test_identity_frames_equal_the_dense_kernel(hw):
    """(S, S, 1.0) frames: the same bits as `assemble_masks` (40 x 40: its general kernel; 64 x 64: its x4 MFMA kernel)."""
    S, K = 4 * hw, 21
    protos, mc, keep_anchor, cnt, g = _inputs(2, hw, hw, K, [21, 3])
    frames = [(S, S, 1.0)] * 2
    pd = protos.to(DEV).contiguous(memory_format=torch.channels_last)
    masks, logits = pp.assemble_masks(pd, mc.to(DEV), keep_anchor.to(DEV), cnt.to(DEV), (S, S), want_logits=True)
    r = _run(protos, mc, keep_anchor, cnt, _boxes(frames, K, g), frames, 4.0, False)
    for b in range(2):
        got = pp.unpack_masks(r["masks"][b], S)
        diff = got != masks[b]
        print(f"image {b}: differing bits {int(diff.sum())}")
        assert not (diff & ~(logits[b].abs() < BAND)).any()
        assert not got[int(cnt[b]):].any()


def test_more_than_32_images_are_chunked():
    S, up, K, B = 64, 4.0, 5, 33
    g0 = torch.Generator().manual_seed(3)
    counts = torch.randint(0, K + 1, (B,), generator=g0).tolist()
    protos, mc, keep_anchor, cnt, g = _inputs(B, 16, 16, K, counts, A=50)
    frames = [((20, 30) if b % 2 == 0 else (30, 20)) + (S / 30,) for b in range(B)]
    boxes = _boxes(frames, K, g)
    r = _run(protos, mc, keep_anchor, cnt, boxes, frames, up, True)
    ref = FR.frame_reference(protos, mc, keep_anchor, cnt, boxes, frames, up, True)
    for b in range(B):
        near = ref[b]["logits"].abs() < BAND
        got = FR.unpack_bits(r["masks"][b], frames[b][1])
        assert not got[:, :, frames[b][1]:].any()
        assert not ((got[:, :, :frames[b][1]] != ref[b]["bits"]) & ~near).any(), b
        assert torch.equal(r["boxes"][b].cpu(), ref[b]["boxes"]), b


def test_detect_and_segment_wiring():
    g = torch.Generator().manual_seed(0)
    B, S, nc = 2, 64, 2
    maps = [(torch.randn(B, 64 + nc, h, w, generator=g) * 3.0).to(DEV) for h, w in [(8, 8), (4, 4), (2, 2)]]
    A = 84
    mc = torch.randn(B, A, 32, generator=g).permute(0, 2, 1).to(DEV)
    protos = torch.randn(B, 32, 16, 16, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    frames = [(100, 80, S / 100), (64, 64, 1.0)]
    plain = pp.detect_and_segment(maps, mc, protos, S)
    assert set(plain) == {"boxes", "scores", "labels", "counts", "keep_idx", "keep_anchor", "n_cand", "masks"}
    out = pp.detect_and_segment(maps, mc, protos, S, frames=frames, crop=True)
    assert set(out) == (set(plain) - {"masks"}) | {"boxes_frame", "masks_frame"}
    assert int(out["counts"].sum()) > 0
    for key in ("boxes", "scores", "labels", "counts", "keep_anchor"):
        assert torch.equal(out[key], plain[key])
    r = pp.masks_to_frames(protos, mc, out["keep_anchor"], out["counts"], out["boxes"], frames, up=S / 16, crop=True)
    torch.cuda.synchronize()
    assert torch.equal(out["boxes_frame"], r["boxes"])
    for b, (H0, W0, _) in enumerate(frames):
        assert tuple(out["masks_frame"][b].shape) == (out["keep_anchor"].shape[1], H0, FR.pitch_of(W0))
        assert torch.equal(out["masks_frame"][b], r["masks"][b])
    assert any(bool(m.any()) for m in out["masks_frame"])
    with pytest.raises(ValueError, match="long side"):
        pp.detect_and_segment(maps, mc, protos, S, frames=[(10, 10, 6.4), (64, 64, 1.0)])
