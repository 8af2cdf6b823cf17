"""The semantic mask in the image frame on the device (`postprocess.seg_to_frames`, `mtbt_seg_to_frames`): both launches bit for bit
against tests/seg_frame_reference.py (a serial fp32 order: no sign-ambiguity band), the layout contract of the packed planes and the
dense logits, and the three places the operator is wired into.  S = 160, G = 40."""
import copy
import functools

import numpy as np
import pytest
import torch

import seg_frame_reference as SG
from test_cpu_slice import BAND, SHARE, SIZES

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import (ConvNeXtBiFPNYOLO, SegmentationMetrics, SurfaceDistanceMetrics, ValidationStep,
                                              calibrate_synthetic_heads_, detect_fused, detect_sliced, init_synthetic_, seg_to_frames,
                                              synthetic_images)
    from multitask_bonetumor_yolo_amd import postprocess as pp
    from multitask_bonetumor_yolo_amd import preprocess as pre

DEV = "cuda:0"
S, G = 160, 40
SEED = 11


def _frames(sizes):
    return [(H0, W0, S / max(H0, W0)) for H0, W0 in sizes]


def _run(passes, projs, frames, orients, weights, tiles=None, blend="constant", threshold=0.0, protos_dev=None, **kw):
    """`seg_to_frames` on numpy inputs with the packed buffer pre-filled with 0xAA and the logits with NaN -> its result."""
    n = sum(fr[0] * 8 * ((fr[1] + 63) // 64) + 16 for fr in frames)
    out = torch.full((n,), 0xAA, dtype=torch.uint8, device=DEV)
    lg = torch.full((sum(fr[0] * fr[1] + 4 for fr in frames),), float("nan"), dtype=torch.float32, device=DEV)
    protos = protos_dev if protos_dev is not None else [torch.from_numpy(P).to(DEV) for P in passes]
    pj = [(torch.from_numpy(q[:32]).to(DEV), torch.from_numpy(q[32:]).to(DEV)) for q in projs]
    r = seg_to_frames(protos, pj, frames, orients=orients, weights=weights, tiles=tiles, blend=blend, threshold=threshold, logits=lg, out=out, **kw)
    torch.cuda.synchronize()
    return r


def _check(r, ref, frames, what=""):
    """Bits and logits bit-equal to the restatement; padding bits zero; every byte and element written (none keeps its pre-fill)."""
    for n, ((H0, W0, _), want) in enumerate(zip(frames, ref)):
        got = r["masks"][n].cpu().numpy()
        assert got.shape == (1, H0, 8 * ((W0 + 63) // 64))
        assert np.array_equal(got[0], SG.pack(want["bits"])), (what, n, "bits")
        lg = r["logits"][n].cpu().numpy()
        assert lg.shape == (H0, W0) and not np.isnan(lg).any(), (what, n, "an element was not written")
        assert np.array_equal(lg.view(np.int32), want["logits"].view(np.int32)), (what, n, "logits", np.abs(lg - want["logits"]).max())
        assert not lg[want["den"] == 0].any() and not want["bits"][want["den"] == 0].any()


@functools.lru_cache(maxsize=None)
def _sliced_inputs():
    tiles = pre.slice_geometry(SIZES, S)
    assert [len(per) for per in tiles] == [10, 10, 1, 5]
    P, q = SG.inputs(SEED, (26, 32, G, G))
    return tiles, P, q


# ---- launch 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,g", [(26, 40), (1, 40), (3, 37)])
def test_projector_logits_are_bit_equal(nt, g):
    s = 4 * g
    P, q = SG.inputs(SEED + nt, (nt, 32, g, g))
    frames = [(s, s, 1.0)] * nt
    r = _run([P], [q], frames, (0,), None, want_low=True)
    ref, low = SG.seg_reference([P], [q], frames, [0], [1.0])
    got = r["low"].cpu().numpy()
    assert got.shape == (nt, g, g)
    assert np.array_equal(got.view(np.int32), np.stack(low).view(np.int32))
    _check(r, ref, frames)


# ---- launch 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.0, 0.7])
@pytest.mark.parametrize("blend", ["gaussian", "tent", "constant"])
def test_tiles_plus_full_view_are_bit_equal(blend, threshold):
    """(a) 300 x 410 and 410 x 300 with 3 x 3 tiles plus the full view, 97 x 120 with one tile, 170 x 260 with five."""
    tiles, P, q = _sliced_inputs()
    frames = _frames(SIZES)
    r = _run([P], [q], frames, (0,), None, tiles=tiles, blend=blend, threshold=threshold)
    ref, _ = SG.seg_reference([P], [q], frames, [0], [1.0], tiles=tiles, tab=pp.seg_blend_table(blend, G), threshold=threshold)
    _check(r, ref, frames, (blend, threshold))
    assert any(w["bits"].any() for w in ref) and not all(w["bits"].all() for w in ref)


def test_eight_views_two_projectors_are_bit_equal():
    """(b) orients 0..7, weights 1..8, two projectors; frames that hit word boundaries, a single-bit last word, a short side equal to G."""
    sizes = [(193, 40), (40, 129), (160, 160), (64, 65)]
    frames = _frames(sizes)
    rng = np.random.default_rng(SEED + 3)
    passes = [rng.standard_normal((4, 32, G, G)).astype(np.float32) for _ in range(8)]
    two = [rng.standard_normal(33).astype(np.float32) for _ in range(2)]
    projs = [two[m & 1] for m in range(8)]
    orients, weights = list(range(8)), [float(m + 1) for m in range(8)]
    r = _run(passes, projs, frames, orients, weights, threshold=0.25)
    ref, _ = SG.seg_reference(passes, projs, frames, orients, weights, threshold=0.25)
    _check(r, ref, frames)


def test_sliced_plus_tta_is_bit_equal():
    """(c) two passes x ten tiles with orients (0, 1): 20 sources."""
    tiles = pre.slice_geometry([(300, 410)], S)
    frames = _frames([(300, 410)])
    rng = np.random.default_rng(SEED + 4)
    passes = [rng.standard_normal((10, 32, G, G)).astype(np.float32) for _ in range(2)]
    projs = [rng.standard_normal(33).astype(np.float32)] * 2
    r = _run(passes, projs, frames, (0, 1), (1.0, 0.5), tiles=tiles, blend="gaussian")
    ref, _ = SG.seg_reference(passes, projs, frames, [0, 1], [1.0, 0.5], tiles=tiles, tab=pp.seg_blend_table("gaussian", G))
    _check(r, ref, frames)


def test_sixty_four_sources_and_unseen_pixels_are_bit_equal():
    """(d) exactly 64 sources on one image: eight passes over eight of the ten tiles.  The two tiles left out leave pixels that no
    source sees: logit 0, bit 0."""
    tiles = [pre.slice_geometry([(300, 410)], S)[0][:8]]
    frames = _frames([(300, 410)])
    rng = np.random.default_rng(SEED + 5)
    passes = [rng.standard_normal((8, 32, G, G)).astype(np.float32) for _ in range(8)]
    projs = [rng.standard_normal(33).astype(np.float32)] * 8
    orients = [3, 0, 5, 6, 1, 7, 2, 4]
    r = _run(passes, projs, frames, orients, None, tiles=tiles, blend="tent", threshold=-0.5)
    ref, _ = SG.seg_reference(passes, projs, frames, orients, [1.0] * 8, tiles=tiles, tab=pp.seg_blend_table("tent", G), threshold=-0.5)
    assert (ref[0]["den"] == 0).any()
    _check(r, ref, frames)


def test_thirty_three_images_take_two_launches():
    """(e) one more image than a launch holds."""
    sizes = [(41 + 3 * n, 200 - 4 * n) for n in range(33)]
    frames = _frames(sizes)
    P, q = SG.inputs(SEED + 6, (33, 32, G, G))
    r = _run([P], [q], frames, (2,), (3.0,))
    ref, _ = SG.seg_reference([P], [q], frames, [2], [3.0])
    _check(r, ref, frames)


def test_any_memory_format_gives_the_same_bytes():
    tiles, P, q = _sliced_inputs()
    frames = _frames(SIZES)
    base = _run([P], [q], frames, (0,), None, tiles=tiles, blend="gaussian")
    t = torch.from_numpy(P).to(DEV)
    wide = torch.zeros((26, 48, G, G), device=DEV).contiguous(memory_format=torch.channels_last)
    wide[:, 8:40] = t
    for other in (t.contiguous(memory_format=torch.channels_last), wide[:, 8:40], t.double()):
        r = _run(None, [q], frames, (0,), None, tiles=tiles, blend="gaussian", protos_dev=[other])
        assert torch.equal(r["buffer"], base["buffer"]) and torch.equal(r["logits_buffer"].view(torch.int32), base["logits_buffer"].view(torch.int32))


def test_one_source_agrees_with_proto_projector_logits():
    """At identity frames and one source the operator is the trainer's projector path: the bits are `proto_projector_logits > 0` except
    where the restatement's |logit| < BAND (the existing operator sums in the MFMA's order)."""
    P, q = SG.inputs(SEED, (3, 32, G, G))
    frames = [(S, S, 1.0)] * 3
    r = _run([P], [q], frames, (0,), None)
    ref, _ = SG.seg_reference([P], [q], frames, [0], [1.0])
    old = pp.proto_projector_logits(torch.from_numpy(P).to(DEV), torch.from_numpy(q[:32]).to(DEV), torch.from_numpy(q[32:]).to(DEV), S)
    want = (old[:, 0] > 0).cpu().numpy()
    v = np.stack([w["logits"] for w in ref])
    band = np.abs(v) < BAND
    got = np.stack([pp.unpack_masks(m, S)[0].cpu().numpy() for m in r["masks"]])
    print(f"in-band share {band.mean():.2e}, differing bits {int((got != want).sum())}")
    assert band.mean() <= SHARE
    assert not ((got != want) & ~band).any()
    assert np.abs(old[:, 0].cpu().numpy() - v).max() <= 1e-5 * np.abs(v).max()


# ---- wiring on a tiny synthetic model ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), seed=0).to(DEV).eval()
    return calibrate_synthetic_heads_(m, synthetic_images(3, S, seed=5).to(DEV))


@pytest.fixture(scope="module")
def projector(model):
    torch.manual_seed(1)
    return torch.nn.Conv2d(model.proto_ch, 1, 1).to(DEV)


def _same(r, masks, logits):
    for a, b in zip(masks, r["masks"]):
        assert a.dtype == torch.uint8 and torch.equal(a, b)
    for a, b in zip(logits, r["logits"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_detect_fused_semantic_is_seg_to_frames(model, projector):
    x = synthetic_images(2, S, seed=9).to(DEV)
    views, weights = (0, 1, 6), (1.0, 2.0)
    other = torch.nn.Conv2d(model.proto_ch, 1, 1).to(DEV)
    plain = detect_fused([model, model], x, S, views=views, weights=weights)
    sem = detect_fused([model, model], x, S, views=views, weights=weights, semantic=[projector, other])
    protos = []
    with torch.no_grad():
        for _ in range(2):
            for v in views:
                protos.append(model(pp.orient_batch(x, v), "infer")["segment_protos"][2])
    pjs = [projector] * 3 + [other] * 3
    r = seg_to_frames(protos, pjs, [(S, S, 1.0)] * 2, orients=views * 2, weights=[1.0] * 3 + [2.0] * 3, logits=True)
    torch.cuda.synchronize()
    assert sorted(k for k in sem if not k.startswith("_")) == sorted([k for k in plain if not k.startswith("_")] + ["seg_frame", "seg_logits"])
    for k in plain:
        if isinstance(plain[k], torch.Tensor):
            assert torch.equal(plain[k], sem[k]), k
    _same(r, sem["seg_frame"], sem["seg_logits"])
    assert tuple(sem["seg_frame"][0].shape) == (1, S, 24) and any(m.any() for m in sem["seg_frame"])
    # in the images' own frames
    frames = [(200, 260, S / 260), (260, 190, S / 260)]
    semf = detect_fused(model, x, S, views=(0, 3), semantic=projector, frames=frames)
    with torch.no_grad():
        p3 = model(pp.orient_batch(x, 3), "infer")["segment_protos"][2]
    rf = seg_to_frames([protos[0], p3], projector, frames, orients=(0, 3), logits=True)
    torch.cuda.synchronize()
    _same(rf, semf["seg_frame"], semf["seg_logits"])
    with pytest.raises(ValueError):
        detect_fused(model, x, S, frames=frames)


def _raw_images():
    x = synthetic_images(2, 260, seed=7)
    crops = [x[0, :, :200, :260], x[1, :, :260, :190]]
    return [(c.flip(0).permute(1, 2, 0) * 255).to(torch.uint8).contiguous().to(DEV) for c in crops]          # BGR uint8 [H0, W0, 3]


def test_detect_sliced_semantic_is_seg_to_frames_and_feeds_the_packed_consumers(model, projector):
    raw = _raw_images()
    sizes = [(200, 260), (260, 190)]
    kw = dict(batch=8, tile_top_k=50, top_k=60)
    plain = detect_sliced(model, raw, S, **kw)
    sem = detect_sliced(model, raw, S, semantic=projector, blend="tent", **kw)
    tiles = pre.slice_geometry(sizes, S)
    x = pre.slice_batch(raw, tiles, S)
    prs = []
    with torch.no_grad():
        for c0 in range(0, x.shape[0], 8):
            prs.append(model(x[c0:c0 + 8], "infer")["segment_protos"][2].float())
    r = seg_to_frames(torch.cat(prs), projector, _frames(sizes), tiles=tiles, blend="tent", logits=True)
    torch.cuda.synchronize()
    assert sorted(k for k in sem if not k.startswith("_")) == sorted([k for k in plain if not k.startswith("_")] + ["seg_frame", "seg_logits"])
    for k in plain:
        if isinstance(plain[k], torch.Tensor):
            assert torch.equal(plain[k], sem[k]), k
    _same(r, sem["seg_frame"], sem["seg_logits"])
    # frame-level counts from the packed planes, against numpy on the unpacked ones
    g = torch.Generator().manual_seed(0)
    gt_bool = [(torch.rand(1, H0, W0, generator=g) > 0.6).to(DEV) for H0, W0 in sizes]
    gt = [pp.pack_masks(t) for t in gt_bool]
    m = SegmentationMetrics(dist_sync=False)
    m.update_packed(sem["seg_frame"], gt, [W0 for _, W0 in sizes])
    counts, score = m.per_image()
    for n, (H0, W0) in enumerate(sizes):
        p, t = pp.unpack_masks(sem["seg_frame"][n], W0)[0].cpu().numpy(), gt_bool[n][0].cpu().numpy()
        assert counts[n].tolist() == [int((p & t).sum()), int((p & ~t).sum()), int((~p & t).sum()), int((~p & ~t).sum())]
    assert counts[:, 0].sum() > 0 and np.allclose(score[counts[:, :2].sum(1) > 0], 1.0)
    assert 0.0 < m.compute()["dice"] < 1.0
    # one tensor for images of one size
    m2 = SegmentationMetrics(dist_sync=False)
    m2.update_packed(torch.stack([sem["seg_frame"][0]] * 2), torch.stack([gt[0]] * 2), 260)
    assert np.array_equal(m2.per_image()[0], np.stack([counts[0]] * 2))
    # the other consumers of packed frame planes take seg_frame as it is
    sd = SurfaceDistanceMetrics(dist_sync=False)
    sd.update_packed(sem["seg_frame"][0], gt[0], 260)
    assert "hd95" in sd.compute()
    lab = pp.label_components(sem["seg_frame"][1], 190)
    torch.cuda.synchronize()
    assert tuple(lab["labels"].shape) == (1, 260, 190)
    assert torch.equal(lab["labels"][0] > 0, pp.unpack_masks(sem["seg_frame"][1], 190)[0])


def _batch(B=2):
    g = torch.Generator().manual_seed(105)
    rows = []
    for b in range(B):
        wh = torch.rand(2, generator=g) * 0.3 + 0.1
        cxy = torch.rand(2, generator=g) * (1 - wh) + wh / 2
        rows.append(torch.cat([torch.tensor([float(b), float(b % 2)]), cxy, wh]))
    masks = (torch.rand(B, 1, S, S, generator=g) > 0.7).float()
    return synthetic_images(B, S, seed=5).to(DEV), torch.stack(rows).to(DEV), masks.to(DEV), torch.randint(0, 2, (B,), generator=g).to(DEV)


def test_validation_step_seg_views_feeds_the_view_averaged_logits(model, projector):
    imgs, det_gt, masks_gt, cls_gt = batch = _batch()
    views = (0, 1)
    tta = ValidationStep(model, projector=projector, img_size=S, views=views, surface=True, lesions=True, dist_sync=False)
    seg = ValidationStep(model, projector=projector, img_size=S, views=views, seg_views=True, surface=True, lesions=True, dist_sync=False)
    # forward(x, "train") moves the heads' running statistics, which the eval-mode view passes read: every route starts from the same state
    state = copy.deepcopy(model.state_dict())
    la = tta.step(*batch)
    model.load_state_dict(state)
    lb = seg.step(*batch)
    model.load_state_dict(state)
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    ca, cb = tta.compute(), seg.compute()
    assert sorted(ca) == sorted(cb)
    # by hand
    _, seg_out, _ = seg.forward(imgs)
    with torch.no_grad():
        p1 = model(pp.orient_batch(imgs, 1), "infer")["segment_protos"][2]
    model.load_state_dict(state)
    r = seg_to_frames([seg_out[2], p1], projector, [(S, S, 1.0)] * 2, orients=views, logits=True)
    logits = torch.stack(r["logits"])[:, None]
    for name, metric, logit in (("tta", tta, pp.proto_projector_logits(seg_out[2], projector.weight, projector.bias, S)), ("seg", seg, logits)):
        m = SegmentationMetrics(dist_sync=False)
        m.update(logit, masks_gt)
        assert np.array_equal(m.per_image()[0], metric.seg.per_image()[0]), name
        sd = SurfaceDistanceMetrics(dist_sync=False)
        sd.update(logit, masks_gt)
        want, got = sd.compute(), metric.surface.compute()
        assert all(np.array_equal(np.asarray(want[k]), np.asarray(got[k]), equal_nan=True) for k in want), name
    # the packed plane is the sign of the same logits
    assert torch.equal(pp.unpack_masks(r["masks"][0], S)[0], r["logits"][0] > 0)
    for k in ca:      # everything but the semantic mask's keys stays on the identity pass / the fused boxes
        if "/seg_" not in k:
            assert np.array_equal(np.asarray(ca[k]), np.asarray(cb[k]), equal_nan=True), k
    with pytest.raises(ValueError, match="seg_views"):
        ValidationStep(model, projector=projector, img_size=S, seg_views=True)
