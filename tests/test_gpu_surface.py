"""The device surface-distance records (`metrics.surface_distances`, csrc/surface_dist.hip) against the brute-force restatement
(tests/surface_reference.py): every integer output bit for bit, `sum_d` to a relative 1e-9 (float64 summation order differs from
numpy's pairwise sum: with n <= 1e5 terms n * eps ~ 1e-11).  Then `SurfaceDistanceMetrics` and `ValidationStep(surface=True)` end to
end.

Shapes: the smallest that reach each path -- a single pixel, a single row, a single column of words, pitches 8, 16 and 24 on both sides
of a 64-bit word boundary -- and one 640 x 640 pair, the realistic row length of the LDS staging.  Contents (`plane_cases`): single
pixels in opposite corners (the longest scan), a full plane (edges = the image border), a plane with a hole, blobs whose nearest edge
lies in another row and column, noise (nearly every pixel an edge), identical planes, A inside B, one side empty, both sides empty."""
import numpy as np
import pytest
import torch

import surface_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (1, 70), (37, 64), (33, 65), (40, 130), (96, 200)]
QUANTILES = (0.0, 0.5, 0.95, 1.0)
TOL2 = 5

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, SurfaceDistanceMetrics, ValidationStep, init_synthetic_, synthetic_images
    from multitask_bonetumor_yolo_amd.metrics import surface_distances
    from multitask_bonetumor_yolo_amd.postprocess import pack_masks, proto_projector_logits


def _device_records(pairs, W, quantiles=QUANTILES, tol2=TOL2, pad_ones=False):
    a = torch.from_numpy(R.pack_bits(np.stack([p[0] for p in pairs]), pad_ones)).to(DEV)
    b = torch.from_numpy(R.pack_bits(np.stack([p[1] for p in pairs]), pad_ones)).to(DEV)
    return surface_distances(a, b, W, quantiles=quantiles, tol2=tol2)


def _assert_records(got, want, what=""):
    for k in ("n_edge", "max_d2", "n_within", "rank_d2"):
        g = got[k].cpu().numpy()
        assert g.dtype == np.int32 and np.array_equal(g.astype(np.int64), want[k]), (what, k, g.tolist(), want[k].tolist())
    s = got["sum_d"].cpu().numpy()
    print(what, "sum_d max relative difference", float(np.max(np.abs(s - want["sum_d"]) / np.maximum(want["sum_d"], 1.0), initial=0.0)))
    assert s.dtype == np.float64 and np.allclose(s, want["sum_d"], rtol=1e-9, atol=0.0), (what, s.tolist(), want["sum_d"].tolist())


@pytest.fixture(scope="module")
def cases():
    """Per shape: (names, pairs, reference records, number of pairs with an empty side), computed once."""
    out = {}
    for i, (H, W) in enumerate(SHAPES):
        cs, n_empty = R.plane_cases(np.random.default_rng(10 + i), H, W)
        pairs = [(a, b) for _, a, b in cs]
        out[(H, W)] = ([c[0] for c in cs], pairs, R.batch_records(pairs, QUANTILES, TOL2), n_empty)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_records_equal_the_restatement(cases, shape):
    names, pairs, want, n_empty = cases[shape]
    got = _device_records(pairs, shape[1])
    assert got["rank_d2"].shape == (len(pairs), 4, 3, 2) and got["shape"] == shape
    _assert_records(got, want, str(shape))
    assert int((want["n_edge"].min(axis=1) == 0).sum()) == n_empty == 3
    # set padding bits X >= W change nothing
    padded = _device_records(pairs, shape[1], pad_ones=True)
    for k in ("n_edge", "max_d2", "n_within", "rank_d2", "sum_d"):
        assert torch.equal(padded[k], got[k]), k


def test_single_pair_no_quantiles_and_empty_batch(cases):
    names, pairs, want, _ = cases[(33, 65)]
    i = names.index("blobs_apart")
    got = _device_records(pairs[i:i + 1], 65, quantiles=(), tol2=TOL2)
    assert got["rank_d2"].shape == (1, 0, 3, 2)
    for k in ("n_edge", "max_d2", "n_within"):
        assert np.array_equal(got[k].cpu().numpy(), want[k][i:i + 1]), k
    one = _device_records(pairs[i:i + 1], 65)
    assert np.array_equal(one["rank_d2"].cpu().numpy(), want["rank_d2"][i:i + 1])
    empty = surface_distances(torch.zeros((0, 33, 16), dtype=torch.uint8, device=DEV), torch.zeros((0, 33, 16), dtype=torch.uint8, device=DEV), 65)
    assert empty["n_edge"].shape == (0, 2) and empty["rank_d2"].shape == (0, 1, 3, 2)


def test_seventy_mixed_pairs_overwrite_prefilled_outputs_and_repeat_bit_for_bit(cases, monkeypatch):
    names, pairs, want, _ = cases[(40, 130)]
    idx = [(7 * i) % len(pairs) for i in range(70)]          # 70 pairs: more than one launch group of 64
    many = [pairs[i] for i in idx]
    real_empty = torch.empty

    def filled(*args, **kw):                                  # every output (and the workspace) starts as 0xFF bytes
        t = real_empty(*args, **kw)
        t.view(torch.uint8).fill_(0xFF)
        return t

    monkeypatch.setattr(torch, "empty", filled)
    first = _device_records(many, 130)
    monkeypatch.undo()
    second = _device_records(many, 130)
    _assert_records(first, {k: v[idx] for k, v in want.items()}, "70 pairs")
    for k in ("n_edge", "max_d2", "n_within", "rank_d2"):
        assert torch.equal(first[k], second[k]), k
    assert torch.equal(first["sum_d"].view(torch.int64), second["sum_d"].view(torch.int64))     # the same bits, sum_d included


def test_blob_pair_at_640():
    rng = np.random.default_rng(5)
    a, b = R.blob(rng, 640, 640, thin=False), R.blob(rng, 640, 640, thin=False)
    a[600:610, 5:9] = True                                     # a detached island far from the blobs
    _assert_records(_device_records([(a, b)], 640), R.batch_records([(a, b)], QUANTILES, TOL2), "640 x 640")


# ---- the metric object ------------------------------------------------------------------------------------------------------------
def _logit_case():
    """logits and masks [3,1,64,64]: a defined pair, a pair whose prediction is empty, a pair of blobs; logits hold exact zeros
    (not set: bit = logit > 0) and the masks hold values below 1 (not set: bit = mask >= 1)."""
    rng = np.random.default_rng(7)
    pred, gt = np.zeros((3, 64, 64), bool), np.zeros((3, 64, 64), bool)
    pred[0, 10:30, 12:40], gt[0, 14:36, 8:33] = True, True
    gt[1, 5:9, 5:9] = True
    pred[2], gt[2] = R.blob(rng, 64, 64), R.blob(rng, 64, 64)
    logits = np.where(pred, rng.uniform(0.1, 3.0, pred.shape), -rng.uniform(0.0, 3.0, pred.shape)).astype(np.float32)
    logits[0, 0, :8] = 0.0
    masks = np.where(gt, 1.0, rng.choice([0.0, 0.5, 0.999], size=gt.shape)).astype(np.float32)
    return pred, gt, torch.from_numpy(logits)[:, None].to(DEV), torch.from_numpy(masks)[:, None].to(DEV)


@pytest.mark.parametrize("mode", ["pooled", "max"])
@pytest.mark.parametrize("undefined", ["skip", "diagonal"])
def test_metric_object_end_to_end(mode, undefined):
    pred, gt, logits, masks = _logit_case()
    kw = dict(quantile=0.95, tolerance=1.5, spacing=0.8, percentile_mode=mode, undefined=undefined)
    m = SurfaceDistanceMetrics(**kw)
    m.update(logits, masks)
    m.update(logits[:2, 0], masks[:2, 0])                      # [B,S,S] too
    per = m.per_image()
    want = [R.metrics(pred[i], gt[i], **kw) for i in (0, 1, 2, 0, 1)]
    assert per["defined"].tolist() == [w["defined"] for w in want] == [True, False, True, True, False]
    for k in ("hd", "hd95", "assd", "nsd"):
        assert np.allclose(per[k], [w[k] for w in want], rtol=1e-9, atol=1e-12, equal_nan=True), (k, per[k])
    got = m.compute()
    assert got["n_pairs"] == 5 and got["n_undefined"] == 2
    for k in ("hd", "hd95", "assd", "nsd"):
        vals = [w[k] for w in want if not np.isnan(w[k])]
        assert len(vals) == (3 if undefined == "skip" else 5) and got[k] == pytest.approx(np.mean(vals), rel=1e-9)
    m.reset()
    assert m.compute()["hd"] == -1.0 and m.compute()["n_pairs"] == 0


def test_update_packed_with_pack_masks_output_and_no_synchronisation():
    rng = np.random.default_rng(8)
    a = np.stack([R.blob(rng, 50, 100) for _ in range(4)])
    b = np.stack([R.blob(rng, 50, 100) for _ in range(4)])
    pa, pb = pack_masks(torch.from_numpy(a).to(DEV)), pack_masks(torch.from_numpy(b).to(DEV))
    m = SurfaceDistanceMetrics(tolerance=3.0)
    m.update_packed(pa, pb, 100)                               # warm-up: the library is loaded
    m.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update_packed(pa, pb, 100)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    per = m.per_image()
    want = [R.metrics(a[i], b[i], tolerance=3.0) for i in range(4)]
    assert per["defined"].all()
    for k in ("hd", "hd95", "assd", "nsd"):
        assert np.allclose(per[k], [w[k] for w in want], rtol=1e-9, atol=1e-12), k
    with pytest.raises(ValueError):
        m.update_packed(pa, pb, 130)                           # pitch 16 is not a width of 130
    with pytest.raises(ValueError):
        m.update_packed(pa, pb[:2], 100)


# ---- ValidationStep(surface=...) --------------------------------------------------------------------------------------------------
KEYS_WITHOUT_SURFACE = (
    [f"val_epoch/loss_{k}" for k in ("total", "seg", "box_iou", "dfl", "det_cls", "img_cls")]
    + ["val_epoch/img_accuracy_epoch", "val_epoch/img_confusion_matrix_epoch", "val_epoch/img_precision_macro", "val_epoch/img_recall_macro",
       "val_epoch/img_f1_macro", "val_epoch/det_confusion_matrix_epoch", "val_epoch_map_iou50/map"]
    + [f"val_epoch/seg_{k}_epoch" for k in ("f1", "precision", "recall", "accuracy", "dice")]
    + [f"val_epoch/{p}_{k}" for p in ("seg_map", "map_iou50", "map_iou50_95")
       for k in ("map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium",
                 "mar_large")])
SURFACE_KEYS = [f"val_epoch/seg_{k}_epoch" for k in ("hd", "hd95", "assd", "nsd")] + ["val_epoch/seg_surface_undefined"]


def test_validation_step_with_surface_metrics():
    torch.manual_seed(0)
    model = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), seed=0).to(DEV)
    proj = torch.nn.Conv2d(model.proto_ch, 1, 1).to(DEV)
    S, Bn = 128, 3
    imgs = synthetic_images(Bn, S, seed=1).to(DEV)
    gt = torch.tensor([[0, 1, 0.4, 0.4, 0.3, 0.3], [2, 0, 0.6, 0.5, 0.2, 0.4]], device=DEV)
    masks = torch.zeros(Bn, 1, S, S, device=DEV)
    masks[0, 0, 30:70, 40:90], masks[2, 0, 60:100, 20:50] = 1.0, 1.0          # image 1: no target, an undefined pair
    cls = torch.tensor([0, 1, 1], device=DEV)
    model.eval()
    with torch.no_grad():                                      # centre the projector: every predicted mask has pixels on both sides of 0
        _, (_, _, protos), _ = model(imgs, "train")
        proj.bias -= proto_projector_logits(protos, proj.weight, proj.bias, S).median()
    off = ValidationStep(model, projector=proj, img_size=S)
    on = ValidationStep(model, projector=proj, img_size=S, surface=dict(tolerance=3.0))
    l_off, l_on = off.step(imgs, gt, masks, cls), on.step(imgs, gt, masks, cls)
    assert all(torch.equal(a, b) for a, b in zip(l_off, l_on))
    r_off, r_on = off.compute(), on.compute()
    assert sorted(r_off) == sorted(KEYS_WITHOUT_SURFACE) and off.surface is None
    assert sorted(r_on) == sorted(KEYS_WITHOUT_SURFACE + SURFACE_KEYS)
    for k in KEYS_WITHOUT_SURFACE:
        assert np.array_equal(np.asarray(r_on[k]), np.asarray(r_off[k])), k

    model.eval()
    with torch.no_grad():
        _, (_, _, protos), _ = model(imgs, "train")
    alone = SurfaceDistanceMetrics(tolerance=3.0)
    alone.update(proto_projector_logits(protos, proj.weight, proj.bias, S), masks)
    want = alone.compute()
    for k in ("hd", "hd95", "assd", "nsd"):
        assert r_on[f"val_epoch/seg_{k}_epoch"] == want[k], k
    print("surface metrics of the step", want)
    assert r_on["val_epoch/seg_surface_undefined"] == want["n_undefined"] == 1 and want["n_pairs"] == Bn and want["hd"] > 0
    on.reset()
    assert on.compute()["val_epoch/seg_hd_epoch"] == -1.0


@pytest.mark.parametrize("shape", [(7, 63), (9, 127)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_padding_bit_in_the_last_word(shape):
    """W % 64 == 63, below and above 64: one padding bit in the last word, where a wrong valid_bits shows: a full plane against noise, noise against noise, and a last column against a first one, padding bits set."""
    H, W = shape
    rng = np.random.default_rng(W)
    noise = lambda: rng.uniform(size=(H, W)) < 0.5
    last, first = np.zeros((H, W), bool), np.zeros((H, W), bool)
    last[:, W - 1] = first[:, 0] = True
    pairs = [(np.ones((H, W), bool), noise()), (noise(), noise()), (last, first)]
    want = R.batch_records(pairs, QUANTILES, TOL2)
    _assert_records(_device_records(pairs, W, pad_ones=True), want, str(shape))
    assert want["max_d2"][2].tolist() == [(W - 1) ** 2] * 2
