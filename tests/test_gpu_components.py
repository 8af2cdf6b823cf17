"""The device connected-component operators (`postprocess.label_components`, `filter_components`, `components_to_instances`;
csrc/components.hip) against the flood-fill restatement (tests/components_reference.py, held against scipy.ndimage in
tests/test_cpu_components.py): every output is an integer and every comparison is exact.  Then `LesionMetrics` and
`ValidationStep(lesions=True)` end to end.

Shapes: the smallest that reach each path -- a single pixel, a single row, a single column of words, pitches 8, 16 and 24 on both sides
of a 64-bit word boundary -- and one 640 x 640 plane.  Contents (`plane_cases`): empty, full, the four corners, a checkerboard (the most
components a plane can have: over any table cap), a serpentine (one component, the longest chain of links), a U and a comb (arms that
join only in the last row; the comb's detached single pixels are components of equal area), a bar and a diagonal across the word
boundaries 63|64 and 127|128, a diagonal line (W components or one), noise at p = 0.5 and near the percolation threshold."""
import numpy as np
import pytest
import torch

import components_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (1, 70), (37, 64), (33, 65), (40, 130), (96, 200)]
CONNS = (4, 8)
CAP = 1024

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import (ConvNeXtBiFPNYOLO, LesionMetrics, SurfaceDistanceMetrics, ValidationStep, components_to_instances,
                                              filter_components, init_synthetic_, label_components, synthetic_images)
    from multitask_bonetumor_yolo_amd.postprocess import proto_projector_logits, unpack_masks


def _pack(planes, pad_ones=False):
    return torch.from_numpy(R.pack_bits(np.stack(planes), pad_ones)).to(DEV)


def _reference(planes, others, conn, cap=CAP):
    """The records of a list of planes stacked as the device lays them out (+ `areas`: a list of the per-id areas of every plane)."""
    recs = [R.records(m, conn, cap, other=o) for m, o in zip(planes, others)]
    out = {k: np.stack([r[k] for r in recs]) for k in ("labels", "area", "box", "first", "inter")}
    out["n_components"] = np.array([r["n_components"] for r in recs])
    out["areas"] = [r["areas"] for r in recs]
    return out


def _assert_records(got, want, what=""):
    for k, g in (("labels", got["labels"]), ("n_components", got["n_components"]), ("area", got["area"]), ("first", got["first"]),
                 ("inter", got["inter"])):
        g = g.cpu().numpy()
        assert g.dtype == np.int32 and g.shape == want[k].shape and np.array_equal(g, want[k]), (what, k)
    b = got["boxes"].cpu().numpy()
    assert b.dtype == np.float32 and np.array_equal(b, want["box"].astype(np.float32)), (what, "boxes")


def _kept_planes(want, planes, min_area, keep_largest):
    """Dense kept planes and their counts by the select rule, from the reference labels and per-id areas."""
    kept, counts = [], []
    for lab, areas in zip(want["labels"], want["areas"]):
        keep = R.keep_rule(areas, min_area, keep_largest)
        kept.append(np.concatenate([[False], keep])[lab])
        counts.append(int(keep.sum()))
    return np.stack(kept), np.array(counts)


def _assert_filter(packed, W, conn, want, planes, min_area, keep_largest, what=""):
    out, n_kept = filter_components(packed, W, min_area=min_area, keep_largest=keep_largest, connectivity=conn)
    kept, counts = _kept_planes(want, planes, min_area, keep_largest)
    assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), R.pack_bits(kept)), (what, min_area, keep_largest)   # padding zero
    assert n_kept.dtype == torch.int32 and np.array_equal(n_kept.cpu().numpy(), counts), (what, min_area, keep_largest)


@pytest.fixture(scope="module")
def cases():
    """Per shape: (names, planes, second planes, {connectivity: reference records}), computed once."""
    out = {}
    for i, (H, W) in enumerate(SHAPES):
        cs = R.plane_cases(np.random.default_rng(20 + i), H, W)
        rng = np.random.default_rng(40 + i)
        planes = [m for _, m in cs]
        others = [rng.uniform(size=(H, W)) < 0.3 for _ in cs]
        out[(H, W)] = ([n for n, _ in cs], planes, others, {c: _reference(planes, others, c) for c in CONNS})
    return out


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labels_and_records_equal_the_restatement(cases, shape, conn):
    names, planes, others, want = cases[shape]
    got = label_components(_pack(planes), shape[1], connectivity=conn, max_components=CAP, other=_pack(others))
    assert got["shape"] == shape and got["boxes"].shape == (len(planes), CAP, 4)
    _assert_records(got, want[conn], f"{shape} {conn}")
    # set padding bits X >= W change nothing, on either stack
    padded = label_components(_pack(planes, True), shape[1], connectivity=conn, max_components=CAP, other=_pack(others, True))
    for k in ("labels", "n_components", "area", "boxes", "first", "inter"):
        assert torch.equal(padded[k], got[k]), k
    # no second stack, no label map: the other outputs stay
    bare = label_components(_pack(planes), shape[1], connectivity=conn, max_components=CAP, want_labels=False)
    assert bare["labels"] is None and bare["inter"] is None
    for k in ("n_components", "area", "boxes", "first"):
        assert torch.equal(bare[k], got[k]), k


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_keeps_by_area_and_rank_with_ties(cases, shape, conn):
    names, planes, others, want = cases[shape]
    packed = _pack(planes, pad_ones=True)
    for min_area, keep_largest in ((0, None), (2, None), (0, 1), (0, 3), (3, 3), (10 ** 6, None)):
        _assert_filter(packed, shape[1], conn, want[conn], planes, min_area, keep_largest, f"{shape} {conn}")
    if shape[0] >= 3:                                          # the comb's single pixels tie: the lower ids are kept
        i = names.index("comb")
        assert (want[4]["areas"][i][1:] == 1).all() and len(want[4]["areas"][i]) > 3


def test_table_cap_on_the_checkerboard(cases):
    names, planes, others, want = cases[(40, 130)]
    i = names.index("checker")
    packed, other = _pack(planes[i:i + 1]), _pack(others[i:i + 1])
    for conn in CONNS:
        got = label_components(packed, 130, connectivity=conn, max_components=8, other=other)
        capped = _reference(planes[i:i + 1], others[i:i + 1], conn, cap=8)
        _assert_records(got, capped, f"cap 8, {conn}")
        assert got["area"].shape == (1, 8) and int(got["n_components"][0]) == (2600 if conn == 4 else 1)     # the true count
        _assert_filter(packed, 130, conn, capped, planes[i:i + 1], 2, None, "cap 8")                          # exact above the cap too
        _assert_filter(packed, 130, conn, capped, planes[i:i + 1], 0, 1500, "cap 8")
    assert (capped["area"][0] == [2600, 0, 0, 0, 0, 0, 0, 0]).all()


def test_seventy_mixed_planes_overwrite_prefilled_outputs_and_repeat_bit_for_bit(cases, monkeypatch):
    names, planes, others, want = cases[(40, 130)]
    idx = [(7 * i) % len(planes) for i in range(70)]          # 70 planes: more than one launch group of 64
    many, many_o = [planes[i] for i in idx], [others[i] for i in idx]
    packed, other = _pack(many), _pack(many_o)
    real_empty = torch.empty

    def filled(*args, **kw):                                  # every output (and the workspace) starts as 0xFF bytes
        t = real_empty(*args, **kw)
        t.view(torch.uint8).fill_(0xFF)
        return t

    for conn in CONNS:
        w = {k: (v[idx] if k != "areas" else [v[i] for i in idx]) for k, v in want[conn].items()}
        monkeypatch.setattr(torch, "empty", filled)
        first = label_components(packed, 130, connectivity=conn, max_components=CAP, other=other)
        f_out, f_kept = filter_components(packed, 130, min_area=2, keep_largest=3, connectivity=conn)
        monkeypatch.undo()
        second = label_components(packed, 130, connectivity=conn, max_components=CAP, other=other)
        s_out, s_kept = filter_components(packed, 130, min_area=2, keep_largest=3, connectivity=conn)
        _assert_records(first, w, f"70 planes, {conn}")
        for k in ("labels", "n_components", "area", "boxes", "first", "inter"):
            assert torch.equal(first[k], second[k]), k
        kept, counts = _kept_planes(w, many, 2, 3)
        assert np.array_equal(f_out.cpu().numpy(), R.pack_bits(kept)) and np.array_equal(f_kept.cpu().numpy(), counts)
        assert torch.equal(f_out, s_out) and torch.equal(f_kept, s_kept)


def test_empty_batch_and_refusals():
    z = torch.zeros((0, 33, 16), dtype=torch.uint8, device=DEV)
    got = label_components(z, 65, other=z)
    assert got["labels"].shape == (0, 33, 65) and got["area"].shape == (0, 1024) and got["boxes"].shape == (0, 1024, 4)
    assert got["n_components"].shape == (0,) and got["inter"].shape == (0, 1024)
    out, n_kept = filter_components(z, 65, min_area=3)
    assert out.shape == (0, 33, 16) and n_kept.shape == (0,)
    p = torch.zeros((2, 33, 16), dtype=torch.uint8, device=DEV)
    for call in (lambda: label_components(p, 130), lambda: label_components(p, 65, connectivity=6), lambda: label_components(p, 65, max_components=0),
                 lambda: label_components(p, 65, other=p[:1]), lambda: label_components(p.int(), 65), lambda: filter_components(p, 65, min_area=-1),
                 lambda: filter_components(p, 64), lambda: components_to_instances(p, 65, max_instances=0)):
        with pytest.raises(ValueError):
            call()


def test_large_plane_at_640():
    rng = np.random.default_rng(6)
    m, other = R.big_plane(rng), R.big_plane(rng)[::-1].copy()
    packed = _pack([m])
    for conn in CONNS:
        want = _reference([m], [other], conn)
        assert want["n_components"][0] > CAP                   # the specks: the tables are truncated, the count and the labels are not
        _assert_records(label_components(packed, 640, connectivity=conn, max_components=CAP, other=_pack([other])), want, f"640, {conn}")
        _assert_filter(packed, 640, conn, want, [m], 5, 2, "640")
        _assert_filter(packed, 640, conn, want, [m], 2, None, "640")


def test_components_to_instances_and_their_consumers(cases):
    names, planes, others, want = cases[(40, 130)]
    packed = _pack(planes)
    K = 5
    for conn, min_area in ((4, 0), (8, 2)):
        got = components_to_instances(packed, 130, max_instances=K, min_area=min_area, connectivity=conn)
        assert got["masks"].shape == (len(planes), K, 40, 24) and got["masks"].dtype == torch.uint8
        counts, boxes, areas = got["counts"].cpu().numpy(), got["boxes"].cpu().numpy(), got["areas"].cpu().numpy()
        for b, (lab, a) in enumerate(zip(want[conn]["labels"], want[conn]["areas"])):
            keep = np.flatnonzero(R.keep_rule(a, min_area, K))
            order = keep[np.argsort(-a[keep], kind="stable")]                   # largest first, the lower id first among equals
            assert counts[b] == len(order)
            dense = unpack_masks(got["masks"][b], 130).cpu().numpy()
            for j in range(K):
                inst = lab == order[j] + 1 if j < len(order) else np.zeros_like(lab, bool)
                assert np.array_equal(dense[j], inst), (conn, names[b], j)
                ys, xs = np.nonzero(inst)
                box = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) if j < len(order) else (0, 0, 0, 0)
                assert tuple(boxes[b, j]) == box and areas[b, j] == inst.sum()
    sd = SurfaceDistanceMetrics()
    b = names.index("u")
    sd.update_packed(got["masks"][b], packed[b:b + 1].expand(K, -1, -1).contiguous(), 130)     # [K, H, pitch] per image, as masks_frame[b]
    per = sd.per_image()
    assert per["defined"].tolist() == [True] + [False] * (K - 1) and per["hd"][0] == 0.0          # the U is one component: itself


# ---- the metric object ------------------------------------------------------------------------------------------------------------
def _logit_case():
    """logits and masks [3,1,64,64] from dense planes: noise against blobs, blobs against shifted blobs, an empty prediction; the
    logits hold exact zeros and a NaN (both not set: bit = logit > 0), the masks values below 1 (not set: bit = mask >= 1)."""
    rng = np.random.default_rng(9)
    pred, gt = np.zeros((3, 64, 64), bool), np.zeros((3, 64, 64), bool)
    gt[0, 5:20, 5:20], gt[0, 30:34, 40:60], gt[0, 50, 50], gt[0, 60:62, 2:4] = True, True, True, True
    pred[0] = rng.uniform(size=(64, 64)) < 0.08
    pred[0, 8:22, 10:30] = True
    for k in range(6):
        y, x = int(rng.integers(0, 54)), int(rng.integers(0, 54))
        gt[1, y:y + 6, x:x + 8] = True
        pred[1, y + 3:y + 9, x + 5:x + 12] = True
    gt[2, 10:20, 10:20] = True
    logits = np.where(pred, rng.uniform(0.1, 3.0, pred.shape), -rng.uniform(0.1, 3.0, pred.shape)).astype(np.float32)
    unset = np.argwhere(~pred[0])
    logits[0][tuple(unset[:9].T)] = 0.0
    logits[0][tuple(unset[9])] = np.nan
    masks = np.where(gt, 1.0, rng.choice([0.0, 0.5, 0.999], size=gt.shape)).astype(np.float32)
    return pred, gt, torch.from_numpy(logits)[:, None].to(DEV), torch.from_numpy(masks)[:, None].to(DEV)


@pytest.mark.parametrize("kw", [dict(), dict(overlap=0.5, connectivity=8), dict(min_area=3), dict(max_components=4)],
                         ids=["default", "overlap_8", "min_area", "cap_4"])
def test_lesion_metrics_equal_the_restatement(kw):
    pred, gt, logits, masks = _logit_case()
    m = LesionMetrics(**kw)
    m.update(logits, masks)
    m.update(logits[:2, 0], masks[:2, 0])                      # [B,S,S] too
    want = R.lesion_metrics([R.lesion_counts(pred[i], gt[i], **kw) for i in (0, 1, 2, 0, 1)])
    got = m.compute()
    print(kw, got)
    assert got == want and got["n_images"] == 5 and got["n_gt"] > 0 and got["n_pred"] > 0
    assert (got["n_truncated"] > 0) == ("max_components" in kw) and 0 < got["lesion_recall"] <= 1 and 0 < got["lesion_precision"] <= 1
    m.reset()
    assert m.compute()["n_images"] == 0
    with pytest.raises(ValueError):
        m.update(logits, masks[:2])


def test_update_packed_launches_without_synchronisation():
    pred, gt, logits, masks = _logit_case()
    pp, pg = _pack(list(pred)), _pack(list(gt))
    m = LesionMetrics(min_area=2)
    m.update_packed(pp, pg, 64)                                # warm-up: the library is loaded
    m.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update_packed(pp, pg, 64)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert m.compute() == R.lesion_metrics([R.lesion_counts(pred[i], gt[i], min_area=2) for i in range(3)])


# ---- ValidationStep(lesions=...) --------------------------------------------------------------------------------------------------
KEYS_WITHOUT_LESIONS = (
    [f"val_epoch/loss_{k}" for k in ("total", "seg", "box_iou", "dfl", "det_cls", "img_cls")]
    + ["val_epoch/img_accuracy_epoch", "val_epoch/img_confusion_matrix_epoch", "val_epoch/img_precision_macro", "val_epoch/img_recall_macro",
       "val_epoch/img_f1_macro", "val_epoch/det_confusion_matrix_epoch", "val_epoch_map_iou50/map"]
    + [f"val_epoch/seg_{k}_epoch" for k in ("f1", "precision", "recall", "accuracy", "dice")]
    + [f"val_epoch/{p}_{k}" for p in ("seg_map", "map_iou50", "map_iou50_95")
       for k in ("map", "map_50", "map_75", "map_small", "map_medium", "map_large", "mar_1", "mar_10", "mar_100", "mar_small", "mar_medium",
                 "mar_large")])
LESION_KEYS = [f"val_epoch/seg_lesion_{k}" for k in ("recall", "precision", "f1", "fp_per_image")]


def test_validation_step_with_lesion_metrics():
    torch.manual_seed(0)
    model = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), seed=0).to(DEV)
    proj = torch.nn.Conv2d(model.proto_ch, 1, 1).to(DEV)
    S, Bn = 64, 3
    imgs = synthetic_images(Bn, S, seed=1).to(DEV)
    gt = torch.tensor([[0, 1, 0.4, 0.4, 0.3, 0.3], [2, 0, 0.6, 0.5, 0.2, 0.4]], device=DEV)
    masks = torch.zeros(Bn, 1, S, S, device=DEV)
    masks[0, 0, 15:35, 20:45], masks[0, 0, 50:54, 5:9], masks[2, 0, 30:50, 10:25] = 1.0, 1.0, 1.0          # image 1: no lesion
    cls = torch.tensor([0, 1, 1], device=DEV)
    model.eval()
    with torch.no_grad():                                      # centre the projector: every predicted mask has pixels on both sides of 0
        _, (_, _, protos), _ = model(imgs, "train")
        proj.bias -= proto_projector_logits(protos, proj.weight, proj.bias, S).median()
    off = ValidationStep(model, projector=proj, img_size=S)
    on = ValidationStep(model, projector=proj, img_size=S, lesions=True)
    l_off, l_on = off.step(imgs, gt, masks, cls), on.step(imgs, gt, masks, cls)
    assert all(torch.equal(a, b) for a, b in zip(l_off, l_on))
    r_off, r_on = off.compute(), on.compute()
    assert sorted(r_off) == sorted(KEYS_WITHOUT_LESIONS) and off.lesions is None       # exactly the keys of before
    assert sorted(r_on) == sorted(KEYS_WITHOUT_LESIONS + LESION_KEYS)
    for k in KEYS_WITHOUT_LESIONS:
        assert np.array_equal(np.asarray(r_on[k]), np.asarray(r_off[k])), k

    model.eval()
    with torch.no_grad():
        _, (_, _, protos), _ = model(imgs, "train")
    alone = LesionMetrics()
    alone.update(proto_projector_logits(protos, proj.weight, proj.bias, S), masks)
    want = alone.compute()
    print("lesion metrics of the step", want)
    for k in ("recall", "precision", "f1"):
        assert r_on[f"val_epoch/seg_lesion_{k}"] == want[f"lesion_{k}"], k
    assert r_on["val_epoch/seg_lesion_fp_per_image"] == want["fp_per_image"]
    assert want["n_images"] == Bn and want["n_gt"] == 3 and want["n_pred"] > 0
    on.reset()
    assert on.compute()["val_epoch/seg_lesion_recall"] == 0.0


@pytest.mark.parametrize("shape", [(7, 63), (9, 127)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_padding_bit_in_the_last_word(shape):
    """W % 64 == 63, below and above 64: one padding bit in the last word, where a wrong valid_bits shows: a full plane, noise, and a plane whose last column and middle row are set, padding bits set on the way in."""
    H, W = shape
    rng = np.random.default_rng(W)
    planes = [np.ones((H, W), bool), rng.uniform(size=(H, W)) < 0.5, np.zeros((H, W), bool)]
    planes[2][:, W - 1] = planes[2][H // 2, :] = True
    others = [rng.uniform(size=(H, W)) < 0.3 for _ in planes]
    for conn in CONNS:
        want = _reference(planes, others, conn)
        got = label_components(_pack(planes, True), W, connectivity=conn, max_components=CAP, other=_pack(others, True))
        _assert_records(got, want, f"{shape} {conn}")
        _assert_filter(_pack(planes, True), W, conn, want, planes, 2, 3, f"{shape} {conn}")
