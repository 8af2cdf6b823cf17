"""Instance-mask mAP on the device (metrics.DeviceMaskMeanAveragePrecision, csrc/mask_eval.hip): `pack_masks` bit-exact against
numpy.packbits, the pixel-count tables exactly equal to numpy on unpacked planes (list and uniform layouts, odd 8-byte aligned planes,
ragged tails, register-group boundaries, planes past `counts` that must not be read), the matching end to end against the plain-loop
restatement `coco_reference.coco_loop_iou` fed from numpy pixel counts, cross-checks against the box class and the single-instance
segmentation mAP, and `ValidationStep(instance_masks=True)` against the public functions by hand."""
import numpy as np
import pytest
import torch

from multitask_bonetumor_yolo_amd import metrics as M
from multitask_bonetumor_yolo_amd.metrics import DeviceMaskMeanAveragePrecision, DeviceMeanAveragePrecision, SegmentationMetrics

import frame_reference as FR
from coco_reference import COCO, _random_set, coco_loop_iou
from mask_reference import loop_image, loop_images, mask_case, pack_np, pair_counts_np, pitch_of, unpack_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import postprocess as pp


def _close(got, want, tol=1e-12):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, v in want.items():
        if isinstance(v, list):
            assert len(got[k]) == len(v) and all(abs(a - b) <= tol for a, b in zip(got[k], v)), (k, got[k], v)
        else:
            assert abs(got[k] - v) <= tol, (k, got[k], v)


# ---- pack ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 1), (5, 40), (5, 64), (5, 70), (33, 130)]


def _planes(H, W, dtype, n=5, seed=0):
    rng = np.random.default_rng(seed + 131 * H + W)
    if dtype == "float32":
        v = rng.choice(np.array([-1.0, 0.0, 1e-30, np.nan, 1.0, 0.5, -0.0, np.inf, -np.inf], np.float32), (n, H, W))
        return v, np.nan_to_num(v, nan=-1.0) > 0
    if dtype == "uint8":
        v = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), (n, H, W))
        return v, v > 0
    v = rng.uniform(size=(n, H, W)) < 0.4
    return v, v


@pytest.mark.parametrize("dtype", ["bool", "uint8", "float32"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_pack_is_bit_exact(H, W, dtype):
    v, bits = _planes(H, W, dtype)
    got = pp.pack_masks(torch.from_numpy(v).to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, H, pitch_of(W))
    want = pack_np(bits)
    assert np.array_equal(want, FR.pack_bits(torch.from_numpy(bits)).numpy())      # the two host packers agree
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(pp.unpack_masks(got, W).cpu(), torch.from_numpy(bits))       # unpack_masks is the inverse
    # a strided source: every second row of a taller tensor, a window of a wider one
    big = torch.zeros((5, 2 * H, W + 3), dtype=torch.from_numpy(v).dtype, device=DEV)
    big[:, ::2, 2:W + 2] = torch.from_numpy(v).to(DEV)
    out = torch.full((5, H, pitch_of(W)), 255, dtype=torch.uint8, device=DEV)         # a caller's buffer full of 0xFF: every byte is rewritten
    assert pp.pack_masks(big[:, ::2, 2:W + 2], out=out) is out
    assert np.array_equal(out.cpu().numpy(), want)
    assert not out[:, :, (W + 7) // 8:].any()                                         # whole padding bytes


@pytest.mark.parametrize("H,W", SHAPES)
def test_pack_crops_and_gathers(H, W):
    v, bits = _planes(H, W, "float32", n=3, seed=1)
    plane_of = np.array([2, 0, 2, 7, 1, -1, 0, 1], np.int32)            # a repeated index, two out of range
    boxes = np.array([[0.5, 0.5, W - 0.5, H - 0.25],                    # fractional edges
                      [0.0, 0.0, W, H],                                 # everything
                      [W / 3, 1.0, W / 3, H],                           # empty: x1 == x2
                      [0.0, 0.0, W, H],                                 # (zero plane anyway)
                      [W + 1.0, H + 1.0, W + 9.0, H + 9.0],             # wholly outside
                      [0.0, 0.0, W, H],
                      [W / 2 - 0.01, H / 2 + 0.01, W * 0.9, H * 0.8],
                      [-5.0, -5.0, 1.0, 1.0]], np.float32)              # only pixel (0, 0)
    n_out = len(plane_of)
    src = np.where(((plane_of >= 0) & (plane_of < 3))[:, None, None], bits[np.clip(plane_of, 0, 2)], False)
    region = FR.crop_region(torch.from_numpy(boxes), H, W).numpy()
    want = pack_np(src & region)
    # the kernel writes into a buffer that this test filled with 0xFF: every byte must be rewritten, zero planes and padding included
    out = torch.full((n_out, H, pitch_of(W)), 255, dtype=torch.uint8, device=DEV)
    got = pp.pack_masks(torch.from_numpy(v).to(DEV), boxes=torch.from_numpy(boxes).to(DEV), plane_of=torch.from_numpy(plane_of).to(DEV), out=out)
    assert got is out and bool((out == 255).all()) is False
    g = got.cpu().numpy()
    assert np.array_equal(g, want)                                                   # every byte
    assert not np.unpackbits(g, axis=-1, bitorder="little")[:, :, W:].any()          # padding bits are zero
    assert not g[:, :, (W + 7) // 8:].any()                                          # and so are the whole padding bytes
    assert not g[2].any() and not g[3].any() and not g[4].any() and not g[5].any()
    assert g[7].sum() == int(src[7, 0, 0])
    # boxes alone: one per source plane
    got = pp.pack_masks(torch.from_numpy(v).to(DEV), boxes=torch.from_numpy(boxes[:3]).to(DEV))
    assert np.array_equal(got.cpu().numpy(), pack_np(bits & region[:3]))


def test_pack_refuses_what_it_does_not_do():
    with pytest.raises(RuntimeError):
        pp.pack_masks(torch.zeros(1, 4, 4, dtype=torch.bool))             # no CPU path
    with pytest.raises(ValueError):
        pp.pack_masks(torch.zeros(1, 4, 4, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        pp.pack_masks(torch.zeros(2, 4, 4, dtype=torch.bool, device=DEV), boxes=torch.zeros(3, 4, device=DEV))
    with pytest.raises(ValueError):                                       # out= of another shape
        pp.pack_masks(torch.zeros(2, 4, 4, dtype=torch.bool, device=DEV), out=torch.zeros(2, 4, 16, dtype=torch.uint8, device=DEV))
    assert tuple(pp.pack_masks(torch.zeros(0, 4, 70, dtype=torch.bool, device=DEV)).shape) == (0, 4, 16)


# ---- pair counts -----------------------------------------------------------------------------------------------------------------
K17, COUNTS, NGT = 17, (0, 3, 17, 9), (0, 1, 5, 9)


def _pair_data(sizes, seed):
    """Image b of the launch has COUNTS[b] live planes and NGT[b] ground-truth planes, whatever its size."""
    rng = np.random.default_rng(seed)
    dets = [rng.uniform(size=(K17, H, W)) < rng.uniform(0.2, 0.8) for H, W in sizes]
    gts = [rng.uniform(size=(g, H, W)) < 0.5 for g, (H, W) in zip(NGT, sizes)]
    return dets, gts


def _want_tables(dets, gts, dead):
    """numpy tables of one launch: planes k >= counts[b] count as empty; flat row `dead` is of no image."""
    inter, darea, garea = [], [], []
    for d, g, c in zip(dets, gts, COUNTS):
        d = d.copy()
        d[c:] = False
        i, da, ga = pair_counts_np(d, g)
        inter.append(i); darea.append(da); garea.append(ga)
    inter, garea = np.concatenate(inter), np.concatenate(garea)
    inter[dead], garea[dead] = 0, 0
    return inter, np.stack(darea), garea


def _packed_dets(dets):
    """Packed detection planes with the planes k >= counts[b] filled with 0xFF, padding included: neither counted nor needed."""
    out = []
    for d, c in zip(dets, COUNTS):
        p = torch.from_numpy(pack_np(d)).to(DEV)
        p[c:] = 255
        out.append(p)
    return out


def _run_list(sizes, dets, gts, dead):
    (c0, c1, g0, gi), = M._mask_launch_layout(NGT)
    gi = gi.copy()
    gi[dead] = -1
    dp, gp = _packed_dets(dets), [torch.from_numpy(pack_np(g)).to(DEV) for g in gts]
    dummy = torch.zeros(8, dtype=torch.uint8, device=DEV)
    images = [(H, W, dp[b], gp[b] if NGT[b] else dummy, g0[b], NGT[b]) for b, (H, W) in enumerate(sizes)]
    assert all(t.data_ptr() % 8 == 0 for t in dp + gp)
    m = sum(NGT)
    # the tables the entry point fills are this test's own, every word 0xFFFFFFFF: a word it leaves undefined shows in the comparison
    out = tuple(torch.full(shape, -1, dtype=torch.int32, device=DEV) for shape in ((m, K17), (len(sizes), K17), (m,)))
    inter, darea, garea = M._pair_counts(images, K17, torch.tensor(COUNTS, dtype=torch.int32, device=DEV), torch.from_numpy(gi).to(DEV), m, DEV, out=out)
    assert inter is out[0] and darea is out[1] and garea is out[2]
    return inter.cpu().numpy().view(np.uint32), darea.cpu().numpy().view(np.uint32), garea.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("order", ["as_listed", "reversed"])
def test_pair_counts_list_layout_with_mixed_sizes(order):
    """as_listed: the (300 x 200) image has 9 live planes and 9 GT (several chunks per thread, a ragged tail, three register groups) and
    the (33 x 64) image all 17 planes and 5 GT: its planes of 33 * 8 = 264 bytes put every second one on an odd 8-byte boundary.  The
    (5 x 40) image has counts = 0 and no GT there, so none of its words is loaded; `reversed` gives it the 9 live planes and the 9 GT
    (planes of 40 bytes, odd ones 8-byte aligned only) and leaves the (300 x 200) image unread."""
    sizes = [(5, 40), (5, 70), (33, 64), (300, 200)]
    assert (5 * pitch_of(40)) % 16 == 8 and (33 * pitch_of(64)) % 16 == 8
    assert (300 * pitch_of(200) // 8) % 256 != 0 and 300 * pitch_of(200) // 8 > 4 * 256
    if order == "reversed":
        sizes = sizes[::-1]
    dets, gts = _pair_data(sizes, 11)
    dead = 4                                                            # a row of image 2
    want = _want_tables(dets, gts, dead)
    got = _run_list(sizes, dets, gts, dead)
    for g, w, name in zip(got, want, ("inter", "det_area", "gt_area")):
        assert g.shape == w.shape and np.array_equal(g.astype(np.int64), w), name     # every word of every table
    assert want[0][6:].any() and want[1][3, :9].all() and not got[1][0].any() and not got[0][:, 9:][6:].any()
    assert want[0][1:6, :].any() and want[1][2].all()                                 # image 2: all 17 planes live against 5 GT


def test_pair_counts_uniform_layout_equals_list_layout():
    sizes = [(64, 96)] * 4
    dets, gts = _pair_data(sizes, 12)
    dead = 9
    want = _want_tables(dets, gts, dead)
    got_list = _run_list(sizes, dets, gts, dead)
    gi = np.repeat(np.arange(4, dtype=np.int32), NGT)
    gi[dead] = -1
    det = torch.stack(_packed_dets(dets))
    gt = torch.from_numpy(pack_np(np.concatenate(gts))).to(DEV)
    got = DeviceMaskMeanAveragePrecision.pair_tables_uniform(det, torch.tensor(COUNTS, device=DEV), gt, torch.from_numpy(gi).to(DEV))
    for g, l, w, name in zip(got, got_list, want, ("inter", "det_area", "gt_area")):
        g = g.cpu().numpy().view(np.uint32)
        assert np.array_equal(g, l) and np.array_equal(g.astype(np.int64), w), name
    # rows in any order: membership is known only on the device
    perm = np.random.default_rng(0).permutation(len(gi))
    got = DeviceMaskMeanAveragePrecision.pair_tables_uniform(det, torch.tensor(COUNTS, device=DEV), gt[torch.from_numpy(perm).to(DEV)],
                                                             torch.from_numpy(gi[perm]).to(DEV))
    assert np.array_equal(got[0].cpu().numpy().astype(np.int64), want[0][perm]) and np.array_equal(got[2].cpu().numpy().astype(np.int64), want[2][perm])


def test_pair_counts_33_images_are_chunked():
    rng = np.random.default_rng(13)
    B, K, H, W = 33, 3, 7, 70
    det = rng.uniform(size=(B, K, H, W)) < 0.5
    gi = rng.integers(-1, B, 50).astype(np.int32)
    gi[:2] = (32, 0)                                                    # the last image (second launch) and the first
    gt = rng.uniform(size=(50, H, W)) < 0.5
    counts = rng.integers(0, K + 1, B).astype(np.int32)
    counts[32] = K
    got = DeviceMaskMeanAveragePrecision.pair_tables_uniform(torch.from_numpy(np.stack([pack_np(d) for d in det])).to(DEV), torch.from_numpy(counts).to(DEV),
                                                             torch.from_numpy(pack_np(gt)).to(DEV), torch.from_numpy(gi).to(DEV))
    live = det & (np.arange(K)[None, :] < counts[:, None])[:, :, None, None]
    inter = np.stack([(pair_counts_np(live[b], gt[m:m + 1])[0][0] if b >= 0 else np.zeros(K, np.int64)) for m, b in enumerate(gi)])
    assert np.array_equal(got[0].cpu().numpy().astype(np.int64), inter) and inter[0].any()
    assert np.array_equal(got[1].cpu().numpy().astype(np.int64), live.reshape(B, K, -1).sum(2))
    assert np.array_equal(got[2].cpu().numpy().astype(np.int64), np.where(gi >= 0, gt.reshape(50, -1).sum(1), 0))


# ---- matching, end to end --------------------------------------------------------------------------------------------------------
SEED = 1


@pytest.fixture(scope="module")
def case():
    c = mask_case(SEED)
    return c, loop_images(c)


def _want(images, thr, md):
    return coco_loop_iou(images, thr, md, class_metrics=True)


def test_case_set_is_not_degenerate(case):
    c, images = case
    want = _want(images, COCO, [1, 10, 100])
    assert 0 < want["map"] < 1 and all(want[k] != -1 for k in ("map_small", "map_medium", "map_large"))
    assert {len(x["gt"]) for x in c} >= {0, 1, 6} and any(x["count"] == 0 for x in c) and any(0 < x["count"] < 12 for x in c)


@pytest.mark.parametrize("thr,md", [(COCO, [1, 10, 100]), ([0.5, 0.75], [1, 3, 10])])
def test_list_update_equals_loop_restatement(case, thr, md):
    c, images = case
    m = DeviceMaskMeanAveragePrecision(iou_thresholds=thr, max_detection_thresholds=md, class_metrics=True)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    preds = [dict(masks=dev(x["det"][:x["count"]]), scores=dev(x["scores"][:x["count"]]), labels=dev(x["labels"][:x["count"]])) for x in c]
    targets = [dict(masks=dev(x["gt"]), labels=dev(x["gt_labels"])) for x in c]
    m.update(preds[:25], targets[:25])
    # the rest already packed, with the width supplied
    for p, t in zip(preds[25:], targets[25:]):
        p["masks"], p["width"], t["masks"], t["width"] = pp.pack_masks(p["masks"]), 160, pp.pack_masks(t["masks"]), 160
    m.update(preds[25:], targets[25:])
    got = m.compute()
    for k in ("map", "map_50", "map_small", "map_medium", "map_large", f"mar_{md[-1]}"):
        print(f"{k}: {got[k]!r}")
    _close(got, _want(images, thr, md))


def _frames_layout(c):
    """The case as `detect_and_segment(..., frames=)` returns it: K slots per image, slots >= counts hold ones and are not read."""
    det = dict(masks_frame=[torch.from_numpy(pack_np(x["det"])).to(DEV) for x in c], scores=torch.from_numpy(np.stack([x["scores"] for x in c])).to(DEV),
               labels=torch.from_numpy(np.stack([x["labels"] for x in c])).to(DEV),
               counts=torch.tensor([x["count"] for x in c], dtype=torch.int32, device=DEV))
    return det, [torch.from_numpy(pack_np(x["gt"])).to(DEV) for x in c], [torch.from_numpy(x["gt_labels"]).to(DEV) for x in c]


def test_batched_and_uniform_updates_equal_loop_restatement(case):
    c, images = case
    want = _want(images, COCO, [1, 10, 100])
    det, gt_masks, gt_labels = _frames_layout(c)
    m = DeviceMaskMeanAveragePrecision(class_metrics=True)
    m.update_batched(det, gt_masks, gt_labels)                           # 40 images: two launches
    _close(m.compute(), want)
    # uniform: one flat GT buffer, rows reordered, membership and class from the collated rows (one row of no image, one fractional)
    rows = np.concatenate([np.stack([np.full(len(x["gt"]), b), x["gt_labels"]], 1) for b, x in enumerate(c)] + [[[40.0, 0.0]], [[1.5, 1.0]]])
    flat = np.concatenate([pack_np(x["gt"]) for x in c] + [np.full((2, 128, 24), 255, np.uint8)])
    perm = np.argsort(-rows[:, 0], kind="stable")                     # images in reverse order, each image's rows in their own order
    gt_rows = np.zeros((len(rows), 6), np.float32)
    gt_rows[:, :2] = rows[perm]
    m = DeviceMaskMeanAveragePrecision(class_metrics=True)
    m.update_uniform(torch.stack(det["masks_frame"]), det["scores"], det["labels"], det["counts"], torch.from_numpy(flat[perm]).to(DEV),
                     torch.from_numpy(gt_rows).to(DEV))
    _close(m.compute(), want)


def test_sizes_must_agree_and_cpu_tensors_are_refused():
    m = DeviceMaskMeanAveragePrecision()
    z = lambda *s: torch.zeros(*s, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError):
        m.update([dict(masks=z(1, 8, 8), scores=torch.ones(1), labels=torch.zeros(1))], [dict(masks=z(1, 8, 9), labels=torch.zeros(1))])
    with pytest.raises(RuntimeError):
        m.update([dict(masks=z(1, 8, 8).cpu(), scores=torch.ones(1), labels=torch.zeros(1))], [dict(masks=z(1, 8, 8), labels=torch.zeros(1))])
    with pytest.raises(ValueError):
        m.update([dict(masks=z(1, 8, 8), scores=torch.ones(1), labels=torch.zeros(1))], [])


def test_a_launch_without_any_gt_plane_needs_no_inter_table():
    """M == 0: `mtbt_mask_pair_counts` takes NULL inter / gt_image / gt_area and still writes the detections' areas."""
    bits = np.random.default_rng(3).uniform(size=(3, 5, 40)) < 0.5
    det = torch.from_numpy(pack_np(bits)).to(DEV)
    out = tuple(torch.full(shape, -1, dtype=torch.int32, device=DEV) for shape in ((0, 3), (1, 3), (0,)))
    M._pair_counts([(5, 40, det, det, 0, 0)], 3, None, torch.zeros(0, dtype=torch.int32, device=DEV), 0, DEV, out=out)
    assert np.array_equal(out[1].cpu().numpy()[0], bits.reshape(3, -1).sum(1))
    m = DeviceMaskMeanAveragePrecision()
    m.update([dict(masks=torch.from_numpy(bits).to(DEV), scores=torch.tensor([0.9, 0.8, 0.7]), labels=torch.zeros(3))],
             [dict(masks=torch.zeros(0, 5, 40, dtype=torch.bool, device=DEV), labels=torch.zeros(0))])
    assert m.compute()["map"] == -1.0


def test_more_than_1024_gt_masks_in_an_image_raise():
    """The walk keeps at most 1024 GT rows of an image in LDS: the 1025th sets the status word and `compute()` raises, as in the box
    class.  Planes of one pixel (8 bytes) keep the case small."""
    z = lambda n: torch.zeros(n, 1, 1, dtype=torch.bool, device=DEV)
    m = DeviceMaskMeanAveragePrecision()
    m.update([dict(masks=z(2), scores=torch.tensor([0.9, 0.8]), labels=torch.zeros(2))], [dict(masks=z(1025), labels=torch.zeros(1025))])
    with pytest.raises(RuntimeError, match="more than 1024 GT masks"):
        m.compute()
    m = DeviceMaskMeanAveragePrecision()                                    # exactly 1024 are fine
    m.update([dict(masks=~z(2), scores=torch.tensor([0.9, 0.8]), labels=torch.zeros(2))], [dict(masks=~z(1024), labels=torch.zeros(1024))])
    got = m.compute()
    # one-pixel masks, all identical: both detections match (IoU 1) and 1022 GT stay unmatched
    # (recall 2 / 1024 at precision 1: of the 101 recall points only r = 0 is reached, at every threshold)
    assert abs(got["map"] - 1 / 101) <= 1e-12 and abs(got["mar_100"] - 2 / 1024) <= 1e-12


# ---- cross-checks ----------------------------------------------------------------------------------------------------------------
def _rect_masks(boxes, S):
    """Filled rectangles with integer corners: pixels x1 <= X < x2, y1 <= Y < y2 (area = the box's area exactly)."""
    b = torch.as_tensor(boxes, dtype=torch.float32, device=DEV).reshape(-1, 4)
    X = torch.arange(S, dtype=torch.float32, device=DEV)
    inx, iny = (b[:, 0, None] <= X) & (X < b[:, 2, None]), (b[:, 1, None] <= X) & (X < b[:, 3, None])
    return iny[:, :, None] & inx[:, None, :]


def test_filled_rectangles_equal_the_box_class():
    S = 608
    preds, targets = _random_set(4, n_img=12)
    for d in preds + targets:
        d["boxes"] = np.clip(np.round(d["boxes"]), 0, S).astype(np.float32)
    t = lambda lst: [{k: torch.as_tensor(v) for k, v in d.items()} for d in lst]
    box = DeviceMeanAveragePrecision(class_metrics=True)
    box.update(t(preds), t(targets))
    want = box.compute()
    m = DeviceMaskMeanAveragePrecision(class_metrics=True)
    m.update([dict(masks=_rect_masks(p["boxes"], S), scores=p["scores"], labels=p["labels"]) for p in preds],
             [dict(masks=_rect_masks(g["boxes"], S), labels=g["labels"]) for g in targets])
    assert 0 < want["map"] < 1 and want["map_small"] > 0 and want["map_large"] > 0
    _close(m.compute(), want)


def test_single_instances_equal_the_segmentation_map():
    rng = np.random.default_rng(6)
    B, S = 14, 112
    Y, X = np.mgrid[0:S, 0:S]
    logits, gt = np.zeros((B, 1, S, S), np.float32), np.zeros((B, 1, S, S), np.float32)
    for b in range(B):
        side = int(rng.choice([12, 30, 32, 60, 96, 100]))
        x, y = rng.integers(0, S - side + 1, 2)
        g = (X >= x) & (X < x + side) & (Y >= y) & (Y < y + side)
        dx, dy = rng.integers(-side // 4, side // 4 + 1, 2)
        p = (X >= x + dx) & (X < x + dx + side) & (Y >= y + dy) & (Y < y + dy + side)
        if b == 3:
            p[:] = False                                                # nothing predicted
        if b == 5:
            g[:], p[:] = False, False                                   # empty against empty: union 0
        gt[b, 0], logits[b, 0] = g, np.where(p, 1.0, -1.0) * rng.uniform(0.5, 3.0, (S, S))
    seg = SegmentationMetrics()
    seg.update(torch.from_numpy(logits).to(DEV), torch.from_numpy(gt).to(DEV))
    want = seg.compute_map()
    _, score = seg.per_image()
    m = DeviceMaskMeanAveragePrecision()
    dev = lambda a: torch.from_numpy(a).to(DEV)
    m.update([dict(masks=dev(logits[b] > 0), scores=score[b:b + 1], labels=np.zeros(1, np.int64)) for b in range(B)],
             [dict(masks=dev(gt[b] > 0), labels=np.zeros(1, np.int64)) for b in range(B)])
    assert 0 < want["map"] < 1
    _close(m.compute(), want)


# ---- ValidationStep(instance_masks=True) -----------------------------------------------------------------------------------------
def _model():
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, init_synthetic_
    torch.manual_seed(0)
    return init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), seed=0).to(DEV)


def _batch(B, S, seed):
    from multitask_bonetumor_yolo_amd import synthetic_images
    g = torch.Generator().manual_seed(100 + seed)
    rows = []
    for b in range(B):
        for _ in range(1 + b % 2):
            wh = torch.rand(2, generator=g) * 0.4 + 0.2
            cxy = torch.rand(2, generator=g) * (1 - wh) + wh / 2
            rows.append(torch.cat([torch.tensor([float(b), float(torch.randint(0, 2, (1,), generator=g))]), cxy, wh]))
    masks = (torch.rand(B, 1, S, S, generator=g) > 0.4).float()
    return synthetic_images(B, S, seed=seed).to(DEV), torch.stack(rows).to(DEV), masks.to(DEV), torch.randint(0, 2, (B,), generator=g).to(DEV)


def _detections(vs, x, S):
    """What `step` keeps of a batch, by the public functions: the NMS output and the kept boxes' uncropped masks as bool [B,K,S,S]
    (the identity-frame path, which test_identity_frames_equal_the_dense_kernel pins to assemble_masks)."""
    det, (_, mc, protos), _ = vs.forward(x)
    d = pp.decode_boxes(det, S, want_scores=False)
    k = pp.nms_batched(d["boxes"], d["best_score"], d["best_label"], float(S), pp.CONF_TH, pp.NMS_IOU, pp.TOP_K)
    r = pp.masks_to_frames(protos, mc, k["keep_anchor"], k["counts"], k["boxes"], [(S, S, 1.0)] * x.shape[0], up=S / protos.shape[3], crop=False)
    return k, [unpack_np(m.cpu().numpy(), S) for m in r["masks"]]


def _planted_batch(vs, B, S, seed):
    """`_batch` with ground truth that the model's own output overlaps, so that the mask mAP is neither 0 nor -1 and a wrong crop rule
    shows: in every image the first GT row becomes one kept box shrunk to 0.85 of its sides (the kept box for which that gives an IoU
    nearest 0.72) with that detection's class, and the image's mask becomes that detection's uncropped mask.  The GT instance is then
    the mask inside the shrunk box, the detection the same mask inside the whole box: an IoU near 0.85^2, above some thresholds only."""
    x, rows, masks, cls = _batch(B, S, seed)
    k, bits = _detections(vs, x, S)
    rows, masks = rows.cpu().clone(), masks.cpu().clone()
    for b in range(B):
        n = int(k["counts"][b])
        assert n > 0, "the synthetic model keeps no box in this image"
        fb = FR.frame_boxes(k["boxes"][b].cpu(), n, S, S, 1.0)[:n]
        c, wh = (fb[:, :2] + fb[:, 2:]) / 2, (fb[:, 2:] - fb[:, :2]) * 0.85
        shrunk = torch.cat([c - wh / 2, c + wh / 2], 1)
        inside = (bits[b][:n] & FR.crop_region(shrunk, S, S).numpy()[:n]).reshape(n, -1).sum(1)
        whole = (bits[b][:n] & FR.crop_region(fb, S, S).numpy()[:n]).reshape(n, -1).sum(1)
        j = int(np.abs(inside / np.maximum(whole, 1) - 0.72).argmin())          # the IoU of the planted pair
        print(f"seed {seed} image {b}: {n} kept, planted on slot {j}, IoU {inside[j]} / {whole[j]}")
        first = int(torch.nonzero(rows[:, 0] == b)[0])
        rows[first] = torch.cat([torch.tensor([float(b), float(k["labels"][b, j])]), c[j] / S, wh[j] / S])
        masks[b, 0] = torch.from_numpy(bits[b][j]).float()
    return x, rows.to(DEV), masks.to(DEV), cls


def test_validation_step_instance_masks_equal_the_public_functions_by_hand():
    from multitask_bonetumor_yolo_amd import ValidationStep
    model, S = _model(), 128
    off, on = ValidationStep(model, img_size=S), ValidationStep(model, img_size=S, instance_masks=True)
    batches = [_planted_batch(on, 2, S, 1), _planted_batch(on, 2, S, 2)]
    on.projector.load_state_dict(off.projector.state_dict())
    images = []
    for x, gt, masks, cls in batches:
        off.step(x, gt, masks, cls)
        on.step(x, gt, masks, cls)
        k, dense = _detections(on, x, S)                                   # uncropped, cropped on the host below
        rows = gt.cpu().numpy().astype(np.float32)
        cx, cy, w, h = (rows[:, i] for i in (2, 3, 4, 5))
        two, fS = np.float32(2), np.float32(S)
        px = np.clip(np.stack([(cx - w / two) * fS, (cy - h / two) * fS, (cx + w / two) * fS, (cy + h / two) * fS], 1), 0, fS).astype(np.float32)
        for b in range(2):
            n = int(k["counts"][b])
            fb = FR.frame_boxes(k["boxes"][b].cpu(), n, S, S, 1.0)
            bits = dense[b][:n] & FR.crop_region(fb, S, S).numpy()[:n]
            mine = rows[:, 0] == b
            g = (masks[b, 0].cpu().numpy() > 0)[None] & FR.crop_region(torch.from_numpy(px[mine]), S, S).numpy()
            images.append(loop_image(k["scores"][b, :n].cpu().numpy(), k["labels"][b, :n].cpu().numpy(), bits, rows[mine, 1].astype(np.int64), g))
    assert sum(len(im[0]) for im in images) > 0 and sum(len(im[3]) for im in images) == 6
    a, b = off.compute(), on.compute()
    want = {f"val_epoch/mask_map_iou50_95_{k}": v for k, v in coco_loop_iou(images, COCO, [1, 10, 100]).items()}
    want.update({f"val_epoch/mask_map_iou50_{k}": v for k, v in coco_loop_iou(images, [0.5], [1, 10, 100]).items()})
    assert not any("mask_map" in k for k in a) and set(b) - set(a) == set(want) and len(want) == 24
    for k in a:                                                           # the option changes nothing else
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    for k, v in want.items():
        print(f"{k}: {b[k]!r}")
        assert abs(b[k] - v) <= 1e-12, (k, b[k], v)
    # the comparison is not one of zeros and -1 alone: the planted ground truth is matched at some thresholds and missed at others
    assert 0 < want["val_epoch/mask_map_iou50_95_map"] < 1 and want["val_epoch/mask_map_iou50_map"] > 0
    on.reset()
    assert on.compute()["val_epoch/mask_map_iou50_map"] == -1.0


def test_step_with_instance_masks_does_not_synchronise():
    from multitask_bonetumor_yolo_amd import ValidationStep
    S = 128
    vs = ValidationStep(_model(), img_size=S, instance_masks=True)
    batch = _batch(2, S, 3)
    vs.step(*batch)                                                        # warm-up: plans are built
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = vs.step(*batch)
        with pytest.raises(RuntimeError):                                  # positive control: the mode fires on this build
            losses[0].item()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert "val_epoch/mask_map_iou50_95_map" in vs.compute()


@pytest.mark.parametrize("W", [63, 65, 127])
def test_pack_next_to_a_word_boundary(W):
    """W % 64 == 63 (below and above 64) and 1: the last word holds all but one pixel, or one."""
    v, bits = _planes(5, W, "bool", n=3)
    out = torch.full((3, 5, pitch_of(W)), 255, dtype=torch.uint8, device=DEV)
    got = pp.pack_masks(torch.from_numpy(v).to(DEV), out=out)
    assert np.array_equal(got.cpu().numpy(), pack_np(bits)) and torch.equal(pp.unpack_masks(got, W).cpu(), torch.from_numpy(bits))
