"""`mtbt_fill_polygons` on the device, bit for bit against tests/polygon_reference.py, and the paths that consume its planes:
`yolo_seg_planes` into the instance-mask mAP, `augment_samples_seg` / `mosaic_samples_seg`, and a training step on their outputs."""
import numpy as np
import pytest
import torch

import polygon_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import postprocess as pp
    from multitask_bonetumor_yolo_amd import preprocess as P
    from multitask_bonetumor_yolo_amd import ConvNeXtBiFPNYOLO, DeviceMaskMeanAveragePrecision, TrainStep

SHAPES = [(1, 1), (1, 70), (37, 64), (33, 65), (40, 130), (96, 200)]
_cache = {}


def _cases(H, W):
    """The named planes of a shape and their reference fills, computed once and shared (never modified)."""
    if (H, W) not in _cache:
        cases = R.polygon_cases(np.random.default_rng(1000 * H + W), H, W)
        _cache[(H, W)] = (cases, [R.fill(p, H, W) for _, p in cases])
    return _cache[(H, W)]


def _check(names, got, area, boxes, want):
    got, area, boxes = got.cpu().numpy(), area.cpu().numpy(), boxes.cpu().numpy()
    assert area.dtype == np.int32 and boxes.dtype == np.float32
    for k, (name, m) in enumerate(zip(names, want)):
        assert np.array_equal(got[k], R.pack_bits(m)), name          # padding bits included: pack_bits leaves them zero
        a, b = R.records(m)
        assert int(area[k]) == a and boxes[k].tolist() == [float(v) for v in b], name


@pytest.mark.parametrize("H,W", SHAPES)
def test_fill_equals_the_reference(H, W):
    cases, want = _cases(H, W)
    names, planes = [n for n, _ in cases], [p for _, p in cases]
    pitch = 8 * ((W + 63) // 64)
    got, area, boxes = pp.fill_polygons(planes, H, W, records=True, device=DEV)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(cases), H, pitch)
    _check(names, got, area, boxes, want)
    assert any(m.any() for m in want) and not want[0].any()
    out = torch.full((len(cases), H, pitch), 0xFF, dtype=torch.uint8, device=DEV)          # every byte is written, whatever it held
    assert pp.fill_polygons(planes, H, W, out=out) is out
    assert torch.equal(out, got)
    assert torch.equal(pp.fill_polygons(planes, H, W, device=DEV), got)                   # without the records


@pytest.mark.parametrize("H,W", SHAPES)
def test_fill_with_clip_rectangles(H, W):
    cases, _ = _cases(H, W)
    names, planes = [n for n, _ in cases], [p for _, p in cases]
    rects = [[(W // 4, H // 4, W - W // 4, H - H // 5), (W // 2, H // 2, W // 2, H), (5, 3, 2, 1), (-7, -3, W + 90, H + 4),
              (W - 1, 0, W + 64, H), (0, H - 1, W, H + 1), (63, 0, 65, H), (W, 0, W + 5, H)][(k + H) % 8] for k in range(len(cases))]
    want = [R.fill(p, H, W, r) for p, r in zip(planes, rects)]
    got, area, boxes = pp.fill_polygons(planes, H, W, clip=np.asarray(rects, dtype=np.int32), records=True, device=DEV)
    _check(names, got, area, boxes, want)
    out = torch.full_like(got, 0xFF)
    pp.fill_polygons(planes, H, W, clip=torch.tensor(rects), out=out)
    assert torch.equal(out, got)


@pytest.mark.parametrize("H,W", [(640, 640), (300, 1000)])
def test_larger_planes(H, W):
    rng = np.random.default_rng(H)
    pick = dict(R.polygon_cases(rng, H, W))
    planes = [pick["circle_3000"], pick["seven_circles_500"]]
    for k in range(30):
        planes.append([np.stack([rng.uniform(-0.3 * W, 1.3 * W, n), rng.uniform(-0.3 * H, 1.3 * H, n)], axis=1)
                       for n in rng.integers(3, 40, 1 + k % 3)])
    want = [R.fill(p, H, W) for p in planes]
    got, area, boxes = pp.fill_polygons(planes, H, W, records=True, device=DEV)
    assert got.shape[2] == 8 * ((W + 63) // 64)
    _check([str(k) for k in range(len(planes))], got, area, boxes, want)


def test_bad_tables_are_clamped():
    """The header's clamping, through the C entry point: offsets outside their table are clamped into it (a decreasing pair is an empty
    range) and coordinates into [-2^24, 2^24], so the planes are those of the clamped tables."""
    import ctypes as C
    from multitask_bonetumor_yolo_amd import _lib as L
    H, W, big = 20, 70, 2 ** 31 - 1
    q = np.array([[80, 40], [big, 100], [300, -big - 1], [-big, -big], [900, 16], [big, big], [40, 300], [16, 16]], dtype=np.int32)
    px = np.clip(q.astype(np.int64), -2 ** 24, 2 ** 24) / 16.0                    # exact in float32: the reference quantises them back
    want = [R.fill([px[0:3]], H, W), R.fill([px[3:8]], H, W), np.zeros((H, W), dtype=bool)]
    assert want[0].any() and want[1].any()
    dev = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(DEV)
    vertices, poly_offsets, plane_offsets = dev(q), dev([-5, 3, 100, 6]), dev([-1, 1, 99, 2])
    out = torch.full((3, H, 16), 0xFF, dtype=torch.uint8, device=DEV)
    area, box = torch.full((3,), -1, dtype=torch.int32, device=DEV), torch.full((3, 4), -1, dtype=torch.int32, device=DEV)
    a = L.FillPolygonsArgs()
    a.vertices, a.poly_offsets, a.plane_offsets, a.out = vertices.data_ptr(), poly_offsets.data_ptr(), plane_offsets.data_ptr(), out.data_ptr()
    a.area, a.box = area.data_ptr(), box.data_ptr()
    a.n, a.n_polys, a.n_vertices, a.H, a.W, a.pitch = 3, 3, 8, H, W, 16
    assert L.load().mtbt_fill_polygons(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    _check(["first", "second", "none"], out, area, box.float(), want)


def test_yolo_seg_planes_as_detections_and_ground_truth():
    rng = np.random.default_rng(3)
    sizes, rows = [(90, 140), (75, 66)], []
    for G in (3, 2):
        rows.append([[float(k % 2)] + R.circle(rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7), rng.uniform(0.1, 0.25), 9, k).reshape(-1).tolist()
                     for k in range(G)] + [[1.0, 0.1, 0.1, 0.9, 0.9]])                           # a two-point row is skipped
    gts, labels = zip(*[pp.yolo_seg_planes(r, H0, W0, DEV) for r, (H0, W0) in zip(rows, sizes)])
    for g, l, r, (H0, W0) in zip(gts, labels, rows, sizes):
        assert tuple(g.shape) == (len(r) - 1, H0, 8 * ((W0 + 63) // 64)) and l.dtype == torch.int64 and l.tolist() == [int(q[0]) for q in r[:-1]]
        for k in range(len(r) - 1):
            v = np.asarray(r[k][1:]).reshape(-1, 2) * [W0, H0]
            assert np.array_equal(g[k].cpu().numpy(), R.pack_bits(R.fill([v], H0, W0)))
    K = 3
    det_planes = [torch.cat([g, torch.zeros((K - g.shape[0],) + tuple(g.shape[1:]), dtype=torch.uint8, device=DEV)]) for g in gts]
    det = dict(masks_frame=det_planes, scores=torch.tensor([[0.9, 0.8, 0.7], [0.6, 0.5, 0.0]], device=DEV),
               labels=torch.stack([torch.cat([l, l.new_zeros(K - l.numel())]) for l in labels]),
               counts=torch.tensor([3, 2], dtype=torch.int32, device=DEV))
    m = DeviceMaskMeanAveragePrecision()
    m.update_batched(det, list(gts), list(labels))
    assert float(m.compute()["map"]) == 1.0
    empty, none = pp.yolo_seg_planes([], 20, 70, DEV)
    assert tuple(empty.shape) == (0, 20, 16) and none.numel() == 0


def _synthetic(rng, B):
    images, seg_rows, box_rows = [], [], []
    for i in range(B):
        H0, W0 = int(rng.integers(60, 200)), int(rng.integers(60, 200))
        images.append(torch.from_numpy(rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)).to(DEV))
        polys = [R.circle(rng.uniform(0.25, 0.75), rng.uniform(0.25, 0.75), rng.uniform(0.12, 0.3), int(rng.integers(3, 14)), k)
                 for k in range(1 + i % 3)]
        seg_rows.append([[float((i + k) % 2)] + p.reshape(-1).tolist() for k, p in enumerate(polys)])
        box_rows.append([[r[0], 0.5, 0.5, 0.2, 0.2] for r in seg_rows[-1]])
    return images, seg_rows, box_rows


def _check_samples(out, per_canvas, S):
    """(imgs, masks, gt_rows, inst) against the reference fill of the host-moved polygons: per_canvas[i] = [(row6, vertices, rect)]."""
    _, masks, gt_rows, inst = out
    items = [(i, it) for i, canvas in enumerate(per_canvas) for it in canvas]
    M, pitch = len(items), 8 * ((S + 63) // 64)
    assert M >= len(per_canvas)
    assert tuple(inst["planes"].shape) == (M, S, pitch) and inst["planes"].dtype == torch.uint8
    assert inst["image"].dtype == torch.int64 and inst["image"].tolist() == [i for i, _ in items]
    assert inst["labels"].dtype == torch.int64 and inst["labels"].tolist() == [int(it[0][1]) for _, it in items]
    assert torch.equal(gt_rows.cpu(), P.collate_boxes([[it[0] for it in canvas] for canvas in per_canvas])) and tuple(gt_rows.shape) == (M, 6)
    want = [R.fill([it[1]], S, S, it[2]) for _, it in items]
    assert np.array_equal(inst["planes"].cpu().numpy(), R.pack_bits(np.stack(want)))
    union = np.zeros((len(per_canvas), 1, S, S), dtype=np.float32)
    for (i, it), w in zip(items, want):
        union[i, 0] = np.maximum(union[i, 0], w)
        outside = np.ones((S, S), dtype=bool)
        outside[it[2][1]:it[2][3], it[2][0]:it[2][2]] = False
        assert not (w & outside).any()
    assert masks.dtype == torch.float32 and np.array_equal(masks.cpu().numpy(), union) and union.any()


def test_augment_samples_seg():
    S, kw = 128, dict(scale=(0.7, 1.6), aspect=0.2, fliplr=0.5, flipud=0.5, transpose=0.5)
    images, seg_rows, box_rows = _synthetic(np.random.default_rng(21), 4)
    out = P.augment_samples_seg(images, seg_rows, S, np.random.default_rng(77), **kw)
    imgs, _, _ = P.augment_samples(images, None, box_rows, S, np.random.default_rng(77), **kw)
    assert torch.equal(out[0], imgs)
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    geom = P.sample_geometry(sizes, S, np.random.default_rng(77), **kw)
    whole = (0, 0, S, S)
    per_canvas = [[(r6, v, whole) for r6, v in P.augment_polygons(r, W0, H0, geom[i], S)] for i, (r, (H0, W0)) in enumerate(zip(seg_rows, sizes))]
    _check_samples(out, per_canvas, S)


def test_mosaic_samples_seg():
    S, kw = 128, dict(prob=0.75, scale=(0.6, 1.2), fliplr=0.5, flipud=0.5, transpose=0.5)
    images, seg_rows, box_rows = _synthetic(np.random.default_rng(22), 4)
    out = P.mosaic_samples_seg(images, seg_rows, S, np.random.default_rng(78), **kw)
    imgs, _, _ = P.mosaic_samples(images, None, box_rows, S, np.random.default_rng(78), **kw)
    assert torch.equal(out[0], imgs)
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    index, geom, centres = P.sample_mosaic(sizes, S, np.random.default_rng(78), **kw)
    per_canvas = [P.mosaic_polygons([seg_rows[k] for k in index[i]], [sizes[k] for k in index[i]], geom[i], centres[i], S) for i in range(4)]
    assert any(tuple(c) != (S, S) for c in centres.tolist())            # at least one canvas is a real mosaic
    _check_samples(out, per_canvas, S)
    for (i, it), plane in zip([(i, it) for i, c in enumerate(per_canvas) for it in c], pp.unpack_masks(out[3]["planes"], S).cpu().numpy()):
        x0, y0, x1, y1 = it[2]
        assert it[2] in P.tile_rects(centres[i], S) and plane.sum() == plane[y0:y1, x0:x1].sum()      # zero outside its tile


def test_nothing_synchronises_with_the_host():
    S = 128
    images, seg_rows, _ = _synthetic(np.random.default_rng(24), 4)
    polys = [np.asarray(r[1:]).reshape(-1, 2) * S for rows in seg_rows for r in rows]
    calls = [lambda: pp.fill_polygons(polys, S, S, records=True, device=DEV),
             lambda: pp.yolo_seg_planes(seg_rows[2], 90, 140, DEV),
             lambda: P.augment_samples_seg(images, seg_rows, S, np.random.default_rng(80)),
             lambda: P.mosaic_samples_seg(images, seg_rows, S, np.random.default_rng(81))]
    for fn in calls:
        fn()                                                               # warm-up: the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [fn() for fn in calls]
        with pytest.raises(RuntimeError):                                  # positive control: the mode fires on this build
            outs[0][1][0].item()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert int(outs[0][1].sum()) > 0 and outs[2][3]["planes"].shape[0] == outs[2][2].shape[0]


def test_train_step_takes_the_polygon_ground_truth():
    S, B = 128, 2
    images, seg_rows, _ = _synthetic(np.random.default_rng(23), B)
    imgs, masks, gt_rows, inst = P.augment_samples_seg(images, seg_rows, S, np.random.default_rng(79), scale=(0.9, 1.2))
    assert gt_rows.shape[0] == inst["planes"].shape[0] >= 1
    torch.manual_seed(0)
    model = ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False).to(DEV).train()
    ts = TrainStep(model, (B, 3, S, S), optimizer="sgd", lr=0.01, iou_match_thresh=0.05, instance_mask_weight=1.0)
    loss = ts.step(imgs, gt_rows, masks, torch.tensor([1, 0], device=DEV))
    torch.cuda.synchronize()
    assert loss.shape == (10,) and bool(torch.isfinite(loss).all())


@pytest.mark.parametrize("H,W", [(7, 63), (9, 127)])
def test_one_padding_bit_in_the_last_word(H, W):
    """W % 64 == 63, below and above 64: one padding bit in the last word, where a wrong valid_bits shows: a rectangle that overshoots the plane on every side, a triangle into the last column, and the rectangle clipped
    to the last column alone; the caller's buffer is full of ones."""
    over = np.asarray([(-5.0, -5.0), (W + 5.0, -5.0), (W + 5.0, H + 5.0), (-5.0, H + 5.0)])
    tri = np.asarray([(W - 20.0, 0.0), (float(W), H / 2.0), (W - 20.0, float(H))])
    planes, rects = [over, tri, over], [(0, 0, W, H), (0, 0, W + 64, H), (W - 1, 0, W + 1, H)]
    want = [R.fill([p], H, W, r) for p, r in zip(planes, rects)]
    out = torch.full((3, H, 8 * ((W + 63) // 64)), 0xFF, dtype=torch.uint8, device=DEV)
    got, area, boxes = pp.fill_polygons(planes, H, W, clip=np.asarray(rects, dtype=np.int32), out=out, records=True)
    _check(["over", "triangle", "last column"], got, area, boxes, want)
    assert want[0].all() and want[1][:, W - 1].any() and int(want[2].sum()) == H
