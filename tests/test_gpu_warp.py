"""HIP affine warp (mtbt_warp_batch) against tests/warp_reference.py: bit-exact, since the rule is integer arithmetic up to a byte lookup and
one correctly rounded fp32 division.  The reference project has no augmentation; the rule is the project's own (include/mtbt_hip.h)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import polygon_reference as PR
from warp_reference import positions, warp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = np.float32(114) / np.float32(255)


def _sample(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), rng.integers(0, 256, size=(h, w), dtype=np.uint8)


def _forward(angle, scale, shear, S, h, w, shift=(0.0, 0.0), flip=False):
    t = math.radians(angle)
    lin = np.array([[math.cos(t), -math.sin(t)], [math.sin(t), math.cos(t)]]) @ np.array([[1.0, shear], [0.0, 1.0]]) * scale
    if flip:
        lin = lin @ np.diag([-1.0, 1.0])
    F = np.zeros((2, 3))
    F[:, :2] = lin
    F[:, 2] = np.array([S / 2 + shift[0], S / 2 + shift[1]]) - lin @ np.array([w / 2, h / 2])
    return F


def _maps(S, h, w):
    """(name, coefficient row): identity, quarter turn, 33 degrees with shear, strong shrink and zoom, a flip, wholly outside, and the
    coefficients at their magnitude limits (some of which still show the source: a = 2^26 walks 1024 source px per canvas px from c)."""
    from multitask_bonetumor_yolo_amd import preprocess as P
    k = lambda F: P.affine_coefficients(F)[0].tolist()
    s = S / max(h, w)
    lim, off = 1 << 26, 1 << 47
    return [
        ("identity", [65536, 0, 0, 0, 65536, 0, 0, 0]),
        ("quarter_turn", [0, 65536, 0, -65536, 0, (h - 1) << 16, 0, 0]),
        ("33_degrees_shear", k(_forward(33.0, 1.3 * s, 0.1, S, h, w))),
        ("scale_0.3", k(_forward(0.0, 0.3 * s, 0.0, S, h, w))),
        ("scale_3", k(_forward(-12.0, 3.0 * s, 0.0, S, h, w))),
        ("flip", k(_forward(20.0, 1.1 * s, -0.2, S, h, w, flip=True))),
        ("outside", k(_forward(33.0, 1.3 * s, 0.1, S, h, w, shift=(3.0 * S, -2.0 * S)))),
        ("limits_far", [lim, -lim, off, -lim, lim, -off, 0, 0]),
        ("limits_near", [lim, lim, -lim * (S // 2), -lim, -lim, lim * (S // 2), 0, 0]),
        ("limits_offset_back", [-lim, 0, off, 0, lim, -off, 0, 0]),
    ]


@pytest.mark.parametrize("S", [32, 64])
@pytest.mark.parametrize("size", [(37, 53), (5, 7), (1, 1)])
def test_warp_matches_reference(size, S):
    from multitask_bonetumor_yolo_amd import preprocess as P
    img, mask = _sample(*size, seed=size[0] * 131 + size[1])
    maps = _maps(S, *size)
    n = len(maps)
    coef = np.array([row for _, row in maps], dtype=np.int64)
    lut = np.random.default_rng(7).integers(0, 256, size=(n, 3, 256), dtype=np.uint8)
    di, dm = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    x0, m0 = P.warp_batch([di] * n, [dm] * n, coef, None, S)
    x1, m1 = P.warp_batch([di] * n, None, coef, torch.from_numpy(lut).to(DEV), S)
    torch.cuda.synchronize()
    assert x0.shape == (n, 3, S, S) and m0.shape == (n, 1, S, S) and x0.dtype == m0.dtype == torch.float32
    assert not m1.any()                                                         # no mask in the descriptor: zeros
    shown = {}
    for i, (name, row) in enumerate(maps):
        rx, rm = warp(img, mask, row, S)
        assert torch.equal(x0[i].cpu(), torch.from_numpy(rx)) and torch.equal(m0[i].cpu(), torch.from_numpy(rm)), f"{size} {name}"
        rx1, _ = warp(img, None, row, S, lut=lut[i])
        assert torch.equal(x1[i].cpu(), torch.from_numpy(rx1)), f"{size} {name} with a table"
        shown[name] = int(positions(row, S, *size)[2].sum())
    # the cases are what their names say: canvas pixels that show the source
    assert shown["identity"] == min(size[0], S) * min(size[1], S) == shown["quarter_turn"]
    assert shown["outside"] == 0 and shown["limits_far"] == 0 and (x1[[name for name, _ in maps].index("outside")] == float(PAD)).all()
    assert shown["limits_near"] == S // 2 + 1                                   # pixel (0, 0) of the source along dx + dy == S / 2
    assert shown["scale_3"] == S * S and 0 < shown["33_degrees_shear"] < S * S and 0 < shown["scale_0.3"] < S * S // 4 and shown["flip"] > 0


def test_row_strided_view_and_a_batch_that_mixes_masks():
    from multitask_bonetumor_yolo_amd import preprocess as P
    S = 32
    wide = torch.from_numpy(np.random.default_rng(9).integers(0, 256, size=(40, 90, 3), dtype=np.uint8)).to(DEV)
    wmask = torch.from_numpy(np.random.default_rng(10).integers(0, 256, size=(40, 90), dtype=np.uint8)).to(DEV)
    imgs = [wide[3:, 10 * i: 10 * i + 23 + i] for i in range(5)]                 # views with a 270-byte row stride
    masks = [None if i % 2 else wmask[3:, 10 * i: 10 * i + 23 + i] for i in range(5)]   # 90-byte mask rows
    assert all(not im.is_contiguous() for im in imgs)
    rng = np.random.default_rng(4)
    coef = P.affine_coefficients(P.sample_affine([tuple(a.shape[:2]) for a in imgs], S, rng, scale=(0.5, 2.0), aspect=0.3, degrees=180.0,
                                                 shear=15.0, translate=0.2, flipud=0.5))
    lut = P.sample_photometric(5, rng)
    x, m = P.warp_batch(imgs, masks, coef, torch.from_numpy(lut).to(DEV), S)
    torch.cuda.synchronize()
    for i in range(5):
        rx, rm = warp(imgs[i].cpu().numpy(), None if masks[i] is None else masks[i].cpu().numpy(), coef[i], S, lut=lut[i])
        assert torch.equal(x[i].cpu(), torch.from_numpy(rx)) and torch.equal(m[i].cpu(), torch.from_numpy(rm)), i
        assert (masks[i] is None) == (not m[i].any())


def test_more_canvases_than_one_launch_holds():
    """count == chunk + 1 at S = 16: the second launch reads its descriptor, coefficients and table and writes its outputs at `first`."""
    from multitask_bonetumor_yolo_amd import _lib as L
    from multitask_bonetumor_yolo_amd import preprocess as P
    S, n = 16, L.WARP_CHUNK + 1
    rng = np.random.default_rng(12)
    srcs = [_sample(9 + i % 5, 11 + i % 7, 100 + i) for i in range(n)]
    di, dm = [torch.from_numpy(a).to(DEV) for a, _ in srcs], [torch.from_numpy(b).to(DEV) for _, b in srcs]
    coef = P.affine_coefficients(P.sample_affine([a.shape[:2] for a, _ in srcs], S, rng, degrees=180.0, shear=10.0, scale=(0.7, 1.5)))
    lut = rng.integers(0, 256, size=(n, 3, 256), dtype=np.uint8)
    x, m = P.warp_batch(di, dm, coef, torch.from_numpy(lut).to(DEV), S)
    torch.cuda.synchronize()
    for i in range(n):
        rx, rm = warp(srcs[i][0], srcs[i][1], coef[i], S, lut=lut[i])
        assert torch.equal(x[i].cpu(), torch.from_numpy(rx)) and torch.equal(m[i].cpu(), torch.from_numpy(rm)), i
    assert (x[n - 1] != float(PAD)).any()


def test_empty_batch_and_no_mask_output():
    from multitask_bonetumor_yolo_amd import _lib as L
    from multitask_bonetumor_yolo_amd import preprocess as P
    lib = L.load()
    S = 32
    img, mask = _sample(20, 30, 3)
    di, dm = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    descs, keep, _ = P._descriptors([di], [dm], "test")
    coef = P.affine_coefficients(_forward(33.0, 1.0, 0.1, S, 20, 30))
    kp = coef.ctypes.data_as(C.POINTER(C.c_int64))
    out = torch.full((1, 3, S, S), -1.0, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mtbt_warp_batch(descs, 0, S, kp, 8, None, out.data_ptr(), None, stream) == 0       # count == 0: nothing is written
    torch.cuda.synchronize()
    assert (out == -1.0).all()
    assert lib.mtbt_warp_batch(descs, 1, S, kp, 8, None, out.data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    rx, _ = warp(img, mask, coef[0], S)
    assert torch.equal(out[0].cpu(), torch.from_numpy(rx))                                         # out_masks = NULL: the image alone


def _synthetic(rng, n):
    """n small images, two polygons each (a blob and a triangle, as YOLO-seg rows) and their boxes as YOLO-txt rows."""
    images, seg_rows, box_rows = [], [], []
    for i in range(n):
        h, w = int(rng.integers(40, 90)), int(rng.integers(40, 90))
        images.append(torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).to(DEV))
        blob = PR.circle(0.45 + 0.1 * rng.random(), 0.5, 0.22, 9, phase=rng.random())
        tri = np.array([[0.2, 0.25], [0.8, 0.3], [0.55, 0.8]]) + rng.uniform(-0.05, 0.05, (3, 2))
        seg, box = [], []
        for cls, poly in ((i % 3, blob), (2, tri)):
            seg.append([cls] + poly.reshape(-1).tolist())
            (x1, y1), (x2, y2) = poly.min(axis=0), poly.max(axis=0)
            box.append([cls, (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1])
        seg_rows.append(seg)
        box_rows.append(box)
    return images, seg_rows, box_rows


def test_affine_samples_seg_end_to_end():
    import multitask_bonetumor_yolo_amd as pkg
    from multitask_bonetumor_yolo_amd import postprocess as pp
    P = pkg.preprocess
    S, kw = 64, dict(scale=(0.8, 1.1), degrees=40.0, shear=5.0, translate=0.05, flipud=0.5)
    images, seg_rows, _ = _synthetic(np.random.default_rng(21), 2)
    imgs, masks, gt_rows, inst = pkg.affine_samples_seg(images, seg_rows, S, np.random.default_rng(77), **kw)
    torch.cuda.synchronize()
    # the same draws by hand: the map, then the tables, from one generator
    rng = np.random.default_rng(77)
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    coef = P.affine_coefficients(P.sample_affine(sizes, S, rng, **kw))
    lut = P.sample_photometric(2, rng)
    for i in range(2):
        rx, _ = warp(images[i].cpu().numpy(), None, coef[i], S, lut=lut[i])
        assert torch.equal(imgs[i].cpu(), torch.from_numpy(rx))
    Fq = P.affine_forward(coef)
    items = [(i, it) for i, (r, (h, w)) in enumerate(zip(seg_rows, sizes)) for it in P.affine_polygons(r, w, h, Fq[i], S)]
    M = len(items)
    assert M == 4 and tuple(gt_rows.shape) == (M, 6) and gt_rows.is_cuda
    assert torch.equal(gt_rows.cpu(), P.collate_boxes([[it[0] for k, it in items if k == i] for i in range(2)]))
    assert inst["image"].tolist() == [i for i, _ in items] and inst["labels"].tolist() == [int(it[0][1]) for _, it in items]
    want = np.stack([PR.fill([it[1]], S, S) for _, it in items])
    assert np.array_equal(inst["planes"].cpu().numpy(), PR.pack_bits(want))       # row for row with gt_rows
    planes = pp.unpack_masks(inst["planes"], S).cpu().numpy().astype(bool)
    for m, (i, it) in enumerate(items):       # every pixel centre of a plane lies in its row's box (the fill quantises vertices to 1/16 px)
        ys, xs = np.nonzero(planes[m])
        cx, cy, bw, bh = (float(v) * S for v in it[0][2:])
        assert len(xs) > 20 and cx - bw / 2 - 1 / 16 <= xs.min() + 0.5 and xs.max() + 0.5 <= cx + bw / 2 + 1 / 16
        assert cy - bh / 2 - 1 / 16 <= ys.min() + 0.5 and ys.max() + 0.5 <= cy + bh / 2 + 1 / 16
    union = np.zeros((2, 1, S, S), dtype=np.float32)
    for m, (i, _) in enumerate(items):
        union[i, 0] = np.maximum(union[i, 0], planes[m])
    assert masks.dtype == torch.float32 and np.array_equal(masks.cpu().numpy(), union) and union.any()


def test_affine_samples_with_raster_masks():
    import multitask_bonetumor_yolo_amd as pkg
    P = pkg.preprocess
    S, kw = 64, dict(scale=(0.8, 1.2), aspect=0.1, degrees=30.0, shear=5.0, flipud=0.5)
    images, seg_rows, box_rows = _synthetic(np.random.default_rng(23), 3)
    sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
    masks_np = [PR.fill([np.asarray(r[1:]).reshape(-1, 2) * [w, h] for r in rows], h, w).astype(np.uint8) * 255 for rows, (h, w) in zip(seg_rows, sizes)]
    dm = [torch.from_numpy(m).to(DEV) for m in masks_np]
    dm[1] = None
    x, m, gt = pkg.affine_samples(images, dm, box_rows, S, np.random.default_rng(5), **kw)
    x2, m2, gt2 = pkg.affine_samples(images, dm, box_rows, S, np.random.default_rng(5), **kw)
    torch.cuda.synchronize()
    for t, shape in ((x, (3, 3, S, S)), (m, (3, 1, S, S))):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
    assert torch.equal(x, x2) and torch.equal(m, m2) and torch.equal(gt, gt2)
    rng = np.random.default_rng(5)
    coef = P.affine_coefficients(P.sample_affine(sizes, S, rng, **kw))
    lut = P.sample_photometric(3, rng)
    for i in range(3):
        rx, rm = warp(images[i].cpu().numpy(), None if dm[i] is None else masks_np[i], coef[i], S, lut=lut[i])
        assert torch.equal(x[i].cpu(), torch.from_numpy(rx)) and torch.equal(m[i].cpu(), torch.from_numpy(rm)), i
    assert m[0].any() and not m[1].any() and m[2].any()
    Fq = P.affine_forward(coef)
    want = P.collate_boxes([P.affine_yolo_labels(r, w, h, Fq[i], S) for i, (r, (h, w)) in enumerate(zip(box_rows, sizes))])
    assert torch.equal(gt.cpu(), want) and gt.is_cuda and want.shape[0] >= 3
    with pytest.raises(TypeError):
        pkg.affine_samples(images, dm, box_rows, S, np.random.default_rng(0), transpose=0.5)
