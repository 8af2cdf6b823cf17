"""HIP training augmentation (mtbt_augment_batch) against tests/augment_reference.py: bit-exact, since everything past the
coefficient set-up is integer arithmetic, the table is a byte lookup and the /255 is one correctly rounded fp32 division.  The
reference project has no augmentation; the arithmetic is the project's own definition (include/mtbt_hip.h)."""
import numpy as np
import pytest
import torch

from augment_reference import augment

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SOURCES = [(1, 5), (5, 1), (2, 2), (64, 63), (129, 127), (37, 91)]


def _sample(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), rng.integers(0, 256, size=(h, w), dtype=np.uint8)


def _geometries(S):
    """Every orientation x resized sizes (1, below S, S, 2.3 S, mixed) x offsets (0, positive, negative down to one visible row / column,
    one corner pixel at the far edge, wholly outside on each side)."""
    big = int(2.3 * S)
    rows = []
    for orient in range(8):
        for nw, nh in ((1, 1), (1, S - 24), (S - 20, S - 30), (S, S), (big, big), (big, S - 30), (S - 1, big)):
            qw, qh = (nh, nw) if orient & 4 else (nw, nh)
            for ox, oy in ((0, 0), (7, 5), (-3, 9), (-(qw - 1), -(qh - 1)), (-(qw // 2), -(qh - 1)), (S - 1, S - 1), (-qw, 0), (0, -qh), (S, 0), (3, S + 40),
                           (-100000, 2)):
                rows.append([nw, nh, ox, oy, orient, 0, 0, 0])
    return np.array(rows, dtype=np.int32)


@pytest.mark.parametrize("size", SOURCES)
def test_augment_matches_reference(size):
    from multitask_bonetumor_yolo_amd import preprocess as P
    S = 64
    img, mask = _sample(*size, seed=size[0] * 131 + size[1])
    geom = _geometries(S)
    n = len(geom)
    lut = np.random.default_rng(7).integers(0, 256, size=(n, 3, 256), dtype=np.uint8)
    di, dm = torch.from_numpy(img).to(DEV), torch.from_numpy(mask).to(DEV)
    x0, m0 = P.augment_batch([di] * n, [dm] * n, geom, None, S)
    x1, m1 = P.augment_batch([di] * n, [dm] * n, geom, torch.from_numpy(lut).to(DEV), S)
    torch.cuda.synchronize()
    assert x0.shape == (n, 3, S, S) and m0.shape == (n, 1, S, S) and x0.dtype == m0.dtype == torch.float32
    x0, m0, x1, m1 = (t.cpu().numpy() for t in (x0, m0, x1, m1))
    for i, g in enumerate(geom):
        rx, rm = augment(img, mask, g, S)
        assert np.array_equal(x0[i], rx) and np.array_equal(m0[i], rm), f"{size} geom {g.tolist()}"
        rx, rm = augment(img, mask, g, S, lut=lut[i])
        assert np.array_equal(x1[i], rx) and np.array_equal(m1[i], rm), f"{size} geom {g.tolist()} with a table"


@pytest.mark.parametrize("S,sizes", [(64, SOURCES), (640, [(480, 640), (1000, 700)])])
def test_identity_geometry_is_letterbox_batch(S, sizes):
    from multitask_bonetumor_yolo_amd import preprocess as P
    imgs, masks = zip(*[_sample(h, w, i) for i, (h, w) in enumerate(sizes)])
    di, dm = [torch.from_numpy(a).to(DEV) for a in imgs], [torch.from_numpy(a).to(DEV) for a in masks]
    x, m, _ = P.letterbox_batch(di, dm, S)
    ax, am = P.augment_batch(di, dm, P.letterbox_geometry(sizes, S), None, S)
    torch.cuda.synchronize()
    assert torch.equal(ax, x) and torch.equal(am, m)


def test_augment_many_images_strided_rows_and_missing_mask():
    from multitask_bonetumor_yolo_amd import preprocess as P
    S = 32
    wide = torch.from_numpy(np.random.default_rng(9).integers(0, 256, size=(40, 90, 3), dtype=np.uint8)).to(DEV)
    imgs = [wide[:, 10 * (i % 5): 10 * (i % 5) + 20 + i] for i in range(35)]     # views with a 270-byte row stride; > 32 images
    masks = [None if i % 2 else (wide[:, :, 0] > 99).to(torch.uint8)[:, 10 * (i % 5): 10 * (i % 5) + 20 + i] * 255 for i in range(35)]
    rng = np.random.default_rng(4)
    geom = P.sample_geometry([tuple(a.shape[:2]) for a in imgs], S, rng, scale=(0.4, 2.5), aspect=0.3, fliplr=0.5, flipud=0.5, transpose=0.5)
    lut = P.sample_photometric(35, rng)
    x, m = P.augment_batch(imgs, masks, geom, torch.from_numpy(lut).to(DEV), S)
    torch.cuda.synchronize()
    assert set(geom[:, 4].tolist()) >= {0, 4} and geom[32:, :2].min() >= 1
    for i in range(35):
        rx, rm = augment(imgs[i].cpu().numpy(), None if masks[i] is None else masks[i].cpu().numpy(), geom[i], S, lut=lut[i])
        assert np.array_equal(x[i].cpu().numpy(), rx) and np.array_equal(m[i].cpu().numpy(), rm), (i, geom[i].tolist())


def test_augment_samples_output_contract():
    import multitask_bonetumor_yolo_amd as pkg
    S, sizes = 64, [(90, 60), (50, 120), (64, 64)]
    imgs, masks = zip(*[_sample(h, w, i) for i, (h, w) in enumerate(sizes)])
    di, dm = [torch.from_numpy(a).to(DEV) for a in imgs], [torch.from_numpy(a).to(DEV) for a in masks]
    rows = [[[1, 0.5, 0.5, 0.6, 0.6], [0, 0.3, 0.4, 0.3, 0.5]], [], [[0, 0.5, 0.5, 0.9, 0.9]]]
    kw = dict(scale=(0.8, 1.2), aspect=0.1, flipud=0.5, transpose=0.5)
    x, m, gt = pkg.augment_samples(di, dm, rows, S, np.random.default_rng(21), **kw)
    x2, m2, gt2 = pkg.augment_samples(di, dm, rows, S, np.random.default_rng(21), **kw)
    torch.cuda.synchronize()
    for t, shape in ((x, (3, 3, S, S)), (m, (3, 1, S, S))):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape
    assert gt.is_cuda and gt.dtype == torch.float32 and gt.dim() == 2 and gt.shape[1] == 6 and 1 <= gt.shape[0] <= 3
    assert set(gt[:, 0].tolist()) <= {0.0, 2.0} and bool(((gt[:, 2:] >= 0) & (gt[:, 2:] <= 1)).all())
    assert torch.equal(x, x2) and torch.equal(m, m2) and torch.equal(gt, gt2)
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0 and set(m.unique().tolist()) <= {0.0, 1.0}
    # the same draws by hand: geometry, then the tables, from one generator
    rng = np.random.default_rng(21)
    geom = pkg.sample_geometry(sizes, S, rng, **kw)
    lut = pkg.sample_photometric(3, rng)
    for i in range(3):
        rx, rm = augment(imgs[i], masks[i], geom[i], S, lut=lut[i])
        assert np.array_equal(x[i].cpu().numpy(), rx) and np.array_equal(m[i].cpu().numpy(), rm)
    want = pkg.preprocess.collate_boxes([pkg.augment_yolo_labels(r, W0, H0, geom[i], S) for i, (r, (H0, W0)) in enumerate(zip(rows, sizes))])
    assert torch.equal(gt.cpu(), want)
    with pytest.raises(TypeError):
        pkg.augment_samples(di, dm, rows, S, np.random.default_rng(0), mosaic=1.0)


def test_augment_rejects_bad_input():
    from multitask_bonetumor_yolo_amd import preprocess as P
    good = np.array([[4, 4, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    ok = torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        P.augment_batch([torch.zeros(4, 4, 3, dtype=torch.uint8)], None, good, None, 64)            # CPU tensor: no CPU path
    with pytest.raises(ValueError):
        P.augment_batch([torch.zeros(4, 4, 3, device=DEV)], None, good, None, 64)                   # not uint8
    with pytest.raises(RuntimeError):
        P.augment_batch([ok], None, good, None, 62)                                                 # S % 4
    bad = good.copy()
    bad[0, 4] = 8
    with pytest.raises(RuntimeError):
        P.augment_batch([ok], None, bad, None, 64)                                                  # orient = 8
    with pytest.raises(ValueError):
        P.augment_batch([ok], None, good[:, :7], None, 64)                                          # not [B, 8]
    with pytest.raises(ValueError):
        P.augment_batch([ok], None, good.astype(np.float32), None, 64)                              # not integers
    with pytest.raises(ValueError):
        P.augment_batch([ok], None, good, torch.zeros(1, 3, 256, dtype=torch.uint8), 64)            # table on the host


def test_null_mask_output_of_the_three_entry_points():
    """out_masks == NULL (and, for the letterbox, out_scales == NULL) through the C entry points themselves -- the Python wrappers always
    pass a mask buffer: the images are bit-equal to the wrappers'."""
    import ctypes as C
    from multitask_bonetumor_yolo_amd import _lib as L
    from multitask_bonetumor_yolo_amd import preprocess as P
    S, n = 64, 8
    lib = L.load()
    imgs, masks = zip(*[_sample(h, w, seed=h * 131 + w) for h, w in SOURCES])
    di, dm = [torch.from_numpy(a).to(DEV) for a in imgs], [torch.from_numpy(a).to(DEV) for a in masks]
    src = [i % len(SOURCES) for i in range(n)]
    bi, bm = [di[k] for k in src], [dm[k] for k in src]
    sizes = [(S - 20, S - 30), (int(2.3 * S), S - 30), (S, S), (1, S - 24), (S - 1, int(2.3 * S)), (S - 20, S - 30), (S, S), (int(2.3 * S), int(2.3 * S))]
    offsets = [(0, 0), (-10, 5), (7, -3), (3, 2), (-9, -70), (30, 40), (-1, -1), (-40, -50)]
    geom = np.array([[nw, nh, ox, oy, orient, 0, 0, 0] for orient, ((nw, nh), (ox, oy)) in enumerate(zip(sizes, offsets))], dtype=np.int32)
    assert set(geom[:, 4].tolist()) == set(range(8))
    lut = torch.from_numpy(np.random.default_rng(7).integers(0, 256, size=(n, 3, 256), dtype=np.uint8)).to(DEV)
    index = np.array([[0, 1, 2, 3], [4, 5, 0, 1], [3, 4, 5, 2]])
    mgeom = np.stack([geom[[0, 1, 2, 3]], geom[[4, 5, 6, 7]], geom[[7, 2, 5, 0]]])
    centres = np.array([[32, 17], [0, 0], [64, 64]], dtype=np.int32)

    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    descs, keep, _ = P._descriptors(bi, bm, "test")
    got = {k: torch.full((b, 3, S, S), -1.0, device=DEV) for k, b in (("letterbox", n), ("augment", n), ("augment+table", n), ("mosaic", 3), ("mosaic+table", 3))}
    assert lib.mtbt_letterbox_batch(descs, n, S, got["letterbox"].data_ptr(), None, None, stream) == 0
    g = i32(geom)
    assert lib.mtbt_augment_batch(descs, n, S, g, 8, None, got["augment"].data_ptr(), None, stream) == 0
    assert lib.mtbt_augment_batch(descs, n, S, g, 8, lut.data_ptr(), got["augment+table"].data_ptr(), None, stream) == 0
    sdescs, skeep, _ = P._descriptors(di, dm, "test")
    tiles = (L.RawImage * 12)()
    for k, s in enumerate(index.reshape(-1)):
        tiles[k] = sdescs[int(s)]
    mg, mc = i32(mgeom), i32(centres)
    assert lib.mtbt_mosaic_batch(tiles, 3, S, mg, 8, mc, None, got["mosaic"].data_ptr(), None, stream) == 0
    assert lib.mtbt_mosaic_batch(tiles, 3, S, mg, 8, mc, lut.data_ptr(), got["mosaic+table"].data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    want = {"letterbox": P.letterbox_batch(bi, bm, S)[0], "augment": P.augment_batch(bi, bm, geom, None, S)[0],
            "augment+table": P.augment_batch(bi, bm, geom, lut, S)[0], "mosaic": P.mosaic_batch(di, dm, index, mgeom, centres, None, S)[0],
            "mosaic+table": P.mosaic_batch(di, dm, index, mgeom, centres, lut[:3], S)[0]}
    torch.cuda.synchronize()
    for k in got:
        assert torch.equal(got[k], want[k]), k
