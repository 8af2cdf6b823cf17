"""HIP CLAHE (mtbt_clahe_batch, csrc/clahe.hip) against tests/clahe_reference.py, bit for bit: the rule is exact in integers
(include/mtbt_hip.h), so every output byte must equal the reference's."""
import ctypes as C

import numpy as np
import pytest
import torch

import clahe_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pre():
    from multitask_bonetumor_yolo_amd import preprocess as P
    return P


def noisy(rng, H, W, ch):
    """Smooth structure plus noise and a flat dark corner: every tile has its own histogram, some heavily clipped."""
    y, x = np.mgrid[0:H, 0:W]
    v = 60 + 120 * np.sin(x / 5.0) * np.cos(y / 7.0) + rng.integers(-40, 41, (H, W))
    v[: H // 3, : W // 3] = 7
    g = np.clip(v, 0, 255).astype(np.uint8)
    if ch == 1:
        return g
    return np.ascontiguousarray(np.stack([g, np.clip(g.astype(int) + rng.integers(-20, 21, (H, W)), 0, 255).astype(np.uint8),
                                          rng.integers(0, 256, (H, W)).astype(np.uint8)], axis=-1))


def expect(img, limit, grid):
    return R.clahe(img, grid, _pre().clahe_clip(limit, img.shape[0], img.shape[1], grid))


def differing(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} of {ref.size} bytes differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, reference {ref[tuple(bad[0])]}" if len(bad) else ""


def run_and_check(imgs, limits, grid):
    P = _pre()
    dev = [torch.from_numpy(a).to(DEV) for a in imgs]
    out = P.clahe_batch(dev, limits, grid)
    torch.cuda.synchronize()
    limits = limits if isinstance(limits, list) else [limits] * len(imgs)
    for i, (a, d, o, lim) in enumerate(zip(imgs, dev, out, limits)):
        assert o.shape == d.shape and o.dtype == torch.uint8 and o.is_contiguous()
        assert torch.equal(d.cpu(), torch.from_numpy(a)), "the source was written"
        msg = differing(o.cpu().numpy(), expect(a, lim, grid))
        assert not msg, f"image {i} {a.shape} grid {grid} limit {lim}: {msg}"


# H x W, grid (gx, gy): reflection on both axes with rows of 159 bytes; tiles of one pixel; one tile; many small tiles; a strip; tiles
# that one workgroup does not cover (640 x 512 at 2 x 2: 256 x 320 pixels each); tiles that lie wholly in the extension (17 wide at 16)
SHAPES = [(37, 53, (4, 3)), (16, 16, (16, 16)), (40, 40, (1, 1)), (33, 70, (8, 8)), (5, 300, (16, 1)), (640, 512, (2, 2)), (20, 17, (16, 7))]


@pytest.mark.parametrize("H,W,grid", SHAPES)
def test_shapes_one_and_three_channels(H, W, grid):
    rng = np.random.default_rng(H * 1000 + W)
    run_and_check([noisy(rng, H, W, 1), noisy(rng, H, W, 3)], 2.0, grid)


def test_clip_values():
    P = _pre()
    H, W, grid = 37, 53, (4, 3)
    area = 14 * 13
    limits = [0.0, 0.001, 6.0, 256.0, 1000.0]
    assert [P.clahe_clip(v, H, W, grid) for v in limits] == [0, 1, 4, area, 710]      # none, 1, a middle value, the area, beyond it
    rng = np.random.default_rng(5)
    run_and_check([noisy(rng, H, W, 1 + 2 * (i % 2)) for i in range(len(limits))], limits, grid)
    run_and_check([noisy(rng, 96, 128, 1)] * 3, [0.0, 40.0, 3.0], (2, 2))              # tiles of 64 x 48: clips 0, 480, 36


def test_radiograph_1536_by_2048():
    img = R.radiograph(np.random.default_rng(1), 1536, 2048, 3)
    assert (img == 0).mean() > 0.3                                                    # mostly background: one bin takes most of many tiles
    run_and_check([img], 2.0, (8, 8))


def test_constant_and_two_level_images():
    """Every pixel of a tile in one or two bins: all lanes of the histogram pass add to the same LDS word."""
    two = np.zeros((256, 512), dtype=np.uint8)
    two[100:140, 200:330] = 255
    two3 = np.ascontiguousarray(np.stack([two, two, two], axis=-1))
    two3[::3, 1::2, 1] = 9                                                            # runs that end inside a 16-pixel group
    const = np.full((200, 300, 3), 0, dtype=np.uint8)
    const1 = np.full((123, 457), 255, dtype=np.uint8)
    run_and_check([two, two3, const, const1], [2.0, 2.0, 0.0, 1.0], (4, 4))
    P = _pre()
    out = P.clahe_batch([torch.from_numpy(const).to(DEV)], 0.0, (4, 4))[0]
    assert (out == 255).all()


def test_row_strided_source_and_destination_leave_the_padding_alone():
    P = _pre()
    rng = np.random.default_rng(8)
    for ch in (1, 3):
        base = rng.integers(0, 256, (40, 100) + ((3,) if ch == 3 else ()), dtype=np.uint8)
        view = np.ascontiguousarray(base[:37, 11:64])                                  # 37 x 53 inside rows of 100 pixels
        ref = expect(view, 3.0, (4, 3))
        d_base = torch.from_numpy(base).to(DEV)
        o_base = torch.full((40, 128) + ((3,) if ch == 3 else ()), 0xAB, dtype=torch.uint8, device=DEV)
        # strided source into a new tensor (source and destination rows are not congruent modulo 16), and into a strided destination
        got = P.clahe_batch([d_base[:37, 11:64]], 3.0, (4, 3))[0]
        ret = P.clahe_batch([d_base[:37, 11:64]], 3.0, (4, 3), out=[o_base[2:39, 5:58]])[0]
        torch.cuda.synchronize()
        assert ret.data_ptr() == o_base[2:39, 5:58].data_ptr()
        assert not differing(got.cpu().numpy(), ref) and not differing(o_base[2:39, 5:58].cpu().numpy(), ref)
        rest = o_base.clone()
        rest[2:39, 5:58] = 0xAB
        assert (rest == 0xAB).all(), "bytes outside the destination's rows were written"
        assert torch.equal(d_base.cpu(), torch.from_numpy(base))


def test_in_place():
    P = _pre()
    rng = np.random.default_rng(9)
    a, b = noisy(rng, 70, 90, 3), noisy(rng, 64, 64, 1)
    base = rng.integers(0, 256, (50, 120, 3), dtype=np.uint8)
    da, db, dbase = (torch.from_numpy(x).to(DEV) for x in (a, b, base))
    view = dbase[3:48, 7:100]
    imgs = [da, db, view]
    out = P.clahe_batch(imgs, [2.0, 4.0, 1.0], (5, 3), out=imgs)
    torch.cuda.synchronize()
    assert all(o.data_ptr() == i.data_ptr() for o, i in zip(out, imgs))
    assert not differing(da.cpu().numpy(), expect(a, 2.0, (5, 3))) and not differing(db.cpu().numpy(), expect(b, 4.0, (5, 3)))
    want = base.copy()
    want[3:48, 7:100] = expect(np.ascontiguousarray(base[3:48, 7:100]), 1.0, (5, 3))
    assert not differing(dbase.cpu().numpy(), want)                                    # the view is equalised, the rest of its rows is not


def test_batch_of_33_mixed_images_and_untouched_ones():
    P = _pre()
    rng = np.random.default_rng(10)
    imgs = [noisy(rng, 9 + 3 * i, 70 - 2 * i + (i % 5), 1 + 2 * (i % 2)) for i in range(33)] + [noisy(rng, 30, 30, 1)]
    limits = [[0.0, 2.0, 8.0][i % 3] for i in range(33)] + [None]
    dev = [torch.from_numpy(a).to(DEV) for a in imgs]
    out = P.clahe_batch(dev, limits, (3, 2))
    torch.cuda.synchronize()
    assert out[33] is dev[33]                                                          # None: the tensor itself
    for i in range(33):
        msg = differing(out[i].cpu().numpy(), expect(imgs[i], limits[i], (3, 2)))
        assert not msg, f"image {i} {imgs[i].shape}: {msg}"


def test_two_calls_share_a_workspace_on_one_stream():
    from multitask_bonetumor_yolo_amd import _lib as L
    P = _pre()
    lib = L.load()
    rng = np.random.default_rng(11)
    grid = (4, 4)
    first, second = [noisy(rng, 100, 130, 3), noisy(rng, 64, 80, 1)], [noisy(rng, 90, 75, 1), noisy(rng, 120, 100, 3)]
    src = [[torch.from_numpy(a).to(DEV) for a in batch] for batch in (first, second)]
    dst = [[torch.empty_like(t) for t in batch] for batch in src]
    descs = []
    for s_batch, d_batch in zip(src, dst):
        arr = (L.ClaheImage * 2)()
        for d, s, o in zip(arr, s_batch, d_batch):
            d.src, d.dst, d.height, d.width, d.channels = s.data_ptr(), o.data_ptr(), s.shape[0], s.shape[1], 1 if s.dim() == 2 else 3
            d.clip, d.src_row_stride, d.dst_row_stride = P.clahe_clip(2.0, s.shape[0], s.shape[1], grid), s.stride(0), o.stride(0)
        descs.append(arr)
    nbytes = lib.mtbt_clahe_workspace_bytes(descs[0], 2, *grid)
    assert nbytes == 2 * 16 * 1280
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for arr in descs:                                                                  # back to back, nothing in between
        assert lib.mtbt_clahe_batch(arr, 2, *grid, ws.data_ptr(), nbytes, stream) == 0
    torch.cuda.synchronize()
    for batch, outs in zip((first, second), dst):
        for a, o in zip(batch, outs):
            assert not differing(o.cpu().numpy(), expect(a, 2.0, grid))
    assert lib.mtbt_clahe_batch(descs[0], 2, *grid, ws.data_ptr() + 8, nbytes, stream) == -2       # the workspace's alignment


def test_clahe_then_letterbox_is_letterbox_of_the_reference():
    P = _pre()
    rng = np.random.default_rng(12)
    raw = [noisy(rng, 200, 150, 3), noisy(rng, 96, 300, 3)]
    dev = [torch.from_numpy(a).to(DEV) for a in raw]
    got, _, scales = P.letterbox_batch(P.clahe_batch(dev), None, 128)
    want, _, scales_ref = P.letterbox_batch([torch.from_numpy(expect(a, 2.0, (8, 8))).to(DEV) for a in raw], None, 128)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and scales == scales_ref
    plain, _, _ = P.letterbox_batch(dev, None, 128)
    assert not torch.equal(got, plain)


def test_augment_samples_with_clahe_is_augment_batch_over_reference_sources():
    P = _pre()
    rng = np.random.default_rng(13)
    raw = [noisy(rng, 120, 90, 3), noisy(rng, 64, 160, 3), noisy(rng, 77, 77, 3), noisy(rng, 50, 40, 3)]
    rows = [[[0, 0.5, 0.5, 0.4, 0.3]], [], [[1, 0.3, 0.6, 0.2, 0.2]], []]
    dev = [torch.from_numpy(a).to(DEV) for a in raw]
    opts = dict(prob=0.7, clip=(1.0, 4.0), grid=(4, 3))
    imgs, masks, gt = P.augment_samples(dev, None, rows, 96, np.random.default_rng(95), clahe=opts)
    again = np.random.default_rng(95)                                                  # the same draws, in the documented order
    sizes = [a.shape[:2] for a in raw]
    geom = P.sample_geometry(sizes, 96, again)
    lut = torch.from_numpy(P.sample_photometric(4, again)).to(DEV)
    limits = P.sample_clahe(4, again, prob=0.7, clip=(1.0, 4.0))
    assert any(v is None for v in limits) and any(v is not None for v in limits)
    sources = [torch.from_numpy(a if v is None else expect(a, v, (4, 3))).to(DEV) for a, v in zip(raw, limits)]
    want, want_masks = P.augment_batch(sources, None, geom, lut, 96)
    plain, _, gt_plain = P.augment_samples(dev, None, rows, 96, np.random.default_rng(95))
    torch.cuda.synchronize()
    assert torch.equal(imgs, want) and torch.equal(masks, want_masks)
    assert torch.equal(gt, gt_plain) and not torch.equal(imgs, plain)                  # the labels do not move, the pixels do
    for a, d in zip(raw, dev):
        assert torch.equal(d.cpu(), torch.from_numpy(a))                               # the caller's images are not equalised in place
