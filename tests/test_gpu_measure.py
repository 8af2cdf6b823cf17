"""The device measurements (`postprocess.measure_regions`, `measure_components`, `measure_detections`; csrc/measure.hip) against the
restatement (tests/measure_reference.py, held against scipy.spatial, numpy and closed forms in tests/test_cpu_measure.py): every table is
an integer table and every comparison is exact.

Shapes: the six of the component and contour tests (a single pixel, a single row, pitches 8, 16 and 24 on both sides of a word boundary)
and one 640 x 640 plane.  Contents: `plane_cases` of the component tests plus a pixel in each corner, the full plane, a disc, a diamond,
the diagonal, a bar across the word boundaries, and padding bits set to one.  Label mode runs on the label maps of `label_components` at
both connectivities (the checkerboard has more components than the tables hold), on a ring with a dot inside its box and on a random map
whose regions are not connected.  One plane of 16384 x 16384 with four set pixels is the only case whose fractions need more than 64 bits."""
import numpy as np
import pytest
import torch

import components_reference as CR
import measure_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (1, 70), (37, 64), (33, 65), (40, 130), (96, 200)]
TABLES = ("sums", "n_hull", "hull", "hull_area2", "caliper", "caliper_at")
VH = 64                                          # the hulls of the small shapes fit; the 640 x 640 plane and the disc test the cap
C_SMALL = 48                                     # the checkerboard of 40 x 130 has 2600 components under connectivity 4: over the cap

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import (fill_polygons, label_components, measure_components, measure_detections, measure_regions,
                                              region_properties)
    from multitask_bonetumor_yolo_amd.postprocess import unpack_masks


def _pack(planes, pad_ones=False):
    return torch.from_numpy(CR.pack_bits(np.stack(planes), pad_ones)).to(DEV)


def _assert_tables(got, want, what=""):
    assert got["sums"].dtype == torch.int64 and got["hull_area2"].dtype == torch.int64 and got["caliper"].dtype == torch.int64
    assert got["n_hull"].dtype == torch.int32 and got["hull"].dtype == torch.int32 and got["caliper_at"].dtype == torch.int32
    for k in TABLES:
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape, (what, k, g.shape, want[k].shape)
        bad = np.argwhere(g != want[k])
        assert len(bad) == 0, (what, k, bad[:4].tolist(), g[tuple(bad[0])], want[k][tuple(bad[0])])


def _cases(i, H, W):
    rng = np.random.default_rng(60 + i)
    return CR.plane_cases(rng, H, W) + R.extra_cases(rng, H, W)


@pytest.fixture(scope="module")
def small():
    """Per shape: (names, planes, plane-mode tables), computed once."""
    out = {}
    for i, (H, W) in enumerate(SHAPES):
        cs = _cases(i, H, W)
        planes = [m for _, m in cs]
        out[(H, W)] = ([n for n, _ in cs], planes, R.plane_tables(planes, VH))
    return out


@pytest.fixture(scope="module")
def big():
    m = CR.big_plane(np.random.default_rng(7))
    return m, R.measure_plane(m)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("pad_ones", [False, True], ids=["pad0", "pad1"])
def test_plane_mode(small, shape, pad_ones):
    names, planes, want = small[shape]
    got = measure_regions(_pack(planes, pad_ones), shape[1], max_hull=VH)
    assert got["shape"] == shape
    _assert_tables(got, want, (shape, names))


def test_plane_mode_640(big):
    m, rec = big
    disc = R.disc(640, 640, 300, 330, 300)
    want = R.tables([[rec], [R.measure_plane(disc)], [R.measure_plane(np.zeros_like(m))]], 512)
    _assert_tables(measure_regions(_pack([m, disc, np.zeros_like(m)]), 640), want, "640")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("conn", [4, 8])
def test_label_mode_on_label_components(small, shape, conn):
    names, planes, _ = small[shape]
    comp, got = measure_components(_pack(planes), shape[1], connectivity=conn, max_components=C_SMALL, max_hull=VH)
    labs = comp["labels"].cpu().numpy()
    if shape[0] > 1 and conn == 4:
        assert int(comp["n_components"].max()) > C_SMALL                   # the checkerboard: ids above C are ignored and still break the perimeter
    _assert_tables(got, R.label_tables(list(labs), C_SMALL, VH), (shape, conn, names))
    area = got["sums"][:, :, 0].cpu().numpy()
    assert np.array_equal(area, comp["area"].cpu().numpy().astype(np.int64))


def test_label_mode_640(big):
    m, _ = big
    comp, got = measure_components(_pack([m]), 640, connectivity=8, max_components=2048)     # some 1200 specks come before the blob
    assert int(got["sums"][0, :, 0].max()) > 100000
    _assert_tables(got, R.label_tables(list(comp["labels"].cpu().numpy()), 2048, 512), "640 labels")


def test_label_mode_on_arbitrary_maps():
    rng = np.random.default_rng(5)
    ring = np.zeros((33, 65), np.int32)
    ring[4:20, 10:40] = 1
    ring[6:18, 12:38] = 0
    ring[11, 25] = 2                                                       # a dot inside the ring's box: its own region
    ring[30, 62:65] = 7                                                    # above C: reported nowhere
    noise = rng.integers(-3, 12, size=(33, 65)).astype(np.int32)           # regions in many pieces, negative labels, ids above C
    rows = np.zeros((33, 65), np.int32)
    rows[0, :] = 3
    rows[32, 64] = 3                                                       # one region in the first row and the last pixel
    maps = [ring, noise, rows]
    got = measure_regions(None, 65, labels=torch.from_numpy(np.stack(maps)).to(DEV), max_regions=5, max_hull=VH)
    _assert_tables(got, R.label_tables(maps, 5, VH), "maps")


def test_max_hull_does_not_change_a_measurement():
    disc = R.disc(200, 230, 98, 120, 90)
    rec = R.measure_plane(disc)
    assert len(rec["hull"]) > 40
    full = measure_regions(_pack([disc]), 230, max_hull=128)
    cut = measure_regions(_pack([disc]), 230, max_hull=4)
    _assert_tables(full, R.tables([[rec]], 128), "max_hull 128")
    _assert_tables(cut, R.tables([[rec]], 4), "max_hull 4")                # n_hull true, four rows written
    for k in ("sums", "n_hull", "hull_area2", "caliper", "caliper_at"):
        assert torch.equal(full[k], cut[k]), k
    assert torch.equal(cut["hull"][0, 0], full["hull"][0, 0, :4]) and not full["hull"][0, 0, len(rec["hull"]):].any()


def test_measure_detections_over_a_stack_of_instance_planes():
    rng = np.random.default_rng(11)
    H, W, K = 96, 200, 5
    planes = [R.disc(H, W, 40, 60, 25), R.diamond(H, W, 50, 120, 30), np.pad(CR.big_plane(rng, 96), ((0, 0), (0, W - 96))),
              np.zeros((H, W), bool), rng.uniform(size=(H, W)) < 0.1]
    packed = _pack(planes)
    out = {"masks_frame": [packed, packed], "counts": torch.tensor([K, 2], device=DEV), "frames": [(H, W, 1.0), (H, W, 1.0)]}
    got = measure_detections(out, spacing=0.5)
    assert len(got) == 2 and got[0]["area"].shape == (K, 1) and got[1]["area"].shape == (2, 1)   # the first counts[b] planes only
    for j in range(K):
        one = region_properties(measure_regions(packed[j:j + 1], W), spacing=0.5)
        for k, v in one.items():
            assert np.array_equal(got[0][k][j], v[0], equal_nan=True), (j, k)
    rec = R.measure_plane(planes[0])
    assert got[1]["area"][0, 0] == rec["sums"][0] * 0.25 and got[1]["feret_max"][0, 0] == np.sqrt(float(rec["caliper"][0])) * 0.5
    assert got[0]["area"][3, 0] == 0 and np.isnan(got[0]["solidity"][3, 0])


def test_the_four_pixels_of_16384_squared():
    """The only case whose fraction comparisons exceed 64 bits (asserted in tests/test_cpu_measure.py)."""
    S = 16384
    packed = torch.zeros((1, S, S // 8), dtype=torch.uint8, device=DEV)
    for x, y in R.BIG_FOUR:
        packed[0, y, x >> 3] |= 1 << (x & 7)
    rec = R.measure_pixels(R.BIG_FOUR, S)
    assert max(R.width_products(rec["hull"])) > 2 ** 64
    _assert_tables(measure_regions(packed, S, max_hull=16), R.tables([[rec]], 16), "16384")


def test_the_hull_covers_its_region(small, big):
    names, planes, _ = small[(96, 200)]
    planes = [m for m in planes if m.any()]
    packed = _pack(planes)
    got = measure_regions(packed, 200, max_hull=256)
    n_hull, hull = got["n_hull"].cpu().numpy(), got["hull"].cpu().numpy()
    polys = [hull[b, 0, :n_hull[b, 0]] for b in range(len(planes))]
    fill = fill_polygons(polys, 96, 200, device=DEV)
    assert not (packed & ~fill).any()
    m, _ = big
    pk = _pack([m])
    g = measure_regions(pk, 640)
    fill = fill_polygons([g["hull"][0, 0, :int(g["n_hull"][0, 0])].cpu().numpy()], 640, 640, device=DEV)
    assert not (pk & ~fill).any() and int(unpack_masks(fill, 640).sum()) * 2 <= int(g["hull_area2"][0, 0])


def test_a_captured_call_equals_the_eager_one(small):
    names, planes, want = small[(40, 130)]
    packed = _pack(planes)
    comp = label_components(packed, 130, max_components=C_SMALL)
    eager = (measure_regions(packed, 130, max_hull=VH), measure_regions(None, 130, labels=comp["labels"], max_regions=C_SMALL, max_hull=VH))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        measure_regions(packed, 130, max_hull=VH)                          # warm-up: the code objects are loaded
        measure_regions(None, 130, labels=comp["labels"], max_regions=C_SMALL, max_hull=VH)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cap = (measure_regions(packed, 130, max_hull=VH), measure_regions(None, 130, labels=comp["labels"], max_regions=C_SMALL, max_hull=VH))
    torch.cuda.current_stream().wait_stream(s)
    for r in cap:
        for k in TABLES:
            r[k].fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    _assert_tables(cap[0], want, "captured planes")
    for k in TABLES:
        assert torch.equal(cap[0][k], eager[0][k]) and torch.equal(cap[1][k], eager[1][k]), k
