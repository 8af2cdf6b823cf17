"""`mtbt_copy_paste` on the device against tests/copy_paste_reference.py, bit for bit in every case: images (`torch.equal`), packed planes
(padding included), canvas mask, the three records, and the label rows compared as int32 bit patterns.  Shapes S = 64 (one word), 96 (two
words, 32 padding bits), 132 (three words, the last with 4 valid bits); the planes of the shift sweep are random bits, so every bit of every
funnel shift counts."""
import numpy as np
import pytest
import torch

import copy_paste_reference as R
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import preprocess as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


def noise_planes(rng, M, S, density=0.3):
    return rng.random((M, S, S)) < density


def blob_planes(rng, M, S):
    yy, xx = np.mgrid[0:S, 0:S]
    out = np.zeros((M, S, S), dtype=bool)
    for m in range(M):
        cx, cy, rx, ry = rng.integers(4, S - 4), rng.integers(4, S - 4), rng.integers(3, S // 3), rng.integers(3, S // 3)
        out[m] = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0
    return out


def label_rows(rng, rows_per_canvas):
    """Rows that are NOT the planes' boxes: an untouched row must come back exactly as it went in."""
    M = int(sum(rows_per_canvas))
    rows = np.zeros((M, 6), dtype=np.float32)
    rows[:, 0] = np.repeat(np.arange(len(rows_per_canvas)), rows_per_canvas)
    rows[:, 1] = rng.integers(0, 7, M)
    rows[:, 2:] = rng.random((M, 4), dtype=np.float32)
    return rows


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def check(images, planes, rows_per_canvas, rows_in, entries_per_canvas, masks=True):
    """Run the device and the reference on one call and compare everything; returns the reference's outputs."""
    B, S, M = images.shape[0], images.shape[-1], planes.shape[0]
    row_off, paste_off = offsets(rows_per_canvas), offsets([len(e) for e in entries_per_canvas])
    entries = np.zeros((paste_off[-1], 8), dtype=np.int32)
    flat = [e for c in entries_per_canvas for e in c]
    if flat:
        entries[:, :4] = np.asarray(flat, dtype=np.int32)
    want = R.copy_paste(images, planes, row_off, rows_in, paste_off, entries)
    d_images, d_planes, d_rows = torch.from_numpy(images).to(DEV), torch.from_numpy(R.pack(planes)).to(DEV), torch.from_numpy(rows_in).to(DEV)
    keep = (d_images.clone(), d_planes.clone(), d_rows.clone())
    out, out_m, rows, inst = P.copy_paste_batch(d_images, d_planes, row_off, d_rows, (paste_off, entries), masks=masks)
    torch.cuda.synchronize()
    P_ = len(entries)
    assert out.shape == (B, 3, S, S) and rows.shape == (M + P_, 6) and inst["planes"].shape == (M + P_, S, R.pitch_of(S))
    assert torch.equal(out.cpu(), torch.from_numpy(want["images"]))
    assert np.array_equal(inst["planes"].cpu().numpy(), R.pack(want["planes"]))            # every byte, padding bits zero
    if masks:
        assert torch.equal(out_m.cpu(), torch.from_numpy(want["masks"]))
    else:
        assert out_m is None
    assert np.array_equal(inst["area_before"].cpu().numpy().astype(np.uint32), want["area_before"])
    assert np.array_equal(inst["area"].cpu().numpy().astype(np.uint32), want["area"])
    assert np.array_equal(inst["boxes"].cpu().numpy(), want["box"])
    assert np.array_equal(rows.cpu().numpy().view(np.int32), want["rows"].view(np.int32))
    assert np.array_equal(inst["image"].cpu().numpy(), want["rows"][:, 0].astype(np.int64))
    assert np.array_equal(inst["labels"].cpu().numpy(), want["rows"][:, 1].astype(np.int64))
    for before, after in zip(keep, (d_images, d_planes, d_rows)):                           # the input is never modified
        assert torch.equal(before, after)
    return want


@pytest.mark.parametrize("S", [64, 96, 132])
def test_shift_sweep_both_flips(S):
    """dx in {0, 1, -1, 63, 64, 65, -64, -65, S, -S} (those within the limit |dx| <= S: 65 and -65 are outside it at S = 64, where the entry
    point refuses them), each with both flips, over dy in {0, 3, -7, S - 1, 1 - S, S, -S}; two entries a canvas, donors on any canvas."""
    rng = np.random.default_rng(S)
    dxs = [v for v in (0, 1, -1, 63, 64, 65, -64, -65, S, -S) if abs(v) <= S]
    dys = [0, 3, -7, S - 1, 1 - S, S, -S]
    combos = [(dx, dys[k % len(dys)], flip) for k, (dx, flip) in enumerate((dx, f) for dx in dxs for f in (0, 1))]
    combos += [(0, dy, f) for dy in (S, -S, S - 1, 1 - S) for f in (0, 1)] + [(dx, 5, f) for dx in (S - 1, 1 - S, 31, -33) for f in (0, 1)]
    B = (len(combos) + 1) // 2
    rows_per_canvas = [1 + (i % 3 == 0) for i in range(B)]
    M = sum(rows_per_canvas)
    images = rng.random((B, 3, S, S), dtype=np.float32)
    planes = noise_planes(rng, M, S)
    entries = [[] for _ in range(B)]
    for k, (dx, dy, flip) in enumerate(combos):
        entries[k // 2].append([int(rng.integers(0, M)), dx, dy, flip])
    want = check(images, planes, rows_per_canvas, label_rows(rng, rows_per_canvas), entries)
    assert B > L.COPY_PASTE_CHUNK and (want["area"][M:] > 0).sum() > len(combos) // 2 and (want["area_before"][M:] == 0).sum() >= 4


def test_self_paste_with_flip_and_mutual_pastes():
    rng, S = np.random.default_rng(1), 96
    images = rng.random((3, 3, S, S), dtype=np.float32)
    planes = blob_planes(rng, 4, S)
    # canvas 0 pastes its own row mirrored; canvases 1 and 2 paste from each other (each reads the other's pristine pixels)
    want = check(images, planes, [1, 1, 2], label_rows(rng, [1, 1, 2]), [[[0, 0, 0, 1]], [[2, 4, -6, 0], [3, -9, 2, 1]], [[1, 11, 3, 1]]])
    assert (want["area"][4:] > 0).all()
    T = planes[0][:, ::-1]
    assert np.array_equal(want["planes"][4], T) and np.array_equal(want["images"][0][:, T], images[0][:, :, ::-1][:, T])


def test_sixteen_overlapping_entries_on_one_canvas():
    rng, S = np.random.default_rng(2), 64
    images = rng.random((2, 3, S, S), dtype=np.float32)
    planes = blob_planes(rng, 3, S) | noise_planes(rng, 3, S, 0.05)
    entries = [[int(rng.integers(0, 3)), int(rng.integers(-10, 11)), int(rng.integers(-10, 11)), int(rng.integers(0, 2))] for _ in range(16)]
    want = check(images, planes, [2, 1], label_rows(rng, [2, 1]), [entries, []])
    hidden = want["area"][3:] < want["area_before"][3:]
    assert hidden[:15].sum() >= 8 and not hidden[15]                                        # the last entry lies on top
    assert len(np.unique(np.nonzero(want["planes"][3:].any(axis=(1, 2)))[0])) >= 8


def test_a_wholly_covered_old_plane_gives_a_zero_row_and_an_empty_canvas_stays():
    rng, S = np.random.default_rng(3), 132
    images = rng.random((3, 3, S, S), dtype=np.float32)
    planes = blob_planes(rng, 2, S)
    rows_in = label_rows(rng, [2, 0, 0])
    # canvas 0: row 0 pasted on itself unmoved covers the old row 0 entirely; canvas 1 has no rows and no entries; canvas 2 only receives
    want = check(images, planes, [2, 0, 0], rows_in, [[[0, 0, 0, 0]], [], [[1, -20, 15, 0]]])
    assert want["area"][0] == 0 and want["area_before"][0] == planes[0].sum() and want["box"][0].tolist() == [0, 0, 0, 0]
    assert want["rows"][0].tolist() == [0.0, float(rows_in[0, 1]), 0.0, 0.0, 0.0, 0.0]
    assert np.array_equal(want["images"][:2], images[:2]) and not want["masks"][1].any()


def test_no_planes_and_no_entries():
    rng, S = np.random.default_rng(4), 64
    images = rng.random((2, 3, S, S), dtype=np.float32)
    want = check(images, np.zeros((0, S, S), dtype=bool), [0, 0], np.zeros((0, 6), dtype=np.float32), [[], []])      # M == 0
    assert np.array_equal(want["images"], images) and not want["masks"].any()
    planes = blob_planes(rng, 3, S)
    rows_in = label_rows(rng, [1, 2])
    want = check(images, planes, [1, 2], rows_in, [[], []], masks=False)                                               # P == 0
    assert np.array_equal(want["planes"], planes) and np.array_equal(want["rows"].view(np.int32), rows_in.view(np.int32))


def test_a_donor_in_the_other_launch():
    rng, S, B = np.random.default_rng(5), 64, L.COPY_PASTE_CHUNK + 1
    images = rng.random((B, 3, S, S), dtype=np.float32)
    rows_per_canvas = [1] * B
    planes = blob_planes(rng, B, S)
    entries = [[] for _ in range(B)]
    entries[0] = [[B - 1, 3, 2, 1]]                  # the first launch reads the last canvas
    entries[B - 1] = [[0, -4, 6, 0], [3, 0, 0, 1]]   # the second launch reads canvases of the first
    want = check(images, planes, rows_per_canvas, label_rows(rng, rows_per_canvas), entries)
    assert (want["area"][B:] > 0).all() and not np.array_equal(want["images"][B - 1], images[B - 1])


SEG_ROWS = [[[0, 0.15, 0.2, 0.55, 0.25, 0.5, 0.6, 0.2, 0.55]], [[2, 0.5, 0.5, 0.9, 0.55, 0.8, 0.9]], [[1, 0.1, 0.1, 0.4, 0.15, 0.3, 0.45], [3, 0.6, 0.6, 0.9, 0.6, 0.9, 0.9, 0.6, 0.9]]]


def test_augment_samples_seg_with_the_option_equals_the_steps():
    rng, S = np.random.default_rng(6), 64
    sizes = [(80, 100), (64, 64), (120, 90)]
    raw = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).to(DEV) for h, w in sizes]
    kw = dict(scale=(0.9, 1.0), fliplr=0.5, min_px=1.0)
    opts = dict(prob=1.0, fraction=1.0, translate=0.2, max_ioa=2.0)
    got = P.augment_samples_seg(raw, SEG_ROWS, S, np.random.default_rng(9), copy_paste=opts, **kw)
    r1, r2 = np.random.default_rng(9), np.random.default_rng(9)
    imgs, masks, gt_rows, inst = P.augment_samples_seg(raw, SEG_ROWS, S, r1, **kw)
    geom = P.sample_geometry(sizes, S, r2, scale=(0.9, 1.0), fliplr=0.5)
    P.sample_photometric(3, r2)
    assert r1.bit_generator.state == r2.bit_generator.state
    per_canvas = [[row6 for row6, _ in P.augment_polygons(r, w, h, geom[i], S, min_px=1.0)] for i, (r, (h, w)) in enumerate(zip(SEG_ROWS, sizes))]
    table = P.sample_copy_paste(per_canvas, S, r1, **opts)
    row_off = offsets([len(c) for c in per_canvas])
    assert row_off[-1] == gt_rows.shape[0] == 4 and len(table[1]) >= 2
    want = P.copy_paste_batch(imgs, inst["planes"], row_off, gt_rows, table)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert sorted(got[3]) == sorted(want[3]) == ["area", "area_before", "boxes", "image", "labels", "planes"]
    for k in want[3]:
        assert torch.equal(got[3][k], want[3][k]), k
    assert not torch.equal(got[0], imgs) and got[2].shape[0] == 4 + len(table[1])
    # and the reference agrees with the device on these canvases too
    planes_bool, clean = R.unpack(inst["planes"].cpu().numpy(), S)
    ref = R.copy_paste(imgs.cpu().numpy(), planes_bool, row_off, gt_rows.cpu().numpy(), table[0], table[1])
    assert clean and torch.equal(got[0].cpu(), torch.from_numpy(ref["images"])) and torch.equal(got[1].cpu(), torch.from_numpy(ref["masks"]))
    assert np.array_equal(got[2].cpu().numpy().view(np.int32), ref["rows"].view(np.int32))
    assert np.array_equal(got[3]["planes"].cpu().numpy(), R.pack(ref["planes"]))


@pytest.mark.parametrize("S", [60, 124])
def test_last_word_four_bits_short(S):
    """A canvas side is a multiple of 4, so S % 64 == 60 is as close under a word boundary as it gets (S = 60: a single, partial word):
    shifts by one pixel either way and by a whole row but one, both flips, donors on the other canvas."""
    rng = np.random.default_rng(S)
    images = rng.random((2, 3, S, S), dtype=np.float32)
    planes = noise_planes(rng, 2, S)
    entries = [[[1, 1, 0, 0], [1, -1, 2, 1]], [[0, S - 1, -3, 1], [0, 1 - S, 0, 0]]]
    want = check(images, planes, [1, 1], label_rows(rng, [1, 1]), entries)
    assert (want["area"][2:] > 0).all()
