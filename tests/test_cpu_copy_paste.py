"""CPU checks of the copy-paste augmentation (include/mtbt_hip.h `mtbt_copy_paste`): the entry point's refusals (none of which launches
anything), the same checks as a stand-alone program under the address and undefined-behaviour sanitizers, tests/copy_paste_reference.py
against the rule's stated properties, `sample_copy_paste`, and the draws of the `*_samples_seg` functions with and without the option."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import copy_paste_reference as R
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import preprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
I32P = C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


# ---- 1. the boundary ---------------------------------------------------------------------------------------------------------------
def test_symbols_struct_size_and_abi(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtbt_hip.h")).read(), flags=re.S)
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("mtbt_copy_paste", "mtbt_sizeof_copy_paste_args"):
        assert re.search(r"\b" + name + r"\s*\(", header) and name in L.SYMBOLS and hasattr(lib, name)
        assert f"`{name}`" in table, f"{name} is missing from INTEGRATION.md's symbol table"
    assert lib.mtbt_sizeof_copy_paste_args(0) == C.sizeof(L.CopyPasteArgs) == 128 and lib.mtbt_sizeof_copy_paste_args(1) == -1
    assert lib.mtbt_abi_version() == L.ABI_VERSION == 5            # additive: the version stays
    assert L.COPY_PASTE_CHUNK == 8 and L.COPY_PASTE_MAX_ENTRIES == 16
    src = open(os.path.join(ROOT, "multitask_bonetumor_yolo_amd", "csrc", "copy_paste_check.h")).read()
    assert re.search(r"constexpr int CHUNK = %d;" % L.COPY_PASTE_CHUNK, src) and re.search(r"MAX_ENTRIES = %d;" % L.COPY_PASTE_MAX_ENTRIES, src)
    import multitask_bonetumor_yolo_amd as pkg
    assert pkg.copy_paste_batch is P.copy_paste_batch and pkg.sample_copy_paste is P.sample_copy_paste


VALID = dict(images=0x10000000, planes=0x20000000, rows_in=0x30000000, out_images=0x40000000, out_planes=0x50000000, out_masks=0x60000000,
             rows_out=0x70000000, area_before=0x71000000, area=0x72000000, box=0x73000000, B=2, M=3, P=3, S=64, pitch=8, entry_stride=8)
ROW_OFF, PASTE_OFF = [0, 2, 3], [0, 1, 3]
ENTRIES = [[2, 5, -3, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0], [1, -64, 64, 1, 0, 0, 0, 0]]


def call(lib, row_off=ROW_OFF, paste_off=PASTE_OFF, entries=ENTRIES, null=(), **kw):
    a = L.CopyPasteArgs()
    for k, v in {**VALID, **kw}.items():
        setattr(a, k, v)
    ro, po = np.asarray(row_off, dtype=np.int32), np.asarray(paste_off, dtype=np.int32)
    en = np.ascontiguousarray(np.asarray(entries, dtype=np.int32).reshape(-1, 8))
    a.row_off, a.paste_off, a.entries = (None if k in null else v.ctypes.data_as(I32P) for k, v in (("row_off", ro), ("paste_off", po), ("entries", en)))
    return lib.mtbt_copy_paste(C.byref(a), None)


def entry(e, field, value):
    rows = [list(r) for r in ENTRIES]
    rows[e][field] = value
    return rows


def test_entry_point_refuses_before_any_launch(lib):
    """No GPU here: a call that got as far as a launch would not return MTBT_EINVAL / MTBT_EALIGN.  A valid call with a misaligned output
    is MTBT_EALIGN, which shows that everything before the alignment checks was accepted."""
    ok = dict(out_images=VALID["out_images"] + 4)                   # an accepted call stops here
    assert call(lib, **ok) == EALIGN
    assert lib.mtbt_copy_paste(None, None) == EINVAL
    for k in ("row_off", "paste_off", "entries"):
        assert call(lib, null=(k,)) == EINVAL, k
    for k in ("images", "planes", "out_images", "out_planes", "area_before", "area", "box", "rows_in"):
        assert call(lib, **{k: None}) == EINVAL, k
    assert call(lib, rows_in=None, rows_out=None, **ok) == EALIGN and call(lib, out_masks=None, **ok) == EALIGN   # both optional
    for k in ("B", "M", "P"):
        assert call(lib, **{k: -1}) == EINVAL, k
    for S in (0, -64, 2, 62, 32772, 1 << 20):
        assert call(lib, S=S, pitch=8 * ((S + 63) // 64)) == EINVAL, S
    for pitch in (0, 7, 16, -8):
        assert call(lib, pitch=pitch) == EINVAL, pitch
    assert call(lib, S=96, pitch=8) == EINVAL and call(lib, S=96, pitch=16, **ok) == EALIGN
    for stride in (0, 4, 7, 9):
        assert call(lib, entry_stride=stride) == EINVAL
    # offset tables: start at 0, never decrease, end at M respectively P; at most 16 entries a canvas
    for bad in ([1, 2, 3], [0, 3, 2], [0, 4, 3], [0, 2, 2], [0, 2, 4]):
        assert call(lib, row_off=bad) == EINVAL, bad
    for bad in ([1, 1, 3], [0, 4, 3], [0, 1, 2], [0, -1, 3]):
        assert call(lib, paste_off=bad) == EINVAL, bad
    zeros = lambda n: np.zeros((n, 8), dtype=np.int32)
    assert call(lib, paste_off=[0, 17, 17], entries=zeros(17), P=17) == EINVAL
    assert call(lib, paste_off=[0, 16, 16], entries=zeros(16), P=16, **ok) == EALIGN
    assert call(lib, paste_off=[0, 16, 32], entries=zeros(32), P=32, **ok) == EALIGN
    # entries: every field of the first and of the last entry
    for e in (0, 2):
        assert call(lib, entries=entry(e, 0, 3)) == EINVAL and call(lib, entries=entry(e, 0, -1)) == EINVAL
        for f in (1, 2):
            for v in (65, -65, 1 << 30, -(1 << 31)):
                assert call(lib, entries=entry(e, f, v)) == EINVAL, (e, f, v)
            for v in (64, -64):
                assert call(lib, entries=entry(e, f, v), **ok) == EALIGN, (e, f, v)
        assert call(lib, entries=entry(e, 3, 2)) == EINVAL and call(lib, entries=entry(e, 3, -1)) == EINVAL
        for f in (4, 5, 6, 7):
            assert call(lib, entries=entry(e, f, 1)) == EINVAL, (e, f)
    # an output range that overlaps an input range: images 98304 bytes, planes 1536, rows_in 72; outputs 98304, 3072, 32768, 144, 24, 24, 96
    v = VALID
    assert call(lib, out_images=v["images"]) == EINVAL and call(lib, out_images=v["images"] + 98304 - 16) == EINVAL
    assert call(lib, out_images=v["images"] + 98304 + 4) == EALIGN               # directly behind: accepted
    assert call(lib, out_masks=v["images"] - 16) == EINVAL and call(lib, out_masks=v["images"] - 32768 - 4) == EALIGN
    assert call(lib, out_planes=v["planes"] + 1536 - 8) == EINVAL and call(lib, out_planes=v["planes"] - 3072 + 8) == EINVAL
    assert call(lib, out_planes=v["planes"] - 3072, **ok) == EALIGN
    assert call(lib, rows_out=v["rows_in"]) == EINVAL and call(lib, box=v["rows_in"] + 68) == EINVAL
    assert call(lib, area=v["planes"] + 4) == EINVAL and call(lib, area_before=v["images"] + 4) == EINVAL
    # alignment, after everything else
    for k, off in (("images", 8), ("out_images", 4), ("out_masks", 8), ("planes", 4), ("out_planes", 1), ("rows_in", 2), ("rows_out", 1),
                   ("area_before", 2), ("area", 3), ("box", 2)):
        assert call(lib, **{k: VALID[k] + off}) == EALIGN, k
        assert call(lib, entries=entry(2, 3, 2), **{k: VALID[k] + off}) == EINVAL, k   # invalid and misaligned together is MTBT_EINVAL
    # B == 0 launches nothing; the other degenerate sizes are accepted
    nothing = {k: None for k in ("images", "planes", "rows_in", "out_images", "out_planes", "out_masks", "rows_out", "area_before", "area", "box")}
    assert call(lib, row_off=[0], paste_off=[0], entries=zeros(0), **{**nothing, "B": 0, "M": 0, "P": 0}) == 0
    images_only = {**nothing, "images": VALID["images"], "out_images": VALID["out_images"] + 4, "M": 0, "P": 0}
    assert call(lib, row_off=[0, 0, 0], paste_off=[0, 0, 0], entries=zeros(0), **images_only) == EALIGN          # M == 0 and P == 0
    assert call(lib, paste_off=[0, 0, 0], entries=zeros(0), P=0, **ok) == EALIGN                                 # P == 0
    assert call(lib, row_off=[0, 0, 0], paste_off=[0, 1, 1], entries=zeros(1), M=0, P=1) == EINVAL               # no plane to paste from


def test_the_checks_alone_under_host_sanitizers(tmp_path):
    """tests/copy_paste_check_main.cpp: csrc/copy_paste_check.h -- exactly what the entry point runs before its first launch -- compiled
    into a program of its own with -fsanitize=address,undefined, fed the rejected tables and the degenerate sizes, run on the CPU."""
    exe = str(tmp_path / "copy_paste_check")
    cmd = [B.HIPCC, "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-I" + B.INCLUDE, "-I" + B.CSRC, os.path.join(ROOT, "tests", "copy_paste_check_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0 and re.search(r"copy_paste_check: \d+ cases ok", r.stdout), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_python_refusals_need_no_device(lib):
    imgs, planes, rows = torch.zeros(1, 3, 64, 64), torch.zeros(0, 64, 8, dtype=torch.uint8), torch.zeros(0, 6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.copy_paste_batch(imgs, planes, [0, 0], rows, ([0, 0], np.zeros((0, 8), dtype=np.int32)))
    with pytest.raises(ValueError):
        P.sample_copy_paste([[]], 64, np.random.default_rng(0), mode="paste")
    with pytest.raises(ValueError):
        P.sample_copy_paste([[]], 64, np.random.default_rng(0), max_per_canvas=17)
    for name in ("augment_samples", "mosaic_samples", "affine_samples"):      # the box-only functions have no planes: they refuse the key
        with pytest.raises(TypeError, match="copy_paste"):
            getattr(P, name)([torch.zeros(8, 8, 3, dtype=torch.uint8)], None, [[]], 64, np.random.default_rng(0), copy_paste=dict())


# ---- 2. the reference against the rule's stated properties -------------------------------------------------------------------------
def scene(S=48, B=3, seed=0, rows=(2, 0, 3), n_entries=(3, 2, 4), reach=None):
    """Random blobs as planes, random canvases, random entries (offsets within +-reach, default S / 2)."""
    rng = np.random.default_rng(seed)
    M = sum(rows)
    images = rng.random((B, 3, S, S), dtype=np.float32)
    planes = np.zeros((M, S, S), dtype=bool)
    yy, xx = np.mgrid[0:S, 0:S]
    for m in range(M):
        cx, cy, rx, ry = rng.integers(4, S - 4), rng.integers(4, S - 4), rng.integers(3, S // 3), rng.integers(3, S // 3)
        planes[m] = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 <= 1.0
    row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    paste_off = np.concatenate([[0], np.cumsum(n_entries)]).astype(np.int32)
    reach = S // 2 if reach is None else reach
    entries = np.zeros((paste_off[-1], 8), dtype=np.int32)
    entries[:, 0] = rng.integers(0, M, len(entries))
    entries[:, 1:3] = rng.integers(-reach, reach + 1, (len(entries), 2))
    entries[:, 3] = rng.integers(0, 2, len(entries))
    rows_in = np.zeros((M, 6), dtype=np.float32)
    rows_in[:, 0] = np.repeat(np.arange(B), rows)
    rows_in[:, 1] = rng.integers(0, 5, M)
    rows_in[:, 2:] = rng.random((M, 4), dtype=np.float32)             # NOT the planes' boxes: an untouched row must come back as it is
    return images, planes, row_off, rows_in, paste_off, entries


def test_pack_and_unpack_are_the_library_layout():
    planes = np.random.default_rng(0).random((2, 132, 132)) < 0.5
    packed = R.pack(planes)
    assert packed.shape == (2, 132, 24) and packed.dtype == np.uint8
    back, clean = R.unpack(packed, 132)
    assert clean and np.array_equal(back, planes)
    one = np.zeros((1, 132, 132), dtype=bool)
    one[0, 5, 70] = True                                              # bit 70 of the row: byte 8, bit 6
    assert R.pack(one)[0, 5, 8] == 1 << 6 and R.pack(one).sum() == 1 << 6


def test_no_entries_is_the_identity():
    images, planes, row_off, rows_in, _, _ = scene()
    out = R.copy_paste(images, planes, row_off, rows_in, np.zeros(4, dtype=np.int32), np.zeros((0, 8), dtype=np.int32))
    assert np.array_equal(out["images"], images) and np.array_equal(out["planes"], planes)
    assert np.array_equal(out["rows"].view(np.int32), rows_in.view(np.int32))
    assert np.array_equal(out["area"], planes.sum(axis=(1, 2))) and np.array_equal(out["area"], out["area_before"])
    for i in range(3):
        assert np.array_equal(out["masks"][i, 0] > 0, planes[row_off[i]:row_off[i + 1]].any(axis=0))


def test_an_unmoved_paste_from_the_same_canvas_leaves_the_pixels():
    images, planes, row_off, rows_in, _, _ = scene()
    entries = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], [4, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int32)
    out = R.copy_paste(images, planes, row_off, rows_in, [0, 2, 2, 3], entries)
    assert np.array_equal(out["images"], images)
    assert np.array_equal(out["planes"][5 + 1], planes[1]) and not out["planes"][1].any()   # the copy lies above its original
    assert out["area"][1] == 0 and out["rows"][1].tolist() == [0.0, float(rows_in[1, 1]), 0, 0, 0, 0]
    # a mirrored self-paste is the mirrored canvas under the mirrored plane, read from the INPUT
    out = R.copy_paste(images, planes, row_off, rows_in, [0, 1, 1, 1], [[0, 0, 0, 1, 0, 0, 0, 0]])
    T = planes[0][:, ::-1]
    assert np.array_equal(out["planes"][5], T) and np.array_equal(out["images"][0][:, T], images[0][:, :, ::-1][:, T])
    assert np.array_equal(out["images"][0][:, ~T], images[0][:, ~T]) and np.array_equal(out["images"][1:], images[1:])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_layering_union_and_untouched_rows(seed):
    images, planes, row_off, rows_in, paste_off, entries = scene(seed=seed)
    out = R.copy_paste(images, planes, row_off, rows_in, paste_off, entries)
    M, touched, kept = planes.shape[0], 0, 0
    for i in range(3):
        es = range(paste_off[i], paste_off[i + 1])
        T = {e: R.translated(planes[entries[e, 0]], *(int(v) for v in entries[e, 1:4]))[0] for e in es}
        U = np.zeros_like(planes[0])
        for e in es:
            U |= T[e]
            assert out["area_before"][M + e] == T[e].sum()
            above = np.zeros_like(U)
            for later in es:
                if later > e:
                    above |= T[later]
                    assert not (out["planes"][M + e] & out["planes"][M + later]).any()      # disjoint from every entry above
            assert np.array_equal(out["planes"][M + e], T[e] & ~above)
        old = np.zeros_like(U)
        for m in range(row_off[i], row_off[i + 1]):
            old |= planes[m]
            assert not (out["planes"][m] & U).any() and np.array_equal(out["planes"][m], planes[m] & ~U)
            if out["area"][m] == out["area_before"][m]:
                kept += 1
                assert np.array_equal(out["rows"][m].view(np.int32), rows_in[m].view(np.int32))   # bit for bit
            else:
                touched += 1
                x1, y1, x2, y2 = out["box"][m]
                want = [rows_in[m, 0], rows_in[m, 1], (x1 + x2) / 96, (y1 + y2) / 96, (x2 - x1) / 48, (y2 - y1) / 48] if out["area"][m] else \
                       [rows_in[m, 0], rows_in[m, 1], 0, 0, 0, 0]
                assert np.allclose(out["rows"][m], want, rtol=1e-7, atol=0)
        planes_of_canvas = [out["planes"][m] for m in range(row_off[i], row_off[i + 1])] + [out["planes"][M + e] for e in es]
        union = np.any(planes_of_canvas, axis=0) if planes_of_canvas else np.zeros_like(U)
        assert np.array_equal(union, old | U) and np.array_equal(out["masks"][i, 0] > 0, old | U)
        # pixels: the topmost entry's donor pixel, else the canvas's own
        owner = np.full(U.shape, -1)
        for e in es:
            owner[T[e]] = e
        assert np.array_equal(out["images"][i][:, owner < 0], images[i][:, owner < 0])
        for e in es:
            sel = owner == e
            r, dx, dy, flip = (int(v) for v in entries[e, :4])
            j = R.canvas_of_row(row_off, r)
            ys, xs = np.nonzero(sel)
            assert np.array_equal(out["images"][i][:, ys, xs], images[j][:, ys - dy, (47 - (xs - dx)) if flip else xs - dx])
    assert touched + kept == M
    for k in range(M + len(entries)):                                           # records of every output plane
        assert (out["area"][k], list(out["box"][k])) == R.record(out["planes"][k])


def test_offsets_of_a_whole_canvas_give_an_empty_paste():
    images, planes, row_off, rows_in, _, _ = scene()
    for dx, dy in ((48, 0), (-48, 0), (0, 48), (0, -48)):
        for flip in (0, 1):
            out = R.copy_paste(images, planes, row_off, rows_in, [0, 1, 1, 1], [[3, dx, dy, flip, 0, 0, 0, 0]])
            assert not out["planes"][5].any() and np.array_equal(out["images"], images) and out["area_before"][5] == 0
            assert out["rows"][5].tolist() == [0.0, float(rows_in[3, 1]), 0, 0, 0, 0] and out["box"][5].tolist() == [0, 0, 0, 0]


# ---- 3. sample_copy_paste -----------------------------------------------------------------------------------------------------------
def random_rows(rng, B, S):
    out = []
    for i in range(B):
        rows = []
        for _ in range(int(rng.integers(0, 7))):
            w, h = rng.uniform(0.03, 0.3, 2)
            rows.append([float(i), float(rng.integers(0, 3)), float(rng.uniform(w / 2, 1 - w / 2)), float(rng.uniform(h / 2, 1 - h / 2)), float(w), float(h)])
        out.append(rows)
    return out


def moved_box(row, S, dx, dy, flip):
    x1, y1, x2, y2 = P._box_px(row, float(S))
    if flip:
        x1, x2 = S - x2, S - x1
    return tuple(min(max(v, 0.0), float(S)) for v in (x1 + dx, y1 + dy, x2 + dx, y2 + dy))


@pytest.mark.parametrize("mode", ["mix", "flip"])
def test_accepted_sets_satisfy_the_ioa_rule_and_the_limits(mode):
    rng, S, pastes = np.random.default_rng(7), 160, 0
    for trial in range(60):
        B = int(rng.integers(1, 6))
        per = random_rows(rng, B, S)
        flat = [r for c in per for r in c]
        first = np.concatenate([[0], np.cumsum([len(c) for c in per])])
        cap = int(rng.integers(1, 5)) if trial % 2 else 16
        max_ioa = float(rng.choice([0.1, 0.3, 0.6]))
        paste_off, entries = P.sample_copy_paste(per, S, rng, prob=0.8, fraction=0.7, mode=mode, translate=0.2, max_ioa=max_ioa, max_per_canvas=cap)
        assert paste_off.dtype == entries.dtype == np.int32 and paste_off.shape == (B + 1,) and entries.shape == (paste_off[-1], 8)
        assert paste_off[0] == 0 and (np.diff(paste_off) >= 0).all() and (np.diff(paste_off) <= cap).all() and not entries[:, 4:].any()
        for i in range(B):
            placed = [P._box_px(r, float(S)) for r in per[i]]
            mine = entries[paste_off[i]:paste_off[i + 1]]
            if len(mine):
                donors = {int(np.searchsorted(first, r, side="right")) - 1 for r in mine[:, 0]}
                assert len(donors) == 1 and len({tuple(e[1:4]) for e in mine.tolist()}) == 1     # one donor, one flip, one offset a canvas
                assert donors == {i} and tuple(mine[0, 1:4]) == (0, 0, 1) if mode == "flip" else i not in donors
                assert (np.diff(mine[:, 0]) > 0).all()                                           # candidates in row order, each once
                assert np.abs(mine[:, 1:3]).max() <= int(0.2 * S)
            for r, dx, dy, flip in mine[:, :4].tolist():
                t = moved_box(flat[r], S, dx, dy, flip)
                assert t[2] - t[0] >= 2.0 and t[3] - t[1] >= 2.0
                for b in placed:                                                                 # against everything placed before it
                    iw, ih = max(min(t[2], b[2]) - max(t[0], b[0]), 0.0), max(min(t[3], b[3]) - max(t[1], b[1]), 0.0)
                    assert iw * ih / ((b[2] - b[0]) * (b[3] - b[1])) < max_ioa
                placed.append(t)
                pastes += 1
    assert pastes > 40


def test_one_canvas_in_mix_mode_pastes_nothing_and_the_draws_are_reproducible():
    per = random_rows(np.random.default_rng(1), 1, 64)
    po, en = P.sample_copy_paste(per, 64, np.random.default_rng(2), prob=1.0, fraction=1.0)
    assert po.tolist() == [0, 0] and en.shape == (0, 8)
    per = random_rows(np.random.default_rng(3), 4, 64)
    kw = dict(prob=0.9, fraction=0.9, translate=0.25, max_ioa=0.9)
    a, b = P.sample_copy_paste(per, 64, np.random.default_rng(5), **kw), P.sample_copy_paste(per, 64, np.random.default_rng(5), **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[1]) > 0
    # the documented order: decisions, donors, flips, offsets, then one candidate vector per receiving canvas
    r0, r1 = np.random.default_rng(5), np.random.default_rng(5)
    po, _ = P.sample_copy_paste(per, 64, r0, **kw)
    on, donors = r1.random(4) < 0.9, r1.integers(0, 3, 4)
    r1.random(4), r1.integers(-16, 17, (4, 2))
    for i in range(4):
        if on[i]:
            r1.random(len(per[int(donors[i]) + (int(donors[i]) >= i)]))
    assert r0.bit_generator.state == r1.bit_generator.state
    assert P.sample_copy_paste(per, 64, np.random.default_rng(5), prob=0.0)[0].tolist() == [0] * 5
    # a paste that would cover an existing box too far is rejected: the donor's box lies exactly on the canvas's own
    same = [[[0, 0, 0.5, 0.5, 0.3, 0.3]], [[1, 1, 0.5, 0.5, 0.3, 0.3]]]
    assert P.sample_copy_paste(same, 64, np.random.default_rng(0), prob=1.0, fraction=1.0)[0].tolist() == [0, 0, 0]
    assert P.sample_copy_paste(same, 64, np.random.default_rng(0), prob=1.0, fraction=1.0, max_ioa=1.01)[0].tolist() == [0, 1, 2]


# ---- 4. draws of the sample functions (device work stubbed) ------------------------------------------------------------------------
SIZES = [(300, 200), (128, 256), (77, 91)]
SEG_ROWS = [[[0, 0.2, 0.2, 0.8, 0.2, 0.8, 0.8, 0.2, 0.8]], [[2, 0.3, 0.3, 0.5, 0.3, 0.5, 0.6, 0.3, 0.6]], [[1, 0.1, 0.1, 0.6, 0.2, 0.4, 0.9]]]


@pytest.mark.parametrize("name", ["augment_samples_seg", "mosaic_samples_seg", "affine_samples_seg"])
def test_without_the_option_the_generator_is_consumed_as_before_and_with_it_the_draws_come_last(monkeypatch, name):
    seen = {"image": [], "clahe": [], "paste": []}

    def fake_image(images, masks, *args):
        seen["image"].append([a.cpu().numpy() if isinstance(a, torch.Tensor) else np.array(a) for a in args[:-1] if a is not None])
        S = args[-1]
        return torch.zeros(len(images), 3, S, S), None

    def fake_clahe(images, clip_limit=2.0, grid=(8, 8), out=None):
        seen["clahe"].append(list(clip_limit))
        return list(images)

    def fake_paste(imgs, planes, row_off, gt_rows, table, *, masks=True):
        seen["paste"].append((np.array(row_off), table))
        return "pasted"

    for k in ("augment_batch", "mosaic_batch", "warp_batch"):
        monkeypatch.setattr(P, k, fake_image)
    monkeypatch.setattr(P, "clahe_batch", fake_clahe)
    monkeypatch.setattr(P, "copy_paste_batch", fake_paste)
    monkeypatch.setattr(P, "_upload", lambda t, dev: t)
    monkeypatch.setattr(P, "_seg_outputs", lambda per_canvas, rects, S, dev: (None, [[it[0] for it in c] for c in per_canvas], {"planes": None}))
    images = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in SIZES]
    kw = dict(scale=(0.8, 1.1), brightness=0.1, min_px=1.0)
    fn = getattr(P, name)
    r0, r1, r2, r3 = (np.random.default_rng(11) for _ in range(4))
    plain = fn(images, SEG_ROWS, 160, r0, **kw)
    none = fn(images, SEG_ROWS, 160, r1, copy_paste=None, **kw)
    # the parent's draws, restated: geometry, then the photometric table -- nothing else
    if name == "augment_samples_seg":
        P.sample_geometry(SIZES, 160, r2, scale=(0.8, 1.1))
    elif name == "mosaic_samples_seg":
        P.sample_mosaic(SIZES, 160, r2, scale=(0.8, 1.1))
    else:
        P.sample_affine(SIZES, 160, r2, scale=(0.8, 1.1))
    P.sample_photometric(3, r2, brightness=0.1)
    assert r0.bit_generator.state == r1.bit_generator.state == r2.bit_generator.state and seen["paste"] == [] and seen["clahe"] == []
    assert plain[2] == none[2] and sum(len(c) for c in plain[2]) >= 2
    for a, b in zip(seen["image"][0], seen["image"][1]):
        assert np.array_equal(a, b)
    # with CLAHE and the option: the same geometry and table, CLAHE's draws, then exactly sample_copy_paste's on the canvases' rows
    opts = dict(prob=1.0, fraction=1.0, translate=0.1, max_ioa=2.0)
    got = fn(images, SEG_ROWS, 160, r3, clahe=dict(prob=0.5), copy_paste=opts, **kw)
    assert got == "pasted" and len(seen["paste"]) == 1
    for a, b in zip(seen["image"][0], seen["image"][2]):
        assert np.array_equal(a, b)
    assert seen["clahe"] == [P.sample_clahe(3, r2, prob=0.5)]
    row_off, table = seen["paste"][0]
    want = P.sample_copy_paste(plain[2], 160, r2, **opts)
    assert r3.bit_generator.state == r2.bit_generator.state
    assert np.array_equal(table[0], want[0]) and np.array_equal(table[1], want[1]) and len(want[1]) >= 1
    assert row_off.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in plain[2]])]).tolist()
