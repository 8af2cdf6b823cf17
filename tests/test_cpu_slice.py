"""CPU checks of sliced inference: the tile geometry (`preprocess.slice_geometry`), the invariants of the merge and mask restatements
(tests/slice_reference.py), the cases in which they must agree with the single-image frame operator (tests/frame_reference.py), and the C
boundary of `mtbt_merge_tiles` / `mtbt_vote_tile_masks` (struct layout, argument checks before any launch).

Shapes: S = 160, G = 40, K = 21; images of 300 x 410 and 410 x 300 (3 x 3 tiles plus the full view), 97 x 120 (smaller than S: one tile)
and 170 x 260 whose tiles are all empty.  Bits are compared outside the band |logit| < 1e-4 * (tiles contributing at the pixel), the
per-source band of test_gpu_mask_vote.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import augment_reference as AR
import frame_reference as FR
import slice_reference as SR
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import postprocess as pp
from multitask_bonetumor_yolo_amd import preprocess as pre
from oracle import preprocess as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, G, K, UP, A = 160, 40, 21, 4, 300
SIZES = [(300, 410), (410, 300), (97, 120), (170, 260)]
EMPTY = (3,)
BAND, SHARE = 1e-4, 8e-4
SEED = 3
EINVAL, EALIGN = -1, -2
# (metric, thr, skip_thr, top_k, class_agnostic): both metrics, the cut, the skip threshold, labels on and off
MERGE_CASES = [("ios", 0.5, 0.0, 21, False), ("iou", 0.5, 0.2, 21, False), ("ios", 0.5, 0.2, 16, True), ("iou", 0.3, 0.0, 16, False),
               ("ios", 0.5, 0.0, 16, False)]
CUT_CASES = (1, 3, 4)       # the cases in which top_k cuts an image's rows: IoU leaves the clipped parts apart, IoS at 16 rows loses one
# (merge case, crop)
BIT_CASES = [(0, False), (1, True), (2, False), (4, True)]


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def tiles_of(sizes=SIZES, **kw):
    return pre.slice_geometry(sizes, S, **kw)


def inputs(seed=SEED):
    tiles = tiles_of()
    return (tiles,) + SR.tile_lists(tiles, K, seed, S, A=A, empty=EMPTY)


def merged_case(case, seed=SEED):
    metric, thr, skip, top_k, agnostic = MERGE_CASES[case]
    tiles, det, mc, protos = inputs(seed)
    return tiles, det, mc, protos, SR.merge_tiles(det, tiles, metric, thr, skip, top_k, agnostic)


def reference_shares(seed=SEED):
    """The reference's own share of in-band pixels per case of BIT_CASES, among the pixels of live planes that some tile votes on."""
    out = []
    for case, crop in BIT_CASES:
        tiles, det, mc, protos, merged = merged_case(case, seed)
        top_k = MERGE_CASES[case][3]
        W, _ = SR.vote_coefficients(det, mc, merged, tiles, top_k)
        ref = SR.vote_reference(W, merged, protos, tiles, crop)
        amb = sum(int(((r["logits"].abs() < BAND * r["contrib"]) & (r["contrib"] > 0)).sum()) for r in ref)
        tot = sum(int((r["contrib"] > 0).sum()) for r in ref)
        out.append(amb / max(tot, 1))
    return out


# ---- 1. geometry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zoom,overlap", [(1.0, 0.2), (0.73, 0.2), (1.0, 0.0), (1.37, 0.35)])
def test_tiles_cover_the_image_and_overlap(zoom, overlap):
    for (H0, W0), per in zip(SIZES, tiles_of(zoom=zoom, overlap=overlap, full_view=False)):
        seen = np.zeros((H0, W0), bool)
        for t in per:
            assert t["ox"] % UP == 0 and t["oy"] % UP == 0 and (t["pox"], t["poy"]) == (t["ox"] // UP, t["oy"] // UP)
            assert 0 <= t["wx0"] < t["wx1"] <= W0 and 0 <= t["wy0"] < t["wy1"] <= H0
            assert 0.0 < t["step"] <= 1.0 and t["step"] == float(np.float32(zoom / UP)) and t["scale"] == float(np.float32(zoom))
            assert (t["fox"], t["foy"]) == (float(t["ox"]), float(t["oy"])) and (t["height"], t["width"]) == (H0, W0)
            seen[t["wy0"]:t["wy1"], t["wx0"]:t["wx1"]] = True
            # the window is the set of pixels whose centre lies in the tile (up to the image's edge for the last tile of an axis)
            new_w = max(1, int(W0 * zoom))
            cx = (np.arange(W0) + 0.5) * zoom
            inside = (cx >= t["ox"]) & (cx < min(t["ox"] + S, new_w))
            if t["ox"] + S >= new_w:
                inside |= cx >= t["ox"]
            assert np.array_equal(np.nonzero(inside)[0], np.arange(t["wx0"], t["wx1"]))
        assert seen.all()
        for axis, L_ in (("ox", max(1, int(W0 * zoom))), ("oy", max(1, int(H0 * zoom)))):
            origins = sorted({t[axis] for t in per})
            assert origins[0] == 0 and origins[-1] + S >= L_
            assert len(origins) == (1 if L_ <= S else int(np.ceil((L_ - S * overlap) / (S * (1 - overlap)))))
            for a, b in zip(origins, origins[1:]):
                assert a + S - b >= overlap * S - UP, (axis, origins)


def test_tile_counts_and_the_full_view():
    tiles = tiles_of()
    assert [len(per) for per in tiles] == [10, 10, 1, 5]
    for n, ((H0, W0), per) in enumerate(zip(SIZES, tiles)):
        assert all(t["image"] == n for t in per)
        if len(per) == 1:
            continue
        full = per[-1]
        scale = S / max(H0, W0)
        (fH, fW, fstep, fscale, pitch, off), = pp._frame_layout(pp.frames_of([torch.zeros(H0, W0, 3)], [scale]), K, float(UP))[0]
        assert (full["height"], full["width"], full["step"], full["scale"]) == (fH, fW, fstep, fscale)
        assert (full["pox"], full["poy"], full["fox"], full["foy"]) == (0, 0, 0.0, 0.0)
        assert (full["wx0"], full["wy0"], full["wx1"], full["wy1"]) == (0, 0, W0, H0)
        assert list(full["geom"]) == list(pre.letterbox_geometry([(H0, W0)], S)[0])
    with pytest.raises(ValueError):
        pre.slice_geometry([(300, 410)], S, zoom=4.5)            # more than one prototype pixel per image pixel
    with pytest.raises(ValueError):
        pre.slice_geometry([(3000, 3000)], S)                    # more than 64 tiles


def test_a_tiles_geometry_row_draws_the_crop_of_the_resized_image():
    rng = np.random.default_rng(0)
    H0, W0, zoom = 230, 310, 0.9
    img = rng.integers(0, 256, size=(H0, W0, 3), dtype=np.uint8)
    per, = tiles_of([(H0, W0)], zoom=zoom)
    assert len(per) == 5
    for t in per:
        new_w, new_h = t["geom"][:2]
        R = O.resize_linear_u8(img, new_w, new_h)
        want = np.full((S, S, 3), 114, np.uint8)
        crop = R[t["oy"]:t["oy"] + S, t["ox"]:t["ox"] + S]
        want[:crop.shape[0], :crop.shape[1]] = crop
        want = (want[:, :, ::-1].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
        got, _ = AR.augment(img, None, t["geom"], S)
        assert np.array_equal(got, want)


# ---- 2. the merge restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(MERGE_CASES)))
def test_merge_invariants(case):
    metric, thr, skip, top_k, agnostic = MERGE_CASES[case]
    tiles, det, mc, protos, m = merged_case(case)
    ms = m["member_slot"]
    assert ms.shape == (sum(len(p) for p in tiles), K) and ms.dtype == np.int32
    free = SR.merge_tiles(det, tiles, metric, thr, skip, 64, agnostic)["counts"]          # the rows without a cut (at most 24 per image)
    t0, cut_seen, multi = 0, False, False
    for n, per in enumerate(tiles):
        T, cnt = len(per), int(m["counts"][n])
        sl = ms[t0:t0 + T]
        live = np.arange(K)[None, :] < det["counts"][t0:t0 + T, None]
        cand = live & (det["scores"][t0:t0 + T] > np.float32(skip))
        assert (sl[~cand] == -1).all() and sl.max(initial=-1) < cnt
        for r in range(top_k):
            assert int((sl == r).sum()) == int(m["n_members"][n, r])                                   # every member, once
        for r in range(cnt):
            assert sl[m["lead_tile"][n, r] - t0, m["lead_slot"][n, r]] == r                             # the leader is a member
            assert m["scores"][n, r] == det["scores"][m["lead_tile"][n, r], m["lead_slot"][n, r]]
            for tl, k in zip(*np.nonzero(sl == r)):
                fb = SR.frame_boxes(det["boxes"][t0 + tl, k], per[tl])[0]
                u = m["boxes_frame"][n, r]
                assert u[0] <= fb[0] and u[1] <= fb[1] and u[2] >= fb[2] and u[3] >= fb[3]              # the union holds every member
                assert agnostic or det["labels"][t0 + tl, k] == m["labels"][n, r]
        assert (np.diff(m["scores"][n, :cnt]) <= 0).all()
        assert (m["scores"][n, cnt:] == 0).all() and (m["labels"][n, cnt:] == -1).all() and (m["lead_tile"][n, cnt:] == -1).all()
        left = int((cand & (sl == -1)).sum())
        assert left == int(m["n_left"][n]) and cnt == min(int(free[n]), top_k)
        assert (left > 0) == (int(free[n]) > top_k)                                                    # n_left > 0 exactly when the cut bit
        cut_seen |= left > 0
        multi |= bool((m["n_members"][n] >= 2).any())
        if n in EMPTY:
            assert cnt == 0 and (sl == -1).all() and left == 0
        t0 += T
    assert cut_seen == (case in CUT_CASES)
    assert multi


def test_merge_without_matches_is_the_frame_boxes_of_the_nms_list():
    """thr = +inf on a single full-view tile: the rows are `frame_reference.frame_boxes` of the list, bit for bit."""
    sizes = SIZES[:3]
    tiles = [pre.slice_geometry([sz], S, zoom=S / max(sz), full_view=False)[0] for sz in sizes]
    assert all(len(per) == 1 for per in tiles)
    det, mc, protos = SR.tile_lists(tiles, K, SEED, S, A=A)
    m = SR.merge_tiles(det, tiles, "ios", np.inf, 0.0, K)
    for n, (H0, W0) in enumerate(sizes):
        cnt = int(det["counts"][n])
        assert cnt > 0 and int(m["counts"][n]) == cnt and (m["n_members"][n, :cnt] == 1).all() and m["n_left"][n] == 0
        want = FR.frame_boxes(torch.from_numpy(det["boxes"][n]), cnt, H0, W0, S / max(H0, W0))
        assert np.array_equal(m["boxes_frame"][n].view(np.uint32), want.numpy().view(np.uint32))
        assert np.array_equal(m["lead_slot"][n, :cnt], np.arange(cnt)) and np.array_equal(m["scores"][n], det["scores"][n])


# ---- 3. the mask restatement -------------------------------------------------------------------------------------------------
def test_single_full_view_tile_is_the_frame_operator():
    sizes = SIZES[:3]
    tiles = [pre.slice_geometry([sz], S, zoom=S / max(sz), full_view=False)[0] for sz in sizes]
    det, mc, protos = SR.tile_lists(tiles, K, SEED, S, A=A)
    m = SR.merge_tiles(det, tiles, "ios", np.inf, 0.0, K)
    W, Ss = SR.vote_coefficients(det, mc, m, tiles, K)
    vote = SR.vote_reference(W, m, protos, tiles, crop=True)
    frames = [(H0, W0, S / max(H0, W0)) for H0, W0 in sizes]
    ref = FR.frame_reference(protos, mc, torch.from_numpy(det["keep_anchor"]).clamp(min=0), det["counts"], torch.from_numpy(det["boxes"]), frames,
                             float(UP), crop=True)
    for n in range(len(sizes)):
        assert np.array_equal(Ss[n], np.float32(0) + det["scores"][n])
        diff = vote[n]["bits"] != ref[n]["bits"]
        assert not (diff & ~(ref[n]["logits"].abs() < BAND)).any()
        assert vote[n]["bits"].any() and not vote[n]["bits"][int(det["counts"][n]):].any()


def disc_case():
    """One object across two native tiles of a 160 x 284 image: a disc of radius 50 at (142, 80).  Both tiles' prototypes sample ONE global
    logit field (channel 0: radius - distance, in prototype pixels) at their own grid positions; each tile reports the part of the box
    it sees, clipped at its border.  Returns (tiles, det, mc, protos, disc bool [H0, W0])."""
    H0, W0, cx, cy, rad = 160, 284, 142.0, 80.0, 50.0
    tiles = pre.slice_geometry([(H0, W0)], S, full_view=False)
    per = tiles[0]
    assert [(t["ox"], t["oy"]) for t in per] == [(0, 0), (124, 0)]
    det = {"boxes": np.zeros((2, K, 4), np.float32), "scores": np.zeros((2, K), np.float32), "labels": np.full((2, K), -1, np.int64),
           "counts": np.ones(2, np.int32), "keep_anchor": np.full((2, K), -1, np.int32)}
    protos = torch.zeros(2, 32, G, G)
    gy, gx = torch.meshgrid(torch.arange(G, dtype=torch.float32), torch.arange(G, dtype=torch.float32), indexing="ij")
    for tl, t in enumerate(per):
        x1, x2 = max(cx - rad - t["ox"], 0.0), min(cx + rad - t["ox"], float(S))
        det["boxes"][tl, 0] = [x1, cy - rad, x2, cy + rad]
        det["scores"][tl, 0], det["labels"][tl, 0], det["keep_anchor"][tl, 0] = (0.9, 0.8)[tl], 1, 7
        px, py = (gx + t["pox"] + 0.5) * UP, (gy + t["poy"] + 0.5) * UP              # centres of the prototype pixels, image pixels
        protos[tl, 0] = (rad - torch.sqrt((px - cx) ** 2 + (py - cy) ** 2)) / UP
    mc = torch.zeros(2, 32, A)
    mc[:, 0, 7] = 1.0
    Y, X = np.mgrid[0:H0, 0:W0]
    disc = (X + 0.5 - cx) ** 2 + (Y + 0.5 - cy) ** 2 < rad ** 2
    return tiles, det, mc, protos, disc


def test_an_object_across_two_tiles_is_merged_and_voted_whole():
    tiles, det, mc, protos, disc = disc_case()
    m = SR.merge_tiles(det, tiles, "ios", 0.5, 0.0, K)
    assert int(m["counts"][0]) == 1 and int(m["n_members"][0, 0]) == 2 and (m["lead_tile"][0, 0], m["lead_slot"][0, 0]) == (0, 0)
    assert m["boxes_frame"][0, 0].tolist() == [92.0, 30.0, 192.0, 130.0]                # the union of the two clipped boxes
    assert int(SR.merge_tiles(det, tiles, "iou", 0.5, 0.0, K)["counts"][0]) == 2        # IoU 36 / 100 would keep the two parts apart
    W, Ss = SR.vote_coefficients(det, mc, m, tiles, K)
    vote = SR.vote_reference(W, m, protos, tiles, crop=True)[0]["bits"][0].numpy()
    lead = SR.vote_reference(W, m, protos, tiles, crop=True, only_tile=[[0] * K])[0]["bits"][0].numpy()
    iou = lambda a, b: (a & b).sum() / (a | b).sum()
    print(f"voted IoU {iou(vote, disc):.4f}, leader-only IoU {iou(lead, disc):.4f}")
    assert iou(vote, disc) >= 0.9 and iou(vote, disc) > iou(lead, disc)
    wx1 = tiles[0][0]["wx1"]
    assert vote[:, wx1:].any() and not lead[:, wx1:].any()                              # bits outside the leader's window


def test_reference_share_of_in_band_pixels():
    shares = reference_shares()
    print("in-band shares of the reference per case of BIT_CASES:", ", ".join(f"{s:.2e}" for s in shares))
    assert all(s <= SHARE for s in shares), shares


# ---- 4. the C boundary -------------------------------------------------------------------------------------------------------
STRUCTS = {"mtbt_tile": L.Tile, "mtbt_tile_merge_args": L.TileMergeArgs, "mtbt_tile_mask_args": L.TileMaskArgs}


def test_struct_layouts_match_the_header(lib, tmp_path):
    for which, st in enumerate(L.TILE_STRUCTS):
        assert lib.mtbt_sizeof_tile_args(which) == C.sizeof(st)
    assert lib.mtbt_sizeof_tile_args(3) == -1 and lib.mtbt_sizeof_tile_args(-1) == -1
    assert lib.mtbt_abi_version() == L.ABI_VERSION == 5
    for name in ("mtbt_merge_tiles", "mtbt_vote_tile_masks", "mtbt_sizeof_tile_args"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){']
    for cname, st in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {f[0]}));' for f in st._fields_]
    lines.append('return 0;}')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = {(a, b): int(c) for a, b, c in (l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    for cname, st in STRUCTS.items():
        assert out[(cname, "size")] == C.sizeof(st), cname
        for f in st._fields_:
            assert out[(cname, f[0])] == getattr(st, f[0]).offset, (cname, f[0])


def _table(n_images=1):
    tiles = pre.slice_geometry([(300, 410)] * n_images, S)
    table, first, _ = pp.tile_table(tiles)
    return tiles, table, first


def _merge_args():
    """Arguments that pass every check of mtbt_merge_tiles (dummy non-null, 16-byte aligned pointers: nothing may be launched)."""
    tiles, table, first = _table()
    a = L.TileMergeArgs()
    a.boxes = a.scores = a.labels = a.counts = a.anchors = a.tiles_dev = 16
    a.tiles, a.first = table, first
    a.N, a.n_tiles, a.K, a.top_k, a.metric, a.class_agnostic, a.thr, a.skip_thr = 1, 10, K, K, 1, 0, 0.5, 0.0
    a.out_boxes = a.out_scores = a.out_labels = a.out_counts = a.n_members = a.lead_tile = a.lead_slot = a.lead_anchor = a.member_slot = a.n_left = 16
    return a, table, first


def test_merge_tiles_rejects_bad_arguments_without_launching(lib):
    def run(edit=None, tile_edit=None, first_edit=None):
        a, table, first = _merge_args()
        a.boxes = 24                      # misaligned too: every EINVAL is reported first
        if edit:
            edit(a)
        if tile_edit:
            tile_edit(table)
        if first_edit:
            first_edit(first)
        return lib.mtbt_merge_tiles(C.byref(a), None)

    assert lib.mtbt_merge_tiles(None, None) == EINVAL
    for kw in (dict(N=-1), dict(K=0), dict(top_k=0), dict(metric=2), dict(metric=-1), dict(thr=float("nan")), dict(skip_thr=float("nan"))):
        assert run(lambda a: [setattr(a, k, v) for k, v in kw.items()]) == EINVAL, kw
    # N == 0 returns before the pointers are looked at
    def empty(a):
        a.N = 0
        a.scores = a.out_boxes = None
    assert run(empty) == 0
    for name in ("boxes", "scores", "labels", "counts", "tiles", "tiles_dev", "first", "out_boxes", "out_scores", "out_labels", "out_counts",
                 "n_members", "lead_tile", "lead_slot", "member_slot", "n_left", "anchors"):       # (anchors: lead_anchor is given)
        assert run(lambda a: setattr(a, name, None)) == EINVAL, name
    assert run(lambda a: setattr(a, "n_tiles", 9)) == EINVAL and run(lambda a: setattr(a, "n_tiles", 11)) == EINVAL
    assert run(lambda a: setattr(a, "K", 4096 // 10 + 1)) == EINVAL                              # T K > 4096
    assert run(first_edit=lambda f: f.__setitem__(0, 1)) == EINVAL
    assert run(first_edit=lambda f: f.__setitem__(1, -1)) == EINVAL
    for field, value in (("image", 1), ("pox", -1), ("poy", -4), ("wx1", 0), ("wy1", 0), ("wx1", 411), ("wy1", 301), ("wx0", -1), ("step", 0.0),
                         ("step", 1.5), ("step", float("nan")), ("scale", 0.0), ("fox", -4.0), ("foy", float("nan")), ("height", 0),
                         ("height", 301), ("width", 409), ("reserved", 1)):
        assert run(tile_edit=lambda t: setattr(t[3], field, value)) == EINVAL, (field, value)
    # more than 64 tiles in one image
    big = (L.Tile * 65)()
    for d in big:
        for k in pp._TILE_FIELDS:
            setattr(d, k, getattr(_table()[1][0], k))
    def many(a):
        a.tiles, a.n_tiles, a.K = big, 65, 1
        a.first = (C.c_int32 * 2)(0, 65)
    assert run(many) == EINVAL
    # then the alignment
    assert run() == EALIGN
    a, table, first = _merge_args()
    a.out_boxes = 24
    assert lib.mtbt_merge_tiles(C.byref(a), None) == EALIGN
    # a NULL anchors is fine without lead_anchor (the call would launch: stop it at the alignment check)
    def no_anchor(a):
        a.anchors = a.lead_anchor = None
    assert run(no_anchor) == EALIGN


def _mask_args():
    tiles, table, first = _table()
    a = L.TileMaskArgs()
    a.protos = a.mc = a.anchors = a.scores = a.member_slot = a.counts = a.boxes = a.tiles_dev = a.W = a.Ss = a.out = 16
    a.mc_batch_stride, a.mc_k_stride, a.mc_c_stride = 32 * A, 1, A
    a.tiles, a.first = table, first
    a.N, a.n_tiles, a.K, a.top_k, a.Tmax, a.nm, a.hp, a.wp, a.crop = 1, 10, K, K, 10, 32, G, G, 1
    fr = (L.Frame * 1)()
    fr[0].height, fr[0].width, fr[0].step, fr[0].scale, fr[0].pitch, fr[0].offset = 300, 410, 0.0, 0.0, 56, 0   # step / scale are ignored
    a.out_bytes = K * 300 * 56
    return a, fr, table, first


def test_vote_tile_masks_rejects_bad_arguments_without_launching(lib):
    def run(edit=None, fr_edit=None, tile_edit=None, first_edit=None, n_frames=1):
        a, fr, table, first = _mask_args()
        a.protos = 24                     # misaligned too: every EINVAL is reported first
        if edit:
            edit(a)
        if fr_edit:
            fr_edit(fr[0])
        if tile_edit:
            tile_edit(table)
        if first_edit:
            first_edit(first)
        return lib.mtbt_vote_tile_masks(C.byref(a), fr, n_frames, None)

    assert lib.mtbt_vote_tile_masks(None, None, 1, None) == EINVAL
    a, fr, table, first = _mask_args()
    assert lib.mtbt_vote_tile_masks(C.byref(a), None, 1, None) == EINVAL
    for name in ("protos", "mc", "anchors", "scores", "member_slot", "counts", "boxes", "tiles", "tiles_dev", "first", "W", "Ss", "out"):
        assert run(lambda a: setattr(a, name, None)) == EINVAL, name                               # (boxes: crop is set)
    for kw in (dict(N=2), dict(nm=16), dict(K=0), dict(top_k=0), dict(top_k=65536), dict(hp=0, wp=0), dict(hp=G + 1), dict(wp=G - 1), dict(Tmax=0),
               dict(Tmax=65), dict(Tmax=9), dict(out_bytes=-1), dict(out_bytes=K * 300 * 56 - 1), dict(reserved=1), dict(n_tiles=9),
               dict(K=4096 // 10 + 1)):
        assert run(lambda a: [setattr(a, k, v) for k, v in kw.items()]) == EINVAL, kw
    assert run(n_frames=0) == EINVAL and run(n_frames=33) == EINVAL
    assert run(first_edit=lambda f: f.__setitem__(0, -1)) == EINVAL and run(first_edit=lambda f: f.__setitem__(1, -1)) == EINVAL
    for field, value in (("pox", -1), ("wx1", 0), ("wy1", 301), ("step", 0.0), ("step", 1.5), ("scale", 0.0), ("fox", -4.0), ("height", 299),
                         ("width", 411), ("reserved", 1)):
        assert run(tile_edit=lambda t: setattr(t[9], field, value)) == EINVAL, (field, value)
    for fe in (lambda f: setattr(f, "pitch", 48), lambda f: setattr(f, "offset", 8), lambda f: setattr(f, "height", 0), lambda f: setattr(f, "width", 0)):
        assert run(fr_edit=fe) == EINVAL
    # a tile's `image` is not looked at here (a chunk of a larger batch keeps its absolute numbering)
    assert run(tile_edit=lambda t: setattr(t[0], "image", 5)) == EALIGN
    # then the alignment
    assert run() == EALIGN
    a, fr, table, first = _mask_args()
    a.out = 24
    assert lib.mtbt_vote_tile_masks(C.byref(a), fr, 1, None) == EALIGN
