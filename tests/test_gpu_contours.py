"""The device contour tracer and run-length encoder (`postprocess.trace_contours`, `rle_encode`, `coco_segm_results`; csrc/contours.hip)
against the restatement (tests/contour_reference.py, held against the fill rule, the component labelling and scipy.ndimage in
tests/test_cpu_contours.py): every output is an integer and every comparison is exact.

Shapes: the smallest that reach each path -- a single pixel, a single row, pitches 8, 16 and 24 on both sides of a 64-bit word boundary
(W = 64: the lattice row is one vertex longer than the last pixel word) -- and one 640 x 640 plane.  Contents: `plane_cases` of the
component tests (empty, full, corners, a checkerboard: the most vertices a plane can have and a saddle at every inner lattice point, a
serpentine: one contour through every row, a U, a comb: the longest column walks, bars and diagonals over the word boundaries, noise)
and the hand-written planes of the restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_reference as CR
import contour_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (1, 70), (37, 64), (33, 65), (40, 130), (96, 200)]
CONNS = (4, 8)
CAP = 4096                                       # the checkerboard of 96 x 200 has 9600 contours under connectivity 4: over the cap
TABLES = ("offset", "count", "area2", "start", "hole")

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import _lib as L
    from multitask_bonetumor_yolo_amd import (ConvNeXtBiFPNYOLO, coco_segm_results, contour_polygons, count_contour_vertices, fill_polygons,
                                              init_synthetic_, label_components, rle_encode, rle_from_string, synthetic_images, trace_contours)
    from multitask_bonetumor_yolo_amd.postprocess import detect_and_segment, unpack_masks


def _pack(planes, pad_ones=False):
    return torch.from_numpy(CR.pack_bits(np.stack(planes), pad_ones)).to(DEV)


def _assert_result(got, want, what=""):
    """Every output of `trace_contours` against `stack_records`; vertex rows from n_vertices on are unspecified."""
    nv = got["n_vertices"].cpu().numpy()
    assert nv.dtype == np.int32 and np.array_equal(nv, want["n_vertices"]), (what, "n_vertices")
    assert np.array_equal(got["n_contours"].cpu().numpy(), want["n_contours"]), (what, "n_contours")
    verts = got["vertices"].cpu().numpy()
    assert verts.dtype == np.int32 and verts.shape[2] == 2
    for b in range(len(nv)):
        if want["n_contours"][b] >= 0:
            assert np.array_equal(verts[b, :nv[b]], want["vertices"][b, :nv[b]]), (what, "vertices", b)
    for k in TABLES:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), (what, k)
    assert got["area2"].dtype == torch.int64 and got["boxes"].dtype == torch.float32
    assert np.array_equal(got["boxes"].cpu().numpy(), want["box"].astype(np.float32)), (what, "boxes")


@pytest.fixture(scope="module")
def cases():
    """Per shape: (names, planes, {connectivity: reference result}), computed once; the hand-written planes under their own keys."""
    out = {}
    for i, (H, W) in enumerate(SHAPES):
        cs = CR.plane_cases(np.random.default_rng(20 + i), H, W)
        planes = [m for _, m in cs]
        out[(H, W)] = ([n for n, _ in cs], planes, {c: R.stack_records(planes, c, CAP) for c in CONNS})
    for name, m in R.hand_planes():
        out[name] = ([name], [m], {c: R.stack_records([m], c, CAP) for c in CONNS})
    return out


@pytest.fixture(scope="module")
def big():
    m = CR.big_plane(np.random.default_rng(6))
    return m, {c: R.stack_records([m], c, 8192) for c in CONNS}


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_contours_equal_the_restatement(cases, shape, conn):
    names, planes, want = cases[shape]
    w = want[conn]
    V = int(w["n_vertices"].max())
    got = trace_contours(_pack(planes), shape[1], connectivity=conn, max_contours=CAP, max_vertices=V)
    assert got["shape"] == shape and got["vertices"].shape == (len(planes), V, 2) and got["component"] is None
    _assert_result(got, w, f"{shape} {conn}")
    padded = trace_contours(_pack(planes, True), shape[1], connectivity=conn, max_contours=CAP, max_vertices=V)   # set padding bits X >= W change nothing
    _assert_result(padded, w, f"{shape} {conn} padded")
    exact = trace_contours(_pack(planes, True), shape[1], connectivity=conn, max_contours=CAP)                   # the counting pass sizes it
    assert exact["vertices"].shape == (len(planes), V, 2)
    _assert_result(exact, w, f"{shape} {conn} max_vertices=None")
    only = count_contour_vertices(_pack(planes, True), shape[1])
    assert only.dtype == torch.int32 and np.array_equal(only.cpu().numpy(), w["n_vertices"])
    roomy = trace_contours(_pack(planes), shape[1], connectivity=conn, max_contours=CAP, max_vertices=2 * shape[0] * shape[1] + 777)
    _assert_result(roomy, w, f"{shape} {conn} roomy")                                                           # more room than any plane can use


@pytest.mark.parametrize("conn", CONNS)
def test_hand_written_planes(cases, conn):
    for name, _ in R.hand_planes():
        _, planes, want = cases[name]
        H, W = planes[0].shape
        got = trace_contours(_pack(planes, True), W, connectivity=conn, max_contours=CAP)
        _assert_result(got, want[conn], f"{name} {conn}")
    saddle = trace_contours(_pack(cases["saddle"][1]), 2, connectivity=conn, max_contours=4)
    assert saddle["n_contours"].tolist() == [2 if conn == 4 else 1] and saddle["count"][0].tolist() == ([4, 4, 0, 0] if conn == 4 else [8, 0, 0, 0])


@pytest.mark.parametrize("conn", CONNS)
def test_large_plane(big, conn):
    m, want = big
    w = want[conn]
    assert 1024 < w["n_contours"][0] <= 8192
    got = trace_contours(_pack([m]), 640, connectivity=conn, max_contours=8192)
    _assert_result(got, w, f"640 {conn}")
    lab = label_components(_pack([m]), 640, connectivity=conn, max_components=8192)
    outer = ~got["hole"][0] & (got["count"][0] > 0)
    first = lab["first"][0, :int(lab["n_components"][0])]
    assert int(outer.sum()) == int(lab["n_components"][0])                                                        # C
    assert torch.equal(got["start"][0][outer], (first // 640) * 641 + first % 640)


def test_capacities_cut_tables_and_refuse_planes(cases):
    names, planes, want = cases[(40, 130)]
    W = 130
    i = names.index("checker")
    for conn in CONNS:
        w = want[conn]
        cut = R.stack_records(planes, conn, 8)
        assert (w["n_contours"] > 8).sum() >= 4                                      # several planes are over the table
        got = trace_contours(_pack(planes), W, connectivity=conn, max_contours=8, max_vertices=int(w["n_vertices"].max()))
        _assert_result(got, cut, f"cap 8, {conn}")                                   # the tables are cut, the vertices complete, the counts true
        assert got["offset"].shape == (len(planes), 8) and int(got["n_contours"][i]) == (2600 if conn == 4 else w["n_contours"][i])
    # max_vertices one below the largest count: that plane alone is refused, its neighbours are untouched and correct
    w = want[4]
    V = int(w["n_vertices"].max()) - 1
    over = R.stack_records(planes, 4, CAP, max_vertices=V)
    assert (over["n_contours"] == -1).sum() == 1 and over["n_contours"][i] == -1 and not over["count"][i].any()
    got = trace_contours(_pack(planes), W, connectivity=4, max_contours=CAP, max_vertices=V)
    _assert_result(got, over, "max_vertices - 1")
    assert int(got["n_vertices"][i]) == V + 1
    none = trace_contours(_pack(planes), W, connectivity=4, max_contours=4, max_vertices=0)      # only the empty plane fits no room at all
    assert none["n_contours"].tolist() == [0 if n == "empty" else -1 for n in names] and not none["count"].any() and not none["start"].any()
    assert np.array_equal(none["n_vertices"].cpu().numpy(), w["n_vertices"])


def _raw_trace(packed, H, W, conn, Cap, V, guard=64):
    """`mtbt_trace_contours` through the C ABI on buffers with `guard` extra words of 0x5A behind each: -> (dict of the buffers, the fill)."""
    lib = L.load()
    n = packed.shape[0]
    fill = 0x5A5A5A5A
    def buf(words, dtype=torch.int32):
        t = torch.empty(words + guard, dtype=dtype, device=DEV)
        t.view(torch.uint8).fill_(0x5A)
        return t
    b = {"n_vertices": buf(n), "n_contours": buf(n), "vertices": buf(n * V * 2), "offset": buf(n * Cap), "count": buf(n * Cap),
         "area2": buf(n * Cap, torch.int64), "box": buf(n * Cap * 4), "start": buf(n * Cap)}
    need = int(lib.mtbt_contours_workspace_bytes(n, H, W, V))
    ws = buf((need + 3) // 4)
    a = L.ContoursArgs()
    a.packed, a.workspace, a.workspace_bytes = packed.data_ptr(), ws.data_ptr(), need
    for k, t in b.items():
        setattr(a, k, t.data_ptr())
    a.n, a.H, a.W, a.pitch, a.connectivity, a.max_contours, a.max_vertices = n, H, W, packed.shape[2], conn, Cap, V
    assert lib.mtbt_trace_contours(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    b["workspace"] = ws
    sizes = {"n_vertices": n, "n_contours": n, "vertices": n * V * 2, "offset": n * Cap, "count": n * Cap, "area2": n * Cap, "box": n * Cap * 4,
             "start": n * Cap, "workspace": (need + 3) // 4}
    return b, sizes, fill


def test_refused_plane_leaves_neighbours_and_guards_alone(cases):
    names, planes, want = cases[(33, 65)]
    H, W = 33, 65
    w = want[8]
    i = int(w["n_vertices"].argmax())
    V, Cap = int(w["n_vertices"][i]) - 1, 16
    over = R.stack_records(planes, 8, Cap, max_vertices=V)
    b, sizes, fill = _raw_trace(_pack(planes, True), H, W, 8, Cap, V)
    n = len(planes)
    for k, t in b.items():                                                           # nothing behind any buffer was touched
        tail = t[sizes[k]:].view(torch.uint8)
        assert bool((tail == 0x5A).all()), k
    assert np.array_equal(b["n_vertices"][:n].cpu().numpy(), over["n_vertices"]) and np.array_equal(b["n_contours"][:n].cpu().numpy(), over["n_contours"])
    assert over["n_contours"][i] == -1 and (over["n_contours"] >= 0).sum() == n - 1
    verts = b["vertices"][:n * V * 2].view(n, V, 2).cpu().numpy()
    for j in range(n):
        if j != i:
            nv = over["n_vertices"][j]
            assert np.array_equal(verts[j, :nv], over["vertices"][j, :nv]), j
            assert (verts[j, nv:] == fill).all(), j                                  # rows past a plane's vertices are not written
    for k, per in (("offset", 1), ("count", 1), ("area2", 1), ("box", 4), ("start", 1)):
        assert np.array_equal(b[k][:n * Cap * per].view(n, Cap, *([4] if per == 4 else [])).cpu().numpy(), over[k]), k   # zero rows of the refused plane too


@pytest.mark.parametrize("conn", CONNS)
def test_device_round_trip_through_fill_polygons_and_components(cases, conn):
    for shape in ((33, 65), (40, 130)):
        names, planes, want = cases[shape]
        H, W = shape
        packed = _pack(planes)
        lab = label_components(packed, W, connectivity=conn, max_components=CAP)
        got = trace_contours(packed, W, connectivity=conn, max_contours=CAP, labels=lab["labels"])
        polys, plane_of = [], []
        for b in range(len(planes)):
            ps = contour_polygons(got, b, holes=True)
            assert len(ps) == want[conn]["n_contours"][b]
            polys += ps
            plane_of += [b] * len(ps)
        filled = unpack_masks(fill_polygons(polys, H, W, device=DEV), W).to(torch.int32)     # every contour a plane of its own
        acc = torch.zeros((len(planes), H, W), dtype=torch.int32, device=DEV).index_add_(0, torch.tensor(plane_of, device=DEV), filled)
        assert torch.equal((acc & 1).bool(), unpack_masks(packed, W))                          # A: the XOR of the fills is the plane
        assert int(got["area2"].sum()) == 2 * int(unpack_masks(packed, W).sum())               # B
        comp, hole, used = got["component"], got["hole"], got["count"] > 0
        for b in range(len(planes)):
            nc = int(lab["n_components"][b])
            outer = used[b] & ~hole[b]
            assert comp[b][outer].tolist() == list(range(1, nc + 1))                           # C: the outer contours are the components, in id order
            hs = torch.nonzero(used[b] & hole[b]).flatten()
            sy, sx = got["start"][b][hs] // (W + 1), got["start"][b][hs] % (W + 1)
            assert torch.equal(comp[b][hs], lab["labels"][b][sy.long(), sx.long()]) and bool((comp[b][hs] > 0).all())
        assert not bool(comp[~used].any())


def test_seventy_planes_overwrite_prefilled_outputs_and_repeat_bit_for_bit(cases, monkeypatch):
    names, planes, want = cases[(40, 130)]
    idx = [(7 * i) % len(planes) for i in range(70)]          # 70 planes: more than one launch group of 64
    packed = _pack([planes[i] for i in idx])
    w = {k: v[idx] for k, v in want[8].items()}
    V = int(w["n_vertices"].max())
    real_empty = torch.empty

    def filled(*args, **kw):                                  # every output (and the workspace) starts as 0xFF bytes
        t = real_empty(*args, **kw)
        t.view(torch.uint8).fill_(0xFF)
        return t

    monkeypatch.setattr(torch, "empty", filled)
    first = trace_contours(packed, 130, connectivity=8, max_contours=CAP, max_vertices=V)
    again = trace_contours(packed, 130, connectivity=8, max_contours=CAP, max_vertices=V)
    monkeypatch.undo()
    _assert_result(first, w, "70 planes")
    for k in ("n_vertices", "n_contours", "offset", "count", "area2", "start", "boxes"):
        assert torch.equal(first[k], again[k]), k
    nv = first["n_vertices"].tolist()
    assert all(torch.equal(first["vertices"][b, :nv[b]], again["vertices"][b, :nv[b]]) for b in range(70))


def test_graph_capture_replays_the_eager_result(cases):
    names, planes, want = cases[(40, 130)]
    w = want[4]
    V = int(w["n_vertices"].max())
    packed = _pack(planes)
    eager = trace_contours(packed, 130, connectivity=4, max_contours=CAP, max_vertices=V)
    eager_runs = rle_encode(packed, 130, max_runs=64)
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        trace_contours(packed, 130, connectivity=4, max_contours=CAP, max_vertices=V)          # warm-up: the code objects are loaded
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            held = trace_contours(packed, 130, connectivity=4, max_contours=CAP, max_vertices=V)
            held_runs = rle_encode(packed, 130, max_runs=64)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(2):
        for t in [held[k] for k in ("n_vertices", "n_contours", "vertices", "offset", "count", "area2", "start")] + list(held_runs):
            t.fill_(-3)
        graph.replay()
        torch.cuda.synchronize()
        for k in ("n_vertices", "n_contours", "offset", "count", "area2", "start"):
            assert torch.equal(held[k], eager[k]), k
        for b, nv in enumerate(w["n_vertices"]):
            assert torch.equal(held["vertices"][b, :nv], eager["vertices"][b, :nv])
        assert torch.equal(held_runs[1], eager_runs[1])
        for b, nr in enumerate(eager_runs[1].tolist()):
            assert torch.equal(held_runs[0][b, :min(nr, 64)], eager_runs[0][b, :min(nr, 64)])


# ---- run lengths ----------------------------------------------------------------------------------------------------------------------
def _assert_runs(planes, W, pad_ones):
    want = [R.rle_counts(m) for m in planes]
    counts, n_runs = rle_encode(_pack(planes, pad_ones), W)
    assert counts.dtype == torch.int32 and n_runs.dtype == torch.int32 and counts.shape == (len(planes), max(len(c) for c in want))
    assert n_runs.tolist() == [len(c) for c in want]
    got = counts.cpu().numpy()
    for b, c in enumerate(want):
        assert got[b, :len(c)].tolist() == c, b
    return want


@pytest.mark.parametrize("shape", SHAPES + [(300, 1), (1, 300), (130, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_run_lengths_equal_the_restatement(shape):
    H, W = shape                                                   # 300 x 1 and 130 x 40: more than one band of 128 rows; W = 1: a single column
    planes = [m for _, m in CR.plane_cases(np.random.default_rng(60 + H), H, W)]
    want = _assert_runs(planes, W, False)
    _assert_runs(planes, W, True)
    assert want[0] == [H * W] and want[1] == [0, H * W]            # empty, full


def test_run_capacity_cuts_and_keeps_the_guard():
    H, W, Rcap, guard = 40, 130, 7, 64
    planes = [m for _, m in CR.plane_cases(np.random.default_rng(3), H, W)]
    want = [R.rle_counts(m) for m in planes]
    assert sum(len(c) > Rcap for c in want) >= 5 and sum(len(c) <= Rcap for c in want) >= 2
    counts, n_runs = rle_encode(_pack(planes), W, max_runs=Rcap)
    assert n_runs.tolist() == [len(c) for c in want] and counts.shape == (len(planes), Rcap)
    lib, n, packed = L.load(), len(planes), _pack(planes, True)
    buf = torch.full((n * Rcap + guard,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    nr = torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    need = int(lib.mtbt_rle_workspace_bytes(n, H, W))
    ws = torch.full(((need + 3) // 4 + guard,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    a = L.RleArgs()
    a.packed, a.workspace, a.workspace_bytes, a.counts, a.n_runs = packed.data_ptr(), ws.data_ptr(), need, buf.data_ptr(), nr.data_ptr()
    a.n, a.H, a.W, a.pitch, a.max_runs = n, H, W, packed.shape[2], Rcap
    assert lib.mtbt_rle_encode(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((buf[n * Rcap:] == 0x5A5A5A5A).all()) and bool((nr[n:] == 0x5A5A5A5A).all()) and bool((ws[(need + 3) // 4:] == 0x5A5A5A5A).all())
    rows = buf[:n * Rcap].view(n, Rcap).cpu().numpy()
    for b, c in enumerate(want):
        k = min(len(c), Rcap)
        assert rows[b, :k].tolist() == c[:k] and (rows[b, k:] == 0x5A5A5A5A).all(), b          # only R runs, and nothing past a plane's own
        assert counts[b, :k].tolist() == c[:k]
    assert nr[:n].tolist() == [len(c) for c in want]


def test_coco_results_decode_back_to_the_frame_masks():
    torch.manual_seed(0)
    model = init_synthetic_(ConvNeXtBiFPNYOLO(2, 2, pretrained_backbone=False), seed=0).to(DEV).eval()
    S = 64
    frames = [(80, 100, S / 100.0), (64, 64, 1.0)]
    with torch.no_grad():
        out = model(synthetic_images(2, S, seed=1).to(DEV), "infer")
    _, mc, protos = out["segment_protos"]
    det = detect_and_segment(out["detect_features"], mc, protos, S, frames=frames)
    kept = det["counts"].tolist()
    assert sum(kept) > 0, "the synthetic model keeps no box"
    res = coco_segm_results(det, [11, 12], category_ids={0: 5, 1: 9}, frames=frames)
    assert len(res) == sum(kept) and [r["image_id"] for r in res] == [11] * kept[0] + [12] * kept[1]
    at = 0
    for b, (H0, W0, _) in enumerate(frames):
        dense = unpack_masks(det["masks_frame"][b], W0).cpu().numpy()
        for j in range(kept[b]):
            r = res[at]
            at += 1
            assert r["segmentation"]["size"] == [H0, W0] and r["category_id"] == {0: 5, 1: 9}[int(det["labels"][b, j])]
            assert r["score"] == float(det["scores"][b, j])
            x1, y1, x2, y2 = det["boxes_frame"][b, j].tolist()
            assert r["bbox"] == [x1, y1, x2 - x1, y2 - y1]
            runs = rle_from_string(r["segmentation"]["counts"])
            assert sum(runs) == H0 * W0 and np.array_equal(R.rle_decode(runs, H0, W0), dense[j]), (b, j)


@pytest.mark.parametrize("shape", [(7, 63), (9, 127)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_padding_bit_in_the_last_word(shape):
    """W % 64 == 63, below and above 64: one padding bit in the last word, where a wrong valid_bits shows: contours and run lengths of a full plane, noise, and a last column with a middle row, padding bits set."""
    H, W = shape
    rng = np.random.default_rng(W)
    planes = [np.ones((H, W), bool), rng.uniform(size=(H, W)) < 0.5, np.zeros((H, W), bool)]
    planes[2][:, W - 1] = planes[2][H // 2, :] = True
    for conn in CONNS:
        got = trace_contours(_pack(planes, True), W, connectivity=conn, max_contours=CAP)
        _assert_result(got, R.stack_records(planes, conn, CAP), f"{shape} {conn}")
    want = _assert_runs(planes, W, True)
    assert want[0] == [0, H * W]
