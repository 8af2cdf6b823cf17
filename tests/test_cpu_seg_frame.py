"""The semantic mask in the image frame (`mtbt_seg_to_frames`, `postprocess.seg_to_frames`) without a GPU: the restatement in
tests/seg_frame_reference.py against a float64 evaluation and against torch's own conv + interpolate, the properties of the rule
(orientations, blending of overlapping tiles), the host's checks and the C boundary."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import seg_frame_reference as SG
from test_cpu_slice import BAND, SHARE, SIZES
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from multitask_bonetumor_yolo_amd import postprocess as pp
from multitask_bonetumor_yolo_amd import preprocess as pre
from multitask_bonetumor_yolo_amd.validate import ValidationStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, G = 160, 40
SEED = 11
EINVAL, EALIGN = -1, -2
REL = 1e-5          # of max |logit|: the fp32 rule against its float64 evaluation


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def orient_protos(P, o):
    """[N, 32, G, G] numpy prototypes as the pass over view `o` would produce them (`orient_batch`'s pixel rule)."""
    return pp.orient_batch(torch.from_numpy(P), o).numpy()


def sliced_case(seed=SEED, blend="gaussian", dtype=np.float32):
    tiles = pre.slice_geometry(SIZES, S)
    NT = sum(len(per) for per in tiles)
    P, q = SG.inputs(seed, (NT, 32, G, G))
    frames = [(H0, W0, S / max(H0, W0)) for H0, W0 in SIZES]
    tab = pp.seg_blend_table(blend, G)
    return SG.seg_reference([P], [q], frames, [0], [1.0], tiles=tiles, tab=tab, dtype=dtype)[0]


def test_fp32_restatement_stays_close_to_float64():
    lo, hi = sliced_case(dtype=np.float32), sliced_case(dtype=np.float64)
    for a, b in zip(lo, hi):
        top = np.abs(b["logits"]).max()
        err = np.abs(a["logits"].astype(np.float64) - b["logits"]).max()
        print(f"max |logit| {top:.3f}, fp32 - fp64 {err:.3e}")
        assert err <= REL * top
        assert np.array_equal(a["den"] > 0, b["den"] > 0) and (b["den"] > 0).all()      # the tiles cover every pixel


def test_one_source_is_the_trainers_conv_and_interpolate():
    """One source, orient 0, weight 1, no blend, identity frame: Conv2d(32, 1, 1) then F.interpolate(bilinear, align_corners=False), the
    reference trainer's formula (running_main_v3.py:251-255)."""
    P, q = SG.inputs(SEED, (2, 32, G, G))
    ref, _ = SG.seg_reference([P], [q], [(S, S, 1.0)] * 2, [0], [1.0])
    low = Fn.conv2d(torch.from_numpy(P).double(), torch.from_numpy(q[:32]).double().view(1, 32, 1, 1), torch.from_numpy(q[32:]).double())
    want = Fn.interpolate(low, size=(S, S), mode="bilinear", align_corners=False)[:, 0].numpy()
    for n in range(2):
        assert np.abs(ref[n]["logits"] - want[n]).max() <= REL * np.abs(want[n]).max()


def test_the_eight_orients_of_one_tensor_agree():
    P, q = SG.inputs(SEED + 1, (1, 32, G, G))
    single, low0 = SG.seg_reference([P], [q], [(S, S, 1.0)], [0], [1.0])
    passes = [orient_protos(P, o) for o in range(8)]
    both, low = SG.seg_reference(passes, [q] * 8, [(S, S, 1.0)], list(range(8)), [1.0] * 8)
    for o in range(8):      # the projector is per pixel: the upright logits of every view are the identity pass's, bit for bit
        assert np.array_equal(SG.upright(low[o], o), low0[0]), o
    hi, _ = SG.seg_reference([P], [q], [(S, S, 1.0)], [0], [1.0], dtype=np.float64)
    top = np.abs(hi[0]["logits"]).max()
    assert np.abs(both[0]["logits"].astype(np.float64) - hi[0]["logits"]).max() <= REL * top
    assert np.abs(single[0]["logits"].astype(np.float64) - hi[0]["logits"]).max() <= REL * top


def test_two_overlapping_tiles_blend_between_their_taps():
    H0, W0 = 100, 260
    tiles = pre.slice_geometry([(H0, W0)], S, full_view=False)
    assert len(tiles[0]) == 2
    t0, t1 = tiles[0]
    assert t1["wx0"] < t0["wx1"] < W0 and t0["wx0"] == 0 and t1["wx1"] == W0
    P, q = SG.inputs(SEED + 2, (2, 32, G, G))
    tab = pp.seg_blend_table("tent", G)
    fr = [(H0, W0, S / W0)]
    ref, low = SG.seg_reference([P], [q], fr, [0], [1.0], tiles=tiles, tab=tab)
    v = ref[0]["logits"]
    taps = [SG.blend_frame(H0, W0, [{"L": low[i], "tile": t, "orient": 0, "weight": 1.0, "blend": False}], None, 0.0)["logits"]
            for i, t in enumerate((t0, t1))]
    tol = REL * np.abs(v).max()
    ov = slice(t1["wx0"], t0["wx1"])
    lo, hi = np.minimum(taps[0], taps[1])[:, ov], np.maximum(taps[0], taps[1])[:, ov]
    assert (v[:, ov] >= lo - tol).all() and (v[:, ov] <= hi + tol).all()
    assert np.abs(v[:, :t1["wx0"]] - taps[0][:, :t1["wx0"]]).max() <= tol        # only the first tile sees these ...
    assert np.abs(v[:, t0["wx1"]:] - taps[1][:, t0["wx1"]:]).max() <= tol        # ... and only the second these
    # the tent hands over: at the first tile's last column its weight is the smaller one
    assert np.abs(v[:, t0["wx1"] - 1] - taps[1][:, t0["wx1"] - 1]).mean() < np.abs(v[:, t0["wx1"] - 1] - taps[0][:, t0["wx1"] - 1]).mean()


@pytest.mark.parametrize("g", [40, 37, 160, 1, 2])
def test_default_tables_are_positive_and_symmetric(g):
    assert pp.seg_blend_table("constant", g) is None
    for name in ("gaussian", "tent"):
        tab = pp.seg_blend_table(name, g)
        assert tab.dtype == np.float32 and tab.shape == (g,)
        assert np.isfinite(tab).all() and (tab > 0).all() and np.array_equal(tab, tab[::-1]) and tab.max() <= 1.0
        assert tab.argmax() in ((g - 1) // 2, g // 2)


def test_reference_share_of_in_band_pixels():
    """The cross-check against `proto_projector_logits` on the GPU leaves out the pixels whose restated |logit| < BAND; their share."""
    P, q = SG.inputs(SEED, (3, 32, G, G))
    ref, _ = SG.seg_reference([P], [q], [(S, S, 1.0)] * 3, [0], [1.0])
    v = np.stack([r["logits"] for r in ref])
    share = float((np.abs(v) < BAND).mean())
    print(f"in-band share of the restatement at seed {SEED}: {share:.2e} (logit sigma {v.std():.2f})")
    assert share <= SHARE


def test_host_checks_raise_value_errors():
    P = torch.zeros((1, 32, G, G))
    pj = (torch.zeros(32), torch.zeros(1))
    fr = [(S, S, 1.0)]
    tiles = pre.slice_geometry([(384, 512)], S)
    assert len(tiles[0]) == 13
    with pytest.raises(ValueError, match="65 sources"):      # 5 passes x 13 tiles
        pp.seg_to_frames([torch.zeros((13, 32, G, G))] * 5, pj, [(384, 512, S / 512)], tiles=tiles)
    with pytest.raises(ValueError, match="65 passes"):
        pp.seg_to_frames([P] * 65, pj, fr, orients=[0] * 65)
    with pytest.raises(ValueError, match="weights"):
        pp.seg_to_frames([P, P], pj, fr, orients=(0, 1), weights=(1.0, 0.0))
    with pytest.raises(ValueError, match="weights"):
        pp.seg_to_frames(P, pj, fr, weights=(float("nan"),))
    bad = np.ones(G, np.float32)
    bad[7] = 0.0
    with pytest.raises(ValueError, match="blend table"):
        pp.seg_to_frames(P, pj, fr, blend=bad)
    bad[7] = -1.0
    with pytest.raises(ValueError, match="blend table"):
        pp.seg_to_frames(P, pj, fr, blend=bad)
    with pytest.raises(ValueError, match="blend"):
        pp.seg_to_frames(P, pj, fr, blend="cosine")
    with pytest.raises(ValueError, match="orients"):
        pp.seg_to_frames(P, pj, fr, orients=(8,))
    with pytest.raises(ValueError, match="prototypes"):
        pp.seg_to_frames(torch.zeros((1, 16, G, G)), pj, fr)
    with pytest.raises(ValueError, match="seg_views"):
        ValidationStep(None, seg_views=True)
    with pytest.raises(RuntimeError, match="MI355X"):       # and with everything in order: no CPU path
        pp.seg_to_frames(P, pj, fr)


# ---- the C boundary ----------------------------------------------------------------------------------------------------------------
STRUCTS = {"mtbt_seg_source": L.SegSource, "mtbt_seg_frame_args": L.SegFrameArgs}


def test_struct_layouts_match_the_header(lib, tmp_path):
    for which, st in enumerate(L.SEG_FRAME_STRUCTS):
        assert lib.mtbt_sizeof_seg_frame_args(which) == C.sizeof(st)
    assert lib.mtbt_sizeof_seg_frame_args(2) == -1 and lib.mtbt_sizeof_seg_frame_args(-1) == -1
    assert lib.mtbt_abi_version() == L.ABI_VERSION == 5
    for name in ("mtbt_seg_to_frames", "mtbt_seg_frame_workspace_bytes", "mtbt_sizeof_seg_frame_args"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert lib.mtbt_seg_frame_workspace_bytes(13, G) == 13 * G * G * 4
    assert lib.mtbt_seg_frame_workspace_bytes(0, G) == 0 and lib.mtbt_seg_frame_workspace_bytes(1, 0) == 0
    cname_of = lambda f: "pass" if f == "pass_" else f
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){']
    for cname, st in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname} {f[0]} %zu\\n", offsetof({cname}, {cname_of(f[0])}));' for f in st._fields_]
    lines.append('return 0;}')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = {(a, b): int(c) for a, b, c in (l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    for cname, st in STRUCTS.items():
        assert out[(cname, "size")] == C.sizeof(st), cname
        for f in st._fields_:
            assert out[(cname, f[0])] == getattr(st, f[0]).offset, (cname, f[0])


def _args():
    """Arguments that pass every check of mtbt_seg_to_frames (dummy non-null, 16-byte aligned pointers: nothing may be launched): the
    ten sources of one pass over the tiles of a 300 x 410 image, blended under the tent."""
    tiles = pre.slice_geometry([(300, 410)], S)
    src, table, first, tab, g = pp._seg_plan([(10, 32, G, G)], [(300, 410, S / 410)], (0,), None, tiles, "tent", 4.0)
    a = L.SegFrameArgs()
    a.protos[0], a.pass_items[0] = 16, 10
    a.proj = a.sources_dev = a.tiles_dev = a.tab_dev = a.workspace = a.out = a.logits = 16
    a.sources, a.tiles, a.first, a.tab = src, table, first, tab.ctypes.data_as(C.POINTER(C.c_float))
    a.workspace_bytes, a.out_bytes, a.logits_floats = 10 * G * G * 4, 300 * 56, 300 * 410
    a.threshold = 0.0
    a.N, a.n_sources, a.n_passes, a.n_proj, a.nm, a.hp, a.wp = 1, 10, 1, 1, 32, G, G
    fr = (L.Frame * 1)()
    fr[0].height, fr[0].width, fr[0].step, fr[0].scale, fr[0].pitch, fr[0].offset = 300, 410, 0.0, 0.0, 56, 0   # step / scale are ignored
    return a, fr, (src, table, first, tab)


def test_seg_to_frames_rejects_bad_arguments_without_launching(lib):
    def run(edit=None, fr_edit=None, src_edit=None, tile_edit=None, first_edit=None, tab_edit=None, n_frames=1):
        a, fr, (src, table, first, tab) = _args()
        a.protos[0] = 24                  # misaligned too: every EINVAL is reported first
        for fn, arg in ((edit, a), (fr_edit, fr[0]), (src_edit, src), (tile_edit, table), (first_edit, first), (tab_edit, tab)):
            if fn:
                fn(arg)
        return lib.mtbt_seg_to_frames(C.byref(a), fr, n_frames, None)

    assert lib.mtbt_seg_to_frames(None, None, 1, None) == EINVAL
    a, fr, keep = _args()
    assert lib.mtbt_seg_to_frames(C.byref(a), None, 1, None) == EINVAL
    for name in ("proj", "sources", "sources_dev", "tiles", "tiles_dev", "first", "workspace", "out", "tab", "tab_dev"):   # (tab: a source blends)
        assert run(lambda a: setattr(a, name, None)) == EINVAL, name
    assert run(lambda a: a.protos.__setitem__(0, None)) == EINVAL
    assert run(n_frames=0) == EINVAL and run(n_frames=33) == EINVAL
    for kw in (dict(N=2), dict(nm=16), dict(hp=0, wp=0), dict(hp=G + 1), dict(wp=G - 1), dict(n_passes=0), dict(n_passes=65), dict(n_proj=0),
               dict(reserved=1), dict(n_sources=9), dict(out_bytes=-1), dict(out_bytes=300 * 56 - 1), dict(threshold=float("nan")),
               dict(workspace_bytes=10 * G * G * 4 - 1), dict(logits_floats=300 * 410 - 1), dict(logits_floats=-1)):
        assert run(lambda a: [setattr(a, k, v) for k, v in kw.items()]) == EINVAL, kw
    assert run(first_edit=lambda f: f.__setitem__(0, -1)) == EINVAL and run(first_edit=lambda f: f.__setitem__(1, -1)) == EINVAL
    assert run(first_edit=lambda f: f.__setitem__(1, 11)) == EINVAL
    for field, value in (("pass_", 1), ("pass_", -1), ("slot", 10), ("slot", -1), ("orient", 8), ("orient", -1), ("weight", 0.0), ("weight", -1.0),
                         ("weight", float("nan")), ("proj", 1), ("proj", -1), ("blend", 2), ("blend", -1)):
        assert run(src_edit=lambda s: setattr(s[3], field, value)) == EINVAL, (field, value)
    assert run(src_edit=lambda s: s[3].reserved.__setitem__(1, 1)) == EINVAL
    for value in (0.0, -0.5, float("nan"), float("inf")):
        assert run(tab_edit=lambda t: t.__setitem__(5, value)) == EINVAL, value
    for field, value in (("pox", -1), ("wx1", 0), ("wy1", 301), ("step", 0.0), ("step", 1.5), ("scale", 0.0), ("fox", -4.0), ("height", 299),
                         ("width", 411), ("reserved", 1)):
        assert run(tile_edit=lambda t: setattr(t[9], field, value)) == EINVAL, (field, value)
    for fe in (lambda f: setattr(f, "pitch", 48), lambda f: setattr(f, "offset", 8), lambda f: setattr(f, "height", 0), lambda f: setattr(f, "width", 0)):
        assert run(fr_edit=fe) == EINVAL
    for off in (-4, 2, 4):                                    # negative, no multiple of 4, the image leaves the buffer
        assert run(lambda a: a.logits_offset.__setitem__(0, off)) == EINVAL, off
    # more than 64 sources for one image
    big_s, big_t = (L.SegSource * 65)(), (L.Tile * 65)()
    _, _, (src, table, _, _) = _args()
    for i in range(65):
        C.memmove(C.byref(big_s[i]), C.byref(src[9]), C.sizeof(L.SegSource))
        C.memmove(C.byref(big_t[i]), C.byref(table[9]), C.sizeof(L.Tile))
    def many(a):
        a.sources, a.tiles, a.n_sources, a.workspace_bytes = big_s, big_t, 65, 65 * G * G * 4
        a.first = (C.c_int32 * 2)(0, 65)
    assert run(many) == EINVAL
    # no table is needed when no source blends
    def no_table(a):
        a.tab = a.tab_dev = None
    def constant(s):
        for d in s:
            d.blend = 0
    assert run(no_table, src_edit=constant) == EALIGN
    # then the alignment
    assert run() == EALIGN
    for name in ("out", "workspace", "logits"):
        a, fr, keep = _args()
        setattr(a, name, 24)
        assert lib.mtbt_seg_to_frames(C.byref(a), fr, 1, None) == EALIGN, name
