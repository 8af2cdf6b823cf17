"""`distance_transform` (mtbt_distance_transform, csrc/distance_transform.hip) against tests/edt_reference.py: both maps EXACTLY, on
the shapes at which the two passes change path (one pixel, a second word, an odd tail, a full word, several words and rows) and on the
contents they can go wrong on (no target at all, the longest distances, one row / column, a checkerboard, blobs, sparse and dense noise).
The reference is exhaustive search (held against scipy in tests/test_cpu_edt.py) and is computed once per shape."""
import functools

import numpy as np
import pytest
import torch

import edt_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import distance_transform, signed_distance
    from multitask_bonetumor_yolo_amd.postprocess import D2_NONE


@functools.lru_cache(maxsize=None)
def cases(shape):
    """(names, dense planes [n, H, W], d2_set [n, H, W], d2_unset) of one shape, computed once."""
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    names, planes = zip(*R.plane_cases(rng, *shape))
    maps = [R.d2_maps(m) for m in planes]
    return names, np.stack(planes), np.stack([a for a, _ in maps]), np.stack([b for _, b in maps])


def dev_maps(planes, W, pad_ones=False, **kw):
    packed = torch.from_numpy(R.pack_bits(planes, pad_ones=pad_ones)).to(DEV)
    out = distance_transform(packed, W, **kw)
    torch.cuda.synchronize()
    return out


def same(got: torch.Tensor, ref: np.ndarray, names):
    got = got.cpu().numpy().astype(np.int64)
    for i, name in enumerate(names):
        bad = np.argwhere(got[i] != ref[i])
        assert len(bad) == 0, (name, len(bad), bad[:4].tolist(), got[i][tuple(bad[0])], ref[i][tuple(bad[0])])


@pytest.mark.parametrize("shape", R.SHAPES)
def test_both_maps_are_exact(shape):
    names, planes, r_set, r_unset = cases(shape)
    assert D2_NONE == R.NONE
    assert (r_set[0] == R.NONE).all() and (r_unset[1] == R.NONE).all()          # the empty and the full plane: the sentinel everywhere
    d_set, d_unset = dev_maps(planes, shape[1], to="both")
    assert d_set.dtype == d_unset.dtype == torch.uint32 and tuple(d_set.shape) == planes.shape
    same(d_set, r_set, names)
    same(d_unset, r_unset, names)
    # garbage in the padding bits X >= W changes nothing
    g_set, g_unset = dev_maps(planes, shape[1], pad_ones=True, to="both")
    assert torch.equal(g_set.view(torch.int32), d_set.view(torch.int32)) and torch.equal(g_unset.view(torch.int32), d_unset.view(torch.int32))
    # each output on its own (the other pointer NULL) is the same map
    assert torch.equal(dev_maps(planes, shape[1], to="set").view(torch.int32), d_set.view(torch.int32))
    assert torch.equal(dev_maps(planes, shape[1], to="unset").view(torch.int32), d_unset.view(torch.int32))
    # and a second run gives the same bits
    again = dev_maps(planes, shape[1], to="both")
    assert torch.equal(again[0].view(torch.int32), d_set.view(torch.int32)) and torch.equal(again[1].view(torch.int32), d_unset.view(torch.int32))


def test_a_training_canvas_is_exact():
    """640 x 640, two lesion-like blobs and a pixel in the far corner: distances of several hundred pixels, ten words a row."""
    H = W = 640
    rng = np.random.default_rng(640)
    m = np.zeros((H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    for cy, cx, ry, rx in ((200, 180, 40, 55), (420, 470, 30, 22)):
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    m &= rng.uniform(size=(H, W)) < 0.97                                        # pinholes: d2_unset is not trivial inside
    m[H - 1, 0] = True
    r_set, r_unset = R.d2_maps(m, pairs=False)
    assert r_set.max() > 300 ** 2
    d_set, d_unset = dev_maps(m[None], W, to="both")
    same(d_set, r_set[None], ["canvas/set"])
    same(d_unset, r_unset[None], ["canvas/unset"])


def test_more_planes_than_a_chunk_and_prefilled_outputs():
    """70 planes in one call (the chunks hold 64 and share the workspace), through the entry point with 0xFF-prefilled outputs: every word
    is written, and plane j of the second chunk is not plane j of the first."""
    import ctypes as C
    from multitask_bonetumor_yolo_amd import _lib as L
    shape = (37, 64)
    names, planes, r_set, r_unset = cases(shape)
    k = len(names)
    pick = [(3 * i + 1) % k for i in range(70)]
    packed = torch.from_numpy(R.pack_bits(planes[pick])).to(DEV)
    outs = [torch.full((70,) + shape, -1, dtype=torch.int32, device=DEV) for _ in range(2)]
    lib = L.load()
    nb = lib.mtbt_distance_transform_workspace_bytes(70, *shape)
    assert nb == lib.mtbt_distance_transform_workspace_bytes(64, *shape)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    a = L.DistanceTransformArgs()
    a.packed, a.workspace, a.workspace_bytes, a.d2_set, a.d2_unset = packed.data_ptr(), ws.data_ptr(), nb, outs[0].data_ptr(), outs[1].data_ptr()
    a.n, a.H, a.W, a.pitch = 70, shape[0], shape[1], 8
    L.check(lib.mtbt_distance_transform(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mtbt_distance_transform")
    torch.cuda.synchronize()
    same(outs[0].view(torch.uint32), r_set[pick], [names[i] for i in pick])
    same(outs[1].view(torch.uint32), r_unset[pick], [names[i] for i in pick])
    assert distance_transform(packed[:0], shape[1]).shape == (0,) + shape         # n == 0 launches nothing


def test_signed_distance_is_the_reference_phi():
    shape = (70, 130)
    names, planes, r_set, r_unset = cases(shape)
    phi = signed_distance(torch.from_numpy(R.pack_bits(planes)).to(DEV), shape[1]).cpu().numpy()
    ref = np.stack([R.phi_of(m, a, b) for m, a, b in zip(planes, r_set, r_unset)])
    assert phi.dtype == np.float32
    # fp32 of an exact float64 sqrt, then one fp32 subtraction: 2^-24 relative each, and d - 1 at d >= sqrt(2) loses under two bits
    np.testing.assert_allclose(phi, ref, rtol=1e-6, atol=0)
    assert not phi[0].any() and not phi[1].any()
