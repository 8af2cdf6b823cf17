"""CPU checks of the frame operator (masks and boxes in the original image frame, bit-packed): the reference restatement
(tests/frame_reference.py) against the oracle at identity frames, the packed layout, and the additive C ABI -- symbols, struct
layouts and every argument error `mtbt_masks_to_frames` returns before a launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import frame_reference as FR
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B
from oracle import postprocess as opp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    B.build()  # no-op when up to date; hipcc cross-compiles without a GPU
    return L.load()


def test_reference_at_identity_frames_equals_the_oracle():
    g = torch.Generator().manual_seed(11)
    nm, hp, wp, K, S = 32, 40, 40, 21, 160
    protos = torch.randn(nm, hp, wp, generator=g)
    co = torch.randn(K, nm, generator=g)
    ref, masks = opp.assemble_masks(co, protos, (S, S))
    mine = FR.frame_logits(co, protos, S, S, 1.0, 4.0)
    assert (ref - mine).abs().max().item() < 1e-5
    assert torch.equal(mine > 0, masks)


@pytest.mark.parametrize("W0", [1, 7, 64, 65, 130])
def test_pack_unpack_round_trip_and_zero_padding(W0):
    g = torch.Generator().manual_seed(W0)
    bits = torch.rand(3, 5, W0, generator=g) > 0.5
    packed = FR.pack_bits(bits)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (3, 5, 8 * ((W0 + 63) // 64))
    allbits = FR.unpack_bits(packed, W0)
    assert torch.equal(allbits[:, :, :W0], bits)
    assert not allbits[:, :, W0:].any()
    # pixel X is bit X & 7 of byte X >> 3
    k, y, x = 1, 2, W0 - 1
    assert bool((int(packed[k, y, x >> 3]) >> (x & 7)) & 1) == bool(bits[k, y, x])
    # the device-side unpack of the package is the same map (torch shifts; runs on any device)
    from multitask_bonetumor_yolo_amd.postprocess import unpack_masks
    assert torch.equal(unpack_masks(packed, W0), bits)


def test_boxes_divide_by_scale_and_clamp():
    H0, W0, scale = 97, 211, 160 / 211
    boxes = torch.tensor([[10.0, 5.0, 100.0, 60.0], [-3.0, -1.0, 170.0, 90.0], [159.5, 73.2, 160.0, 73.6], [1.0, 2.0, 3.0, 4.0]])
    out = FR.frame_boxes(boxes, 3, H0, W0, scale)
    s = np.float32(scale)
    assert out[0].tolist() == [float(np.float32(v) / s) for v in (10.0, 5.0, 100.0, 60.0)]
    assert out[1].tolist() == [0.0, 0.0, float(W0), float(H0)]
    assert out[2, 2].item() == min(float(np.float32(160.0) / s), float(W0)) and out[2, 3].item() == min(float(np.float32(73.6) / s), float(H0))
    assert out[3].tolist() == [0.0] * 4                     # k >= count


def test_new_symbols_are_exported_and_bound(lib):
    for name in ("mtbt_masks_to_frames", "mtbt_sizeof_frame_args"):
        assert name in L.SYMBOLS and hasattr(lib, name)
    assert len(L.ARG_STRUCTS) == 10 and lib.mtbt_sizeof_args(10) == -1      # the ABI is additive
    assert lib.mtbt_abi_version() == L.ABI_VERSION == 5
    assert lib.mtbt_sizeof_frame_args(0) == C.sizeof(L.Frame)
    assert lib.mtbt_sizeof_frame_args(1) == C.sizeof(L.FrameMaskArgs)
    assert lib.mtbt_sizeof_frame_args(2) == -1 and lib.mtbt_sizeof_frame_args(-1) == -1


def test_frame_struct_layouts_match_header(tmp_path):
    probes = {
        "mtbt_frame": (L.Frame, ["height", "width", "step", "scale", "pitch", "offset"]),
        "mtbt_frame_mask_args": (L.FrameMaskArgs, ["protos", "coeff", "coeff_batch_stride", "coeff_k_stride", "coeff_c_stride", "gather_idx", "counts",
                                                   "boxes", "boxes_frame", "out", "out_bytes", "N", "K", "nm", "hp", "wp", "crop"]),
    }
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){']
    for cname, (_, fields) in probes.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f in fields:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, (ct, fields) in probes.items():
        assert int(out[cname]) == C.sizeof(ct), cname
        for f in fields:
            assert int(out[f"{cname}.{f}"]) == getattr(ct, f).offset, f"{cname}.{f}"


def _valid_call(n=2, K=3):
    """An argument block that passes every check (dummy non-null, 16-byte aligned pointers; never launched on the CPU box because
    each test breaks one rule)."""
    a = L.FrameMaskArgs()
    a.protos = a.coeff = a.gather_idx = a.counts = a.boxes = a.boxes_frame = a.out = 4096
    a.coeff_batch_stride, a.coeff_k_stride, a.coeff_c_stride = 300 * 32, 32, 1
    a.N, a.K, a.nm, a.hp, a.wp, a.crop = n, K, 32, 40, 40, 0
    fr = (L.Frame * n)()
    off = 0
    for i, (H0, W0) in enumerate([(97, 211), (211, 97)][:n]):
        fr[i].height, fr[i].width = H0, W0
        fr[i].scale = 160 / max(H0, W0)
        fr[i].step = 160 / max(H0, W0) / 4
        fr[i].pitch = 8 * ((W0 + 63) // 64)
        fr[i].offset = off
        off = (off + K * H0 * fr[i].pitch + 15) // 16 * 16
    a.out_bytes = off
    return a, fr


def _breakers():
    def null_ptr(field):
        def f(a, fr):
            setattr(a, field, None)
        return f

    def frame(field, value, i=1):
        def f(a, fr):
            setattr(fr[i], field, value)
        return f

    def args(field, value):
        def f(a, fr):
            setattr(a, field, value)
        return f

    def crop_without_boxes(a, fr):
        a.crop, a.boxes, a.boxes_frame = 1, None, None

    return {
        "null protos": null_ptr("protos"), "null coeff": null_ptr("coeff"), "null out": null_ptr("out"),
        "N != n_frames": args("N", 3),
        "step zero": frame("step", 0.0), "step negative": frame("step", -0.25), "step above one": frame("step", 1.0001),
        "step nan": frame("step", float("nan")),
        "pitch not 8*ceil(W/64)": frame("pitch", 8), "pitch too wide": frame("pitch", 40, i=0),
        "offset misaligned": frame("offset", 8, i=0),
        "plane range past out_bytes": args("out_bytes", 1000),
        "offset past out_bytes": frame("offset", 1 << 40),
        "nm != 32": args("nm", 16),
        "crop without boxes": crop_without_boxes,
    }


@pytest.mark.parametrize("case", sorted(_breakers()))
def test_argument_errors_return_einval_before_any_launch(lib, case):
    a, fr = _valid_call()
    _breakers()[case](a, fr)
    assert lib.mtbt_masks_to_frames(C.byref(a), fr, 2, None) == -1, case


def test_null_blocks_and_frame_count_are_refused(lib):
    a, fr = _valid_call()
    assert lib.mtbt_masks_to_frames(None, fr, 2, None) == -1
    assert lib.mtbt_masks_to_frames(C.byref(a), None, 2, None) == -1
    assert lib.mtbt_masks_to_frames(C.byref(a), fr, 0, None) == -1
    a.N = 33
    big = (L.Frame * 33)()
    assert lib.mtbt_masks_to_frames(C.byref(a), big, 33, None) == -1


def test_python_layer_refuses_frames_outside_the_supported_range():
    from multitask_bonetumor_yolo_amd import postprocess as pp
    rows, total = pp._frame_layout([(97, 211, 160 / 211), (1, 70, 160 / 70)], 21, 4.0)
    assert [r[4] for r in rows] == [32, 16] and rows[1][5] % 16 == 0 and rows[1][5] >= 21 * 97 * 32
    assert total >= rows[1][5] + 21 * 1 * 16
    assert rows[0][2] == FR.frame_step(160 / 211, 4.0)
    with pytest.raises(ValueError, match="long side"):
        pp._frame_layout([(30, 30, 160 / 30)], 21, 4.0)        # step = 1.33: the image is smaller than the prototype grid
    with pytest.raises(ValueError, match="long side"):
        pp._frame_layout([(30, 30, 0.0)], 21, 4.0)
