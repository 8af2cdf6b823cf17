"""CPU checks of the instance-mask loss: the torch restatement the GPU tests compare against (tests/mask_loss_reference.py) equals an
independent per-positive, per-pixel loop and its autograd gradients equal the closed form; the named cases have the properties the
GPU tests rely on; `mtbt_mask_loss_args` matches its ctypes mirror; the entry point refuses bad arguments before any launch."""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B

import mask_loss_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PTR = 4096                                       # non-null, aligned dummy: every call below is refused before any launch


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def _bce(x, t):
    return max(x, 0.0) - x * t + math.log1p(math.exp(-abs(x)))


def test_restatement_equals_a_per_pixel_loop():
    """Case 1 (S = 64): every positive, every prototype pixel, in plain Python floats (fp64) from the definition."""
    c = R.case(1)
    S, (B_, nm, hp, wp) = c["kw"]["img_size"], c["protos"].shape
    val, n_pos, _, _ = R.reference(1)
    total, count = 0.0, 0
    for b, (pos, gi, gx) in enumerate(R.match(c["det"], c["gt"], S)):
        for a, g in zip(pos.tolist(), gi.tolist()):
            q = (gx[g] * torch.tensor([wp / S, hp / S, wp / S, hp / S])).tolist()          # one fp32 multiply per coordinate
            s = 0.0
            for y in range(hp):
                for x in range(wp):
                    if x >= q[0] and x < q[2] and y >= q[1] and y < q[3]:
                        logit = float((c["mc"][b, a].double() * c["protos"][b, :, y, x].double()).sum())
                        s += _bce(logit, float(c["masks"][b, 0, y * (S // hp), x * (S // wp)]))
            total += s / ((q[2] - q[0]) * (q[3] - q[1]))
            count += 1
    assert count == n_pos > 0
    assert abs(total / count - float(val)) <= 1e-5 * abs(total / count)


@pytest.mark.parametrize("k", [1, 2])
def test_autograd_equals_the_closed_form(k):
    """r = weight (sigmoid(logit) - t) / (norm area) inside the box; d_mc = r . protos, d_protos = sum over positives of r . mc."""
    c, weight = R.case(k), 0.7
    S, (B_, nm, hp, wp) = c["kw"]["img_size"], c["protos"].shape
    _, n_pos, d_mc, d_pr = R.mask_loss_and_grads(c, weight)
    tgt = c["masks"][:, 0, ::S // hp, ::S // wp]
    xs, ys = torch.arange(wp, dtype=torch.float32)[None, None, :], torch.arange(hp, dtype=torch.float32)[None, :, None]
    want_mc, want_pr = torch.zeros_like(d_mc), torch.zeros_like(d_pr)
    for b, (pos, gi, gx) in enumerate(R.match(c["det"], c["gt"], S)):
        if pos.numel() == 0:
            continue
        q = gx[gi] * torch.tensor([wp / S, hp / S, wp / S, hp / S])
        inside = (xs >= q[:, 0, None, None]) & (xs < q[:, 2, None, None]) & (ys >= q[:, 1, None, None]) & (ys < q[:, 3, None, None])
        logits = torch.einsum("pc,chw->phw", c["mc"][b][pos], c["protos"][b])
        area = (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
        r = weight * (torch.sigmoid(logits) - tgt[b]) * inside / (n_pos * area)[:, None, None]
        want_mc[b, pos] = torch.einsum("phw,chw->pc", r, c["protos"][b])
        want_pr[b] = torch.einsum("phw,pc->chw", r, c["mc"][b][pos])
    for got, want in ((d_mc, want_mc), (d_pr, want_pr)):
        assert want.abs().max() > 0
        assert (got - want).abs().max() <= 1e-5 * want.abs().max()
        assert torch.equal(got == 0, want == 0)


def _overlap_targets(c, b, rows):
    S, hp = c["kw"]["img_size"], c["protos"].shape[2]
    q = R.gt_rows_of(c["gt"], b, S)[rows] * (hp / S)
    x1, y1, x2, y2 = q[:, 0].max(), q[:, 1].max(), q[:, 2].min(), q[:, 3].min()
    t = c["masks"][b, 0, ::S // hp, ::S // hp]
    ys, xs = torch.meshgrid(torch.arange(hp, dtype=torch.float32), torch.arange(hp, dtype=torch.float32), indexing="ij")
    return t[(xs >= x1) & (xs < x2) & (ys >= y1) & (ys < y2)]


def test_cases_have_the_properties_the_gpu_tests_rely_on():
    c1, c2, c3 = R.case(1), R.case(2), R.case(3)
    # case 1: S = 64, B = 3, A = 84, 16 x 16 prototypes; two overlapping boxes of image 0 both with positives, targets of both values
    # in the overlap, image 1 without GT, fractional box edges
    assert c1["A"] == 84 and tuple(c1["protos"].shape) == (3, 32, 16, 16)
    p1 = R.positives_per_gt(c1)
    assert len(p1) == 3 and p1[0] > 0 and p1[1] > 0
    ov = _overlap_targets(c1, 0, [0, 1])
    assert ov.numel() > 0 and (ov == 0).any() and (ov == 1).any()
    assert not (c1["gt"][:, 0] == 1).any()
    q = torch.cat([R.gt_rows_of(c1["gt"], b, 64) for b in range(3)]) * (16 / 64)
    assert (q != q.round()).any(dim=1).all()
    # case 2: S = 128, B = 4, A = 336, 32 x 32 prototypes; > 64 positives on one GT, none on another of the same image, a box equal
    # to the whole image, a box across the image border
    assert c2["A"] == 336 and tuple(c2["protos"].shape) == (4, 32, 32, 32)
    p2 = R.positives_per_gt(c2)
    assert max(p2) > 64
    assert (p2[0] == 0) != (p2[1] == 0)                                   # image 0: one of its two rows has none
    assert R.gt_rows_of(c2["gt"], 2, 128).tolist() == [[0.0, 0.0, 128.0, 128.0]]
    edge = R.gt_rows_of(c2["gt"], 3, 128)[0]                              # left and bottom edges on / beyond the image border
    assert edge[0] <= 0 and edge[3] >= 128 and p2[3] > 0
    # case 3: the model's anchor and prototype counts, several boxes per image
    assert c3["A"] == 8400 and tuple(c3["protos"].shape) == (2, 32, 160, 160)
    assert all(n > 0 for n in R.positives_per_gt(c3)) and len(R.gt_rows_of(c3["gt"], 1, 640)) == 3
    # case 4: nothing to match
    val, n_pos, d_mc, d_pr = R.reference(4)
    assert float(val) == 0 and n_pos == 0 and not d_mc.any() and not d_pr.any()


def test_struct_layout_matches_the_header(tmp_path, lib):
    name, st = "mtbt_mask_loss_args", L.MaskLossArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mtbt_hip.h"', 'int main(void){', f'printf("{name} %zu\\n", sizeof({name}));']
    lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in st._fields_]
    lines.append('return 0;}')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out[name]) == C.sizeof(st) == lib.mtbt_sizeof_mask_loss_args()
    for f, _ in st._fields_:
        assert int(out[f"{name}.{f}"]) == getattr(st, f).offset, f
    assert lib.mtbt_abi_version() == 5
    for sym in ("mtbt_mask_loss_workspace_bytes", "mtbt_instance_mask_loss", "mtbt_sizeof_mask_loss_args"):
        assert sym in L.SYMBOLS


def _args(lib):
    a = L.MaskLossArgs()
    for i, h in enumerate((16, 8, 4)):
        a.map[i], a.h[i], a.w[i], a.map_pixel_stride[i] = PTR, h, h, 66
    a.n_levels, a.N, a.reg_max, a.img_size, a.iou_thresh, a.n_gt = 3, 4, 16, 128.0, 0.5, 4
    a.gt_xyxy = a.gt_off = a.mc = a.protos = a.gt_masks = a.d_mc = a.d_protos = a.workspace = a.out = PTR
    a.mc_batch_stride, a.mc_anchor_stride, a.mc_channel_stride = 336 * 32, 32, 1
    a.hp, a.wp, a.nm, a.weight = 32, 32, 32, 1.0
    a.workspace_bytes = lib.mtbt_mask_loss_workspace_bytes(4, 336, 32, 32, 32)
    return a


@pytest.mark.parametrize("field,value", [("gt_xyxy", None), ("gt_off", None), ("mc", None), ("protos", None), ("gt_masks", None), ("out", None),
                                         ("workspace", None), ("hp", 24), ("wp", 48), ("img_size", 128.5), ("nm", 16), ("nm", 64),
                                         ("workspace_bytes", -1), ("n_gt", -1), ("n_levels", 0), ("dprotos_dtype", 3)])
def test_entry_point_rejects_bad_arguments_without_launching(lib, field, value):
    assert lib.mtbt_instance_mask_loss(None, None) == EINVAL
    a = _args(lib)
    if field == "workspace_bytes":
        value = a.workspace_bytes - 1
    setattr(a, field, value)
    assert lib.mtbt_instance_mask_loss(C.byref(a), None) == EINVAL


def test_missing_map_and_workspace_size(lib):
    a = _args(lib)
    a.map[1] = None
    assert lib.mtbt_instance_mask_loss(C.byref(a), None) == EINVAL
    assert lib.mtbt_mask_loss_workspace_bytes(4, 336, 32, 32, 32) >= 3 * 4 * 336 * 4       # match, positive list, per-positive loss for ALL anchors
    assert lib.mtbt_mask_loss_workspace_bytes(4, 336, 32, 32, 16) == 0 and lib.mtbt_mask_loss_workspace_bytes(0, 336, 32, 32, 32) == 0


def test_cpu_tensors_raise():
    from multitask_bonetumor_yolo_amd import InstanceMaskLoss, instance_mask_loss  # noqa: F401
    c = R.case(1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        instance_mask_loss(c["det"], c["mc"], c["protos"], c["gt"], c["masks"], img_size=64)
