"""The instance-mask loss on the task-aligned assignment without a GPU: the CPU restatement (tests/seg_tal_reference.py) against an
independent per-anchor, per-pixel loop, the margin condition at topk = 20 that makes the chained GPU comparison legitimate, the proof
that the feature is not a no-op (the two assignments differ on every case with positives), the C ABI of the new entry point, and the
argument checks of `TrainStep` / `ValidationStep`."""
import ctypes as C
import math
import os
import subprocess

import pytest
import torch

import mask_loss_reference as M
import seg_tal_reference as R
import tal_reference as T

from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PTR = 4096                                       # non-null, aligned dummy: every call below is refused before any launch


def _bce(x, t):
    return max(x, 0.0) - x * t + math.log1p(math.exp(-abs(x)))


@pytest.mark.parametrize("k", [1, 2, 5])
def test_restatement_equals_a_per_anchor_per_pixel_loop(k):
    """Every foreground anchor, every prototype pixel, in double precision straight from the definition in include/mtbt_hip.h."""
    c = T.case(k)
    S, (B_, nm, hp, wp) = c["kw"]["img_size"], c["protos"].shape
    asg = R.assignment(k)
    val, n_fg, _, _ = R.reference(k)
    mc, pr = c["mc"].double().numpy(), c["protos"].double().permute(0, 2, 3, 1).numpy()
    total, count = 0.0, 0
    for b in range(B_):
        gx = M.gt_rows_of(c["gt"], b, S)
        for a, g in enumerate(asg["assigned"][b].tolist()):
            if g < 0:
                continue
            q = (gx[g - asg["off"][b]] * torch.tensor([wp / S, hp / S, wp / S, hp / S])).tolist()      # one fp32 multiply per coordinate
            s = 0.0
            for y in range(hp):
                for x in range(wp):
                    if x >= q[0] and x < q[2] and y >= q[1] and y < q[3]:
                        s += _bce(float(mc[b, a] @ pr[b, y, x]), float(c["masks"][b, 0, y * (S // hp), x * (S // wp)]))
            total += s / ((q[2] - q[0]) * (q[3] - q[1]))
            count += 1
    print(f"case {k}: restatement {float(val):.7f} loop {total / count:.7f}, fg {n_fg} / {count}")
    assert count == n_fg > 0
    assert abs(total / count - float(val)) <= 1e-5 * abs(total / count)


ROW_COUNTS_TOPK20 = {1: [15, 15, 9], 2: [20, 18, 20, 20], 3: [20, 20, 20, 20, 20], 5: [15, 15, 0, 9]}


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_margin_condition_at_topk_20(k):
    """tests/test_cpu_tal.py::test_margin_condition at topk = 20: the 20th and 21st metric of every GT with more than 20 positive
    metrics differ by >= 1e-4 (relative), the two largest overlaps at every contested anchor by >= 1e-4.  The per-row counts cover one
    short of a 16-group, a full group plus a remainder, and a row without positives."""
    topk = 20
    asg = R.assignment(k, topk)
    tight_m, tight_o = R.margins(asg, topk)
    n_rows = sum(gx.shape[0] for gx, _ in asg["rows"])
    counts = [int((asg["assigned"] == r).sum()) for r in range(n_rows)]
    print(f"case {k}: tightest relative metric gap {tight_m:.3e}, tightest contested overlap gap {tight_o:.3e}, per-row counts {counts}")
    assert tight_m >= 1e-4 and tight_o >= 1e-4
    assert counts == ROW_COUNTS_TOPK20[k]


# (foreground anchors, loss) on the task-aligned assignment at topk 10, (positives, loss) of the IoU-matched mask loss
EXPECTED = {1: ((26, 1.215371), (18, 1.243259)), 2: ((40, 1.342929), (124, 1.313563)), 3: ((50, 1.392110), (252, 1.346220)),
            5: ((26, 1.215371), (18, 1.243259))}


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_the_two_assignments_differ_on_every_case_with_positives(k):
    c = T.case(k)
    val, n_fg, d_mc, d_pr = R.reference(k)
    iou_val, iou_n, iou_mc, _ = M.mask_loss_and_grads(c)
    print(f"case {k}: task-aligned {n_fg} anchors, loss {float(val):.6f}; IoU-matched {iou_n} positives, loss {float(iou_val):.6f}")
    if k == 4:
        assert n_fg == 0 and iou_n == 0 and float(val) == 0.0 and not d_mc.any() and not d_pr.any()
        return
    (want_n, want_v), (want_in, want_iv) = EXPECTED[k]
    assert n_fg == want_n and iou_n == want_in and n_fg != iou_n
    assert abs(float(val) - want_v) <= 5e-6 and abs(float(iou_val) - want_iv) <= 5e-6
    assert abs(float(val) - float(iou_val)) > 1e-2
    assert not torch.equal((d_mc != 0).any(-1), (iou_mc != 0).any(-1))           # a different set of anchors gets a gradient


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def test_header_compiles_and_the_symbol_resolves(tmp_path, lib):
    """The declaration has the prototype the issue names (a C compiler checks the assignment), `mtbt_mask_loss_args` is unchanged, and
    the library exports the symbol."""
    use, size, exe = tmp_path / "use.c", tmp_path / "size.c", tmp_path / "size"
    use.write_text('#include "mtbt_hip.h"\n'
                   'int (*probe)(const mtbt_mask_loss_args*, const int32_t*, void*) = mtbt_instance_mask_loss_assigned;\n')
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(use), "-o", str(tmp_path / "use.o")], check=True)
    size.write_text('#include <stdio.h>\n#include "mtbt_hip.h"\nint main(void){ printf("%zu\\n", sizeof(mtbt_mask_loss_args)); return 0; }\n')
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(size), "-o", str(exe)], check=True)
    got = int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert got == C.sizeof(L.MaskLossArgs) == lib.mtbt_sizeof_mask_loss_args()                           # the struct did not change
    assert "mtbt_instance_mask_loss_assigned" in L.SYMBOLS
    assert getattr(C.CDLL(L.LIB_PATH), "mtbt_instance_mask_loss_assigned") is not None
    assert lib.mtbt_abi_version() == L.ABI_VERSION == 5                                                 # additive: the version stays


def _args(lib, maps=True):
    a = L.MaskLossArgs()
    for i, h in enumerate((16, 8, 4)):
        a.h[i], a.w[i] = h, h
        if maps:
            a.map[i], a.map_pixel_stride[i] = PTR, 66
    a.n_levels, a.N, a.reg_max, a.img_size, a.iou_thresh, a.n_gt = 3, 4, 16, 128.0, 0.5, 4
    a.gt_xyxy = a.gt_off = a.mc = a.protos = a.gt_masks = a.d_mc = a.d_protos = a.workspace = a.out = PTR
    a.mc_batch_stride, a.mc_anchor_stride, a.mc_channel_stride = 336 * 32, 32, 1
    a.hp, a.wp, a.nm, a.weight = 32, 32, 32, 1.0
    a.workspace_bytes = lib.mtbt_mask_loss_workspace_bytes(4, 336, 32, 32, 32)
    return a


@pytest.mark.parametrize("field,value", [("assigned", None), ("out", None), ("workspace_bytes", -1), ("gt_xyxy", None), ("gt_off", None), ("mc", None),
                                         ("protos", None), ("gt_masks", None), ("workspace", None), ("hp", 24), ("img_size", 128.5), ("nm", 16),
                                         ("n_gt", -1), ("n_levels", 0), ("dprotos_dtype", 3)])
@pytest.mark.parametrize("maps", [True, False])
def test_entry_point_rejects_bad_arguments_without_launching(lib, field, value, maps):
    """With the NULL stream and dummy pointers any launch would fault: MTBT_EINVAL comes back before one.  `maps=False`: NULL map
    pointers, zero pixel strides and (below) a reg_max of 0 are NOT errors of this entry point, so the refusal is the field's."""
    assert lib.mtbt_instance_mask_loss_assigned(None, PTR, None) == EINVAL
    a = _args(lib, maps)
    if not maps:
        a.reg_max = 0
    assigned = PTR
    if field == "assigned":
        assigned = None
    else:
        setattr(a, field, a.workspace_bytes - 1 if field == "workspace_bytes" else value)
    assert lib.mtbt_instance_mask_loss_assigned(C.byref(a), assigned, None) == EINVAL


def test_misaligned_buffers_are_refused(lib):
    a = _args(lib, maps=False)
    a.d_mc = PTR + 4
    assert lib.mtbt_instance_mask_loss_assigned(C.byref(a), PTR, None) == -2


# ---- the steps' argument checks: before any device work -------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(mask_assign="tal"), dict(mask_assign="tal", instance_mask_weight=1.0),
                                dict(mask_assign="tal", det_loss="tal"), dict(mask_assign="tal", det_loss="tal", instance_mask_weight=0.0),
                                dict(mask_assign="hungarian", det_loss="tal", instance_mask_weight=1.0), dict(mask_assign="hungarian")])
def test_steps_refuse_a_mask_assignment_they_cannot_run(kw):
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    from multitask_bonetumor_yolo_amd.validate import ValidationStep
    with pytest.raises(ValueError, match="mask_assign"):
        TrainStep(None, (2, 3, 128, 128), **kw)
    with pytest.raises(ValueError, match="mask_assign"):
        ValidationStep(None, img_size=128, **kw)


def test_validation_step_checks_det_loss_like_trainstep():
    from multitask_bonetumor_yolo_amd.validate import ValidationStep
    with pytest.raises(ValueError, match="det_loss"):
        ValidationStep(None, det_loss="hungarian")
    with pytest.raises(ValueError, match="tal"):
        ValidationStep(None, tal=dict(topk=13))
    with pytest.raises(ValueError, match="instance_mask_weight"):
        ValidationStep(None, instance_mask_weight=-1.0)


def test_group_gt_rows_is_group_gt_rows_cls():
    """One definition of the row order that `assigned` relies on (CPU tensors: device-side tensor ops only, no kernel of ours)."""
    from multitask_bonetumor_yolo_amd.loss import group_gt_rows, group_gt_rows_cls
    gt = torch.cat([T.case(5)["gt"], torch.tensor([[7, 0, .5, .5, .1, .1], [-1, 1, .5, .5, .1, .1]])])[torch.tensor([3, 0, 6, 4, 1, 5, 2])]
    xyxy, off = group_gt_rows(gt, 3, 64.0)
    xyxy2, cls, off2 = group_gt_rows_cls(gt, 3, 64.0)
    assert torch.equal(xyxy, xyxy2) and torch.equal(off, off2) and cls.shape == (7,)
    assert off.tolist() == [0, 2, 3, 4]
    assert group_gt_rows_cls(gt, 3, 64.0, want_cls=False)[1] is None
    e_xyxy, e_off = group_gt_rows(gt[:0], 3, 64.0)
    assert tuple(e_xyxy.shape) == (1, 4) and e_off.tolist() == [0, 0, 0, 0]
