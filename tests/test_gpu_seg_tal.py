"""Device instance-mask loss on a GIVEN assignment (csrc/mask_loss.hip `mtbt_instance_mask_loss_assigned`, `instance_mask_loss(assigned=)`)
against the CPU restatement of its definition (tests/seg_tal_reference.py): value and both gradients with the assignment uploaded from
the CPU reference (the mask kernels independently of the assigner), the chained path behind `task_aligned_det_loss`, a hand-made
assignment that runs the loop over further 16-positive groups, out-of-range entries, layouts, determinism, the accumulate form, NULL
map pointers and the autograd node `TaskAlignedSegLoss`.  Bounds: those of tests/test_gpu_mask_loss.py."""
import ctypes as C

import pytest
import torch

import seg_tal_reference as R
import tal_reference as T

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import TaskAlignedSegLoss, instance_mask_loss, task_aligned_det_loss
    from multitask_bonetumor_yolo_amd import _lib as L
    from multitask_bonetumor_yolo_amd.loss import group_gt_rows

DEV = "cuda:0"
W = 0.7           # the gradients are those of W * mask_loss


def _i32(assigned):
    return assigned.to(torch.int32).to(DEV)


def _run(k, assigned, *, weight=W, grads=True, mc=None, **kw):
    c = T.case(k)
    mc = c["mc"].to(DEV) if mc is None else mc
    return instance_mask_loss([d.to(DEV) for d in c["det"]], mc, c["protos"].to(DEV), c["gt"].to(DEV), c["masks"].to(DEV), weight=weight,
                              with_grads=grads, img_size=c["kw"]["img_size"], assigned=assigned, **kw)


def _check(tag, got, want, fg_rows):
    """n_fg exact, value within 2e-4 max(1, |want|), gradients within 1e-4 of the reference's largest entry, background rows of d_mc
    exactly zero.  -> (relative value error, d_mc error / scale, d_protos error / scale)."""
    (val, n), g = got
    want_v, want_n, want_mc, want_pr = want
    verr = abs(float(val) - float(want_v)) / max(1.0, abs(float(want_v)))
    print(f"{tag}: value {float(val):.7f} reference {float(want_v):.7f} (relative error {verr:.3e}), n_fg {int(n)} reference {want_n}")
    assert int(n) == want_n
    assert verr <= 2e-4
    errs = []
    for name, x, y in (("mc", g["mc"].cpu(), want_mc), ("protos", g["protos"].float().cpu(), want_pr)):
        assert x.shape == y.shape
        err, scale = (x - y).abs().max().item(), y.abs().max().item()
        print(f"{tag} d_{name}: max error {err:.3e}, max |want| {scale:.3e}")
        assert scale > 0 and err <= 1e-4 * scale, (name, err, scale)
        errs.append(err / scale)
    assert int(fg_rows.sum()) == want_n
    assert not g["mc"].cpu()[~fg_rows].any()
    assert torch.equal((g["mc"].cpu() != 0).any(-1), (want_mc != 0).any(-1))
    assert torch.equal((g["protos"].cpu() != 0).any(1), (want_pr != 0).any(1))
    return verr, errs[0], errs[1]


@pytest.mark.parametrize("topk", [10, 20])
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_value_and_gradients_match_the_reference_on_an_uploaded_assignment(k, topk):
    asg = R.assignment(k, topk)
    got = _run(k, _i32(asg["assigned"]))
    _check(f"case {k} topk {topk}", got, R.reference(k, topk, W), asg["assigned"] >= 0)
    val, n = _run(k, _i32(asg["assigned"]), grads=False)              # the value-only form returns the same bits
    assert torch.equal(val, got[0][0]) and torch.equal(n, got[0][1])


def test_no_gt_gives_zero_loss_and_gradients_written_whole():
    c = T.case(4)
    B, nm, hp, wp = c["protos"].shape
    assigned = torch.full((B, c["A"]), -1, dtype=torch.int32, device=DEV)
    buf = {"mc": torch.full((B, c["A"], nm), 3.0, device=DEV), "protos": torch.full((B, hp, wp, nm), 3.0, device=DEV)}
    (val, n), g = _run(4, assigned, grad_out=buf)
    assert float(val) == 0.0 and int(n) == 0
    assert not buf["mc"].any() and not buf["protos"].any() and not g["mc"].any() and not g["protos"].any()
    want = R.reference(4, 10, W)
    assert float(want[0]) == 0.0 and want[1] == 0


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_chained_behind_the_task_aligned_loss_equals_the_uploaded_assignment(k):
    c = T.case(k)
    _, assigned, _ = task_aligned_det_loss([d.to(DEV) for d in c["det"]], c["gt"].to(DEV), img_size=c["kw"]["img_size"], nc_det=T.NC,
                                           reg_max=c["kw"]["reg_max"], want_assignment=True)
    (v0, n0), g0 = _run(k, assigned)
    (v1, n1), g1 = _run(k, _i32(R.assignment(k)["assigned"]))
    assert int(n0) > 0
    assert torch.equal(v0, v1) and torch.equal(n0, n1) and torch.equal(g0["mc"], g1["mc"]) and torch.equal(g0["protos"], g1["protos"])


def _hand_made():
    """Case 2 (S = 128, A = 336): every anchor of image 0 on row 0 -- 21 groups of 16, more than the 16 in flight, so the loop over
    further groups runs; image 2's single row on every third anchor; the rest background."""
    c = T.case(2)
    off = R.offsets_of(c)
    assert c["A"] == 336 and off == [0, 2, 2, 3]
    assigned = torch.full((4, 336), -1, dtype=torch.long)
    assigned[0, :] = 0
    assigned[2, ::3] = off[2]
    return c, assigned, off


def test_hand_made_assignment_runs_the_loop_over_further_groups():
    c, assigned, off = _hand_made()
    want = R.mask_loss_assigned(c, assigned, off, W)
    assert want[1] == 336 + 112
    _check("hand-made", _run(2, _i32(assigned)), want, assigned >= 0)


def test_out_of_range_entries_are_background():
    """Another image's row, n_gt, n_gt + 7 and -5 are background and never used as an index: bit-identical to -1 at those places."""
    c = T.case(1)
    asg = R.assignment(1)
    n_gt = c["gt"].shape[0]
    assert n_gt == 3 and asg["off"] == [0, 2, 2]
    clean = asg["assigned"].clone()
    fg0, bg0 = torch.nonzero(clean[0] >= 0).flatten(), torch.nonzero(clean[0] < 0).flatten()
    fg2 = torch.nonzero(clean[2] >= 0).flatten()
    poison = [(0, int(fg0[0]), 2), (0, int(bg0[0]), 2), (2, int(fg2[0]), 0), (2, int(fg2[1]), 1), (1, 5, 2), (1, 6, 0),
              (0, int(fg0[1]), n_gt), (0, int(fg0[2]), n_gt + 7), (2, int(fg2[2]), -5), (1, 7, n_gt + 7), (0, int(bg0[1]), -5)]
    dirty = clean.clone()
    for b, a, v in poison:
        dirty[b, a] = v
        clean[b, a] = -1
    (v0, n0), g0 = _run(1, _i32(clean))
    (v1, n1), g1 = _run(1, _i32(dirty))
    assert int(n0) == int((clean >= 0).sum()) > 0
    assert torch.equal(v0, v1) and torch.equal(n0, n1) and torch.equal(g0["mc"], g1["mc"]) and torch.equal(g0["protos"], g1["protos"])
    _check("poisoned", ((v1, n1), g1), R.mask_loss_assigned(c, clean, asg["off"], W), clean >= 0)


def test_input_layouts_and_two_calls_give_identical_bits():
    c, assigned, _ = _hand_made()
    a = _i32(assigned)
    (v0, n0), g0 = _run(2, a)
    mc_module = c["mc"].to(DEV).permute(0, 2, 1).contiguous()           # the module's [B, nm, A]
    runs = [_run(2, a), _run(2, a, mc=mc_module, mc_layout="bnA"), _run(2, a, mc=mc_module.permute(0, 2, 1), mc_layout="bAn")]
    for (v, n), g in runs:
        assert torch.equal(v, v0) and torch.equal(n, n0) and torch.equal(g["mc"], g0["mc"]) and torch.equal(g["protos"], g0["protos"])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_storage_is_the_fp32_result_rounded_once(dtype):
    a = _i32(R.assignment(2, 20)["assigned"])
    _, g32 = _run(2, a)
    _, g = _run(2, a, protos_grad_dtype=dtype)
    assert g["protos"].dtype == dtype
    assert torch.equal(g["protos"], g32["protos"].to(dtype))
    assert torch.equal(g["mc"], g32["mc"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_accumulate_adds_to_the_buffers(dtype):
    """buffer + gradient, rounded once to the storage type, from the fp32 overwrite result: met exactly."""
    c = T.case(2)
    a = _i32(R.assignment(2, 20)["assigned"])
    B, nm, hp, wp = c["protos"].shape
    _, g32 = _run(2, a)
    gen = torch.Generator().manual_seed(3)
    buf_mc = (torch.randn(B, c["A"], nm, generator=gen) * g32["mc"].abs().max().item()).to(DEV)
    buf_pr = (torch.randn(B, hp, wp, nm, generator=gen) * g32["protos"].abs().max().item()).to(dtype).to(DEV)
    want_mc = buf_mc + g32["mc"]
    want_pr = (buf_pr.float() + g32["protos"].permute(0, 2, 3, 1)).to(dtype)
    before = buf_pr.clone()
    _run(2, a, grad_out={"mc": buf_mc, "protos": buf_pr}, accumulate=True)
    assert torch.equal(buf_mc, want_mc)
    assert torch.equal(buf_pr, want_pr)
    assert not torch.equal(buf_pr, before)


def _raw_call(k, assigned, with_maps):
    """`mtbt_instance_mask_loss_assigned` through ctypes: real map pointers, or NULL ones with zero strides and reg_max 0."""
    lib = L.load()
    c = T.case(k)
    S, (B, nm, hp, wp), A = c["kw"]["img_size"], c["protos"].shape, c["A"]
    a = L.MaskLossArgs()
    maps = [d.to(DEV).permute(0, 2, 3, 1).contiguous() for d in c["det"]]
    for i, m in enumerate(maps):
        a.h[i], a.w[i] = m.shape[1], m.shape[2]
        if with_maps:
            a.map[i], a.map_pixel_stride[i] = m.data_ptr(), m.shape[3]
    a.n_levels, a.N, a.img_size, a.n_gt = len(maps), B, float(S), int(c["gt"].shape[0])
    if with_maps:
        a.reg_max, a.iou_thresh = 16, 0.5
    xyxy, off = group_gt_rows(c["gt"].to(DEV), B, float(S))
    mc = c["mc"].to(DEV).contiguous()
    pr = c["protos"].to(DEV).permute(0, 2, 3, 1).contiguous()
    tgt = c["masks"].to(DEV).contiguous()
    d_mc, d_pr = torch.empty(B, A, nm, device=DEV), torch.empty(B, hp, wp, nm, device=DEV)
    a.gt_xyxy, a.gt_off, a.mc, a.protos, a.gt_masks = xyxy.data_ptr(), off.data_ptr(), mc.data_ptr(), pr.data_ptr(), tgt.data_ptr()
    a.mc_batch_stride, a.mc_anchor_stride, a.mc_channel_stride = A * nm, nm, 1
    a.hp, a.wp, a.nm, a.weight = hp, wp, nm, W
    a.d_mc, a.d_protos, a.dprotos_dtype = d_mc.data_ptr(), d_pr.data_ptr(), L.F32
    nbytes = lib.mtbt_mask_loss_workspace_bytes(B, A, hp, wp, nm)
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=DEV)
    out = torch.empty(2, device=DEV)
    a.workspace, a.workspace_bytes, a.out = ws.data_ptr(), nbytes, out.data_ptr()
    L.check(lib.mtbt_instance_mask_loss_assigned(C.byref(a), assigned.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "raw call")
    torch.cuda.synchronize()
    return out, d_mc, d_pr


def test_null_map_pointers_give_the_same_bits_as_real_ones():
    a = _i32(R.assignment(1)["assigned"]).contiguous()
    o0, m0, p0 = _raw_call(1, a, True)
    o1, m1, p1 = _raw_call(1, a, False)
    assert torch.equal(o0, o1) and torch.equal(m0, m1) and torch.equal(p0, p1)
    (v, n), g = _run(1, a)
    assert torch.equal(o0[0], v) and torch.equal(o0[1], n) and torch.equal(m0, g["mc"]) and torch.equal(p0.permute(0, 3, 1, 2), g["protos"])


def test_autograd_node_scales_the_operators_gradients():
    c = T.case(1)
    ref, mref = T.reference(1), R.reference(1, 10, 1.0)
    wb, wd, wc = T.WEIGHTS
    det0 = [d.to(DEV) for d in c["det"]]
    vals, g_maps, assigned, _ = task_aligned_det_loss(det0, c["gt"].to(DEV), img_size=c["kw"]["img_size"], nc_det=T.NC, reg_max=16,
                                                      weights=T.WEIGHTS, with_grads=True, want_assignment=True)
    (mval, _), g = _run(1, assigned)
    mc = c["mc"].to(DEV).permute(0, 2, 1).contiguous().requires_grad_()           # as the module returns it
    protos = c["protos"].to(DEV).requires_grad_()
    det = [d.to(DEV).requires_grad_() for d in c["det"]]
    loss, n_fg = TaskAlignedSegLoss.apply(mc, protos, c["gt"].to(DEV), c["masks"].to(DEV), c["kw"]["img_size"], 16, T.NC, 10, 0.5, 6.0, wb, wd, wc, W,
                                          "bnA", *det)
    want = wb * ref["values"][0] + wd * ref["values"][1] + wc * ref["values"][2] + W * float(mref[0])
    assert int(n_fg) == ref["values"][3] == mref[1]
    assert abs(float(loss.detach()) - want) <= 2e-4 * max(1.0, abs(want))
    assert torch.equal(loss.detach(), wb * vals[0] + wd * vals[1] + wc * vals[2] + W * mval)          # w . terms of the operators
    (loss * 0.37).backward()
    assert torch.allclose(mc.grad, 0.37 * g["mc"].permute(0, 2, 1), rtol=1e-6, atol=0)
    assert torch.allclose(protos.grad, 0.37 * g["protos"], rtol=1e-6, atol=0)
    for d, x in zip(det, g_maps):                                     # the assignment is a constant: the task-aligned gradient only
        assert d.grad.dtype == d.dtype and torch.allclose(d.grad, 0.37 * x, rtol=1e-6, atol=0)
    assert mc.grad.dtype == mc.dtype and protos.grad.dtype == protos.dtype
