"""Device task-aligned detection loss (csrc/det_loss_tal.hip) against the CPU restatement of its definition (tests/tal_reference.py):
the assignment exactly (tests/test_cpu_tal.py::test_margin_condition is what makes that legitimate), the values, the gradient and
its exact zero pattern, input layouts, determinism, the accumulate form and the autograd node of the drop-in route."""
import pytest
import torch

import tal_reference as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import TaskAlignedDetLoss, task_aligned_det_loss

DEV = "cuda:0"
W = R.WEIGHTS
CASES = [1, 2, 3, 4, 5]


def _run(k, *, det=None, **kw):
    c = R.case(k)
    det = [d.to(DEV) for d in c["det"]] if det is None else det
    return task_aligned_det_loss(det, c["gt"].to(DEV), img_size=c["kw"]["img_size"], nc_det=R.NC, reg_max=c["kw"]["reg_max"], weights=W, **kw)


@pytest.mark.parametrize("k", CASES)
def test_assignment_and_values_match_the_reference(k):
    ref = R.reference(k)
    vals, assigned, tscore = _run(k, want_assignment=True)
    want_a = ref["asg"]["assigned"]
    assert assigned.dtype == torch.int32 and assigned.shape == want_a.shape
    diff = int((assigned.cpu().long() != want_a).sum())
    print(f"case {k}: {diff} of {want_a.numel()} anchors assigned differently; fg {int(vals[3])} reference {ref['values'][3]}")
    assert diff == 0
    assert float(vals[3]) == float(ref["values"][3])
    terr = (tscore.cpu() - ref["asg"]["t"]).abs().max().item()
    print(f"case {k}: target score max error {terr:.3e}")
    assert terr <= 2e-4
    for name, got, want in zip(("box", "dfl", "cls", "n_fg", "mean ov"), vals, ref["values"]):
        err = abs(float(got) - float(want))
        print(f"case {k} {name}: {float(got):.7f} reference {float(want):.7f} error {err:.3e}")
        assert err <= 2e-4 * max(1.0, abs(float(want))), (name, float(got), float(want))
    if k == 4:
        assert float(vals[0]) == 0.0 and float(vals[1]) == 0.0 and float(vals[4]) == 0.0 and float(vals[2]) > 0
    vals2, _ = _run(k, with_grads=True)                        # the form that also writes the gradient returns the same values
    assert all(torch.equal(x, y) for x, y in zip(vals, vals2))


@pytest.mark.parametrize("k", CASES)
def test_gradient_matches_autograd_and_its_zero_pattern(k):
    ref = R.reference(k)
    _, grads = _run(k, with_grads=True)
    bg = ref["asg"]["assigned"] < 0
    rows = []
    for lvl, (got, want) in enumerate(zip(grads, ref["grads"])):
        assert got.shape == want.shape
        err, scale = (got.cpu() - want).abs().max().item(), want.abs().max().item()
        print(f"case {k} level {lvl}: max error {err:.3e}, max |want| {scale:.3e}")
        assert scale > 0 and err <= 1e-4 * scale, (lvl, err, scale)
        rows.append(got.cpu().permute(0, 2, 3, 1).reshape(got.shape[0], -1, got.shape[1]))
    flat = torch.cat(rows, 1)
    assert not flat[bg][:, :64].any()                          # the distribution channels of background anchors: exactly zero
    assert (flat[bg][:, 64:] != 0).all()
    if k == 4:
        assert bg.all()
    else:
        assert (flat[~bg][:, :64] != 0).any()


def test_input_layouts_give_identical_bits():
    c = R.case(2)
    v0, g0, a0, t0 = _run(2, with_grads=True, want_assignment=True)
    v1, g1, a1, t1 = _run(2, det=[d.to(DEV).contiguous(memory_format=torch.channels_last) for d in c["det"]], with_grads=True, want_assignment=True)
    assert all(torch.equal(x, y) for x, y in zip(v0, v1)) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert torch.equal(a0, a1) and torch.equal(t0, t1)


@pytest.mark.parametrize("k", [2, 3])
def test_two_calls_give_identical_bits(k):
    v0, g0, a0, t0 = _run(k, with_grads=True, want_assignment=True)
    v1, g1, a1, t1 = _run(k, with_grads=True, want_assignment=True)
    assert all(torch.equal(x, y) for x, y in zip(v0, v1)) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    assert torch.equal(a0, a1) and torch.equal(t0, t1)


def test_accumulate_adds_to_the_buffers():
    c = R.case(2)
    _, g = _run(2, with_grads=True)
    gen = torch.Generator().manual_seed(3)
    bufs = [(torch.randn(x.shape[0], x.shape[2], x.shape[3], x.shape[1], generator=gen) * x.abs().max().item()).to(DEV) for x in g]
    want = [b + x.permute(0, 2, 3, 1) for b, x in zip(bufs, g)]
    before = [b.clone() for b in bufs]
    _run(2, grad_out=bufs, accumulate=True)
    for b, w, o in zip(bufs, want, before):
        assert torch.equal(b, w) and not torch.equal(b, o)
    _run(2, grad_out=bufs)                                     # without the flag the buffers are overwritten whole
    assert all(torch.equal(b, x.permute(0, 2, 3, 1)) for b, x in zip(bufs, g))
    assert c["A"] == sum(x.shape[2] * x.shape[3] for x in g)


def test_autograd_node_scales_the_operators_gradient():
    c = R.case(1)
    ref = R.reference(1)
    _, g = _run(1, with_grads=True)
    det = [d.to(DEV).requires_grad_() for d in c["det"]]
    loss, n_fg = TaskAlignedDetLoss.apply(c["gt"].to(DEV), c["kw"]["img_size"], 16, R.NC, 10, 0.5, 6.0, W[0], W[1], W[2], *det)
    want = sum(w * v for w, v in zip(W, ref["values"][:3]))
    assert int(n_fg) == ref["values"][3] and abs(float(loss.detach()) - want) <= 2e-4 * max(1.0, abs(want))
    (loss * 0.37).backward()
    for d, x in zip(det, g):
        assert d.grad.dtype == d.dtype and torch.allclose(d.grad, 0.37 * x, rtol=1e-6, atol=0)
