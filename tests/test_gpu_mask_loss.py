"""Device instance-mask loss (csrc/mask_loss.hip) against the CPU restatement of its definition (tests/mask_loss_reference.py):
value, both gradients and their exact zero pattern, input layouts, determinism, d_protos storage types, the accumulate form and the
autograd node of the drop-in route."""
import pytest
import torch

import mask_loss_reference as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import InstanceMaskLoss, instance_mask_loss

DEV = "cuda:0"
W = 0.7           # the gradients are those of W * mask_loss


def _case(k):
    return R.empty(R.case(1)) if k == 4 else R.case(k)


def _run(k, *, weight=W, grads=True, mc=None, det=None, **kw):
    c = _case(k)
    det = [d.to(DEV) for d in c["det"]] if det is None else det
    mc = c["mc"].to(DEV) if mc is None else mc
    return instance_mask_loss(det, mc, c["protos"].to(DEV), c["gt"].to(DEV), c["masks"].to(DEV), weight=weight, with_grads=grads,
                              **c["kw"], **kw)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_value_matches_the_reference(k):
    want, n_pos, _, _ = R.reference(k, W)
    got, got_n = _run(k, grads=False)
    print(f"case {k}: value {float(got):.7f} reference {float(want):.7f}, positives {int(got_n)} reference {n_pos}")
    assert int(got_n) == n_pos
    assert abs(float(got) - float(want)) <= 2e-4 * max(1.0, abs(float(want)))
    (got2, got_n2), _ = _run(k)                              # the form that also writes the gradients returns the same value
    assert torch.equal(got2, got) and torch.equal(got_n2, got_n)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_gradients_match_autograd_and_its_zero_pattern(k):
    _, n_pos, want_mc, want_pr = R.reference(k, W)
    _, g = _run(k)
    assert g["mc"].shape == want_mc.shape and g["protos"].shape == want_pr.shape
    for name, got, want in (("mc", g["mc"].cpu(), want_mc), ("protos", g["protos"].cpu(), want_pr)):
        err, scale = (got - want).abs().max().item(), want.abs().max().item()
        print(f"case {k} d_{name}: max error {err:.3e}, max |want| {scale:.3e}")
        assert scale > 0 and err <= 1e-4 * scale, (name, err, scale)
    # non-positive anchors and prototype pixels outside every matched box: exactly zero, and nowhere else by construction of the reference
    c = R.case(k)
    pos_rows = torch.zeros(want_mc.shape[:2], dtype=torch.bool)
    for b, (pos, _, _) in enumerate(R.match(c["det"], c["gt"], c["kw"]["img_size"])):
        pos_rows[b, pos] = True
    assert int(pos_rows.sum()) == n_pos
    assert not g["mc"].cpu()[~pos_rows].any()
    assert torch.equal((g["mc"].cpu() != 0).any(-1), (want_mc != 0).any(-1))
    assert torch.equal((g["protos"].cpu() != 0).any(1), (want_pr != 0).any(1))


def test_input_layouts_give_identical_bits():
    c = R.case(2)
    (v0, n0), g0 = _run(2)
    mc_module = c["mc"].to(DEV).permute(0, 2, 1).contiguous()           # the module's [B, nm, A]
    (v1, n1), g1 = _run(2, mc=mc_module)
    (v2, n2), g2 = _run(2, mc=mc_module.permute(0, 2, 1))               # [B, A, nm] view of it: strided
    (v3, n3), g3 = _run(2, det=[d.to(DEV).contiguous(memory_format=torch.channels_last) for d in c["det"]])
    for v, n, g in ((v1, n1, g1), (v2, n2, g2), (v3, n3, g3)):
        assert torch.equal(v, v0) and torch.equal(n, n0)
        assert torch.equal(g["mc"], g0["mc"]) and torch.equal(g["protos"], g0["protos"])


def test_two_calls_give_identical_bits():
    (v0, n0), g0 = _run(2)
    (v1, n1), g1 = _run(2)
    assert torch.equal(v0, v1) and torch.equal(n0, n1) and torch.equal(g0["mc"], g1["mc"]) and torch.equal(g0["protos"], g1["protos"])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_storage_is_the_fp32_result_rounded_once(dtype):
    _, g32 = _run(2)
    _, g = _run(2, protos_grad_dtype=dtype)
    assert g["protos"].dtype == dtype
    assert torch.equal(g["protos"], g32["protos"].to(dtype))
    assert torch.equal(g["mc"], g32["mc"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_accumulate_adds_to_the_buffers(dtype):
    """buffer + gradient, rounded once to the storage type: the expectation is built from the fp32 overwrite result, so it has no
    second rounding and must be met exactly (the issue allows 1 ulp of the storage type)."""
    c = R.case(2)
    B, nm, hp, wp = c["protos"].shape
    _, g32 = _run(2)
    gen = torch.Generator().manual_seed(3)
    buf_mc = (torch.randn(B, c["A"], nm, generator=gen) * g32["mc"].abs().max().item()).to(DEV)
    buf_pr = (torch.randn(B, hp, wp, nm, generator=gen) * g32["protos"].abs().max().item()).to(dtype).to(DEV)
    want_mc = buf_mc + g32["mc"]
    want_pr = (buf_pr.float() + g32["protos"].permute(0, 2, 3, 1)).to(dtype)
    before = buf_pr.clone()
    _run(2, grad_out={"mc": buf_mc, "protos": buf_pr}, accumulate=True)
    assert torch.equal(buf_mc, want_mc)
    assert torch.equal(buf_pr, want_pr)
    assert not torch.equal(buf_pr, before)


def test_autograd_node_scales_the_operators_gradients():
    c = R.case(1)
    _, g = _run(1)
    mc = c["mc"].to(DEV).permute(0, 2, 1).contiguous().requires_grad_()           # as the module returns it
    protos = c["protos"].to(DEV).requires_grad_()
    det = [d.to(DEV).requires_grad_() for d in c["det"]]
    loss, n_pos = InstanceMaskLoss.apply(mc, protos, c["gt"].to(DEV), c["masks"].to(DEV), c["kw"]["img_size"], 16, 0.5, W, "bnA", *det)
    want, want_n, _, _ = R.reference(1, W)
    assert int(n_pos) == want_n and abs(float(loss.detach()) - W * float(want)) <= 2e-4 * max(1.0, W * float(want))
    (loss * 0.37).backward()
    assert torch.allclose(mc.grad, 0.37 * g["mc"].permute(0, 2, 1), rtol=1e-6, atol=0)
    assert torch.allclose(protos.grad, 0.37 * g["protos"], rtol=1e-6, atol=0)
    assert all(d.grad is None for d in det)                        # the maps are inputs of the node; the matching carries no gradient
    assert mc.grad.dtype == mc.dtype and protos.grad.dtype == protos.dtype
