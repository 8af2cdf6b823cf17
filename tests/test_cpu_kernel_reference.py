"""CPU checks of tests/kernel_reference.py: the per-element bounds are tight enough to mean something, and every row of the conv variant
table reaches the kernel it names (mtbt_conv_kernel_choice: no launch, no GPU)."""
import pytest
import torch

import kernel_reference as R


def _fp16_row_reference(row, seed=0):
    """A variant-table row as tests/test_gpu_fp16.py builds it: fp16 operands, fp32 scale / shift, fp64 reference and bound."""
    g = torch.Generator().manual_seed(seed)
    x = R.storage(torch.randn(row.N, row.C, row.H, row.W, generator=g), torch.float16)
    w = R.storage(torch.randn(row.K, row.C, row.k, row.k, generator=g) / (row.C * row.k * row.k) ** 0.5, torch.float16)
    scale = torch.rand(row.K, generator=g) + 0.5
    shift = torch.randn(row.K, generator=g) * 0.1
    res = R.storage(torch.randn(row.N, row.K, row.Ho, row.Wo, generator=g), torch.float16) if row.res else None
    return R.conv_ref(x, w, row.stride, row.pad, scale, shift, row.act, res, torch.float16)


@pytest.mark.parametrize("name", ["g128x64n", "g96x128w", "g64x64n", "direct128"])
def test_bound_accepts_one_fp16_rounding_and_rejects_bf16_and_4_ulps(name):
    ref, bnd = _fp16_row_reference(R.ROWS[name])
    R.check(ref.half(), ref, bnd, "correctly rounded fp16")
    assert not R.within(ref.bfloat16(), ref, bnd), "bf16 rounding passed the fp16 bound"
    flat = ref.flatten()
    for i in (int(flat.abs().argmax()), int(flat.abs().argsort()[flat.numel() // 2]), int(flat.abs().argsort()[flat.numel() // 4])):
        bad = ref.half().flatten().clone()
        ulp = (bad[i].float().abs().to(torch.float16).view(torch.int16) + 1).view(torch.float16).float() - bad[i].float().abs()
        bad[i] = bad[i].float() + 4 * ulp
        assert not R.within(bad.view_as(ref), ref, bnd), f"a 4-ulp error at element {i} passed"


def test_bound_rejects_double_rounding_of_residual_sum():
    """Rounding the conv result to fp16 and then adding the residual (two roundings) must not pass the single-rounding bound."""
    row = R.ROWS["g128x64n"]
    g = torch.Generator().manual_seed(1)
    x = R.storage(torch.randn(row.N, row.C, row.H, row.W, generator=g) * 30, torch.float16)
    w = R.storage(torch.randn(row.K, row.C, 3, 3, generator=g), torch.float16)
    res = R.storage(torch.randn(row.N, row.K, row.Ho, row.Wo, generator=g) * 300, torch.float16)
    ref, bnd = R.conv_ref(x, w, 1, 1, None, None, R.ACT_NONE, res, torch.float16)
    R.check(ref.half(), ref, bnd)
    twice = ((ref - res).half().double() + res).half()
    assert not R.within(twice, ref, bnd)


def test_gelu_poly64_matches_documented_error():
    x = torch.linspace(-12, 12, 200001, dtype=torch.float64)
    assert (R.gelu_poly64(x) - torch.nn.functional.gelu(x)).abs().max().item() <= R.GELU_POLY_ERR


def test_ln_bound_accepts_fp16_rounding_and_rejects_bf16():
    g = torch.Generator().manual_seed(2)
    v = R.storage(torch.randn(64, 768, generator=g) + 1000.0, torch.float16)
    lw, lb = torch.rand(768, generator=g) + 0.5, torch.randn(768, generator=g) * 0.1
    y = torch.nn.functional.layer_norm(v, (768,), lw.double(), lb.double(), 1e-6)
    bnd = R.ln_bound(y, v, lw, lb, 1e-6, 0.0, torch.float16)
    R.check(y.half(), y, bnd)
    assert not R.within(y.bfloat16(), y, bnd)


def test_variant_table_covers_every_variant():
    """Per dtype: all eight implicit-GEMM tiles with wide and narrow K-steps, both direct formulations at TC 64 and 128, the streaming head
    conv (16-bit only), the ConvT 2x2 mode; across the rows: ragged pixel tiles, K tails, stride 2, residual, every activation, fp32 output
    and the misaligned slice."""
    for dt in R.DTYPES:
        rows = [r for r in R.VARIANTS if dt in r.dtypes]
        got = {r.expect for r in rows}
        for tc in (128, 96, 64, 32):
            for tp in (128, 64):
                assert (0, tc, tp, 1) in got and (0, tc, tp, 0) in got, (dt, tc, tp)
        for tc in (64, 128):
            assert (1, tc, 256, 1) in got and (1, tc, 256, 0) in got, (dt, tc)
        assert any(r.expect[0] == 2 for r in rows) == (dt != torch.float32)
        assert any(r.convt for r in rows)
    V = R.VARIANTS
    assert any((r.N * r.Ho * r.Wo) % r.expect[2] for r in V if r.expect[0] == 0)
    assert any(r.K % r.expect[1] for r in V if r.expect[0] == 0) and any(r.K == 2 for r in V) and any(r.K == 48 and r.expect[1] == 64 for r in V)
    assert any(r.stride == 2 for r in V) and any(r.res for r in V)
    assert {r.act for r in V} >= {R.ACT_NONE, R.ACT_SILU, R.ACT_ELU, R.ACT_GELU, R.ACT_GELU_POLY}
    assert any(r.out == "f32" for r in V) and any(r.out == "slice" for r in V)


@pytest.mark.parametrize("row,dtype", [(r, d) for r in R.VARIANTS for d in r.dtypes], ids=lambda v: getattr(v, "name", R.DNAME.get(v)))
def test_variant_table_kernel_choice(row, dtype):
    from multitask_bonetumor_yolo_amd import _lib as L
    assert R.kernel_choice(L, L.load(), R.conv_args(L, row, dtype)) == row.expect
