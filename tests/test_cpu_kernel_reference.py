"""CPU checks of tests/kernel_reference.py: the per-element bounds are tight enough to mean something, and every row of the conv variant
table reaches the kernel it names (mtbt_conv_kernel_choice: no launch, no GPU)."""
import dataclasses

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


# ---------------------------------------------------------------------------------------------------------------------------------------
# The training face: references, bounds and the training variant table
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", [("d_128x128n", "y"), ("d_96x64w_ds", "y"), ("y2_128x64n", "y2")])
def test_train_bound_accepts_one_fp16_rounding_and_rejects_bf16_and_4_ulps(name, which):
    _, refs = R.train_row_reference(R.TRAIN_ROWS[name], torch.float16)
    ref, bnd = refs[which]
    R.check(ref.half(), ref, bnd, "correctly rounded fp16")
    assert not R.within(ref.bfloat16(), ref, bnd), "bf16 rounding passed the fp16 bound"
    flat = ref.flatten()
    order = flat.abs().argsort()
    for i in (int(order[-1]), int(order[flat.numel() // 2]), int(order[flat.numel() // 4])):
        bad = ref.half().flatten().clone()
        ulp = (bad[i].float().abs().to(torch.float16).view(torch.int16) + 1).view(torch.float16).float() - bad[i].float().abs()
        bad[i] = bad[i].float() + 4 * ulp
        assert not R.within(bad.view_as(ref), ref, bnd), f"a 4-ulp error at element {i} passed"


def test_act_grad64_closed_forms_match_autograd():
    z = torch.linspace(-9, 9, 20001, dtype=torch.float64)
    for act, fwd in ((R.ACT_DSILU, torch.nn.functional.silu), (R.ACT_DELU, torch.nn.functional.elu), (R.ACT_DGELU, torch.nn.functional.gelu)):
        zz = z.clone().requires_grad_()
        (g,) = torch.autograd.grad(fwd(zz).sum(), zz)
        assert (R.act_grad64(z, act) - g).abs().max().item() <= 1e-14, act
    assert torch.equal(R.act_grad64(torch.tensor([3.0, -200.0], dtype=torch.float64), R.ACT_DELU)[:1], torch.ones(1, dtype=torch.float64))
    assert R.act_grad64(torch.tensor([-200.0], dtype=torch.float64), R.ACT_DELU).item() < 2.0 ** -280


def test_act_grad64_gelu_poly_equals_central_difference():
    """g = gelu_poly64 is a polynomial of degree 14 inside |x| < 4 and linear outside.  Central difference with h = 2^-14: truncation
    h^2 / 6 max |g'''| <= 6.3e-10 * 8; fp64 rounding of the two forward values, whose Horner terms reach |x xc| * 12 <= 600 at
    |x| = 12: 2 * 4 * 2^-53 * 600 / (2 h) <= 4.4e-9.  Tolerance 1e-8; points within h of the kinks at |x| = 4 are left out."""
    h = 2.0 ** -14
    x = torch.linspace(-12, 12, 48001, dtype=torch.float64) + 1e-3
    x = x[((x.abs() - 4.0).abs() > 2 * h)]
    cd = (R.gelu_poly64(x + h) - R.gelu_poly64(x - h)) / (2 * h)
    assert (R.act_grad64(x, R.ACT_DGELU_POLY) - cd).abs().max().item() <= 1e-8


def _gelu_poly_grad_fp32(x):
    """common.h gelu_poly_grad step by step in fp32 (numpy float32; an FMA = the fp64 product and sum rounded once, exact for fp32 operands
    up to the double rounding no test below depends on).  Derivative coefficients: (j + 1) c_j rounded to fp32, as the kernel's constants."""
    import numpy as np
    f32, f64 = np.float32, np.float64
    c = [f32(v) for v in R.GELU_POLY_C]
    n = len(c)
    fma = lambda a, b, d: (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(d, f64)).astype(f32)
    xc = np.clip(x, f32(-4), f32(4))
    s = (xc * xc).astype(f32)
    k = [f32(f32(n - i) * c[i]) for i in range(n)]
    q = fma(k[0], s, k[1])
    for kk in k[2:]:
        q = fma(q, s, kk)
    p16 = c[0]
    for cc in c[1:]:
        p16 = f32(f32(p16 * f32(16)) + cc)
    return np.where(np.abs(x) < 4, fma(f32(2) * xc, q, 0.5), fma(xc, p16, 0.5))


def test_gelu_poly_grad_bound_covers_a_faithful_fp32_evaluation_and_needs_its_horner_term():
    import numpy as np
    x = np.linspace(-8, 8, 400001).astype(np.float32)
    x = x[np.abs(x) != 4]
    z = torch.from_numpy(x.astype(np.float64))
    err = (torch.from_numpy(_gelu_poly_grad_fp32(x).astype(np.float64)) - R.act_grad64(z, R.ACT_DGELU_POLY)).abs()
    assert (err <= R.act_grad_error(z, R.ACT_DGELU_POLY)).all()
    plain = R.ACT_EVAL * (1.0 + z.abs())
    assert (err > 2 * plain).any() and not (err > plain)[z.abs() < 3].any(), "the Horner term is needed near |z| = 4 only"
    # the term stays a small part of the derivative's scale away from the clamp: below ACT_EVAL (1 + |z|) for |z| <= 2
    assert (2.0 ** -23 * R.gelu_poly_grad_condition(z) <= plain)[z.abs() <= 2].all()


PERM_TILES = {(128, 128), (128, 64), (96, 128), (64, 128), (64, 64), (32, 128), (32, 64)}      # even fragment count per wave; 96x64: 3


def test_train_variant_table_covers_every_training_epilogue():
    """What TRAIN_VARIANTS has to contain (the issue's list): tiles x modes x K-step widths, activations per body, column sums, pixel and
    channel tails, layouts, the 3x3 rows the chooser keeps off the direct kernels, and the in-place accumulation on every kernel."""
    V = R.TRAIN_VARIANTS
    assert len({r.name for r in V}) == len(V)
    tiles = [(tc, tp) for tc in (128, 96, 64, 32) for tp in (128, 64)]
    for dt in (torch.float16, torch.bfloat16):
        for mode in ("y2", "deriv"):
            rows = [r for r in V if r.mode == mode and dt in r.dtypes]
            assert {r.expect[1:3] for r in rows if r.expect[0] == 0} >= set(tiles), (dt, mode)
            assert {r.expect[3] for r in rows} == {0, 1}
    assert all(set(r.dtypes) == set(R.DTYPES) for r in V)
    y2, dv, ac = ([r for r in V if r.mode == m] for m in ("y2", "deriv", "accum"))
    # y2: the fast body's three activations and the general body's two; a residual next to y2
    assert {r.act for r in y2} >= {R.ACT_NONE, R.ACT_GELU, R.ACT_GELU_POLY, R.ACT_SILU, R.ACT_ELU}
    assert any(r.res for r in y2) and all(r.act < R.ACT_DSILU for r in y2)
    # deriv: each D* code on a PERM tile and on the one non-PERM tile
    assert all(r.res for r in dv)
    for act in (R.ACT_DSILU, R.ACT_DELU, R.ACT_DGELU, R.ACT_DGELU_POLY):
        assert any(r.act == act and r.expect[1:3] in PERM_TILES for r in dv), act
        assert any(r.act == act and r.expect[1:3] == (96, 64) for r in dv), act
    # column sums: ACT_NONE and DGELU_POLY on every tile that allows them, DGELU once, never on a 96-channel tile
    for act in (R.ACT_NONE, R.ACT_DGELU_POLY):
        assert {r.expect[1:3] for r in V if r.colsum and r.act == act and r.expect[0] == 0} == set(R.CS_TILES), act
    assert sum(1 for r in V if r.colsum and r.act == R.ACT_DGELU) == 1
    assert set(R.CS_TILES) == {t for t in tiles if t[0] != 96} and not any(r.colsum and r.expect[1] == 96 for r in V)
    # pixel tails: 126 pixels (ragged for both pixel tiles, 14 rows in the last slab), fewer than 16 pixels in all
    for mode_rows in (y2, dv, ac):
        assert any(r.N * r.Ho * r.Wo == 126 and r.expect[2] == 128 for r in mode_rows) and any(r.N * r.Ho * r.Wo == 126 and r.expect[2] == 64 for r in mode_rows)
        assert any(r.N * r.Ho * r.Wo < 16 for r in mode_rows)
    assert 126 % 16 == 14
    # channel tails: K = TC + 8
    for mode_rows in (y2, dv, ac):
        assert any(r.K == r.expect[1] + 8 and r.expect[0] == 0 and r.layout == "dense" for r in mode_rows)
    # layouts, for both training outputs; the layouts are what they say
    for mode_rows in (y2, dv):
        assert {r.layout for r in mode_rows} == set(R.LAYOUTS)
    for r in V:
        (yw, yc, yr), (rw, rc, rr) = r.view("y"), r.view("res")
        assert r.view("y2")[0] == yw and r.view("y2")[2] == yr
        if r.layout == "slice16":
            assert yc % 8 == 0 and yw % 8 == 0 and r.view("y2")[1] % 8 == 0 and rc % 8 == 0 and rw % 8 == 0 and rw != yw and yw > r.K
        if r.layout == "batchgap":
            assert yr > r.Ho * r.Wo and r.N > 1
        if r.layout == "slice2":
            assert yc == 2 and yw == r.K + 2 and r.view("y2")[1] == 0
        if r.mode == "accum":
            assert r.res and r.view("res") == r.view("y")
    # 3x3 / stride 1 / pad 1 on a 16-aligned map stays on the implicit GEMM with y2 and with a D* act
    for mode_rows in (y2, dv):
        assert any(r.k == 3 and r.stride == 1 and r.pad == 1 and r.H % 16 == 0 and r.W % 16 == 0 and (r.hint >> 26) & 1 == 0 and r.expect[0] == 0
                   for r in mode_rows)
    # accum: a wide and a narrow tile per TC 128 / 64 / 32, 96x64, the 2x2 / stride-2 form, both direct formulations at both TC
    plain = [r for r in ac if not r.colsum]
    for tc in (128, 64, 32):
        assert {r.expect[3] for r in plain if r.expect[0] == 0 and r.expect[1] == tc} == {0, 1}, tc
        assert {r.expect[2] for r in plain if r.expect[0] == 0 and r.expect[1] == tc} == {128, 64}, tc
    assert any(r.expect[:3] == (0, 96, 64) for r in plain)
    assert any(r.k == 2 and r.stride == 2 for r in plain)
    assert {r.expect for r in ac if r.colsum and r.expect[0] == 1} == {(1, tc, 256, f) for tc in (64, 128) for f in (0, 1)}
    for tc in (64, 128):
        for first in (0, 1):
            assert any(r.expect == (1, tc, 256, first) and r.H * r.W // 256 * (4 if first else 8) > 1 for r in plain), (tc, first)


TRAIN_PARAMS = [(r, d) for r in R.TRAIN_VARIANTS for d in r.dtypes]


@pytest.mark.parametrize("row,dtype", TRAIN_PARAMS, ids=[f"{r.name}-{R.DNAME[d]}" for r, d in TRAIN_PARAMS])
def test_train_variant_table_kernel_choice(row, dtype):
    from multitask_bonetumor_yolo_amd import _lib as L
    assert R.kernel_choice(L, L.load(), R.train_conv_args(L, row, dtype)) == row.expect


# ---------------------------------------------------------------------------------------------------------------------------------------
# The depthwise kernels: variant table, choice query, and what the parity check of tests/test_gpu_dwconv_variants.py can see
# ---------------------------------------------------------------------------------------------------------------------------------------
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32


def _dw(rows, dt, **want):
    """Rows that run in dt and whose choice fields / attributes have the wanted values."""
    out = []
    for r in rows:
        if dt not in r.dtypes:
            continue
        if all((r.field(dt, k) if k in R.DW_FIELDS else getattr(r, k)) == v for k, v in want.items()):
            out.append(r)
    return out


def test_dw_variant_table_covers_every_instantiation_and_the_tile_walk():
    V = R.DW_VARIANTS
    assert len({r.name for r in V}) == len(V)
    for r in V:
        assert r.C % 8 == 0 and r.Co <= 768 and r.k in (3, 7) and not (r.ln and (r.res or r.M)) and not (r.raw and not r.ln)
        for dt in r.dtypes:
            th, tw = r.field(dt, "th"), r.field(dt, "tw")
            assert r.field(dt, "tiles") == r.N * -(-r.H // th) * -(-r.W // tw), r.name
            assert r.field(dt, "full") == int(dt != F32 and r.H % th == 0 and r.W % tw == 0), r.name
            assert r.field(dt, "gx") % 8 == 0
            assert (r.e16 is not None and r.e32 is not None) or r.walk, r.name
    plain = [r for r in V if not r.M]
    for dt in R.DTYPES:
        fulls = (0, 1) if dt != F32 else (0,)
        ln, af = [r for r in plain if r.ln], [r for r in plain if not r.ln]
        # LayerNorm form: 7x7 and 3x3 x MAXCH 1, 2, 3, 6 (x FULL / bounds-checked for the 16-bit types); the six-chunk kernel at 4, 5 and 6 live
        # chunks; a last chunk of 8 channels in a one-chunk and in a multi-chunk kernel
        for k in (7, 3):
            for maxch in (1, 2, 3, 6):
                for full in fulls:
                    assert _dw(ln, dt, k=k, maxch=maxch, full=full, walk=False), (dt, k, maxch, full)
            live = {-(-r.C // 128) for r in _dw(ln, dt, k=k, maxch=6)}
            assert live >= {4, 5, 6}, (dt, k, live)
            assert _dw(ln, dt, k=k, maxch=1, walk=True), (dt, k)
        assert _dw(ln, dt, C=8, maxch=1)
        assert any(r.C % 128 == 8 and r.field(dt, "maxch") > 1 for r in _dw(ln, dt))
        assert {r.field(dt, "maxch") for r in _dw(ln, dt) if r.C % 128 == 8} >= {2, 3, 6}
        assert any(r.raw for r in _dw(ln, dt, k=3)) and any(r.raw for r in _dw(ln, dt, k=7)) and any(not r.raw for r in _dw(ln, dt))
        for maxch in (2, 3, 6):
            assert _dw(ln, dt, k=7, maxch=maxch, walk=True), (dt, maxch)
        # scale / shift form: 3x3 and 7x7; one grid row, two, three or more with a ragged last chunk; full- and half-width tiles; FULL and
        # bounds-checked; the activation as the NONE constant, the SILU constant and at run time
        for k in (7, 3):
            assert _dw(af, dt, k=k, gy=1) and any(r.C % 128 for r in _dw(af, dt, k=k, gy=2))
            assert any(r.C % 128 for r in af if dt in r.dtypes and r.k == k and r.field(dt, "gy") >= 3)
            for full in fulls:
                assert _dw(af, dt, k=k, full=full, walk=False), (dt, k, full)
            assert {r.res for r in _dw(af, dt, k=k)} == {"", "buf", "y"}
            assert any(r.res for r in af if dt in r.dtypes and r.k == k and r.field(dt, "gy") > 1)
        for xb in (8, 4):
            assert _dw(af, dt, k=7, xb=xb, walk=False) and _dw(af, dt, k=7, xb=xb, walk=True, gy=1), (dt, xb)
            assert any(r.res for r in _dw(af, dt, k=7, xb=xb))
        assert _dw(af, dt, k=3, walk=True, gy=1)
        if dt != F32:
            for k in (7, 3):
                assert {r.field(dt, "act") for r in _dw(af, dt, k=k)} >= {R.ACT_NONE, R.ACT_SILU, -1}, (dt, k)
            assert _dw(af, dt, k=7, xb=4, full=1) and _dw(af, dt, k=7, xb=4, full=0)
        else:
            assert {r.field(dt, "act") for r in _dw(af, dt)} == {-1}
        assert {r.act for r in _dw(af, dt)} >= {R.ACT_NONE, R.ACT_SILU, R.ACT_ELU}
        # multiplier form: M = 1 and 2, C = 128 and 256, ragged and full tiles
        mu = [r for r in V if r.M and dt in r.dtypes]
        assert {(r.M, r.C) for r in mu} == {(1, 128), (2, 128), (1, 256), (2, 256)}
        assert {r.H % 4 == 0 and r.W % r.field(dt, "tw") == 0 for r in mu} == {True, False}
        assert all(r.field(dt, "gy") == r.M * r.C // 128 for r in mu)
        # image edges
        rows = _dw(V, dt)
        assert sum(r.N >= 2 for r in rows if not r.walk) > 0.8 * sum(not r.walk for r in rows)
        for n in (1, 2):
            assert any(r.H == n for r in rows) and any(r.W == n for r in rows), (dt, n)
        assert any(r.H == 3 for r in rows)
        for tw in {r.field(dt, "tw") for r in rows}:
            assert any(r.W == tw - 1 for r in _dw(rows, dt, tw=tw)), (dt, tw)
        # the walk: one chunk -- some workgroup runs a first, a middle and a last tile; several chunks -- some workgroup takes a second tile
        for r in _dw(V, dt, walk=True):
            tiles, gx = r.field(dt, "tiles"), r.field(dt, "gx")
            assert r.field(dt, "gy") == 1
            assert tiles >= 2 * gx + 1 if r.field(dt, "maxch") == 1 else tiles > gx, (r.name, tiles, gx)
    # 3x3 LayerNorm walk rows in bf16 for MAXCH 1 and 3
    assert _dw(V, BF16, k=3, ln=True, walk=True, maxch=1) and _dw(V, BF16, k=3, ln=True, walk=True, maxch=3)


DW_PARAMS = [(r, d) for r in R.DW_VARIANTS for d in r.dtypes]
DW_IDS = [f"{r.name}-{R.DNAME[d]}" for r, d in DW_PARAMS]


@pytest.mark.parametrize("row,dtype", DW_PARAMS, ids=DW_IDS)
def test_dw_variant_table_kernel_choice(row, dtype):
    from multitask_bonetumor_yolo_amd import _lib as L
    assert R.dw_choice(L, L.load(), row, dtype) == row.expect(dtype)


def test_dw_choice_is_the_launch_rule_not_a_copy():
    """The query's tile count and grid follow the shape: the tiles of a 16-bit 4 x 16 tiling, a grid capped at the resident workgroups
    (a multiple of the 8 XCDs), grid rows for the scale / shift form only; and the errors of the entry point."""
    import ctypes as C
    from multitask_bonetumor_yolo_amd import _lib as L
    lib = L.load()
    out = (C.c_int32 * 9)()
    assert lib.mtbt_dwconv_kernel_choice(1, 400, 4096, 96, 7, 1, 0, L.BF16, out) == 0
    assert tuple(out)[:7] == (4, 16, 8, 1, 1, 0, 100 * 256) and out[7] % 256 == 0 and out[7] <= 1024 and out[8] == 1
    assert lib.mtbt_dwconv_kernel_choice(1, 8, 16, 384, 7, 0, 0, L.BF16, out) == 0 and out[8] == 3 and out[3] == 1
    assert lib.mtbt_dwconv_kernel_choice(1, 8, 16, 384, 7, 1, 0, L.BF16, out) == 0 and out[8] == 1 and out[3] == 3
    for bad in ((0, 8, 8, 96, 7, 1, 0, L.BF16), (1, 8, 8, 100, 7, 1, 0, L.BF16), (1, 8, 8, 776, 7, 1, 0, L.BF16), (1, 8, 8, 96, 5, 1, 0, L.BF16),
                (1, 8, 8, 96, 7, 0, 9, L.BF16), (1, 8, 8, 96, 7, 0, -1, L.BF16), (1, 8, 8, 96, 7, 1, 0, 3)):
        assert lib.mtbt_dwconv_kernel_choice(*bad, out) == -1, bad
    assert lib.mtbt_dwconv_kernel_choice(1, 8, 8, 96, 7, 1, 0, L.BF16, None) == -1
    for bad in ((1, 8, 8, 96, 1, 0, L.BF16), (1, 8, 8, 128, 3, 0, L.BF16), (1, 8, 8, 512, 2, 0, L.BF16), (1, 8, 8, 128, 2, 9, L.BF16), (1, 8, 8, 128, 2, 0, 3)):
        assert lib.mtbt_dwconv3x3_mult_kernel_choice(*bad, out) == -1, bad


def _rounded(ref, dtype):
    return ref.to(dtype).double()


def _swap_first_tiles(out, row, dtype):
    """The output with tile 0's pixels replaced by its right neighbour's (a stale or mis-indexed tile)."""
    th, tw = row.field(dtype, "th"), row.field(dtype, "tw")
    bad = out.clone()
    wn = min(tw, row.W - tw)
    bad[:, :, :th, :wn] = out[:, :, :th, tw:tw + wn]
    return bad


@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=lambda d: R.DNAME[d])
def test_dw_parity_check_rejects_defective_layernorm_kernels(dtype):
    row = R.DW_ROWS["ln7_c264_r"]
    o, refs = R.dw_row_reference(dataclasses.replace(row, raw=True), dtype)
    for which, (ref, bnd) in refs.items():
        R.check(_rounded(ref, dtype), ref, bnd, f"correctly rounded {which}")
    w = o["w"].clone()
    w[:, 2, 5] = 0                                                                            # one tap dropped
    acc, mag = R.dw_sums(o["x"], w)
    bad = R.dw_ln_ref(acc, mag, o["v0"], o["v1"], o["v2"], dtype)
    assert not R.within(_rounded(bad["y"][0], dtype), *refs["y"]) and not R.within(_rounded(bad["raw"][0], dtype), *refs["raw"])
    acc, mag = R.dw_sums(o["x"], o["w"])
    bad = R.dw_ln_ref(acc, mag, o["v0"], o["v1"], o["v2"], dtype, stat_channels=128)          # statistics over the first chunk only
    assert not R.within(_rounded(bad["y"][0], dtype), *refs["y"])
    for which, (ref, bnd) in refs.items():                                                    # a tile's output replaced by its neighbour's
        assert not R.within(_swap_first_tiles(_rounded(ref, dtype), row, dtype), ref, bnd), which


@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=lambda d: R.DNAME[d])
def test_dw_parity_check_rejects_defective_affine_kernels(dtype):
    row = R.DW_ROWS["af7_c128_r"]
    assert row.act == R.ACT_SILU and row.res == "buf"
    o, refs = R.dw_row_reference(row, dtype)
    ref, bnd = refs["y"]
    R.check(_rounded(ref, dtype), ref, bnd, "correctly rounded")
    w = o["w"].clone()
    w[:, 6, 0] = 0                                                                            # one tap dropped
    bad, _ = R.affine_act_ref(*R.dw_sums(o["x"], w), o["v0"], o["v1"], row.act, o["res"], dtype)
    assert not R.within(_rounded(bad, dtype), ref, bnd)
    assert not R.within(_swap_first_tiles(_rounded(ref, dtype), row, dtype), ref, bnd)        # a tile's output replaced by its neighbour's
    acc, _ = R.dw_sums(o["x"], o["w"])                                                        # the residual added before the activation
    pre = acc * o["v0"].double().view(1, -1, 1, 1) + o["v1"].double().view(1, -1, 1, 1)
    assert not R.within(_rounded(R.act64(pre + o["res"], row.act), dtype), ref, bnd)


def test_dw_exact_operands_need_rounding_and_see_a_stale_tile():
    """The integer operands of the bit-exact tests: the LayerNorm input and the scale / shift output need rounding in the 16-bit types, and
    a tile replaced by its neighbour's differs bit for bit, at a pixel dw_tile_of places in tile 0."""
    for name in ("ln7_c264_r", "af7_c264_r"):
        row = R.DW_ROWS[name]
        for dtype in (F16, BF16):
            _, exact = R.dw_exact_operands(row, dtype)
            e = exact["raw" if row.ln else "y"]
            want = R.rounded_once(e, dtype)
            assert (want != e).float().mean().item() > 0.3
            diff = _swap_first_tiles(want, row, dtype) != want
            n, _, y, x = (int(v) for v in diff.nonzero()[0])
            assert R.dw_tile_of(row, dtype, n, y, x) == (0, 0, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The fused inference kernels (UPCONV_VARIANTS, NODE_VARIANTS, MLP_VARIANTS): the references against torch, the conditions on the inputs
# (flip shares), and for every row that the correctly rounded reference passes its bound while each defective kernel fails it.
# ---------------------------------------------------------------------------------------------------------------------------------------
FLIP_CAP = 0.2        # share of rounded intermediates that may be flagged as possible rounding flips (the cap of test_fp16_convnext_mlp_fused)
UP_PARAMS = [(r, d) for r in R.UPCONV_VARIANTS for d in r.dtypes]
NODE_PARAMS = [(r, d) for r in R.NODE_VARIANTS for d in r.dtypes]
MLP_PARAMS = [(r, d) for r in R.MLP_VARIANTS for d in r.dtypes]
_row_ids = lambda params: [f"{r.name}-{R.DNAME[d]}" for r, d in params]


def test_fused_tables_cover_every_instantiation_and_path():
    up = {(d, a) for r, d in UP_PARAMS for a in r.acts}
    assert up == {(d, a) for d in R.DTYPES for a in (R.ACT_NONE, R.ACT_SILU)}                        # upconv_fused_kernel<T, ACT>
    for d in R.DTYPES:
        rows = [r for r, dd in UP_PARAMS if dd == d]
        slab = 16 if d == F32 else 32
        assert any(r.tiles == 1 and r.channels(d) == slab for r in rows), "one tile, one slab"
        assert any((r.channels(d) // slab) % 2 == 1 and r.channels(d) > slab for r in rows), "an odd slab count above one"
        assert any(r.W > 16 for r in rows) and any(r.H > 16 for r in rows), "tile seams"
        assert any(r.K == 256 and set(r.acts) == {R.ACT_NONE, R.ACT_SILU} and r.exact for r in rows), "cbase = 128"
        assert {3, 9} <= {r.tiles for r in rows}, "two fill levels of the XCD walk"
        assert any(r.layout == "slice" and r.N > 1 for r in rows)
    assert any(r.C == 256 and r.K == 256 for r in R.UPCONV_VARIANTS), "the model's channel counts"
    assert {(d, r.C, r.kind) for r, d in NODE_PARAMS} == {(d, c, k) for d in R.NODE_DTYPES for c in (128, 256) for k in ("td", "out")}
    for kind in ("td", "out"):
        rows = [r for r in R.NODE_VARIANTS if r.kind == kind]
        assert any(r.wdev for r in rows) and any(r.slice for r in rows) and {r.act for r in rows} >= {R.ACT_NONE, R.ACT_ELU}
    N, H, W = R.NODE_SHAPE["td"]
    assert (H * W) % 64 and N * H * W > 128 and H % 2 == 0 and W % 2 == 0, "workgroups that span two images"
    N, H, W = R.NODE_SHAPE["out"]
    assert (H * W) % 64 and N * H * W > 64 and H % 2 and W % 2, "an odd map"
    inf = {(d, r.D, r.M, r.res) for r, d in MLP_PARAMS if not r.train}
    assert inf >= {(d, D, M, True) for d in R.MLP_DTYPES for D in (96, 192, 384) for M in (1, 17, 33, 127, 129, 300)}
    assert inf >= {(d, D, 129, False) for d in R.MLP_DTYPES for D in (96, 192, 384)}
    assert {(d, r.D, r.M) for r, d in MLP_PARAMS if r.train} == {(BF16, D, M) for D in (96, 192) for M in (17, 129, 300)}


@pytest.mark.parametrize("H,W", [(16, 16), (16, 32)])
@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_SILU])
def test_upconv_ref_equals_convtranspose_then_conv3x3(H, W, act):
    """upconv_ref (written from the header's formula) on model.compose_upconv's weights against fp64 conv_transpose2d -> conv2d -> affine -> act
    of the uncomposed operands, every pixel: all nine border classes.  compose_upconv returns fp32: 2^-24 of the summed magnitudes."""
    import torch.nn.functional as F
    from multitask_bonetumor_yolo_amd.model import compose_upconv
    g = torch.Generator().manual_seed(H + W + act)
    N, C, K = 2, 8, 16
    wt, bt = torch.randn(C, C, 2, 2, generator=g).double() * 0.3, torch.randn(C, generator=g).double() * 0.5
    w3 = torch.randn(K, C, 3, 3, generator=g).double() * 0.2
    sc, sh = torch.rand(K, generator=g).double() + 0.5, torch.randn(K, generator=g).double() * 0.2
    x = torch.randn(N, C, H, W, generator=g).double()
    pair = R.act64(F.conv2d(F.conv_transpose2d(x, wt, bt, stride=2), w3, padding=1) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), act)
    wc, s9 = compose_upconv(wt, bt, w3, sc, sh)
    assert all(not torch.equal(s9[i], s9[j]) for i in range(9) for j in range(i)), "nine different class vectors"
    ref, _, mag = R.upconv_ref(x, wc.double().view(4, K, 2, 2, C), s9, act, F32)
    tol = R.ACT_LIPSCHITZ[act] * 2.0 ** -24 * (mag + R.upconv_shift(s9, H, W).abs()) + 1e-13
    assert bool(((ref - pair).abs() <= tol).all()), ((ref - pair).abs() / tol).max().item()
    border = (ref - pair).abs()[:, :, [0, -1]].max().item(), (ref - pair).abs()[:, :, :, [0, -1]].max().item()
    assert max(border) < 1e-6


def test_node_resampling_equals_torch():
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(4)
    for shape in ((2, 3, 3, 5), (1, 2, 1, 1), (2, 2, 4, 2)):
        x = torch.randn(*shape, generator=g).double()
        assert torch.allclose(R.bilinear_up2(x), F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False), rtol=0, atol=1e-14)
    x = torch.randn(2, 3, 10, 14, generator=g).double()
    assert torch.allclose(R.mean2x2(x), F.avg_pool2d(x, 2), rtol=0, atol=1e-15)
    a, b, c = torch.randn(2, 3, 5, 7, generator=g).double(), torch.randn(2, 3, 5, 7, generator=g).double(), x
    s, mag = R.node_fused([a, b, c], (0.5, 0.25, 2.0), R.NODE_MODES["out"])
    assert torch.allclose(s, 0.5 * a + 0.25 * b + 2.0 * F.avg_pool2d(c, 2), rtol=0, atol=1e-14) and bool((mag >= s.abs() - 1e-14).all())
    assert R.f32_values([0.55])[0] != 0.55 and R.f32_values([0.5])[0] == 0.5                        # the weights are fp32 values


def test_mlp_ref_without_hidden_rounding_is_the_plain_mlp():
    import torch.nn.functional as F
    t, res, w1, b1, w2, b2 = R.mlp_operands(R.MLP_ROWS["d96_m33"], BF16)
    ref = R.mlp_ref(t, res, w1, b1, w2, b2, BF16, round_h=False)[0]
    pre = t @ w1.t() + b1.double()
    assert torch.allclose(ref, res + R.gelu_poly64(pre) @ w2.t() + b2.double(), rtol=0, atol=1e-13)
    assert bool(((ref - (res + F.gelu(pre) @ w2.t() + b2.double())).abs() <= R.GELU_POLY_ERR * w2.abs().sum(1) + 1e-13).all())
    nores = R.mlp_ref(t, None, w1, b1, w2, b2, BF16, round_h=False)[0]
    assert torch.allclose(nores, ref - res, rtol=0, atol=1e-13)
    for dt in (BF16, F16):                                                   # the spacing helpers on both 16-bit grids
        v = torch.tensor([1.0, 1.5, 2.0, 0.0], dtype=torch.float64)
        eps = 2.0 ** (-7 if dt == BF16 else -10)
        assert R.spacing_below(v, dt).tolist()[:3] == [eps / 2, eps, eps] and R.spacing_above(v, dt).tolist()[:3] == [eps, eps, 2 * eps]
        assert R.spacing_below(v, dt)[3].item() > 0


@pytest.mark.parametrize("row,dtype", UP_PARAMS, ids=_row_ids(UP_PARAMS))
def test_upconv_check_rejects_defective_kernels(row, dtype):
    x, wc, s9 = R.up_operands(row, dtype)
    acc, mag = R.upconv_sums(x, wc)
    sh = R.upconv_shift(s9, row.H, row.W)
    acc1 = R.upconv_sums(torch.roll(x, 1, dims=3 if row.W > 16 else 2), wc)[0] if row.tiles > row.N else None
    for act in row.acts:
        ref, bnd = R.upconv_bound(acc, mag, sh, act, dtype)
        assert torch.equal(ref, R.upconv_ref(x, wc, s9, act, dtype)[0])
        R.check(_rounded(ref, dtype), ref, bnd, "correctly rounded")
        bad = lambda a, s: not R.within(_rounded(R.act64(a + s, act), dtype), ref, bnd)
        m = sh.clone()
        m[:, :, 0] = sh[:, :, 1]                                             # the interior row class on the first output row
        assert bad(acc, m), "interior shift on a border row"
        m = acc.clone()
        m[..., 0::2], m[..., 1::2] = acc[..., 1::2], acc[..., 0::2]          # the two column parities swapped
        assert bad(m, sh), "column parities swapped"
        if acc1 is not None:                                                 # the second tile reads its source one pixel off
            m = acc.clone()
            if row.W > 16:
                m[..., 32:] = acc1[..., 32:]
            else:
                m[..., 32:, :] = acc1[..., 32:, :]
            assert bad(m, sh), "source shifted at a tile seam"
        if row.K > 128:                                                      # channel tile 1 with the shifts of channel tile 0
            m = sh.clone()
            m[:, 128:256] = sh[:, 0:128]
            assert bad(acc, m), "shift of channel tile 0 on channel tile 1"


@pytest.mark.parametrize("row,dtype", [(r, d) for r, d in UP_PARAMS if r.exact], ids=_row_ids([(r, d) for r, d in UP_PARAMS if r.exact]))
def test_upconv_exact_operands_need_rounding(row, dtype):
    _, _, _, exact = R.up_exact_operands(row, dtype)
    want = R.rounded_once(exact, dtype)
    if dtype != F32:
        assert (want != exact).float().mean().item() > 0.3
    else:
        assert torch.equal(want, exact)


@pytest.mark.parametrize("row,dtype", NODE_PARAMS, ids=_row_ids(NODE_PARAMS))
def test_node_check_rejects_defective_kernels(row, dtype):
    (inputs, w, shift), (ref, bnd, flip) = R.node_row_reference(row, dtype)
    assert flip.double().mean().item() <= FLIP_CAP, "a condition on the inputs"
    R.check(_rounded(ref, dtype), ref, bnd, "correctly rounded")
    wg = R.NODE_WGT[row.kind]
    assert row.shape[0] >= 2, "a second image"
    out = lambda s, mag: _rounded(R.node_output(s, mag, w, shift, row.act, dtype)[0], dtype)
    s, mag = R.node_fused(inputs, wg, row.modes)
    if row.kind == "td":                                                     # bilinear source rows clamped one row early
        assert not R.within(out(*R.node_fused(inputs, wg, row.modes, clamp_early=1)), ref, bnd), "clamped early"
    # the pixel index not reduced modulo H * W from the second image on: the row index runs past the map -- the bilinear rows clamp to the
    # last source row, the 2 x 2 mean reads the next image
    wrong = list(inputs)
    wrong[-1] = inputs[-1][:, :, -1:, :].expand_as(inputs[-1]) if row.kind == "td" else torch.roll(inputs[-1], -1, dims=0)
    s2 = s.clone()
    s2[1:] = R.node_fused(wrong, wg, row.modes)[0][1:]
    assert not R.within(out(s2, mag), ref, bnd), "pixel index not reduced"
    if row.wdev:                                                             # wgt[] (other values) instead of wgt_dev
        assert not R.within(out(*R.node_fused(inputs, R.NODE_WGT_OTHER[row.kind], row.modes)), ref, bnd), "wgt[] used"


@pytest.mark.parametrize("row,dtype", MLP_PARAMS, ids=_row_ids(MLP_PARAMS))
def test_mlp_check_rejects_defective_kernels(row, dtype):
    (t, res, w1, b1, w2, b2), (ref, bnd, pre, pbnd, flip) = R.mlp_row_reference(row, dtype)
    assert flip.double().mean().item() <= FLIP_CAP, "a condition on the inputs"
    R.check(_rounded(ref, dtype), ref, bnd, "correctly rounded y")
    R.check(_rounded(pre, dtype), pre, pbnd, "correctly rounded pre-activation")
    D, M = row.D, row.M
    if row.train:                                                            # one chunk of fc1 rows left in natural order under the staged permutation
        rows = torch.arange(4 * D)
        rows[:32] = R.mlp_train_rows(32)
        y, _, p, _, _ = R.mlp_ref(t, res, w1[rows], b1[rows], w2, b2, dtype)
        assert not R.within(_rounded(y, dtype), ref, bnd) and not R.within(_rounded(p, dtype), pre, pbnd), "chunk 0 left natural"
    else:                                                                    # one chunk of fc2 columns left in natural order
        cols = torch.arange(4 * D)
        cols[:32] = R.mlp_hidden_order()
        assert not R.within(_rounded(R.mlp_ref(t, res, w1, b1, w2[:, cols], b2, dtype)[0], dtype), ref, bnd), "chunk 0 left natural"
    if res is not None:                                                      # the residual dropped for the last partial fragment
        assert M % 16
        y = ref.clone()
        y[M - M % 16:] -= res[M - M % 16:]
        assert not R.within(_rounded(y, dtype), ref, bnd), "residual dropped"
    assert not R.within(_rounded(R.mlp_ref(t, res, w1, b1, w2, b2, dtype, round_h=False)[0], dtype), ref, bnd), "h not rounded"
