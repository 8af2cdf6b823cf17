"""Kernel-level tests of the TRAINING face of mtbt_conv2d_nhwc, per tile: the second output y2 (conv_epilogue.h MODE 1), the derivative
epilogues y = affine * act'(res) (MODE 2, MTBT_ACT_D*, with and without column sums) and a residual that IS the output buffer (a gradient
accumulating in place, on the implicit-GEMM and on both direct 3x3 kernels).

The rows come from kernel_reference.TRAIN_VARIANTS; every launch first asserts (mtbt_conv_kernel_choice, on the very arguments it launches
with) that it reaches the kernel the row names, and afterwards that nothing outside the y / y2 views was written.  Residual buffers are
NaN outside their view: a residual read with the wrong pitch, batch stride or past the pixel tail poisons the output.

1. parity: y and y2 against fp64 references with per-element bounds built from stated terms (kernel_reference.deriv_ref / preact_ref /
   affine_act_ref); column sums against the sums of the stored output.
2. bit-exact: integer operands, power-of-two scale, dyadic shift (kernel_reference.exact_operands) -- every product and partial sum is
   exact in fp32, so the output must equal the exact result rounded ONCE, whatever the accumulation order:
     * y2 == rounded_once(pre) and y == rounded_once(pre + res): y computed from the ROUNDED y2 would differ (asserted to be detectable);
     * DELU with a residual drawn from {+3, -200}: act' is exactly 1 (z > 0) or exactly 0 (exp2(-288.5) underflows), so the output is
       rounded_once(pre) under the mask and zero elsewhere -- this pins the residual's addressing (pitch, batch stride, PERM position, tail
       guards) independently of any arithmetic;
     * column sums of those cases: the stored values are multiples of 2^-2 with 4 * sum |stored| < 2^24, so fp32 sums are exact in any
       order and must equal the fp64 sum of the stored output; the accumulate form gives exactly twice that;
     * res == y: rounded_once(exact + g0), and a second launch on the same buffer rounded_once(that + exact)."""
import dataclasses

import pytest
import torch

import kernel_reference as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import _lib as L
    from multitask_bonetumor_yolo_amd.engine import Act, Plan

DEV = "cuda:0"
SENTINEL = 7.0
F32 = torch.float32


def ids(params):
    return [f"{r.name}-{R.DNAME[d]}" for r, d in params]


def out_dtype(row, dtype):
    return F32 if row.layout == "f32" else dtype


class RowLaunch:
    """One launch of a training row.  x / w / res NCHW fp64 in storage precision, scale / shift fp32 (or None).  Mode "accum": `res` is
    what y holds before the launch, and the residual pointer is y itself."""

    def __init__(self, row, dtype, x, w, scale, shift, res):
        self.row, self.dtype = row, dtype
        odt = out_dtype(row, dtype)
        self.plan = p = Plan(torch.device(DEV))
        p.conv_policy = row.policy
        self.bufs = {"y": self._buffer("y", odt, SENTINEL)}
        ya = self._view("y")
        ra = None
        if row.mode == "accum":
            self._fill("y", res)
            ra = ya
        elif res is not None:
            self.bufs["res"] = self._buffer("res", dtype, float("nan"))
            self._fill("res", res)
            ra = self._view("res")
        wp = w.permute(0, 2, 3, 1).reshape(row.K, -1).contiguous().to(DEV, dtype)
        xa = Act.of(x.permute(0, 2, 3, 1).contiguous().to(DEV, dtype))
        self.args = a = p.conv(xa, wp, ya, R=row.k, S=row.k, stride=row.stride, pad=row.pad, scale=scale.to(DEV) if scale is not None else None,
                               shift=shift.to(DEV) if shift is not None else None, act=row.act, res=ra, tile_hint=row.hint)
        if row.mode == "y2":
            self.bufs["y2"] = self._buffer("y2", odt, SENTINEL)
            a.y2 = self._view("y2").ptr
        self.sums = None
        if row.colsum:    # sums only, no shift
            self.sums = torch.full((row.K,), SENTINEL, device=DEV)
            nb = p.lib.mtbt_conv_colsum_workspace_bytes(row.N * row.Ho * row.Wo, row.K, 0)
            self.ws = torch.empty(nb // 4 + 4, device=DEV)
            a.colsum, a.colsum_shift, a.colsum_sq, a.colsum_accumulate = self.sums.data_ptr(), None, 0, 0
            a.colsum_ws, a.colsum_ws_bytes = self.ws.data_ptr(), nb
        assert R.kernel_choice(L, p.lib, a) == row.expect, row.name

    def _buffer(self, which, dt, fill):
        width, _, rows = self.row.view(which)
        return torch.full((self.row.N, rows, width), fill, dtype=dt, device=DEV)

    def _view(self, which):
        r = self.row
        width, c0, rows = r.view(which)
        return Act(self.bufs[which], c0, r.N, r.Ho, r.Wo, r.K, width, rows * width)

    def _fill(self, which, t):
        r = self.row
        _, c0, _ = r.view(which)
        buf = self.bufs[which]
        buf[:, :r.Ho * r.Wo, c0:c0 + r.K] = t.permute(0, 2, 3, 1).reshape(r.N, -1, r.K).to(DEV, buf.dtype)

    def run(self, accumulate_sums=False):
        if self.sums is not None:
            self.args.colsum_accumulate = 1 if accumulate_sums else 0
        self.plan.run()
        torch.cuda.synchronize()
        return self

    def out(self, which="y"):
        """The view as NCHW fp64, after checking that nothing outside it was written."""
        r = self.row
        _, c0, _ = r.view(which)
        full = self.bufs[which].double().cpu()
        inside = torch.zeros_like(full, dtype=torch.bool)
        inside[:, :r.Ho * r.Wo, c0:c0 + r.K] = True
        assert torch.all(full[~inside] == SENTINEL), f"{r.name}: written outside the {which} view"
        return full[:, :r.Ho * r.Wo, c0:c0 + r.K].reshape(r.N, r.Ho, r.Wo, r.K).permute(0, 3, 1, 2)

    def colsums(self):
        return self.sums.double().cpu()


def worst_ratio(out, ref, bnd):
    return ((out - ref).abs() / bnd).max().item()


def assert_bits(got, want, what, exact=None):
    diff = got != want
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.numel()} outputs differ from the once-rounded exact result, e.g. got " \
                           f"{got[diff][:4].tolist()} want {want[diff][:4].tolist()}" + (f" exact {exact[diff][:4].tolist()}" if exact is not None else "")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. parity: every row of the training table, every dtype, against the fp64 references
# ---------------------------------------------------------------------------------------------------------------------------------------
TRAIN_PARAMS = [(r, d) for r in R.TRAIN_VARIANTS for d in r.dtypes]


@pytest.mark.parametrize("row,dtype", TRAIN_PARAMS, ids=ids(TRAIN_PARAMS))
def test_train_variant_parity(row, dtype):
    (x, w, scale, shift, res), refs = R.train_row_reference(row, dtype)
    ln = RowLaunch(row, dtype, x, w, scale, shift, res).run()
    tag = f"{row.name} {R.DNAME[dtype]}"
    for which, (ref, bnd) in refs.items():
        got = ln.out(which)
        print(f"RATIO {row.mode}{'+colsum' if row.colsum else ''} {R.DNAME[dtype]} {row.name} {which} {worst_ratio(got, ref, bnd):.3f}")
        R.check(got, ref, bnd, f"{tag} {which}")
    if row.colsum:
        # the criterion of test_conv_column_sums: the sums are those of the STORED values, up to the fp32 order of summation
        stored = ln.out("y")
        want = stored.sum((0, 2, 3))
        tol = 2e-5 if dtype == F32 else 2e-4
        assert (ln.colsums() - want).abs().max() <= tol * stored.abs().sum((0, 2, 3)).max() + 1e-6, tag


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. bit-exact, on integer operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def seed_of(name):
    return torch.Generator().manual_seed(sum(map(ord, name)))


def y2_exact_case(row, dtype):
    """ACT_NONE + residual on a y2 row: operands, the exact pre-activation and the exact y = pre + res."""
    row = dataclasses.replace(row, act=R.ACT_NONE, res=True)
    x, w, scale, shift, res, exact = R.exact_operands(row, dtype, seed_of(row.name))
    return row, (x, w, scale, shift, res), exact - res, exact


def delu_exact_case(row, dtype):
    """DELU on a deriv row with z drawn per element from {+3, -200}: operands (res = z), the exact pre-activation and the mask z > 0."""
    row = dataclasses.replace(row, act=R.ACT_DELU)
    g = seed_of(row.name)
    x, w, scale, shift, _, pre = R.exact_operands(dataclasses.replace(row, res=False), dtype, g)
    mask = torch.rand(pre.shape, generator=g) < 0.5
    z = torch.where(mask, torch.full_like(pre, 3.0), torch.full_like(pre, -200.0))
    assert torch.equal(R.storage(z, dtype), z)
    return row, (x, w, scale, shift, z), pre, mask


def one_row_per_tile(mode):
    """The first dense row without column sums of every implicit-GEMM tile."""
    rows = {}
    for r in R.TRAIN_VARIANTS:
        if r.mode == mode and r.layout == "dense" and not r.colsum and r.expect[0] == 0:
            rows.setdefault(r.expect[1:3], r)
    assert len(rows) == 8
    return list(rows.values())


Y2_TILE_PARAMS = [(r, d) for r in one_row_per_tile("y2") for d in R.DTYPES]


@pytest.mark.parametrize("row,dtype", Y2_TILE_PARAMS, ids=ids(Y2_TILE_PARAMS))
def test_y2_and_y_are_each_rounded_once(row, dtype):
    row, ops, pre, exact = y2_exact_case(row, dtype)
    res = ops[4]
    want_y2, want_y = R.rounded_once(pre, dtype), R.rounded_once(exact, dtype)
    if dtype != F32:
        assert (want_y2 != pre).float().mean().item() > 0.3 and (want_y != exact).float().mean().item() > 0.3, "the test values must need rounding"
        assert (R.rounded_once(want_y2 + res, dtype) != want_y).any(), "y from the rounded y2 (double rounding) must be detectable"
    ln = RowLaunch(row, dtype, *ops).run()
    assert_bits(ln.out("y2"), want_y2, f"{row.name} y2", pre)
    assert_bits(ln.out("y"), want_y, f"{row.name} y", exact)


DERIV_PARAMS = [(r, d) for r in R.TRAIN_VARIANTS if r.mode == "deriv" for d in r.dtypes]


@pytest.mark.parametrize("row,dtype", DERIV_PARAMS, ids=ids(DERIV_PARAMS))
def test_delu_mask_is_applied_exactly(row, dtype):
    """Every deriv row (every tile and layout) with DELU, without column sums: the fast MODE 2 body wherever the row's layout allows it."""
    row, ops, pre, mask = delu_exact_case(dataclasses.replace(row, colsum=False), dtype)
    odt = out_dtype(row, dtype)
    want = torch.where(mask, R.rounded_once(pre, odt), torch.zeros_like(pre))
    assert 0.3 < mask.float().mean().item() < 0.7
    if odt != F32:
        assert (R.rounded_once(pre, odt) != pre).float().mean().item() > 0.3, "the test values must need rounding"
    assert_bits(RowLaunch(row, dtype, *ops).run().out("y"), want, row.name, pre)


CS_Y2_PARAMS = [(r, d) for r in one_row_per_tile("y2") if r.expect[1] != 96 for d in R.DTYPES]
CS_DERIV_PARAMS = [(r, d) for r in one_row_per_tile("deriv") if r.expect[1] != 96 for d in R.DTYPES]


def check_exact_sums(ln, want, tag):
    """want: the once-rounded exact output the launch must store.  Multiples of 2^-2 whose absolute sums stay below 2^22 per channel are
    summed exactly by fp32 in any order."""
    assert torch.equal((want * 4).round(), want * 4), "stored values must be multiples of 2^-2"
    assert (4 * want.abs().sum((0, 2, 3))).max().item() < 2.0 ** 24
    assert_bits(ln.out("y"), want, tag)
    sums = want.sum((0, 2, 3))
    assert torch.equal(ln.colsums(), sums), f"{tag}: column sums differ from the sums of the stored output, by up to {(ln.colsums() - sums).abs().max().item()}"
    ln.run(accumulate_sums=True)
    assert torch.equal(ln.colsums(), 2 * sums), f"{tag}: the accumulate form must give exactly twice the sums"


@pytest.mark.parametrize("row,dtype", CS_Y2_PARAMS, ids=ids(CS_Y2_PARAMS))
def test_column_sums_exact_next_to_y2(row, dtype):
    row, ops, pre, exact = y2_exact_case(dataclasses.replace(row, colsum=True), dtype)
    ln = RowLaunch(row, dtype, *ops).run()
    assert_bits(ln.out("y2"), R.rounded_once(pre, dtype), f"{row.name} y2", pre)
    check_exact_sums(ln, R.rounded_once(exact, dtype), row.name)


@pytest.mark.parametrize("row,dtype", CS_DERIV_PARAMS, ids=ids(CS_DERIV_PARAMS))
def test_column_sums_exact_under_delu_mask(row, dtype):
    row, ops, pre, mask = delu_exact_case(dataclasses.replace(row, colsum=True), dtype)
    want = torch.where(mask, R.rounded_once(pre, dtype), torch.zeros_like(pre))
    check_exact_sums(RowLaunch(row, dtype, *ops).run(), want, row.name)


ACCUM_PARAMS = [(r, d) for r in R.TRAIN_VARIANTS if r.mode == "accum" for d in r.dtypes]


@pytest.mark.parametrize("row,dtype", ACCUM_PARAMS, ids=ids(ACCUM_PARAMS))
def test_gradient_accumulates_in_place_exactly(row, dtype):
    """res is y, preloaded with an integer gradient g0: rounded_once(conv + g0); a second launch on the same buffer adds the conv again."""
    x, w, scale, shift, g0, exact = R.exact_operands(row, dtype, seed_of(row.name), target=2000.0)     # (twice the conv stays below 65504)
    conv = exact - g0
    first = R.rounded_once(exact, dtype)
    second = R.rounded_once(first + conv, dtype)
    if dtype != F32:
        assert (first != exact).float().mean().item() > 0.3 and (second != first + conv).float().mean().item() > 0.3, "the test values must need rounding"
    ln = RowLaunch(row, dtype, x, w, scale, shift, g0).run()
    assert_bits(ln.out("y"), first, f"{row.name} first launch", exact)
    assert_bits(ln.run().out("y"), second, f"{row.name} second launch", first + conv)
