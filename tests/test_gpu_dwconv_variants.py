"""Kernel-level tests of the depthwise family (csrc/dwconv.inc, dwconv_body.inc) per instantiation and over the persistent tile walk:
mtbt_dwconv_nhwc, mtbt_dwconv_nhwc_train and mtbt_dwconv3x3_mult_nhwc, launched through the C ABI.

The rows come from kernel_reference.DW_VARIANTS.  Every launch first asserts (mtbt_dwconv_kernel_choice, host only) that it reaches the
tile, chunk count, instantiation and grid its row names.  x, the residual, the taps and the per-channel vectors sit at 16-byte-aligned
offsets inside larger NaN-filled allocations: whatever the halo DMA reads past a narrow last chunk, a row's end or the tensor must never
reach an output (outputs are asserted finite).  y and raw sit inside sentinel-filled allocations whose guard regions before and after
must be untouched after the launch.

a. parity: every row x dtype against the fp64 reference with per-element bounds (kernel_reference.dw_row_reference);
b. bit-exact on integer operands (every product and partial sum exact in fp32, so the output is the exact result rounded ONCE):
   raw of every LayerNorm row; every scale / shift row with act none, with a residual, and with the residual being y (two launches on one
   buffer); every multiplier row against M plain calls on its blocks;
c. the walk rows (workgroups take a second tile; one-chunk kernels a first, a middle and a last one): a and b on the same shape -- a stale
   or half-landed tile shows as a bit mismatch, reported with its tile coordinates -- and two launches on fresh buffers bit-identical."""
import dataclasses

import pytest
import torch

import kernel_reference as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import _lib as L

DEV = "cuda:0"
SENTINEL = 7.0
GUARD = 8 * 1031          # elements before and after every view: a multiple of 8, so 16-byte alignment holds for every element size
F32 = torch.float32


def ids(params):
    return [f"{r.name}-{R.DNAME[d]}" for r, d in params]


class Guarded:
    """A tensor as a view at element GUARD of a flat allocation filled with `fill`."""

    def __init__(self, shape, dtype, fill, value=None):
        n = 1
        for s in shape:
            n *= s
        self.n, self.fill = n, fill
        self.alloc = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
        self.view = self.alloc[GUARD:GUARD + n].view(shape)
        if value is not None:
            self.view.copy_(value.to(DEV, dtype))
        assert self.ptr % 16 == 0

    @property
    def ptr(self):
        return self.view.data_ptr()

    def guards_untouched(self):
        return bool((self.alloc[:GUARD] == self.fill).all()) and bool((self.alloc[GUARD + self.n:] == self.fill).all())


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


class DwLaunch:
    """One launch of a table row through the C ABI.  `o`: the operands of kernel_reference.dw_operands / dw_exact_operands (x, w, res NCHW fp64
    in storage precision; v0, v1, v2 the fp32 per-channel vectors).  res == "y": y is preloaded with o["res"] and passed as the residual."""

    def __init__(self, row, dtype, o, raw=None):
        self.row, self.dtype = row, dtype
        self.lib = L.load()
        self.code = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}[dtype]
        assert R.dw_choice(L, self.lib, row, dtype) == row.expect(dtype), row.name
        nan = float("nan")
        Co, k = row.Co, row.k
        self.x = Guarded((row.N, row.H, row.W, row.C), dtype, nan, nhwc(o["x"]))
        self.w = Guarded((k * k, Co), dtype, nan, o["w"].reshape(Co, k * k).t().contiguous())
        self.vec = [Guarded((Co,), F32, nan, v) if v is not None else None for v in (o["v0"], o["v1"], o["v2"])]
        shape = (row.N, row.H, row.W, Co)
        self.y = Guarded(shape, dtype, SENTINEL, nhwc(o["res"]) if row.res == "y" else None)
        self.res = Guarded(shape, dtype, nan, nhwc(o["res"])) if row.res == "buf" else None
        self.raw = Guarded(shape, dtype, SENTINEL) if (row.raw if raw is None else raw) else None

    def run(self):
        r, p = self.row, (lambda g: g.ptr if g is not None else None)
        s = torch.cuda.current_stream().cuda_stream
        v0, v1, v2 = self.vec
        if r.M:
            rc = self.lib.mtbt_dwconv3x3_mult_nhwc(self.x.ptr, self.w.ptr, p(v0), p(v1), r.act, self.y.ptr, r.N, r.H, r.W, r.C, r.M, self.code, s)
        else:
            ln = (p(v0), p(v1), p(v2), R.DW_EPS, None, None) if r.ln else (None, None, None, 0.0, p(v0), p(v1))
            res = self.y if r.res == "y" else self.res
            if self.raw is not None or res is not None:
                rc = self.lib.mtbt_dwconv_nhwc_train(self.x.ptr, self.w.ptr, *ln, r.act, self.y.ptr, p(self.raw), p(res), r.N, r.H, r.W, r.C, r.k,
                                                     self.code, s)
            else:
                rc = self.lib.mtbt_dwconv_nhwc(self.x.ptr, self.w.ptr, *ln, r.act, self.y.ptr, r.N, r.H, r.W, r.C, r.k, self.code, s)
        assert rc == 0, (r.name, rc)
        torch.cuda.synchronize()
        return self

    def out(self, which="y"):
        """The output as NCHW fp64, after checking its guards and that it is finite."""
        g = self.raw if which == "raw" else self.y
        assert g.guards_untouched(), f"{self.row.name}: written outside {which}"
        assert bool(torch.isfinite(g.view).all()), f"{self.row.name}: {which} is not finite (a read outside the operands reached an output)"
        return g.view.double().cpu().permute(0, 3, 1, 2)

    def bits(self, which="y"):
        g = self.raw if which == "raw" else self.y
        return g.alloc.view(torch.int32 if self.dtype == F32 else torch.int16).cpu()


def worst_ratio(out, ref, bnd):
    return ((out - ref).abs() / bnd).max().item()


def assert_bits(row, dtype, got, want, what, exact=None):
    """Bit equality; a mismatch names the tiles (walk order index, image, tile row, tile column) of the first differing pixels."""
    diff = got != want
    if diff.any():
        px = diff.any(1).nonzero()[:4].tolist()
        tiles = [R.dw_tile_of(row, dtype, *p) for p in px]
        raise AssertionError(f"{row.name} {R.DNAME[dtype]} {what}: {int(diff.sum())} of {diff.numel()} outputs differ from the once-rounded exact result; "
                             f"first pixels (n, y, x) {px} in tiles (index, n, ty, tx) {tiles} of {row.field(dtype, 'tiles')} on "
                             f"{row.field(dtype, 'gx')} workgroups; got {got[diff][:4].tolist()} want {want[diff][:4].tolist()}"
                             + (f" exact {exact[diff][:4].tolist()}" if exact is not None else ""))


def needs_rounding(want, exact, dtype):
    if dtype != F32:
        assert (want != exact).float().mean().item() > 0.3, "the test values must need rounding"


# ---------------------------------------------------------------------------------------------------------------------------------------
# a. parity (the walk rows included: c)
# ---------------------------------------------------------------------------------------------------------------------------------------
def form(row):
    return ("mult" if row.M else "ln" if row.ln else "affine") + str(row.k) + ("-walk" if row.walk else "")


def check_parity(row, dtype):
    o, refs = R.dw_row_reference(row, dtype)
    ln = DwLaunch(row, dtype, o).run()
    for which, (ref, bnd) in refs.items():
        got = ln.out(which)
        print(f"RATIO {form(row)} {R.DNAME[dtype]} {row.name} {which} {worst_ratio(got, ref, bnd):.3f} tiles {row.field(dtype, 'tiles')} "
              f"grid {row.field(dtype, 'gx')}x{row.field(dtype, 'gy')}")
        R.check(got, ref, bnd, f"{row.name} {R.DNAME[dtype]} {which}")


SMALL_PARAMS = [(r, d) for r in R.DW_VARIANTS if not r.walk for d in r.dtypes]
WALK_PARAMS = [(r, d) for r in R.DW_VARIANTS if r.walk for d in r.dtypes]


@pytest.mark.parametrize("row,dtype", SMALL_PARAMS, ids=ids(SMALL_PARAMS))
def test_dw_variant_parity(row, dtype):
    check_parity(row, dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. bit-exact, on integer operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_raw_exact(row, dtype):
    """conv + bias leaves the LayerNorm kernels rounded once, whichever entry point's y goes with it."""
    o, exact = R.dw_exact_operands(row, dtype)
    want = R.rounded_once(exact["raw"], dtype)
    needs_rounding(want, exact["raw"], dtype)
    ln = DwLaunch(row, dtype, o, raw=True).run()
    ln.out("y")
    assert_bits(row, dtype, ln.out("raw"), want, "raw", exact["raw"])


def check_affine_exact(row, dtype):
    """act none: rounded_once(conv * scale + shift [+ res]); res is y: a second launch on the same buffer adds the conv again."""
    assert row.act == R.ACT_NONE
    o, exact = R.dw_exact_operands(row, dtype, target=2000.0 if row.res == "y" else 4000.0)     # (twice the conv stays below 65504)
    first = R.rounded_once(exact["y"], dtype)
    needs_rounding(first, exact["y"], dtype)
    ln = DwLaunch(row, dtype, o).run()
    assert_bits(row, dtype, ln.out("y"), first, "first launch", exact["y"])
    if row.res == "y":
        second = R.rounded_once(first + exact["conv"], dtype)
        needs_rounding(second, first + exact["conv"], dtype)
        assert_bits(row, dtype, ln.run().out("y"), second, "second launch on the same buffer", first + exact["conv"])


LN_PARAMS = [(r, d) for r, d in SMALL_PARAMS if r.ln]
AFFINE_NONE_PARAMS = [(r, d) for r, d in SMALL_PARAMS if not r.ln and not r.M and r.act == R.ACT_NONE]
MULT_PARAMS = [(r, d) for r, d in SMALL_PARAMS if r.M]


@pytest.mark.parametrize("row,dtype", LN_PARAMS, ids=ids(LN_PARAMS))
def test_dw_layernorm_input_is_rounded_once(row, dtype):
    check_raw_exact(row, dtype)


@pytest.mark.parametrize("row,dtype", AFFINE_NONE_PARAMS, ids=ids(AFFINE_NONE_PARAMS))
def test_dw_affine_is_rounded_once(row, dtype):
    check_affine_exact(row, dtype)


@pytest.mark.parametrize("row,dtype", MULT_PARAMS, ids=ids(MULT_PARAMS))
def test_dw_multiplier_equals_plain_calls_on_its_blocks(row, dtype):
    """Channels [m C, (m + 1) C) of the multiplier form are bit-identical to the plain entry on the m-th block of w / scale / shift; with
    act none and integer operands both are the once-rounded exact result."""
    o, exact = R.dw_exact_operands(row, dtype) if row.act == R.ACT_NONE else (R.dw_operands(row, dtype), None)
    got = DwLaunch(row, dtype, o).run().out("y")
    if exact is not None:
        want = R.rounded_once(exact["y"], dtype)
        needs_rounding(want, exact["y"], dtype)
        assert_bits(row, dtype, got, want, "multiplier form", exact["y"])
    Cx = row.C
    for m in range(row.M):
        blk = slice(m * Cx, (m + 1) * Cx)
        plain = dataclasses.replace(row, M=0, name=f"{row.name}[{m}]")
        plain_expect = R.dw_choice(L, L.load(), plain, dtype)
        ob = dict(x=o["x"], w=o["w"][blk], v0=o["v0"][blk], v1=o["v1"][blk], v2=None, res=None)
        ln = DwLaunch(dataclasses.replace(plain, e16=plain_expect, e32=plain_expect), dtype, ob)
        # the block runs the instantiation the multiplier form runs: tile, activation constant, full-tile form
        assert plain_expect[:7] == row.expect(dtype)[:7], (plain_expect, row.expect(dtype))
        assert torch.equal(ln.run().out("y"), got[:, blk]), f"{row.name}: block {m} differs from the plain call"


# ---------------------------------------------------------------------------------------------------------------------------------------
# c. the walk rows
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row,dtype", WALK_PARAMS, ids=ids(WALK_PARAMS))
def test_dw_walk_parity(row, dtype):
    check_parity(row, dtype)


@pytest.mark.parametrize("row,dtype", WALK_PARAMS, ids=ids(WALK_PARAMS))
def test_dw_walk_exact(row, dtype):
    (check_raw_exact if row.ln else check_affine_exact)(row, dtype)


@pytest.mark.parametrize("row,dtype", WALK_PARAMS, ids=ids(WALK_PARAMS))
def test_dw_walk_two_launches_are_bit_identical(row, dtype):
    o = R.dw_operands(row, dtype)
    a, b = DwLaunch(row, dtype, o).run(), DwLaunch(row, dtype, o).run()
    for which in ("y", "raw") if row.raw else ("y",):
        a.out(which)
        same = torch.equal(a.bits(which), b.bits(which))
        print(f"REPEAT {form(row)} {R.DNAME[dtype]} {row.name} {which} {'identical' if same else 'DIFFERENT'}")
        if not same:
            assert_bits(row, dtype, a.out(which), b.out(which), f"{which}: two launches on fresh buffers")
        assert same
