"""Kernel-level tests of the three fused inference kernels per instantiation and per element, through the C ABI:
  upconv_fused.hip  mtbt_convt2x2_conv3x3_nhwc     upconv_fused_kernel<{f32, bf16, f16}, {NONE, SILU}>
  node_gemm.hip     mtbt_bifpn_node_nhwc           node_gemm_kernel<{bf16, f16}, {128, 256}, {top-down, output}>
  mlp_fused.hip     mtbt_convnext_mlp_fused_dt     streaming d = 96, pipelined d = 192, the d = 384 pair kernel
                    mtbt_convnext_mlp_fused_train  the two training (HP) forms

The rows come from kernel_reference.UPCONV_VARIANTS / NODE_VARIANTS / MLP_VARIANTS, the references (fp64 on the operands exactly as the kernel
reads them) and the per-element bounds from the same module; tests/test_cpu_kernel_reference.py shows on the CPU that each check fails for
a set of defective kernels and that the conditions on the inputs (flip shares) hold for every row.  No tolerance is defined here.

Every output lives inside a sentinel-filled allocation with guard pixel rows before and behind it (and, for the slice layouts, channels
beside it and rows between the images): everything outside the view must be unchanged after the launch.  The strided x of the upconv slice
row sits in a NaN-filled buffer: a read outside the slice that reached an output would make it non-finite."""
import ctypes as C

import pytest
import torch

import kernel_reference as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import _lib as L

DEV = "cuda:0"
SENTINEL = 7.0
GUARD_ROWS = 3            # pixel rows before and behind every output view
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
EINVAL, EALIGN = -1, -2
FLIP_CAP = 0.2            # share of rounded intermediates that may lie at a rounding midpoint (asserted for every row on the CPU too)


def ids(params):
    return ["-".join(str(R.DNAME.get(v, getattr(v, "name", v))) for v in p) for p in params]


def code_of(dtype):
    return {F32: L.F32, BF16: L.BF16, F16: L.F16}[dtype]


def esize(dtype):
    return 4 if dtype == F32 else 2


def stream():
    return torch.cuda.current_stream().cuda_stream


def worst_ratio(out, ref, bnd):
    return ((out.double() - ref).abs() / bnd).max().item()


class OutView:
    """An output of `rows` pixel rows x `width` channels as a view into a sentinel-filled [GUARD_ROWS + total_rows + GUARD_ROWS][pitch]
    allocation: `mask` marks what the kernel may write."""

    def __init__(self, total_rows, pitch, dtype):
        self.buf = torch.full((total_rows + 2 * GUARD_ROWS, pitch), SENTINEL, dtype=dtype, device=DEV)
        self.mask = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)
        self.pitch, self.es = pitch, esize(dtype)

    def ptr(self, row, c0):
        return self.buf.data_ptr() + ((GUARD_ROWS + row) * self.pitch + c0) * self.es

    def allow(self, row, nrows, c0, width):
        self.mask[GUARD_ROWS + row:GUARD_ROWS + row + nrows, c0:c0 + width] = True

    def read(self, row, nrows, c0, width):
        return self.buf[GUARD_ROWS + row:GUARD_ROWS + row + nrows, c0:c0 + width].double().cpu()

    def assert_untouched(self, what):
        assert bool((self.buf[~self.mask] == SENTINEL).all()), f"{what}: written outside the output view"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. upconv_fused.hip
# ---------------------------------------------------------------------------------------------------------------------------------------
DENSE = dict(xpad=0, xc0=0, xgap=0, ypad=0, yc0=0, ygap=0)


def run_upconv(row, dtype, act, x, wc, shift9):
    """Launch a row: x [N, C, H, W], wc [4, K, 2, 2, C] fp64 in storage precision, shift9 [9, K] fp32.  Returns the output NCHW fp64 after
    checking that nothing outside the view was written and that every output is finite."""
    N, H, W, K, Cc = row.N, row.H, row.W, row.K, row.channels(dtype)
    lay = R.UP_SLICE if row.layout == "slice" else DENSE
    ldx, xrows = Cc + lay["xpad"], H * W + lay["xgap"]
    xbuf = torch.full((N, xrows, ldx), float("nan"), dtype=dtype, device=DEV)
    xbuf[:, :H * W, lay["xc0"]:lay["xc0"] + Cc] = x.permute(0, 2, 3, 1).reshape(N, H * W, Cc).to(DEV, dtype)
    ldy, yrows = K + lay["ypad"], 4 * H * W + lay["ygap"]
    y = OutView(N * yrows, ldy, dtype)
    for n in range(N):
        y.allow(n * yrows, 4 * H * W, lay["yc0"], K)
    w = wc.reshape(4 * K, 4 * Cc).to(DEV, dtype).contiguous()
    s9 = shift9.to(DEV).contiguous()
    a = L.UpconvArgs()
    a.x, a.w, a.y, a.shift = xbuf.data_ptr() + lay["xc0"] * esize(dtype), w.data_ptr(), y.ptr(0, lay["yc0"]), s9.data_ptr()
    a.x_batch_stride, a.y_batch_stride, a.x_pixel_stride, a.y_pixel_stride = xrows * ldx, yrows * ldy, ldx, ldy
    a.N, a.H, a.W, a.C, a.K, a.dtype, a.act = N, H, W, Cc, K, code_of(dtype), act
    rc = L.load().mtbt_convt2x2_conv3x3_nhwc(C.byref(a), stream())
    assert rc == 0, (row.name, rc)
    torch.cuda.synchronize()
    y.assert_untouched(f"{row.name} {R.DNAME[dtype]}")
    out = torch.stack([y.read(n * yrows, 4 * H * W, lay["yc0"], K) for n in range(N)]).view(N, 2 * H, 2 * W, K).permute(0, 3, 1, 2)
    assert bool(torch.isfinite(out).all()), f"{row.name}: a read outside the x slice reached an output"
    return out


UP_PARAMS = [(r, d, a) for r in R.UPCONV_VARIANTS for d in r.dtypes for a in r.acts]
UP_EXACT = [(r, d) for r in R.UPCONV_VARIANTS if r.exact for d in r.dtypes]


def up_id(p):
    return f"{p[0].name}-{R.DNAME[p[1]]}" + (f"-act{p[2]}" if len(p) > 2 else "")


@pytest.mark.parametrize("row,dtype,act", UP_PARAMS, ids=[up_id(p) for p in UP_PARAMS])
def test_upconv_variant_parity(row, dtype, act):
    """Every element against kernel_reference.upconv_ref.  Bound (upconv_bound, the terms of affine_act_ref with a unit scale and the shift of
    the pixel's border class): ACT_LIPSCHITZ * (ACC * sum |wc x| + EPI * (|pre| + |shift|)) + act_error(pre) + EPI * |y| + output_rounding."""
    x, wc, s9 = R.up_operands(row, dtype)
    ref, bnd, _ = R.upconv_ref(x, wc, s9, act, dtype)
    out = run_upconv(row, dtype, act, x, wc, s9)
    print(f"RATIO upconv {up_id((row, dtype, act))} {worst_ratio(out, ref, bnd):.3f} tiles {row.tiles}")
    R.check(out, ref, bnd, f"upconv {up_id((row, dtype, act))}")


@pytest.mark.parametrize("row,dtype", UP_EXACT, ids=[up_id(p) for p in UP_EXACT])
def test_upconv_exact_rounding(row, dtype):
    """Integer x and wc, a shift9 in steps of 1/64 with nine different class vectors, no activation: every partial sum is exact in fp32, so
    the output must equal, bit for bit, the exact result rounded ONCE -- whatever the slab order, for every border class and channel tile."""
    x, wc, s9, exact = R.up_exact_operands(row, dtype)
    want = R.rounded_once(exact, dtype)
    if dtype != F32:
        assert (want != exact).float().mean().item() > 0.3, "the test values must need rounding"
    got = run_upconv(row, dtype, R.ACT_NONE, x, wc, s9)
    diff = got != want
    assert not diff.any(), f"{int(diff.sum())} of {diff.numel()} outputs differ from the once-rounded exact result; first (n, k, Y, X) " \
                           f"{diff.nonzero()[:4].tolist()}: got {got[diff][:4].tolist()} want {want[diff][:4].tolist()} exact {exact[diff][:4].tolist()}"


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: R.DNAME[d])
def test_upconv_refusals(dtype):
    """MTBT_EINVAL for H = 24, K = 64, C = 40 and act = ELU; MTBT_EALIGN for a y pointer offset by 2 bytes and an odd y_pixel_stride.  The
    buffers hold the largest of these shapes; the unchanged arguments launch."""
    x = torch.zeros(1, 32, 16, 64, dtype=dtype, device=DEV)
    w = torch.zeros(4 * 128, 4 * 64, dtype=dtype, device=DEV)
    y = torch.zeros(1, 64, 32, 260, dtype=dtype, device=DEV)
    s9 = torch.zeros(9, 128, device=DEV)

    def call(**kw):
        a = L.UpconvArgs()
        a.x, a.w, a.y, a.shift = x.data_ptr(), w.data_ptr(), y.data_ptr() + kw.pop("y_offset", 0), s9.data_ptr()
        a.N, a.H, a.W, a.C, a.K, a.dtype, a.act = 1, 16, 16, 64, 128, code_of(dtype), R.ACT_SILU
        for k, v in kw.items():
            setattr(a, k, v)
        a.x_batch_stride, a.x_pixel_stride = a.H * a.W * a.C, a.C
        if not a.y_pixel_stride:
            a.y_pixel_stride = a.K
        a.y_batch_stride = 4 * a.H * a.W * a.y_pixel_stride
        if a.y_pixel_stride % 2:
            a.y_batch_stride = 4 * a.H * a.W * (a.y_pixel_stride + 1)
        return L.load().mtbt_convt2x2_conv3x3_nhwc(C.byref(a), stream())

    assert call() == 0
    torch.cuda.synchronize()
    for kw in (dict(H=24), dict(K=64), dict(C=40), dict(act=R.ACT_ELU)):
        assert call(**kw) == EINVAL, kw
    assert call(y_offset=2) == EALIGN and call(y_pixel_stride=129) == EALIGN


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. node_gemm.hip
# ---------------------------------------------------------------------------------------------------------------------------------------
def nhwc_dev(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def node_args(row, dtype, tensors, w, shift, yptr):
    """mtbt_node_args filled the way engine.Plan.node does, plus what it leaves alone: wgt_dev and a y slice."""
    N, H, W = row.shape
    a = L.NodeArgs()
    wgt = R.NODE_WGT_OTHER[row.kind] if row.wdev else R.NODE_WGT[row.kind]
    for i, (t, wv, m) in enumerate(zip(tensors, wgt, row.modes)):
        a.fuse.x[i], a.fuse.wgt[i], a.fuse.resample[i] = t.data_ptr(), float(wv), m
    a.fuse.n_in = len(tensors)
    a.fuse.N, a.fuse.H, a.fuse.W, a.fuse.C, a.fuse.dtype, a.fuse.add_weight_bug = N, H, W, row.C, code_of(dtype), 0
    a.w, a.shift, a.y, a.y_pixel_stride, a.K, a.act = w.data_ptr(), shift.data_ptr(), yptr, row.pitch, row.C, row.act
    return a


NODE_PARAMS = [(r, d) for r in R.NODE_VARIANTS for d in r.dtypes]


@pytest.mark.parametrize("row,dtype", NODE_PARAMS, ids=ids(NODE_PARAMS))
def test_node_variant_parity(row, dtype):
    """Every element against kernel_reference.node_ref: act(W round_T(s) + shift) with s the fp64 weighted sum of the plainly resampled
    inputs (not fuse_fetch.h's arithmetic).  Bound (node_output): affine_act_ref's terms with a unit scale -- ACT_LIPSCHITZ * (ACC * sum |W s|
    + EPI * (|pre| + |shift|)) + act_error(pre) + EPI * |y| + output_rounding -- plus, for the elements of s that lie within 4 EPI * sum
    |wgt_i resample_i(x_i)| of a rounding midpoint (round_flips), their spacing through ACT_LIPSCHITZ * |W|.  The share of such elements is a
    condition on the inputs, asserted for every row on the CPU.  The top-down rows put 60 pixels in an image, so three of the 64-pixel
    workgroups span two images; the output rows are an odd 5 x 7 map."""
    (inputs, w, shift), (ref, bnd, flip) = R.node_row_reference(row, dtype)
    assert flip.double().mean().item() <= FLIP_CAP, "a condition on the inputs"
    N, H, W = row.shape
    M, K = N * H * W, row.C
    tensors = [nhwc_dev(t, dtype) for t in inputs]
    wd, sd = w.to(DEV, dtype).contiguous(), shift.to(DEV)
    y = OutView(M, row.pitch, dtype)
    y.allow(0, M, row.c0, K)
    a = node_args(row, dtype, tensors, wd, sd, y.ptr(0, row.c0))
    wdev = torch.tensor(list(R.NODE_WGT[row.kind]) + [0.0], dtype=torch.float32, device=DEV) if row.wdev else None
    a.fuse.wgt_dev = wdev.data_ptr() if row.wdev else None
    rc = L.load().mtbt_bifpn_node_nhwc(C.byref(a), stream())
    assert rc == 0, (row.name, rc)
    torch.cuda.synchronize()
    y.assert_untouched(f"{row.name} {R.DNAME[dtype]}")
    out = y.read(0, M, row.c0, K).view(N, H, W, K).permute(0, 3, 1, 2)
    print(f"RATIO node {row.name} {R.DNAME[dtype]} {worst_ratio(out, ref, bnd):.3f} flips {flip.double().mean().item():.4f}")
    R.check(out, ref, bnd, f"node {row.name} {R.DNAME[dtype]}")


def test_node_refusals():
    """MTBT_EINVAL for n_in = 2 with modes (0, 2), a top-down node on an odd W, C = 64, K != C and fp32; the unchanged arguments launch."""
    row = R.NODE_ROWS["td256"]
    N, H, W = row.shape
    tensors = [torch.zeros(N, 2 * H, 2 * W, 256, dtype=BF16, device=DEV) for _ in range(3)]       # large enough for every mode
    w, shift = torch.zeros(256, 256, dtype=BF16, device=DEV), torch.zeros(256, device=DEV)
    y = torch.zeros(N * H * W + 64, 256, dtype=BF16, device=DEV)
    lib = L.load()

    def call(edit=None):
        a = node_args(row, BF16, tensors[:2], w, shift, y.data_ptr())
        if edit:
            edit(a)
        return lib.mtbt_bifpn_node_nhwc(C.byref(a), stream())

    def modes02(a):
        a.fuse.resample[1] = R.RES_DOWN_MEAN

    def odd_w(a):
        a.fuse.W = W - 3

    def c64(a):
        a.fuse.C, a.K, a.y_pixel_stride = 64, 64, 64

    def k_ne_c(a):
        a.K, a.y_pixel_stride = 128, 128

    def fp32(a):
        a.fuse.dtype = L.F32

    assert call() == 0
    torch.cuda.synchronize()
    for edit in (modes02, odd_w, c64, k_ne_c, fp32):
        assert call(edit) == EINVAL, edit.__name__


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. mlp_fused.hip
# ---------------------------------------------------------------------------------------------------------------------------------------
MLP_INFER = [(r, d) for r in R.MLP_VARIANTS if not r.train for d in r.dtypes]
MLP_TRAIN = [(r, d) for r in R.MLP_VARIANTS if r.train for d in r.dtypes]


def ptr(t):
    return t.data_ptr() if t is not None else None


def guarded(M, width, dtype):
    return torch.full((M + GUARD_ROWS, width), SENTINEL, dtype=dtype, device=DEV)


@pytest.mark.parametrize("row,dtype", MLP_INFER, ids=ids(MLP_INFER))
def test_mlp_variant_parity(row, dtype):
    """mtbt_convnext_mlp_fused_dt, bf16 and fp16, every element against kernel_reference.mlp_ref (the kernel's polynomial GELU in fp64, h
    rounded to the storage type as the kernel feeds it to the second MFMA).  Bound: output_rounding(ref) + ACC * (sum |W2 h| + |res| +
    |b2|), plus for the hidden units within ACT_LIPSCHITZ * ACC * (sum |W1 t| + |b1|) + ACT_EVAL / 2 * (1 + |h|) of a rounding midpoint
    (round_flips) their spacing through |W2|; their share is a condition on the inputs, asserted for every row on the CPU.  M = 1, 17, 33,
    127, 129, 300 against the 16-pixel fragments, 32-pixel waves and 128-pixel workgroups; res = NULL rows; three guard rows behind y."""
    (t, res, w1, b1, w2, b2), (ref, bnd, _, _, flip) = R.mlp_row_reference(row, dtype)
    assert flip.double().mean().item() <= FLIP_CAP, "a condition on the inputs"
    M, D = row.M, row.D
    dev = [v.to(DEV, dtype).contiguous() if v is not None else None for v in (t, res, w1, R.mlp_permute_w2(w2))]
    b1d, b2d = b1.to(DEV), b2.to(DEV)
    y = guarded(M, D, dtype)
    rc = L.load().mtbt_convnext_mlp_fused_dt(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(b1d), ptr(dev[3]), ptr(b2d), y.data_ptr(), M, D,
                                             code_of(dtype), stream())
    assert rc == 0, (row.name, rc)
    torch.cuda.synchronize()
    got = y.double().cpu()
    assert bool((got[M:] == SENTINEL).all()), "written past row M"
    print(f"RATIO mlp {row.name} {R.DNAME[dtype]} {worst_ratio(got[:M], ref, bnd):.3f} flips {flip.double().mean().item():.4f}")
    R.check(got[:M], ref, bnd, f"mlp {row.name} {R.DNAME[dtype]}")


@pytest.mark.parametrize("row,dtype", MLP_TRAIN, ids=ids(MLP_TRAIN))
def test_mlp_train_variant_parity(row, dtype):
    """mtbt_convnext_mlp_fused_train (bf16, d = 96 / 192): y per element against the same reference and bound as the inference entry (the fc1
    rows permuted as the header states, fc2 natural), and the kept pre-activation per element: |hpre - pre| <= output_rounding(pre, bf16) +
    ACC * (sum |W1 t| + |b1|).  Three guard rows behind both outputs."""
    (t, res, w1, b1, w2, b2), (ref, bnd, pre, pbnd, flip) = R.mlp_row_reference(row, dtype)
    assert flip.double().mean().item() <= FLIP_CAP, "a condition on the inputs"
    M, D = row.M, row.D
    perm = R.mlp_train_rows(4 * D)
    dev = [v.to(DEV, dtype).contiguous() for v in (t, res, w1[perm], w2)]
    b1d, b2d = b1[perm].contiguous().to(DEV), b2.to(DEV)
    y, hp = guarded(M, D, dtype), guarded(M, 4 * D, dtype)
    rc = L.load().mtbt_convnext_mlp_fused_train(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(b1d), ptr(dev[3]), ptr(b2d), y.data_ptr(), hp.data_ptr(),
                                                M, D, stream())
    assert rc == 0, (row.name, rc)
    torch.cuda.synchronize()
    got, gp = y.double().cpu(), hp.double().cpu()
    assert bool((got[M:] == SENTINEL).all()) and bool((gp[M:] == SENTINEL).all()), "written past row M"
    print(f"RATIO mlp {row.name} y {worst_ratio(got[:M], ref, bnd):.3f} hpre {worst_ratio(gp[:M], pre, pbnd):.3f} "
          f"flips {flip.double().mean().item():.4f}")
    R.check(gp[:M], pre, pbnd, f"mlp {row.name} hpre")
    R.check(got[:M], ref, bnd, f"mlp {row.name} y")


def test_mlp_train_refuses_d384():
    M, D = 17, 384
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=DEV)
    t, res, w1, w2, y, hp = z(M, D), z(M, D), z(4 * D, D), z(D, 4 * D), z(M, D), z(M, 4 * D)
    b1, b2 = z(4 * D, dt=F32), z(D, dt=F32)
    assert L.load().mtbt_convnext_mlp_fused_train(ptr(t), ptr(res), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(y), ptr(hp), M, D, stream()) == EINVAL
