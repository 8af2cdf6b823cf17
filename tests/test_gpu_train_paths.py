"""The training kernels on the paths the batch-32 step takes and the one-shape tests never reach: the tall-matrix pre-reduction of
csrc/rowreduce.h (more than 768 partial rows), the four-rows-in-flight trip and the grid caps of the BatchNorm apply passes, the general
(C / 8 not a power of two) BatchNorm kernels, the multi-workgroup partials and grid caps of csrc/resample_bwd.hip, the projector backward at
non-integer resize ratios, and mtbt_gap_fc_backward / mtbt_channel_sum / mtbt_sumsq / mtbt_add_nhwc at the sizes where their launch shape
or reduction path changes.

References: CPU float64, plain torch (autograd through F.interpolate / F.max_pool2d / an explicit BatchNorm / Linear, or explicit sums), from
the inputs the kernel sees (bf16 cases: the inputs are rounded to bf16 first, then taken to float64, so only the kernel's own arithmetic and
its one output rounding differ).

Bounds: elementwise  |got - want| <= u_T * |want| + ACC * sum|terms|,  u_T = 2^-8 (bf16: one rounding, factor 2 of slack) or 2^-22 (fp32),
ACC = 2e-5 = the fp32 accumulation bound of test_conv_column_sums, sum|terms| = the sum of the absolute values of the terms that form the
element, taken from the float64 reference (so a cancelling sum is judged against what was added up, not against what is left).  Where the
result is added onto an earlier value the rounding term is relative to |prev + want|.  Where a kernel result feeds another (statistics ->
normalised value -> derivative), the first result's own term list enters the second's with its first-order factor; the docstrings say how.
Every check prints its largest error next to the bound of that element."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from multitask_bonetumor_yolo_amd import _lib as L
    from multitask_bonetumor_yolo_amd.engine import Act, Plan

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
CODE = {F32: 0, BF16: 1}
U = {F32: 2.0 ** -22, BF16: 2.0 ** -8}
ACC = 2e-5
SENTINEL = -12345.0


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(t, dtype):
    """The value the kernel sees: rounded to `dtype`, kept as fp32."""
    return t.to(dtype).float()


def nhwc(t, dtype=F32):
    """[N,C,H,W] (CPU, any float type) -> dense NHWC on the device in `dtype`."""
    return t.permute(0, 2, 3, 1).contiguous().to(DEV, dtype)


def back(t):
    """device NHWC -> CPU float64 [N,C,H,W]."""
    return t.detach().cpu().double().permute(0, 3, 1, 2)


def within(what, got, want, bound):
    """Elementwise |got - want| <= bound; prints the largest error and the bound of the element that comes closest to (or passes) it."""
    got, want, bound = got.detach().cpu().double().reshape(-1), want.detach().double().reshape(-1), bound.detach().double().reshape(-1)
    assert got.shape == want.shape == bound.shape, f"{what}: shapes {got.shape} {want.shape} {bound.shape}"
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(bound).all()), f"{what}: the reference itself is not finite"
    err = (got - want).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    if err.numel() == 0:
        return
    i = int((err - bound).argmax())
    bad = int((err > bound).sum())
    print(f"{what}: max err {err.max().item():.3e}; nearest the bound: err {err[i].item():.3e} (bound {bound[i].item():.3e}) at {i}, want {want[i].item():.6g} "
          f"got {got[i].item():.6g}; {bad} of {err.numel()} outside")
    assert bad == 0, f"{what}: {bad} of {err.numel()} elements outside the bound, worst at flat index {i}: got {got[i].item()!r}, want {want[i].item()!r}, " \
                     f"err {err[i].item():.3e} > bound {bound[i].item():.3e}"


# ----------------------------------------------------------------------------------------------------------------------------------
# float64 BatchNorm + activation, forward and backward, and the term lists of the bounds
# ----------------------------------------------------------------------------------------------------------------------------------
ACTS = {"none": (0, lambda v: v), "silu": (1, F.silu), "elu": (2, F.elu), "gelu": (3, F.gelu)}   # codes: _lib.ACT_NONE / SILU / ELU / GELU


def bn_reference(x, dy, gamma, beta, eps, act, mean=None, var=None):
    """y = act((x - mean) * rstd * gamma + beta) and its gradients by autograd; x, dy [P, C] float64.  mean / var given: constants (running
    statistics); else the batch mean and biased variance, differentiated through (what BatchNorm2d in train mode does -- BatchNorm2d itself
    refuses one value per channel, the kernels do not)."""
    xl, g, b = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    if mean is None:
        mean = xl.mean(0)
        var = ((xl - mean) ** 2).mean(0)
    rstd = (var + eps).rsqrt()
    xh = (xl - mean) * rstd
    u = xh * g + b
    u.retain_grad()
    y = ACTS[act][1](u)
    y.backward(dy)
    return dict(y=y.detach(), mean=mean.detach(), var=var.detach(), rstd=rstd.detach(), xh=xh.detach(), du=u.grad.detach(), dx=xl.grad, dgamma=g.grad,
                dbeta=b.grad)


def bn_terms(r, x, dy, gamma, beta, running, t_mean=0.0, t_var=0.0):
    """sum|terms| (in units of ACC) of every BatchNorm result.  t_mean / t_var: the term lists of the statistics the kernel normalises with
    (0 when they are exact inputs); they enter xhat with their first-order factors rstd and xhat * rstd^2 / 2.  |act'| <= 1.2 and |act''| <= 1
    for the four activations, so du = dy * act'(u) carries |dy| * t_u plus its own product."""
    M = x.shape[0]
    mu, rstd, xh, du = r["mean"], r["rstd"], r["xh"], r["du"]
    ga = gamma.abs()
    t_xh = (x.abs() + mu.abs()) * rstd + t_mean * rstd + xh.abs() * 0.5 * t_var * rstd ** 2     # x - mean without cancellation, + the statistics
    t_u = t_xh * ga + beta.abs()
    t_du = dy.abs() * t_u + du.abs()
    gr = ga * rstd
    t_gr = 1.0 + 0.5 * t_var * rstd ** 2                                                           # gamma * rstd, relative
    if running:
        t_dx = gr * (t_du + du.abs() * t_gr)
    else:
        s2 = (du * xh).sum(0)
        inner = t_du + t_du.mean(0) + du.abs().mean(0) + xh.abs() * ((t_du * xh.abs() + du.abs() * t_xh).mean(0) + (du * xh).abs().mean(0)) + t_xh * s2.abs() / M
        t_dx = gr * (inner + (du.abs() + du.abs().mean(0) + xh.abs() * (du * xh).abs().mean(0)) * t_gr)
    return dict(y=1.2 * t_u, dx=t_dx, dgamma=(t_du * xh.abs() + du.abs() * t_xh + (du * xh).abs()).sum(0), dbeta=(t_du + du.abs()).sum(0))


def stat_terms(x):
    """sum|terms| / P of the forward's statistics as csrc/bn_train.hip forms them: per 256-row block sums shifted by the block's first
    row (M2_b = sum d^2 - (sum d)^2 / n_b), combined exactly (Chan et al.): mean = sum n_b mean_b / P, M2 = sum M2_b + n_b (mean_b - mean)^2."""
    P = x.shape[0]
    mu = x.mean(0)
    t_var = torch.zeros_like(mu)
    for r0 in range(0, P, 256):
        blk = x[r0:r0 + 256]
        nb = blk.shape[0]
        d = blk - blk[0]
        sd = d.abs().sum(0)
        off = (blk.mean(0) - mu).abs()
        t_var += (d ** 2).sum(0) + sd ** 2 / nb + nb * off ** 2 + 2 * nb * off * (blk[0].abs() + sd / nb + mu.abs())
    return x.abs().mean(0) + mu.abs(), t_var / P


def running_update(old, new, momentum, b_new, scale=1.0):
    """(1 - m) * old + m * new * scale in float64 with the fp32 momentum, and its bound: four fp32 roundings (1 - m, two products, the
    sum) = 2^-22 of the two addends, plus the statistic's own bound."""
    m = float(torch.tensor(momentum, dtype=torch.float32))
    want = (1.0 - m) * old + m * new * scale
    return want, U[F32] * (((1.0 - m) * old).abs() + (m * new * scale).abs()) + m * scale * b_new


# ----------------------------------------------------------------------------------------------------------------------------------
# A. tall partial matrices (csrc/rowreduce.h: colsum_prereduce / colsum_tile_kernel above 768 rows)
# ----------------------------------------------------------------------------------------------------------------------------------
def partial_stats_reference(M64, shift, n, Cc):
    """statistics from partial rows [rows][>= 2C] (float64): mean = shift + s1 / n, var = (s2 - n m1^2) / n, and their bounds: the two column
    sums with ACC * sum|terms|; m1^2 carries 2 |m1| e1 (+ e1^2); the fp32 operations behind the sums round results no larger than
    s2 / n, m1^2 and the variance itself."""
    t1, t2 = M64[:, :Cc], M64[:, Cc:2 * Cc]
    s1, s2 = t1.sum(0), t2.sum(0)
    e1, e2 = ACC * t1.abs().sum(0), ACC * t2.abs().sum(0)
    m1 = s1 / n
    mean = shift + m1
    m2 = s2 - n * m1 ** 2
    var = m2 / n
    b_mean = e1 / n + U[F32] * (shift.abs() + m1.abs())
    b_var = (e2 + 2 * m1.abs() * e1 + e1 ** 2 / n) / n + U[F32] * (s2.abs() / n + 2 * m1 ** 2 + var.abs())
    return mean, var, m2, b_mean, b_var


def run_bn_partials(lib, buf, rows, pitch, x, dtype, Cc, gamma, beta, shift, rm0, rv0, momentum, eps, act):
    """mtbt_bn_forward_partials_nhwc on the partial matrix at the head of `buf`; returns (stats, running_mean, running_var, y)."""
    n = x.shape[0]
    xd = x.to(DEV, dtype)
    y = torch.empty_like(xd)
    stats = torch.full((2 * Cc,), 7.0, device=DEV)
    rm, rv = rm0.float().to(DEV), rv0.float().to(DEV)
    g, b, sh = gamma.float().to(DEV), beta.float().to(DEV), shift.float().to(DEV)
    L.check(lib.mtbt_bn_forward_partials_nhwc(xd.data_ptr(), y.data_ptr(), Cc, g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), C.c_float(momentum),
                                              C.c_float(eps), ACTS[act][0], n, Cc, CODE[dtype], buf.data_ptr(), rows, pitch, sh.data_ptr(), stats.data_ptr(), S()),
            "bn from partial rows")
    torch.cuda.synchronize()
    return stats, rm, rv, y


def check_bn_partials(tag, got, M64, x, dtype, Cc, gamma, beta, shift, rm0, rv0, momentum, eps, act):
    stats, rm, rv, y = got
    n = x.shape[0]
    mean, var, m2, b_mean, b_var = partial_stats_reference(M64, shift, n, Cc)
    assert bool((m2 > 0.25 * M64[:, Cc:2 * Cc].sum(0)).all()), "the test's own data: s2 - n m1^2 must stay well above zero"
    within(f"{tag} mean", stats[:Cc], mean, b_mean)
    within(f"{tag} var", stats[Cc:], var, b_var)
    want, bound = running_update(rm0, mean, momentum, b_mean)
    within(f"{tag} running_mean", rm, want, bound)
    want, bound = running_update(rv0, var, momentum, b_var, n / (n - 1.0))
    within(f"{tag} running_var", rv, want, bound)
    # y under the statistics the kernel itself stored: what is left is the apply pass's own fp32 arithmetic and one output rounding
    km, kv = stats[:Cc].cpu().double(), stats[Cc:].cpu().double()
    rstd = (kv + eps).rsqrt()
    xh = (x.double() - km) * rstd
    want = ACTS[act][1](xh * gamma + beta)
    within(f"{tag} y", y, want, U[dtype] * want.abs() + 1.2 * ACC * (xh.abs() * gamma.abs() + beta.abs()))


@pytest.mark.parametrize("extra", [0, 24], ids=["pitch2C", "pitch2C+24"])
@pytest.mark.parametrize("Cc", [8, 24, 64])
@pytest.mark.parametrize("rows", [768, 769, 1000, 12288, 12289, 51200])
def test_bn_forward_from_tall_partial_rows(rows, Cc, extra):
    """A1.  rows: 768 = the last size without a fold; 769 = 4 segments of 193 rows, the last ragged; 12288 = 48 segments of 256; 12289 =
    the cap of 48 segments, 257 rows each; 51200 = the tallest matrix of the batch-32 step.  C = 8: one 16-column block exactly; 24: three;
    64: eight.  A pitch wider than 2C leaves sentinel columns between the rows; a sentinel guard follows the matrix.  The fold works in place,
    so the bit-identity check runs on a fresh copy.  (fp32 x with the dense pitch, bf16 x with the padded one.)"""
    lib = L.load()
    dtype = F32 if extra == 0 else BF16
    g = torch.Generator().manual_seed(rows * 131 + Cc + extra)
    pitch, n, GUARD = 2 * Cc + extra, 64, 4096
    M = torch.full((rows, pitch), SENTINEL)
    M[:, :Cc] = torch.randn(rows, Cc, generator=g) * 0.5
    M[:, Cc:2 * Cc] = torch.rand(rows, Cc, generator=g) + 0.25
    flat = torch.cat([M.reshape(-1), torch.full((GUARD,), SENTINEL)])
    x = rnd(torch.randn(n, Cc, generator=g) * 1.5 + 0.2, dtype)
    gamma, beta = (torch.rand(Cc, generator=g) + 0.5).double(), (torch.randn(Cc, generator=g) * 0.2).double()
    shift, rm0, rv0 = (torch.randn(Cc, generator=g) * 0.1 + 0.4).double(), (torch.randn(Cc, generator=g) * 0.1).double(), (torch.rand(Cc, generator=g) + 0.5).double()
    args = (x, dtype, Cc, gamma, beta, shift, rm0, rv0, 0.03, 1e-3, "silu")
    buf = flat.to(DEV)
    got = run_bn_partials(lib, buf, rows, pitch, *args)
    check_bn_partials(f"rows {rows} C {Cc} pitch {pitch}", got, M.double(), *args)
    after = buf.cpu()
    assert bool((after[:rows * pitch].view(rows, pitch)[:, 2 * Cc:] == SENTINEL).all()), "the columns past 2C are not the kernel's"
    assert bool((after[rows * pitch:] == SENTINEL).all()), "nothing behind the matrix is touched"
    again = run_bn_partials(lib, flat.to(DEV), rows, pitch, *args)
    for a, b, what in zip(got, again, ("stats", "running_mean", "running_var", "y")):
        assert torch.equal(a, b), f"{what}: a second call on a fresh copy of the matrix is bit-identical"


@pytest.mark.parametrize("running", [0, 1], ids=["batch", "running"])
@pytest.mark.parametrize("dtype,Cc", [(F32, 8), (BF16, 16)], ids=["f32-C8", "bf16-C16"])
def test_bn_backward_tall_partials(dtype, Cc, running):
    """A2.  P = 769 * 256 - 100 pixels: 769 partial rows, folded in 4 segments of 193 with a ragged last one and a ragged last workgroup;
    dy is read from a channel slice.  The statistics are an input here (the float64 ones, rounded to fp32: 2^-24 relative, inside the
    (|x| + |mean|) * rstd term); accumulate = 1 onto preset d gamma / d beta must give preset + sum."""
    lib = L.load()
    g = torch.Generator().manual_seed(7 + Cc + running)
    P, LD, OFF, eps = 769 * 256 - 100, Cc + 8, 8, 1e-3
    x = rnd(torch.randn(P, Cc, generator=g) * 1.5 + 0.2, dtype).double()
    dy = rnd(torch.randn(P, Cc, generator=g), dtype).double()
    gamma, beta = (torch.rand(Cc, generator=g) + 0.5).float().double(), (torch.randn(Cc, generator=g) * 0.2).float().double()
    if running:
        mean, var = (torch.randn(Cc, generator=g) * 0.1 + 0.2).float().double(), (torch.rand(Cc, generator=g) + 1.5).float().double()
        r = bn_reference(x, dy, gamma, beta, eps, "silu", mean, var)
    else:
        r = bn_reference(x, dy, gamma, beta, eps, "silu")
        mean, var = r["mean"], r["var"]
    t = bn_terms(r, x, dy, gamma, beta, bool(running))
    stats = torch.cat([mean, var]).float().to(DEV)
    dcat = torch.zeros(P, LD, dtype=dtype, device=DEV)
    dcat[:, OFF:OFF + Cc] = dy.to(DEV, dtype)
    xd = x.to(DEV, dtype)
    dx = torch.empty(P, Cc, dtype=dtype, device=DEV)
    pre_g, pre_b = torch.randn(Cc, generator=g).double() * 50, torch.randn(Cc, generator=g).double() * 50
    gd, bd = gamma.float().to(DEV), beta.float().to(DEV)
    assert (P + 255) // 256 > 768
    nb = lib.mtbt_bn_backward_workspace_bytes(P, Cc)
    ws = torch.empty(nb // 4, device=DEV)
    for accumulate in (0, 1):
        dg, db = pre_g.float().to(DEV), pre_b.float().to(DEV)
        L.check(lib.mtbt_bn_backward_nhwc(dcat.view(-1)[OFF:].data_ptr(), LD, xd.data_ptr(), stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), C.c_float(eps),
                                          ACTS["silu"][0], running, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), accumulate, P, Cc, CODE[dtype], ws.data_ptr(), nb,
                                          S()), "bn_backward")
        torch.cuda.synchronize()
        tag = f"P {P} C {Cc} {'running' if running else 'batch'} accumulate {accumulate}"
        wg, wb = r["dgamma"] + accumulate * pre_g.float().double(), r["dbeta"] + accumulate * pre_b.float().double()
        within(f"{tag} dgamma", dg, wg, U[F32] * wg.abs() + ACC * t["dgamma"])
        within(f"{tag} dbeta", db, wb, U[F32] * wb.abs() + ACC * t["dbeta"])
        if accumulate == 0:
            within(f"{tag} dx", dx, r["dx"], U[dtype] * r["dx"].abs() + ACC * t["dx"])


COLSUM_CASES = [
    # (N, H, W, C, K, k, tile_hint, policy)
    (2, 80, 80, 64, 64, 1, (64 << 16) | 64, 0),     # implicit GEMM 1x1 on the 64-pixel tile: 200 pixel tiles x 4 wave rows = 800 partial rows
    (4, 112, 112, 64, 64, 3, 0, 16),                # direct 3x3, first formulation: 196 tiles of 16 x 16 x 4 rows = 784 partial rows
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cfg", COLSUM_CASES, ids=["gemm1x1", "direct3x3"])
def test_conv_column_sums_above_768_rows(dtype, cfg):
    """A3.  The conv epilogue's column sums where the second level folds first: the finished sums against float64 sums over the stored
    output (tolerances of test_conv_column_sums, per channel), then the partial-rows form through mtbt_bn_forward_partials_nhwc with the
    bounds of A1.  The `rows > 768` precondition keeps a change of the dispatch from turning this into a small-matrix test."""
    N, H, W, Cc, K, k, hint, policy = cfg
    lib = L.load()
    torch.manual_seed(41 + k)
    x = rnd(torch.randn(N, Cc, H, W), dtype)
    w = rnd(torch.randn(K, Cc, k, k) / (Cc * k * k) ** 0.5, dtype)
    shift = torch.randn(K) * 0.1 + 0.4
    p = Plan(torch.device(DEV))
    y = Act.of(torch.empty(N, H, W, K, dtype=dtype, device=DEV))
    wp = w.permute(0, 2, 3, 1).reshape(K, -1).contiguous().to(DEV, dtype)
    a = p.conv(Act.of(nhwc(x, dtype)), wp, y, R=k, S=k, pad=k // 2, shift=(torch.randn(K) * 0.3 + 0.5).to(DEV), tile_hint=hint, policy=policy)
    sh = shift.to(DEV)
    a.colsum_shift, a.colsum_sq = sh.data_ptr(), 1
    a.colsum_ws, a.colsum_ws_bytes = 0x1000, 1 << 30        # (the query dereferences nothing)
    rows, pitch = C.c_int64(0), C.c_int32(0)
    L.check(lib.mtbt_conv_colsum_layout(C.byref(a), C.byref(rows), C.byref(pitch)), "layout")
    rows, pitch = rows.value, pitch.value
    assert rows > 768 and pitch == 2 * K, f"{rows} partial rows of pitch {pitch}: this case must reach the pre-reduction"
    n, GUARD = rows * pitch, 4096
    # finished sums
    buf = torch.cat([torch.full((n,), float("nan")), torch.full((GUARD,), SENTINEL)]).to(DEV)
    sums = torch.full((2 * K,), 7.0, device=DEV)
    a.colsum, a.colsum_accumulate = sums.data_ptr(), 0
    a.colsum_ws, a.colsum_ws_bytes = buf.data_ptr(), n * 4
    p.run()
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all()), "nothing behind the announced rows is touched"
    d = y.buf.float().cpu().reshape(-1, K).double() - shift.double()
    want1, want2 = d.sum(0), (d ** 2).sum(0)
    tol = 2e-5 if dtype == F32 else 2e-4        # (test_conv_column_sums: accumulation order only, the summed values are the stored ones)
    within(f"{rows} rows: column sums", sums[:K], want1, tol * d.abs().sum(0) + 1e-6)
    within(f"{rows} rows: column sums of squares", sums[K:], want2, tol * want2 + 1e-6)
    # partial rows -> BatchNorm statistics
    a.colsum = None
    buf2 = torch.cat([torch.full((n,), float("nan")), torch.full((GUARD,), SENTINEL)]).to(DEV)
    a.colsum_ws, a.colsum_ws_bytes = buf2.data_ptr(), n * 4
    p.run()
    torch.cuda.synchronize()
    M = buf2[:n].cpu().view(rows, pitch)
    assert bool(torch.isfinite(M).all()), "every announced float is written"
    P = N * H * W
    g = torch.Generator().manual_seed(5)
    gamma, beta = (torch.rand(K, generator=g) + 0.5).double(), (torch.randn(K, generator=g) * 0.2).double()
    rm0, rv0 = shift.double(), (torch.rand(K, generator=g) + 0.5).double()
    xin = y.buf.float().cpu().reshape(-1, K)
    args = (xin, dtype, K, gamma, beta, shift.double(), rm0, rv0, 0.03, 1e-3, "silu")
    got = run_bn_partials(lib, buf2, rows, pitch, *args)
    check_bn_partials(f"{rows} conv rows", got, M.double(), *args)
    assert bool((buf2[n:] == SENTINEL).all()), "the fold stays inside the matrix"
    # ... and they are the statistics of the stored map (the partial rows were written by the epilogue, not by this test)
    mean, var = xin.double().mean(0), xin.double().var(0, unbiased=False)
    within(f"{rows} conv rows: mean of the stored map", got[0][:K], mean, tol * d.abs().sum(0) / P + U[F32] * (mean.abs() + shift.abs().double()))
    within(f"{rows} conv rows: variance of the stored map", got[0][K:], var,
           tol * (want2 + 2 * want1.abs() / P * d.abs().sum(0)) / P + U[F32] * (want2 / P + 2 * (want1 / P) ** 2 + var))


# ----------------------------------------------------------------------------------------------------------------------------------
# B. csrc/resample_bwd.hip
# ----------------------------------------------------------------------------------------------------------------------------------
def fuse_resample(x, mode):
    if mode == 0:
        return x * 1.0
    return F.interpolate(x, scale_factor=2 if mode == 1 else 0.5, mode="bilinear", align_corners=False)


def fuse_in_shape(mode, H, W):
    return {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W)}[mode]


FUSE_SMALL = [(N, H, W, Cc, mode) for (N, H, W, Cc), modes in (((1, 2, 2, 8), (0, 1, 2)),       # mode 1: a 1 x 1 input, both bilinear taps clamp
                                                               ((1, 5, 7, 24), (0, 2)),          # odd sizes; 3 chunks per pixel
                                                               ((3, 6, 10, 8), (0, 1, 2)))       # one chunk per pixel, several images
              for mode in modes]
FUSE_BIG = [(2, 64, 66, 256, mode) for mode in (0, 1, 2)]       # 270 336 output items: past the dot's 1024 workgroups of 256


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", FUSE_SMALL + FUSE_BIG, ids=lambda s: "x".join(map(str, s[:4])) + f"-mode{s[4]}")
def test_bifpn_fuse_backward_paths(dtype, shape):
    """B1.  dx (+)= w * resample^T(dy), dwgt (+)= <dy, resample(x)>.  Terms: for dx the transposed resampling of |dy| times |w|; for dwgt
    sum |dy| * resample(|x|) (the bilinear value is itself an fp32 sum of four products).  Small shapes run every accumulate combination and
    both NULL forms; the large one runs one combination (its point is the 1024-workgroup cap and scalar_final over 1024 partials)."""
    N, H, W, Cc, mode = shape
    lib = L.load()
    g = torch.Generator().manual_seed(100 * mode + H)
    hi, wi = fuse_in_shape(mode, H, W)
    big = N * H * W * Cc // 8 > 262144
    x, dy = torch.randn(N, Cc, hi, wi, generator=g), torch.randn(N, Cc, H, W, generator=g)
    if big:       # all products of one sign: each of the 1024 partials is ~ 1 / 1024 of the sum, far above the accumulation bound, so a lost one shows
        x, dy = x.abs() + 0.25, dy.abs() + 0.25
    x = rnd(x, dtype).double().requires_grad_()
    dy = rnd(dy, dtype).double()
    wv = 0.37
    wgt = float(torch.tensor(wv, dtype=torch.float32))
    r = fuse_resample(x, mode)
    (tx,) = torch.autograd.grad(r, x, dy, retain_graph=True)                    # resample^T(dy)
    (ta,) = torch.autograd.grad(r, x, dy.abs())                                 # resample^T(|dy|)
    want_dx, t_dx = wgt * tx, abs(wgt) * ta
    want_dw = (dy * r.detach()).sum()
    t_dw = (dy.abs() * fuse_resample(x.detach().abs(), mode)).sum()
    prev = rnd(torch.randn(N, hi, wi, Cc, generator=g), dtype)
    pre_w = 3.25
    wdev = torch.tensor([wv], device=DEV)
    nb = lib.mtbt_bifpn_fuse_backward_workspace_bytes()
    ws = torch.empty(nb // 4, device=DEV)
    dyd, xd = nhwc(dy, dtype), nhwc(x.detach(), dtype)
    combos = [(0, 1)] if big else [(0, 0), (0, 1), (1, 0), (1, 1)]
    tag = f"fuse {shape} {dtype}"
    for acc_dx, acc_dw in combos:
        dx = prev.clone().to(DEV, dtype)
        dwg = torch.tensor([pre_w], device=DEV)
        L.check(lib.mtbt_bifpn_fuse_backward(dyd.data_ptr(), xd.data_ptr(), mode, wdev.data_ptr(), dx.data_ptr(), acc_dx, dwg.data_ptr(), acc_dw, N, H, W, Cc,
                                             CODE[dtype], ws.data_ptr(), nb, S()), "fuse bwd")
        torch.cuda.synchronize()
        want = want_dx + acc_dx * prev.double().permute(0, 3, 1, 2)
        within(f"{tag} dx accumulate {acc_dx}", back(dx), want, U[dtype] * want.abs() + ACC * t_dx)
        want = want_dw + acc_dw * pre_w
        within(f"{tag} dwgt accumulate {acc_dw}", dwg, want.view(1), (U[F32] * want.abs() + ACC * t_dw).view(1))
    if big:
        return
    # dx = NULL: only the weight gradient
    dwg = torch.tensor([pre_w], device=DEV)
    L.check(lib.mtbt_bifpn_fuse_backward(dyd.data_ptr(), xd.data_ptr(), mode, wdev.data_ptr(), None, 0, dwg.data_ptr(), 0, N, H, W, Cc, CODE[dtype], ws.data_ptr(), nb,
                                         S()), "fuse bwd, dx NULL")
    torch.cuda.synchronize()
    within(f"{tag} dwgt alone", dwg, want_dw.view(1), (U[F32] * want_dw.abs() + ACC * t_dw).view(1))
    # dwgt = NULL: no forward input and no workspace needed
    dx = prev.clone().to(DEV, dtype)
    L.check(lib.mtbt_bifpn_fuse_backward(dyd.data_ptr(), None, mode, wdev.data_ptr(), dx.data_ptr(), 0, None, 0, N, H, W, Cc, CODE[dtype], None, 0, S()),
            "fuse bwd, dwgt NULL")
    torch.cuda.synchronize()
    within(f"{tag} dx alone", back(dx), want_dx, U[dtype] * want_dx.abs() + ACC * t_dx)
    assert lib.mtbt_bifpn_fuse_backward(dyd.data_ptr(), xd.data_ptr(), mode, wdev.data_ptr(), None, 0, dwg.data_ptr(), 0, N, H, W, Cc, CODE[dtype], None, 0, S()) != 0, \
        "a weight gradient without a workspace is refused"


def test_bifpn_fuse_backward_past_the_dx_grid_cap():
    """B1.  Mode 2 at an output of 2 x 96 x 88 x 256: the input has 2 x 192 x 176 x 32 = 2 162 688 work items, more than 8192 workgroups of
    256, so the grid-stride loop of fuse_bwd_dx takes a second trip.  dx = w * dy / 4 at the pooled position: one term."""
    lib = L.load()
    N, H, W, Cc = 2, 96, 88, 256
    assert N * 2 * H * 2 * W * (Cc // 8) > 8192 * 256
    g = torch.Generator().manual_seed(9)
    dy = torch.randn(N, H, W, Cc, generator=g)
    wgt = float(torch.tensor(0.37, dtype=torch.float32))
    want = (wgt * 0.25) * dy.double().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)       # NHWC; == autograd through the 2x2 mean (checked on a corner)
    xs = torch.zeros(1, 1, 4, 4, dtype=torch.float64, requires_grad=True)
    (gs,) = torch.autograd.grad(F.interpolate(xs, scale_factor=0.5, mode="bilinear", align_corners=False), xs, torch.tensor([[[[1.0, 2.0], [3.0, 4.0]]]], dtype=torch.float64))
    assert torch.equal(gs[0, 0], 0.25 * torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64).repeat_interleave(2, 0).repeat_interleave(2, 1))
    wdev = torch.tensor([0.37], device=DEV)
    dyd = dy.to(DEV)
    dx = torch.full((N, 2 * H, 2 * W, Cc), SENTINEL, device=DEV)
    L.check(lib.mtbt_bifpn_fuse_backward(dyd.data_ptr(), None, 2, wdev.data_ptr(), dx.data_ptr(), 0, None, 0, N, H, W, Cc, 0, None, 0, S()), "fuse bwd")
    torch.cuda.synchronize()
    within("fuse dx past 8192 workgroups", dx, want, U[F32] * want.abs() + ACC * want.abs())


def resample_ref(x, mode):
    return x * 1.0 if mode == 0 else (F.interpolate(x, scale_factor=2, mode="nearest") if mode == 3 else F.max_pool2d(x, 2))


RESAMPLE_CASES = [(N, H, W, Cc, mode) for (N, H, W, Cc), modes in (((1, 2, 2, 8), (0, 3, 4)), ((1, 5, 7, 24), (0, 4)), ((3, 6, 10, 8), (0, 3, 4)),
                                                                   ((2, 96, 88, 256), (4,)))    # 2 162 688 input items: past 8192 workgroups
                  for mode in modes]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", RESAMPLE_CASES, ids=lambda s: "x".join(map(str, s[:4])) + f"-mode{s[4]}")
def test_resample_backward_paths(dtype, shape):
    """B2.  Identity, nearest x2 (sum of the 2 x 2 block of dy: terms = that sum of |dy|) and 2 x 2 max pooling (dy to the first maximum
    in row-major order; the pooled input carries the tie patterns of test_resample_backward_of_the_src_model_py_neck wherever it is large
    enough, and in bf16 random data ties on its own)."""
    N, H, W, Cc, mode = shape
    lib = L.load()
    g = torch.Generator().manual_seed(10 + mode + H)
    hi, wi = {0: (H, W), 3: (H // 2, W // 2), 4: (2 * H, 2 * W)}[mode]
    x = rnd(torch.randn(N, Cc, hi, wi, generator=g), dtype)
    if mode == 4:
        x[:, :, 0:2, 0:2] = 0.5                           # a constant window
        if hi >= 6 and wi >= 6:
            x[:, :, 2, 2] = x[:, :, 3, 3] = 9.0           # first and last position tie
            x[:, :, 4, 5] = x[:, :, 5, 4] = 9.0           # second and third position tie
    x = x.double().requires_grad_()
    dy = rnd(torch.randn(N, Cc, H, W, generator=g), dtype).double()
    r = resample_ref(x, mode)
    (want0,) = torch.autograd.grad(r, x, dy, retain_graph=True)
    (terms,) = torch.autograd.grad(r, x, dy.abs())
    dyd, xd = nhwc(dy, dtype), nhwc(x.detach(), dtype)
    for accumulate in (0, 1):
        prev = rnd(torch.randn(N, hi, wi, Cc, generator=g), dtype)
        dx = prev.clone().to(DEV, dtype)
        L.check(lib.mtbt_resample_backward(dyd.data_ptr(), xd.data_ptr(), mode, dx.data_ptr(), accumulate, N, H, W, Cc, CODE[dtype], S()), "resample bwd")
        torch.cuda.synchronize()
        want = want0 + accumulate * prev.double().permute(0, 3, 1, 2)
        within(f"resample {shape} {dtype} accumulate {accumulate}", back(dx), want, U[dtype] * want.abs() + ACC * terms)


def test_max_pool_backward_nan_windows():
    """B2.  A window with one NaN and a window with two: the pooled value is NaN either way; which POSITION receives the gradient is
    compared with CPU torch (dy is finite, so the gradients are)."""
    lib = L.load()
    g = torch.Generator().manual_seed(77)
    N, Cc, H, W = 1, 8, 3, 4
    x = torch.randn(N, Cc, 2 * H, 2 * W, generator=g)
    nan = float("nan")
    x[:, :, 0, 1] = nan                                   # one NaN, second position
    x[:, 0::2, 2, 2] = nan; x[:, 0::2, 3, 3] = nan        # two NaNs: first and last position
    x[:, 1::2, 2, 3] = nan; x[:, 1::2, 3, 2] = nan        # two NaNs: second and third position
    x[:, :, 4, 6] = nan; x[:, :, 4, 7] = 50.0             # a NaN in front of a larger finite value
    xr = x.double().requires_grad_()
    dy = torch.rand(N, Cc, H, W, generator=g) + 0.5
    F.max_pool2d(xr, 2).backward(dy.double())
    want = xr.grad
    dx = torch.full((N, 2 * H, 2 * W, Cc), SENTINEL, device=DEV)
    dyd, xd = nhwc(dy), nhwc(x)
    L.check(lib.mtbt_resample_backward(dyd.data_ptr(), xd.data_ptr(), 4, dx.data_ptr(), 0, N, H, W, Cc, 0, S()), "resample bwd")
    torch.cuda.synchronize()
    got = back(dx)
    print("positions that receive a gradient, per window row-major, kernel vs torch:", (got != 0).sum().item(), (want != 0).sum().item())
    assert torch.equal(got != 0, want != 0), "the gradient goes to the window position torch chooses"
    within("max pooling with NaN windows", got, want, U[F32] * want.abs())


PROJ_SHAPES = [(12, 12, 50, 49), (12, 10, 13, 11), (8, 8, 9, 9), (7, 5, 20, 23), (12, 12, 12, 12), (1, 1, 5, 5), (12, 12, 48, 48)]


def projector_case(N, nm, hp, wp, Ho, Wo, seed):
    """float64 autograd through F.interpolate(conv1x1(protos), size=(Ho, Wo), mode="bilinear", align_corners=False) from fp32 inputs."""
    g = torch.Generator().manual_seed(seed)
    protos = torch.randn(N, nm, hp, wp, generator=g)
    w = torch.randn(nm, generator=g) * 0.3
    dseg = torch.randn(N, 1, Ho, Wo, generator=g)
    pr, wr, br = protos.double().requires_grad_(), w.double().requires_grad_(), torch.zeros(1, dtype=torch.float64, requires_grad=True)
    low = (pr * wr.view(1, nm, 1, 1)).sum(1, keepdim=True) + br
    low.retain_grad()
    up = F.interpolate(low, size=(Ho, Wo), mode="bilinear", align_corners=False)
    up.backward(dseg.double(), retain_graph=True)
    (t_low,) = torch.autograd.grad(up, low, dseg.double().abs())                 # bilinear^T(|dseg|) >= |d_low|
    ref = dict(dp=pr.grad, dw=wr.grad, db=br.grad, dlow=low.grad,
               t_dp=wr.detach().abs().view(1, nm, 1, 1) * t_low, t_dw=2 * (t_low * pr.detach().abs()).sum((0, 2, 3)), t_db=t_low.sum().view(1))
    return protos, w, dseg, ref


def run_projector(lib, protos, w, dseg, dtype, acc_dp, acc_dw, prev_dp, prev_dw, prev_db, with_dw=True):
    N, nm, hp, wp = protos.shape
    Ho, Wo = dseg.shape[2:]
    nb = lib.mtbt_projector_backward_workspace_bytes(N, hp, wp, nm)
    ws = torch.empty(nb // 4, device=DEV)
    dp = prev_dp.clone().to(DEV, dtype)
    dw, db = prev_dw.clone().to(DEV), prev_db.clone().to(DEV)
    pd, wd = nhwc(protos), w.to(DEV).contiguous()
    dsd = dseg.view(N, Ho, Wo).to(DEV).contiguous()
    L.check(lib.mtbt_projector_backward(dsd.data_ptr(), pd.data_ptr(), wd.data_ptr(), dp.data_ptr(), CODE[dtype], acc_dp, dw.data_ptr() if with_dw else None,
                                        db.data_ptr() if with_dw else None, acc_dw, N, hp, wp, nm, Ho, Wo, ws.data_ptr(), nb, S()), "projector bwd")
    torch.cuda.synchronize()
    return dp, dw, db


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("N,nm", [(1, 8), (3, 32), (1, 248), (3, 248)])     # 144 and 432 rows at 12 x 12: one workgroup and two; nm 248 = the documented maximum
@pytest.mark.parametrize("shape", PROJ_SHAPES, ids=lambda s: "x".join(map(str, s[:2])) + "to" + "x".join(map(str, s[2:])))
def test_projector_backward_any_ratio(shape, N, nm, dtype):
    """B3.  The resize ratio need not be an integer: 12 -> 50 / 49 / 13, 8 -> 9 (the gather window once drifted above its lower edge for the
    later rows and dropped contributions), 7 -> 20, 5 -> 23, 12 -> 12, 1 -> 5 (both taps clamp everywhere) and the trainer's 12 -> 48.
    Terms: d_low = bilinear^T(dseg), bounded through bilinear^T(|dseg|) (the weights are >= 0); d protos = w (x) d_low; d w = <d_low, protos>
    carries d_low's own bound and the second sum; d b = sum d_low."""
    hp, wp, Ho, Wo = shape
    lib = L.load()
    protos, w, dseg, ref = projector_case(N, nm, hp, wp, Ho, Wo, seed=hp * 1000 + Ho * 10 + N)
    g = torch.Generator().manual_seed(3)
    prev_dp, prev_dw, prev_db = rnd(torch.randn(N, hp, wp, nm, generator=g), dtype), torch.randn(nm, generator=g), torch.randn(1, generator=g)
    tag = f"projector {hp}x{wp} -> {Ho}x{Wo} N {N} nm {nm} {dtype}"
    for acc_dp, acc_dw in ((0, 0), (1, 1), (0, 1), (1, 0)):
        dp, dw, db = run_projector(lib, protos, w, dseg, dtype, acc_dp, acc_dw, prev_dp, prev_dw, prev_db)
        want = ref["dp"] + acc_dp * prev_dp.double().permute(0, 3, 1, 2)
        within(f"{tag} d protos accumulate {acc_dp}", back(dp), want, U[dtype] * want.abs() + ACC * ref["t_dp"])
        want = ref["dw"] + acc_dw * prev_dw.double()
        within(f"{tag} dw accumulate {acc_dw}", dw, want, U[F32] * want.abs() + ACC * ref["t_dw"])
        want = ref["db"] + acc_dw * prev_db.double()
        within(f"{tag} db accumulate {acc_dw}", db, want, U[F32] * want.abs() + ACC * ref["t_db"])
    dp, dw, db = run_projector(lib, protos, w, dseg, dtype, 0, 0, prev_dp, prev_dw, prev_db, with_dw=False)
    within(f"{tag} d protos, dw NULL", back(dp), ref["dp"], U[dtype] * ref["dp"].abs() + ACC * ref["t_dp"])
    assert torch.equal(dw.cpu(), prev_dw) and torch.equal(db.cpu(), prev_db)


def test_projector_backward_4x_is_deterministic():
    """B3.  The 12 -> 48 case the trainer uses, fp32, twice: bit-identical (a wider gather window only adds zero-weight terms, which are
    skipped; the non-zero terms are visited in the same order)."""
    lib = L.load()
    protos, w, dseg, _ = projector_case(2, 32, 12, 12, 48, 48, seed=1)
    z = (torch.zeros(2, 12, 12, 32), torch.zeros(32), torch.zeros(1))
    a = run_projector(lib, protos, w, dseg, F32, 0, 0, *z)
    b = run_projector(lib, protos, w, dseg, F32, 0, 0, *z)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ----------------------------------------------------------------------------------------------------------------------------------
# C. BatchNorm forward + backward where the paths switch
# ----------------------------------------------------------------------------------------------------------------------------------
BN_CASES = [
    # (C, P, act, use_running)
    (8, 1, "silu", 0),         # one pixel: the `pixels > 1` branch of the unbiased variance; variance 0, xhat 0
    (24, 255, "elu", 0),       # C / 8 = 3: the general (!fixed) kernels; one ragged workgroup
    (24, 255, "silu", 1),      # the same on running statistics (nothing updated, dx = gamma * rstd * du)
    (64, 256, "none", 0),      # exactly one workgroup of rows
    (96, 257, "gelu", 0),      # C / 8 = 12, !fixed, and one row into a second workgroup; GELU is dispatched at run time
    (64, 600, "silu", 0),      # P * C / 8 = 4800 >= 4096: the four-rows-in-flight trip of the fixed apply passes runs (5 workgroups, 3 * 1280 < 4800)
    (8, 5000, "gelu", 0),      # the same trip with one chunk per pixel and the run-time activation on the fixed path
    (96, 44000, "elu", 0),     # general path: 528 000 pieces, past the backward apply pass's 2048 workgroups of 256
    (2048, 300, "silu", 0),    # the channel cap: 256 pieces per pixel = one row group per workgroup; a full workgroup of rows and a ragged one of 44
]
BN_CASES_BF16_ONLY = [
    (512, 33000, "none", 0),   # fixed path: 2 112 000 pieces, past 2048 workgroups of 1024 pieces (forward and backward apply)
]


def run_bn_case(dtype, Cc, P, act, running):
    lib = L.load()
    g = torch.Generator().manual_seed(Cc * 7 + P)
    eps, mom, LD, OFF = 1e-3, 0.03, Cc + 24, 8
    x = rnd(torch.randn(P, Cc, generator=g) * 1.5 + 0.2, dtype).double()
    dy = rnd(torch.randn(P, Cc, generator=g), dtype).double()
    gamma, beta = (torch.rand(Cc, generator=g) + 0.5).float().double(), (torch.randn(Cc, generator=g) * 0.2).float().double()
    rm0, rv0 = (torch.randn(Cc, generator=g) * 0.1 + 0.2).float().double(), (torch.rand(Cc, generator=g) + 1.5).float().double()
    if running:
        r = bn_reference(x, dy, gamma, beta, eps, act, rm0, rv0)
        t_mean, t_var = 0.0, 0.0
    else:
        r = bn_reference(x, dy, gamma, beta, eps, act)
        t_mean, t_var = stat_terms(x)
    t = bn_terms(r, x, dy, gamma, beta, bool(running), t_mean, t_var)
    tag = f"bn C {Cc} P {P} {act} {'running' if running else 'batch'} {dtype}"
    # forward into a channel slice
    xd = x.to(DEV, dtype)
    sentinel = float(torch.tensor(SENTINEL).to(dtype))
    ycat = torch.full((P, LD), sentinel, dtype=dtype, device=DEV)
    stats = torch.zeros(2 * Cc, device=DEV)
    rm, rv = rm0.float().to(DEV), rv0.float().to(DEV)
    gd, bd = gamma.float().to(DEV), beta.float().to(DEV)
    nb = lib.mtbt_bn_train_workspace_bytes(P, Cc)
    ws = torch.empty(nb // 4 + 16, device=DEV)
    L.check(lib.mtbt_bn_forward_nhwc(xd.data_ptr(), ycat.view(-1)[OFF:].data_ptr(), LD, gd.data_ptr(), bd.data_ptr(), rm.data_ptr(), rv.data_ptr(), C.c_float(mom),
                                     C.c_float(eps), ACTS[act][0], P, Cc, CODE[dtype], running, stats.data_ptr(), ws.data_ptr(), nb, S()), "bn_forward")
    torch.cuda.synchronize()
    b_mean, b_var = U[F32] * r["mean"].abs() + ACC * t_mean, U[F32] * r["var"].abs() + ACC * t_var
    within(f"{tag} mean", stats[:Cc], r["mean"], b_mean)
    within(f"{tag} var", stats[Cc:], r["var"], b_var)
    if running:
        assert torch.equal(rm.cpu(), rm0.float()) and torch.equal(rv.cpu(), rv0.float()), "running statistics are not updated in eval mode"
    else:
        want, bound = running_update(rm0, r["mean"], mom, b_mean)
        within(f"{tag} running_mean", rm, want, bound)
        want, bound = running_update(rv0, r["var"], mom, b_var, P / (P - 1.0) if P > 1 else 1.0)
        within(f"{tag} running_var", rv, want, bound)
    within(f"{tag} y", ycat[:, OFF:OFF + Cc], r["y"], U[dtype] * r["y"].abs() + ACC * t["y"])
    yc = ycat.cpu().float()
    assert bool((yc[:, :OFF] == sentinel).all()) and bool((yc[:, OFF + Cc:] == sentinel).all()), "the channels outside the slice are not the kernel's"
    # backward from a channel slice, with the statistics the forward stored
    dcat = torch.zeros(P, LD, dtype=dtype, device=DEV)
    dcat[:, OFF:OFF + Cc] = dy.to(DEV, dtype)
    dx = torch.empty(P, Cc, dtype=dtype, device=DEV)
    dg, db = torch.empty(Cc, device=DEV), torch.empty(Cc, device=DEV)
    nb2 = lib.mtbt_bn_backward_workspace_bytes(P, Cc)
    ws2 = torch.empty(nb2 // 4, device=DEV)
    L.check(lib.mtbt_bn_backward_nhwc(dcat.view(-1)[OFF:].data_ptr(), LD, xd.data_ptr(), stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), C.c_float(eps), ACTS[act][0],
                                      running, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, P, Cc, CODE[dtype], ws2.data_ptr(), nb2, S()), "bn_backward")
    torch.cuda.synchronize()
    within(f"{tag} dx", dx, r["dx"], U[dtype] * r["dx"].abs() + ACC * t["dx"])
    within(f"{tag} dgamma", dg, r["dgamma"], U[F32] * r["dgamma"].abs() + ACC * t["dgamma"])
    within(f"{tag} dbeta", db, r["dbeta"], U[F32] * r["dbeta"].abs() + ACC * t["dbeta"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: f"C{c[0]}-P{c[1]}-{c[2]}-{'running' if c[3] else 'batch'}")
def test_bn_forward_backward_paths(dtype, case):
    """C.  mtbt_bn_forward_nhwc (into a channel slice) then mtbt_bn_backward_nhwc (from one) against the float64 BatchNorm + activation;
    the per-case comments of BN_CASES name the path each one is there for.  The statistics' terms follow the kernel's documented
    algorithm (stat_terms); they enter y, dx, d gamma and d beta through xhat (bn_terms)."""
    run_bn_case(dtype, *case)


@pytest.mark.parametrize("case", BN_CASES_BF16_ONLY, ids=lambda c: f"C{c[0]}-P{c[1]}-{c[2]}")
def test_bn_forward_backward_past_the_fixed_grid_cap(case):
    run_bn_case(BF16, *case)


def test_bn_reference_is_batchnorm2d():
    """The explicit float64 reference of this module is torch's BatchNorm2d in train mode followed by the activation."""
    g = torch.Generator().manual_seed(1)
    P, Cc = 37, 24
    x, dy = torch.randn(P, Cc, generator=g, dtype=torch.float64), torch.randn(P, Cc, generator=g, dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(Cc, eps=1e-3).double()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.2)
    xi = x.t().reshape(1, Cc, P, 1).clone().requires_grad_()
    F.silu(bn(xi)).backward(dy.t().reshape(1, Cc, P, 1))
    r = bn_reference(x, dy, bn.weight.detach(), bn.bias.detach(), 1e-3, "silu")
    assert (r["dx"] - xi.grad.view(Cc, P).t()).abs().max().item() < 1e-12
    assert (r["dgamma"] - bn.weight.grad).abs().max().item() < 1e-11 and (r["dbeta"] - bn.bias.grad).abs().max().item() < 1e-11


# ----------------------------------------------------------------------------------------------------------------------------------
# D. mtbt_gap_fc_backward, mtbt_channel_sum, mtbt_sumsq, mtbt_add_nhwc
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("HW", [1, 20, 400])
@pytest.mark.parametrize("Cc,nout", [(8, 1), (96, 5), (256, 2), (2048, 5), (8, 5), (2048, 1)])
def test_gap_fc_backward_shapes(Cc, nout, HW, dtype):
    """D.  The row-group count G = threads / (C / 8) of the pooling workgroup: 256 at C = 8, 21 at C = 96 (252 of 256 threads work), 8 at
    C = 256, 1 at C = 2048; HW = 1 and 20 leave most row groups without a pixel.  Reference: float64 Linear(mean(x)).  Terms: pool = mean |x|;
    dx = sum_j |dl W| / HW; dW = sum_n |dl| * mean |x|; db = sum_n |dl|."""
    lib = L.load()
    g = torch.Generator().manual_seed(Cc + HW + nout)
    N = 3
    x = rnd(torch.randn(N, HW, Cc, generator=g), dtype).double()
    Wt, dl = torch.randn(nout, Cc, generator=g).double() * 0.1, torch.randn(N, nout, generator=g).double()
    xl, wl, bl = x.clone().requires_grad_(), Wt.clone().requires_grad_(), torch.zeros(nout, dtype=torch.float64, requires_grad=True)
    F.linear(xl.mean(1), wl, bl).backward(dl)
    pool_abs = x.abs().mean(1)
    t_dx = ((dl.abs() @ Wt.abs()) / HW)[:, None, :].expand(N, HW, Cc)
    t_dw = dl.abs().t() @ pool_abs
    xd, dld, wd = x.to(DEV, dtype), dl.float().to(DEV), Wt.float().to(DEV).contiguous()
    prev = rnd(torch.randn(N, HW, Cc, generator=g) * 0.01, dtype)
    prev_w, prev_b = torch.randn(nout, Cc, generator=g), torch.randn(nout, generator=g)
    tag = f"gap_fc C {Cc} HW {HW} nout {nout} {dtype}"
    for acc_dx, acc_dw in ((0, 0), (1, 1)):
        dx = prev.clone().to(DEV, dtype)
        dw, db = prev_w.clone().to(DEV), prev_b.clone().to(DEV)
        pool = torch.full((N, Cc), SENTINEL, device=DEV)
        L.check(lib.mtbt_gap_fc_backward(xd.data_ptr(), dld.data_ptr(), wd.data_ptr(), dx.data_ptr(), acc_dx, dw.data_ptr(), db.data_ptr(), acc_dw, pool.data_ptr(),
                                         N, HW, Cc, nout, CODE[dtype], S()), "gap_fc bwd")
        torch.cuda.synchronize()
        want = x.mean(1)
        within(f"{tag} pool", pool, want, U[F32] * want.abs() + ACC * pool_abs)
        want = xl.grad + acc_dx * prev.double()
        within(f"{tag} dx accumulate {acc_dx}", dx, want, U[dtype] * want.abs() + ACC * t_dx)
        want = wl.grad + acc_dw * prev_w.double()
        within(f"{tag} dw accumulate {acc_dw}", dw, want, U[F32] * want.abs() + 2 * ACC * t_dw)
        want = bl.grad + acc_dw * prev_b.double()
        within(f"{tag} db accumulate {acc_dw}", db, want, U[F32] * want.abs() + ACC * dl.abs().sum(0))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("second", [0, 1], ids=["sum", "product"])
def test_channel_sum_wider_than_a_workgroup(second, dtype):
    """D.  mtbt_channel_sum at C = 2056: 257 pieces per pixel, more than the 256 threads of a workgroup, so rows_reduce (csrc/rowreduce.h)
    gives every thread whole columns of pieces, serial over the rows (thread 0 takes pieces 0 and 256); P = 300 = a full workgroup of rows
    and a ragged one of 44.  Both operands are read from rows wider than C (different pitches), with and without the second operand,
    accumulate 0 and 1.  Terms: the |x| (or |x * x2|) of the column.  A second call gives the same bits."""
    lib = L.load()
    Cc, P, LD, LD2, OFF = 2056, 300, 2056 + 24, 2056 + 8, 8
    g = torch.Generator().manual_seed(2056 + second)
    a, b = rnd(torch.randn(P, LD, generator=g), dtype), rnd(torch.randn(P, LD2, generator=g) + 0.5, dtype)
    prev = torch.randn(Cc, generator=g)
    terms = a[:, OFF:OFF + Cc].double() * (b[:, :Cc].double() if second else 1.0)
    ad, bd = a.to(DEV, dtype), b.to(DEV, dtype)
    nb = lib.mtbt_channel_sum_workspace_bytes(P, Cc)
    ws = torch.empty(nb // 4, device=DEV)
    es = ad.element_size()
    for accumulate in (0, 1):
        outs = []
        for _ in range(2):
            out = prev.clone().to(DEV)
            L.check(lib.mtbt_channel_sum(ad.data_ptr() + OFF * es, bd.data_ptr() if second else None, P, Cc, LD, LD2, CODE[dtype], out.data_ptr(), accumulate,
                                         ws.data_ptr(), nb, S()), "channel_sum")
            torch.cuda.synchronize()
            outs.append(out)
        want = terms.sum(0) + accumulate * prev.double()
        within(f"channel_sum C {Cc} P {P} second {second} accumulate {accumulate} {dtype}", outs[0], want, U[F32] * want.abs() + ACC * terms.abs().sum(0))
        assert torch.equal(outs[0], outs[1]), "a second call gives other bits"


@pytest.mark.parametrize("n", [0, 1, 4095, 4097, 1024 * 4096 + 5])
def test_sumsq_sizes(n):
    """D.  One workgroup per 4096 elements, at most 1024: the last size is 5 elements past the cap (1024 workgroups, every thread takes 16
    trips of the grid-stride loop and five threads a 17th).  All terms are positive: sum|terms| = the sum."""
    lib = L.load()
    g = torch.Generator().manual_seed(n + 1)
    v = torch.randn(max(n, 1), generator=g)
    want0 = (v[:n].double() ** 2).sum()
    vd = v.to(DEV)
    nb = lib.mtbt_sumsq_workspace_bytes()
    ws = torch.empty(nb // 4, device=DEV)
    for accumulate, preset in ((0, 3.5), (1, 3.5)):
        out = torch.tensor([preset], device=DEV)
        L.check(lib.mtbt_sumsq(vd.data_ptr(), n, out.data_ptr(), accumulate, ws.data_ptr(), nb, S()), "sumsq")
        torch.cuda.synchronize()
        want = want0 + accumulate * preset
        within(f"sumsq n {n} accumulate {accumulate}", out, want.view(1), (U[F32] * want.abs() + ACC * want0).view(1))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("Cc", [8, 96])
def test_add_nhwc_slices(dtype, Cc):
    """D.  dst += src where both sides are channel slices of wider buffers with spare pixels between the images (pixel stride > C, batch
    stride != pixels * stride); one fp32 addition and one output rounding; everything outside the slice keeps its bits."""
    lib = L.load()
    g = torch.Generator().manual_seed(Cc)
    N, P = 3, 301
    LDd, OFFd, PADd = Cc + 16, 8, 5
    LDs, OFFs, PADs = Cc + 8, 0, 2
    dst0 = rnd(torch.randn(N, P + PADd, LDd, generator=g), dtype)
    src = rnd(torch.randn(N, P + PADs, LDs, generator=g), dtype)
    dst = dst0.clone().to(DEV, dtype)
    sd = src.to(DEV, dtype)
    es = dst.element_size()
    L.check(lib.mtbt_add_nhwc(dst.data_ptr() + OFFd * es, (P + PADd) * LDd, LDd, sd.data_ptr() + OFFs * es, (P + PADs) * LDs, LDs, N, P, Cc, CODE[dtype], S()), "add")
    torch.cuda.synchronize()
    got = dst.cpu().float()
    want = dst0[:, :P, OFFd:OFFd + Cc].double() + src[:, :P, OFFs:OFFs + Cc].double()
    within(f"add_nhwc C {Cc} {dtype}", got[:, :P, OFFd:OFFd + Cc], want, U[dtype] * want.abs())
    rest = got.clone()
    rest[:, :P, OFFd:OFFd + Cc] = dst0[:, :P, OFFd:OFFd + Cc]
    assert torch.equal(rest, dst0), "channels and pixels outside the slice are untouched"
    # refusals (no launch): C or a stride that is no multiple of 8, a NULL side, an empty batch; a pointer that is not 16-byte aligned
    a = (dst.data_ptr(), (P + PADd) * LDd, LDd, sd.data_ptr(), (P + PADs) * LDs, LDs, N, P, Cc, CODE[dtype], S())
    for i, bad in ((8, Cc + 4), (2, LDd + 4), (5, LDs + 4), (1, (P + PADd) * LDd + 4), (3, None), (0, None), (6, 0), (7, 0), (9, 7)):
        b = list(a)
        b[i] = bad
        assert lib.mtbt_add_nhwc(*b) == -1, f"argument {i} = {bad}: MTBT_EINVAL"
    b = list(a); b[0] = dst.data_ptr() + es
    assert lib.mtbt_add_nhwc(*b) == -2, "misaligned dst: MTBT_EALIGN"
    b = list(a); b[3] = sd.data_ptr() + es
    assert lib.mtbt_add_nhwc(*b) == -2, "misaligned src: MTBT_EALIGN"
    assert torch.equal(dst.cpu().float(), got), "a refused call changes nothing"
