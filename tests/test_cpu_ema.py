"""Weight EMA, resume and warm-up: what can be checked without a GPU.  The symbols exist and refuse bad arguments before any launch, the
decay ramp and the schedule are host arithmetic, and the numpy restatement (tests/ema_reference.py) the GPU tests compare the kernels with
is torch's CPU `e.mul_(d); e.add_((1 - d) * p)` bit for bit -- the rounding order the kernels must follow."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import ema_reference as R
from multitask_bonetumor_yolo_amd import _lib as L
from multitask_bonetumor_yolo_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mtbt_adamw_step_ema", "mtbt_sgd_step_ema", "mtbt_ema_update")
OK, EINVAL, EALIGN = 0, -1, -2
P, ODD = 4096, 4100                 # dummy non-null addresses, 16-byte aligned / not: every call below returns before it would launch


@pytest.fixture(scope="module")
def lib():
    B.build()
    return L.load()


def adamw(lib, *, ema=P, n=8, decay=0.9, param=P, grad=P, m=P, v=P):
    return lib.mtbt_adamw_step_ema(param, grad, m, v, ema, n, 1e-3, 0.9, 0.999, 1e-8, 5e-4, 1, None, decay, None)


def sgd(lib, *, ema=P, n=8, decay=0.9):
    return lib.mtbt_sgd_step_ema(P, P, P, ema, n, 1e-2, 0.9, 0.0, 5e-4, 0, 1, None, decay, None)


def update(lib, *, ema=P, src=P, n=8, decay=0.9):
    return lib.mtbt_ema_update(ema, src, n, decay, None)


def test_symbols_are_declared_bound_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mtbt_hip.h")).read(), flags=re.S)
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/mtbt_hip.h"
        assert name in L.SYMBOLS, f"{name} has no ctypes binding"
        assert hasattr(lib, name), f"{name} is not exported"
        assert f"`{name}`" in table, f"{name} is missing from INTEGRATION.md's symbol table"
    assert C.c_double in L.SYMBOLS["mtbt_ema_update"][1]            # the decay travels in double: it is rounded once, in the library
    assert lib.mtbt_abi_version() == L.ABI_VERSION == 5            # additive: the version stays
    import multitask_bonetumor_yolo_amd as pkg
    from multitask_bonetumor_yolo_amd import checkpoints, trainstep
    assert pkg.ema_decay_at is trainstep.ema_decay_at and pkg.TrainStep is trainstep.TrainStep
    assert pkg.save_train_state is checkpoints.save_train_state and pkg.load_train_state is checkpoints.load_train_state


@pytest.mark.parametrize("call", [adamw, sgd, update])
def test_argument_checks_fire_before_any_launch(lib, call):
    assert call(lib, ema=None) == EINVAL
    assert call(lib, n=-1) == EINVAL
    for bad in (-1e-9, 1.0 + 1e-9, 2.0, float("nan"), float("inf"), -float("inf")):
        assert call(lib, decay=bad) == EINVAL, bad
    for edge in (0.0, 1.0, 0.9999):                                    # the closed interval is accepted; n == 0 launches nothing
        assert call(lib, n=0, decay=edge) == OK, edge
    assert call(lib, n=0, ema=None) == EINVAL                          # a null average is refused whatever n


def test_null_source_and_alignment(lib):
    assert update(lib, src=None) == EINVAL
    assert update(lib, ema=ODD) == EALIGN and update(lib, src=ODD) == EALIGN
    assert update(lib, ema=ODD, n=0) == OK
    # mtbt_adamw_step wants 16-byte aligned buffers, so its EMA form wants them of every buffer including the average ...
    assert lib.mtbt_adamw_step(ODD, P, P, P, 8, 1e-3, 0.9, 0.999, 1e-8, 5e-4, 1, None, None) == EALIGN
    for k in ("param", "grad", "m", "v", "ema"):
        assert adamw(lib, **{k: ODD}) == EALIGN, k
    # ... and what the plain entry points refuse, the EMA forms refuse too (step 0, a null gradient)
    assert lib.mtbt_adamw_step_ema(P, P, P, P, P, 8, 1e-3, 0.9, 0.999, 1e-8, 5e-4, 0, None, 0.9, None) == EINVAL
    assert adamw(lib, grad=None) == EINVAL
    assert lib.mtbt_sgd_step_ema(P, None, P, P, 8, 1e-2, 0.9, 0.0, 5e-4, 0, 1, None, 0.9, None) == EINVAL
    assert lib.mtbt_sgd_step_ema(P, P, None, P, 8, 1e-2, 0.9, 0.0, 5e-4, 0, 1, None, 0.9, None) == EINVAL     # momentum without a buffer


def test_ema_decay_at_hand_values():
    from multitask_bonetumor_yolo_amd.trainstep import ema_decay_at
    assert ema_decay_at(1, 0.9999, 2000.0) == 0.9999 * (1.0 - math.exp(-1.0 / 2000.0))
    assert abs(ema_decay_at(1, 0.9999, 2000.0) - 4.99825e-4) < 1e-8                   # u = 1: almost no memory
    assert abs(ema_decay_at(2000, 0.9999, 2000.0) - 0.9999 * (1.0 - 1.0 / math.e)) < 1e-15    # u = tau: decay * (1 - 1/e) = 0.63205...
    assert abs(ema_decay_at(2000, 0.9999, 2000.0) - 0.632057) < 1e-6
    assert abs(ema_decay_at(2, 0.9, 2.0) - 0.9 * 0.6321205588285577) < 1e-15
    big = ema_decay_at(10 ** 6, 0.9999, 2000.0)
    assert big <= 0.9999 and 0.9999 - big < 1e-15                                      # tends to decay, never above it
    assert [ema_decay_at(u, 0.9999, 2000.0) for u in range(1, 50)] == sorted(ema_decay_at(u, 0.9999, 2000.0) for u in range(1, 50))
    for tau in (0, 0.0, None):
        assert ema_decay_at(1, 0.99, tau) == 0.99 and ema_decay_at(12345, 0.99, tau) == 0.99
    for u in (1, 2, 3, 2000, 10 ** 6):
        assert R.decay_at(u, 0.9999, 2000.0) == ema_decay_at(u, 0.9999, 2000.0)
        assert R.decay_at(u, 0.9, None) == ema_decay_at(u, 0.9, None)


class _Rate:
    """`warmup_cosine_lr` / `cosine_lr` touch nothing but `self.lr`: call them on a bare object, no device needed."""
    lr = 0.0


def _schedule(**kw):
    from multitask_bonetumor_yolo_amd.trainstep import TrainStep
    holder = _Rate()
    holder.cosine_lr = lambda *a, **k: TrainStep.cosine_lr(holder, *a, **k)
    return holder, (lambda it: TrainStep.warmup_cosine_lr(holder, 1e-2, it, **kw))


def test_warmup_cosine_lr_equals_torch_sequential_lr():
    base, warm, total, start = 1e-2, 5, 25, 0.1                      # 5 + 20; torch's LinearLR refuses a start factor of 0
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    lin = torch.optim.lr_scheduler.LinearLR(opt, start_factor=start, end_factor=1.0, total_iters=warm)
    cos = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=total - warm, eta_min=0.01 * base)
    sch = torch.optim.lr_scheduler.SequentialLR(opt, [lin, cos], milestones=[warm])
    holder, at = _schedule(warmup_its=warm, total_its=total, eta_min_ratio=0.01, start_ratio=start)
    for it in range(total + 1):
        want = opt.param_groups[0]["lr"]
        got = at(it)
        assert holder.lr == got                                       # like cosine_lr: sets self.lr and returns it
        assert abs(got - want) < 1e-12, (it, got, want)
        opt.step()
        sch.step()
    assert at(warm) == base and abs(at(total) - 0.01 * base) < 1e-18


def test_warmup_defaults_start_from_zero():
    holder, at = _schedule(warmup_its=4, total_its=10)
    assert [at(i) for i in range(5)] == [0.0, 0.0025, 0.005, 0.0075, 1e-2]
    assert at(7) == 1e-4 + (1e-2 - 1e-4) * (1 + math.cos(math.pi * 3 / 6)) / 2
    holder, at = _schedule(warmup_its=0, total_its=10)               # no warm-up: cosine_lr itself
    assert at(0) == 1e-2 and at(10) == pytest.approx(1e-4, abs=1e-18)


@pytest.mark.parametrize("decay", [0.0, 1.0, 0.5, 0.9, 0.9999, 0.9 * (1.0 - math.exp(-0.5)), 1e-4])
def test_restatement_is_torchs_cpu_mul_add_bit_for_bit(decay):
    g = torch.Generator().manual_seed(int(decay * 1e6) + 3)
    e = torch.randn(20011, generator=g) * torch.rand(20011, generator=g).mul(8).sub(4).exp()      # magnitudes over several binades
    p = torch.randn(20011, generator=g) * torch.rand(20011, generator=g).mul(8).sub(4).exp()
    want = e.clone()
    want.mul_(decay)
    want.add_((1 - decay) * p)
    got = R.ema_update(e.numpy(), p.numpy(), decay)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
    if decay == 0.0:
        assert np.array_equal(got, p.numpy())
    if decay == 1.0:
        assert np.array_equal(got, e.numpy())
    # three updates in a row through `run`, with the ramp
    e3 = e.clone()
    for u, src in enumerate((p, e * 0.5, p + 1), start=1):
        d = R.decay_at(u, 0.9, 2.0)
        e3.mul_(d)
        e3.add_((1 - d) * src)
    got3 = R.run(e.numpy(), [p.numpy(), (e * 0.5).numpy(), (p + 1).numpy()], 0.9, 2.0)
    assert np.array_equal(got3.view(np.uint32), e3.numpy().view(np.uint32))
