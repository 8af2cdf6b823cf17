"""Numpy restatement of the weight EMA (`mtbt_adamw_step_ema` / `mtbt_sgd_step_ema` / `mtbt_ema_update`, include/mtbt_hip.h) and of
its decay ramp (`trainstep.ema_decay_at`).  TEST INFRASTRUCTURE.

The reference project keeps no averaged weights, so this arithmetic is the project's own definition and has no counterpart in oracle/:

    d   = float32(decay)        omd = float32(1.0 - decay)          in double first, each rounded once
    e   = e * d                                                        one float32 rounding
    e   = e + omd * p                                                  the product rounded to float32, then the sum

(numpy float32 arrays round every elementwise operation on its own: there is no fused multiply-add to contract into), and

    decay of update u (from 1) = decay * (1 - exp(-u / tau)),   constant `decay` for tau 0 / None               (Python floats)
"""
import math

import numpy as np


def ema_update(e: np.ndarray, p: np.ndarray, decay: float) -> np.ndarray:
    """The new average of float32 `e` after seeing float32 `p`.  Returns a new array."""
    assert e.dtype == np.float32 and p.dtype == np.float32
    d, omd = np.float32(decay), np.float32(1.0 - float(decay))
    e = e * d
    t = omd * p
    return e + t


def decay_at(u: int, decay: float, tau) -> float:
    if not tau:
        return float(decay)
    return float(decay) * (1.0 - math.exp(-float(u) / float(tau)))


def run(e0: np.ndarray, snapshots, decay: float, tau, first_update: int = 1) -> np.ndarray:
    """The average that starts at `e0` and sees `snapshots` in turn, update numbers first_update, first_update + 1, ..."""
    e = np.array(e0, dtype=np.float32, copy=True)
    for i, p in enumerate(snapshots):
        e = ema_update(e, np.asarray(p, dtype=np.float32), decay_at(first_update + i, decay, tau))
    return e
