"""The arithmetic of oeh_grad_norm_amp's finalize, oeh_adamw_step_amp and oeh_loss_scale_update (include/oeh.h) restated in numpy, one
numpy operation per rounding: what the kernels must give bit for bit.  The element arithmetic is tests/_adamw_ref.py's; what is new is
where bc2 and ss come from (binary exponentiation in double, as the advance launch forms them), the coefficient that carries 1 / scale,
the skip, and the scaler's rule.  No GPU, no torch."""
import math

import numpy as np

from tests import _adamw_ref as R

F32 = np.float32


def pw(beta, t):
    """beta^t as the device forms it: r = 1; base = beta; while n: if n & 1: r *= base; n >>= 1; if n: base *= base.  Python floats are
    IEEE doubles and `*` is one rounding."""
    r, base, n = 1.0, float(beta), int(t)
    while n:
        if n & 1:
            r *= base
        n >>= 1
        if n:
            base *= base
    return r


def pw_many(beta, ts):
    """`pw` over an int64 array of step numbers at once: the same multiplications element by element, the skipped ones masked out."""
    n = np.asarray(ts, dtype=np.int64).copy()
    r, base = np.ones(n.shape, np.float64), np.full(n.shape, float(beta), np.float64)
    while n.any():
        r = np.where(n & 1, r * base, r)
        n >>= 1
        with np.errstate(under="ignore"):
            base = np.where(n != 0, base * base, base)
    return r


def amp_constants(lr, beta1, beta2, t):
    """(bc2, ss) as fp32 for step number t (after the increment) from the descriptor's fp32 fields; zeros when t < 1."""
    if t < 1:
        return F32(0.0), F32(0.0)
    lr, b1, b2 = (float(F32(x)) for x in (lr, beta1, beta2))
    return F32(math.sqrt(1.0 - pw(b2, t))), F32(lr / (1.0 - pw(b1, t)))


def amp_constants_many(lr, beta1, beta2, ts):
    lr, b1, b2 = (float(F32(x)) for x in (lr, beta1, beta2))
    return np.sqrt(1.0 - pw_many(b2, ts)).astype(F32), (lr / (1.0 - pw_many(b1, ts))).astype(F32)


def clip_coef(norm, max_norm):
    """oeh_grad_norm's coefficient in double: 1 for max_norm None, <= 0, NaN or inf."""
    if max_norm is None or not (max_norm > 0.0 and max_norm < math.inf):
        return 1.0
    with np.errstate(all="ignore"):
        c = np.float64(max_norm) / (np.float64(norm) + np.float64(1e-6))
    return float(c) if not c > 1.0 else 1.0


def norm_amp(sumsq, max_norm, s=None, found_in=False):
    """out4 of oeh_grad_norm_amp from the float64 sum of squares of the gradients as stored; s None: no grad_scale."""
    s = 1.0 if s is None else float(F32(s))
    with np.errstate(all="ignore"):
        norm = float(np.sqrt(np.float64(sumsq)) / np.float64(s))
        coef = float(np.float64(clip_coef(norm, max_norm)) / np.float64(s))
    found = (not math.isfinite(sumsq)) or bool(found_in) or not (s > 0.0 and math.isfinite(s))
    return np.array([sumsq, norm, coef, 1.0 if found else 0.0], np.float64)


def step32_amp(p, g, m, v, c, hyper, t):
    """(p', m', v') in fp32 for step number t; hyper = (lr, beta1, beta2, eps, weight_decay); g the gradient as stored, as fp32; c the fp32
    coefficient (clip / scale).  _adamw_ref.step32's operations with bc2 and ss from `amp_constants`."""
    lr, b1, b2, eps, wd = hyper
    decay, omb1, b2c, omb2, _, epsc, _ = R.constants32(lr, b1, b2, eps, wd, 1)
    bc2, ss = amp_constants(lr, b1, b2, t)
    p, g, m, v, c = (np.asarray(a, dtype=F32) for a in (p, g, m, v, c))
    with np.errstate(all="ignore"):
        gc = g * c
        p1 = p * decay
        mn = m + (gc - m) * omb1
        vn = v * b2c + (gc * gc) * omb2
        den = np.sqrt(vn) / bc2 + epsc
        pn = p1 - ss * (mn / den)
    assert pn.dtype == F32 and mn.dtype == F32 and vn.dtype == F32
    return pn, mn, vn


def scaler_update(state, growth_factor, backoff_factor, growth_interval):
    """oeh_loss_scale_update on state = [scale, tracker, found, skipped] (fp32 values): the new state."""
    scale, tracker, found, skipped = (F32(x) for x in state)
    with np.errstate(all="ignore"):
        if found != 0:
            scale, tracker, skipped = scale * F32(backoff_factor), F32(0), skipped + F32(1)
        elif tracker + F32(1) == F32(growth_interval):
            ns = scale * F32(growth_factor)
            scale, tracker = (ns if np.isfinite(ns) else scale), F32(0)
        else:
            tracker = tracker + F32(1)
    return np.array([scale, tracker, 0.0, skipped], F32)
