"""The arithmetic of oeh_adamw_step (include/oeh.h) restated twice from the same fp32 inputs: `step32`, fp32 numpy arrays with one numpy
operation per rounding and the constants rounded as the header lists them - what the kernel must give bit for bit - and `step64`, the same
formulas in float64 with double constants - what the bounds of DESIGN.md section 17 are measured against.  No GPU, no torch."""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24  # half an ulp of 1 in fp32: the relative error of one rounding


def fields(lr, beta1, beta2, eps, weight_decay):
    """The descriptor's fp32 fields as Python floats (doubles holding fp32 values): what both evaluations start from."""
    return tuple(float(F32(x)) for x in (lr, beta1, beta2, eps, weight_decay))


def constants64(lr, beta1, beta2, eps, weight_decay, step):
    """decay, 1 - beta1, beta2, 1 - beta2, sqrt(1 - beta2^t), eps, lr / (1 - beta1^t) in double, from the fp32 fields; pow and sqrt are libm's."""
    lr, b1, b2, eps, wd = fields(lr, beta1, beta2, eps, weight_decay)
    t = float(int(step))
    return (1.0 - lr * wd, 1.0 - b1, b2, 1.0 - b2, math.sqrt(1.0 - math.pow(b2, t)), eps, lr / (1.0 - math.pow(b1, t)))


def constants32(*hyper):
    """RN32 of each: the kernel's constants."""
    return tuple(F32(x) for x in constants64(*hyper))


def step32(p, g, m, v, c, hyper):
    """(p', m', v') in fp32; g is the gradient as fp32 (the storage type's values are fp32 numbers), c the fp32 clip coefficient."""
    decay, omb1, b2, omb2, bc2, eps, ss = constants32(*hyper)
    p, g, m, v, c = (np.asarray(a, dtype=F32) for a in (p, g, m, v, c))
    with np.errstate(all="ignore"):
        gc = g * c
        p1 = p * decay
        mn = m + (gc - m) * omb1
        vn = v * b2 + (gc * gc) * omb2
        den = np.sqrt(vn) / bc2 + eps
        pn = p1 - ss * (mn / den)
    assert pn.dtype == F32 and mn.dtype == F32 and vn.dtype == F32
    return pn, mn, vn


def step64(p, g, m, v, c, hyper):
    """The same in float64: (p', m', v', g', den, upd) - the last three are what the bounds are written in."""
    decay, omb1, b2, omb2, bc2, eps, ss = constants64(*hyper)
    p, g, m, v = (np.asarray(a, dtype=F32).astype(np.float64) for a in (p, g, m, v))
    c = float(F32(c))
    with np.errstate(all="ignore"):
        gc = g * c
        mn = m + (gc - m) * omb1
        vn = v * b2 + (gc * gc) * omb2
        den = np.sqrt(vn) / bc2 + eps
        upd = ss * (mn / den)
        pn = p * decay - upd
    return pn, mn, vn, gc, den, upd


def bound_ratios(p, g, m, v, c, hyper, got=None):
    """Worst |fp32 - float64| over its bound for (m', v', p'); `got` = (p', m', v') from somewhere else than step32.
    With S_m = |m| + |g'|, S_v = |v| + g'^2, upd = lr / (1 - beta1^t) * m' / den, u = 2^-24:
    To first order in u, k = 1 - beta1 <= 1, k2 = 1 - beta2:
      m' = m + (g' - m) * k.  g' = RN(g c) is off by u |g'|; the difference inherits that and adds u |g' - m| <= u S_m; the product with RN(k)
        adds 2 u k |g' - m| (the constant's rounding and its own): k (u |g'| + 3 u S_m) <= 4 u k S_m; the sum adds u |m'| <= u S_m: 5 u S_m.
      v' = v b2 + (g' g') k2.  The square carries g' twice and its own rounding (3 u), RN(k2) and the product one each: 5 u k2 g'^2; v b2 (b2 is
        a field: exact) u b2 v; the sum u v': 6 u k2 g'^2 + 2 u b2 v <= 6 u v' <= 6 u S_v.
      p' = p decay - ss (m' / den).  RN(decay) and the product: 2 u |p|.  den = sqrt(v') / bc2 + eps: v' within 6 u v' gives 3 u under the
        root, the root 1, RN(bc2) and the quotient 2, the sum 1: 7 u den.  upd = ss (m' / den): RN(ss), the quotient, the product 3 u, den 7 u:
        10 u |upd|, and m' enters linearly: 5 u S_m ss / den.  The difference adds u |p'| <= u (|p| + |upd|).
        Together u (3 |p| + 11 |upd| + 5 ss S_m / den)."""
    pn, mn, vn = step32(p, g, m, v, c, hyper) if got is None else got
    p64, m64, v64, gc, den, upd = step64(p, g, m, v, c, hyper)
    ss = constants64(*hyper)[6]
    a = lambda x: np.abs(np.asarray(x, dtype=np.float64))  # noqa: E731
    s_m = a(m) + np.abs(gc)
    s_v = a(v) + gc * gc
    bm = 5 * U * s_m
    bv = 6 * U * s_v
    bp = U * (3 * a(p) + 11 * np.abs(upd) + 5 * ss * s_m / den)
    with np.errstate(all="ignore"):
        rm = np.abs(mn.astype(np.float64) - m64) / bm
        rv = np.abs(vn.astype(np.float64) - v64) / bv
        rp = np.abs(pn.astype(np.float64) - p64) / bp
    return float(np.nanmax(rm)), float(np.nanmax(rv)), float(np.nanmax(rp))


def random_state(rng, n, gscale, first=False):
    """p, g, m, v as fp32 with the outlier elements (x40, x-25), a stretch where m is within a few ulp of g (the cancellation in g' - m at
    c = 1) and, unless `first`, a non-zero state.  |g| >= 0.01 gscale: squares times 1 - beta2 stay far above the denormal range."""
    g = rng.standard_normal(n)
    g = (np.sign(g) + (g == 0)) * (np.abs(g) + 0.01) * gscale
    if n > 8:
        g[7 % n] *= 40.0
        g[n - 3] *= -25.0
    g = g.astype(F32)
    p = rng.standard_normal(n).astype(F32)
    if first:
        return p, g, np.zeros(n, F32), np.zeros(n, F32)
    m = (0.3 * gscale * rng.standard_normal(n)).astype(F32)
    k = n // 4
    m[:k] = g[:k] * (1 + rng.integers(-3, 4, k) * 2.0 ** -23).astype(F32)
    v = ((gscale * (0.2 + np.abs(rng.standard_normal(n)))) ** 2).astype(F32)
    return p, g, m, v
