"""float64 / numpy restatement of `oeh_act_quant` (include/oeh.h) and of the fused feed-forward's index rules, for tests/test_act_quant_*.py and
tests/test_ffn_modules_gpu.py.  No GPU, no torch kernels: numpy and math.erf only.

Two kinds of statement:
  exact   - the quantiser in IEEE fp32 as the kernels compute it (`fq_index32`: a true fp32 division, rint, clamp), for identities that hold
            index for index;
  interval - an activation evaluated in float64 with a bound delta on what the fp32 evaluation may differ by, both ends rounded to the
            storage type and quantised: the kernel's index must lie in [idx_lo, idx_hi].  An element is "ambiguous" when idx_lo != idx_hi;
            the tests assert, from these numbers alone, that few elements are, so that no rounding boundary is judged by luck."""
import math

import numpy as np

K_ERF = 16.0  # ulp bound of erf in fp32: the OpenCL conformance bound (the device library's erff is held to it)
_erf = np.vectorize(math.erf, otypes=[np.float64])


def fq_index32(v, scale, zp, qmax=255.0):
    """clamp(rint(v / scale) + zp, 0, qmax) in IEEE fp32 - uniform_quantizers.py:114-115 on fp32 tensors."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint(v / np.float32(scale)) + np.float32(zp)
    return np.clip(q, np.float32(0.0), np.float32(qmax))


def dequant32(idx, scale, zp):
    return (np.float32(scale) * (np.asarray(idx, dtype=np.float32) - np.float32(zp))).astype(np.float32)


def relu(v):
    return np.maximum(v, 0)


def gelu64(v):
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * v * (1.0 + _erf(v / math.sqrt(2.0)))


def gelu_delta(v, a):
    """What fp32 0.5 v (1 + erf(v / sqrt 2)) may differ from the float64 value `a` by: the roundings of v / sqrt 2 (through erf's slope, at
    most one more ulp of erf's result scale), erff (K_ERF ulp of a result <= 1), 1 + ., and the two products:
    (0.5 (K_ERF + 4) |v| + 2 |a|) 2^-24."""
    return (0.5 * (K_ERF + 4.0) * np.abs(np.asarray(v, dtype=np.float64)) + 2.0 * np.abs(a)) * 2.0 ** -24


def round_to(x, dtype: str):
    """float64 -> the storage type's values (as float64), round to nearest even; a 16-bit type through fp32, as the kernel rounds its fp32
    result (RN16 o RN32 is monotone, so interval ends stay ends)."""
    x32 = np.asarray(x, dtype=np.float64).astype(np.float32)
    if dtype == "f32":
        return x32.astype(np.float64)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).astype(np.float64)
    if dtype == "bf16":
        b = x32.view(np.uint32).astype(np.uint64)
        r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
        out = r.astype(np.uint32).view(np.float32).astype(np.float64)
        return np.where(np.isfinite(x32), out, x32.astype(np.float64))
    raise ValueError(dtype)


def index_interval(lo, hi, scale, zp, qmax=255.0, slack=2.0 ** -22):
    """[idx_lo, idx_hi] of values known to lie in [lo, hi]: the quotient by fl32(scale) with a relative slack (the fp32 quotient is correctly
    rounded: 2^-24; the rest is margin), rint, + zp, clamp."""
    s = float(np.float32(scale))
    qlo, qhi = np.asarray(lo, dtype=np.float64) / s, np.asarray(hi, dtype=np.float64) / s
    qlo, qhi = qlo - np.abs(qlo) * slack, qhi + np.abs(qhi) * slack
    return np.clip(np.rint(qlo) + zp, 0.0, qmax), np.clip(np.rint(qhi) + zp, 0.0, qmax)


def gelu_index_interval(v, scale, zp, dtype: str):
    """The index interval of fq(RN_dtype(gelu(v))) for the kernel's fp32 evaluation: (idx_lo, idx_hi, a = gelu64(v))."""
    a = gelu64(v)
    d = gelu_delta(v, a)
    lo, hi = index_interval(round_to(a - d, dtype), round_to(a + d, dtype), scale, zp)
    return lo, hi, a


def percentile_grid(a, lo_q=0.001, hi_q=99.999):
    """(delta, zero_float) of the asymmetric 8-bit grid over the percentile range of `a`, x_min clamped to <= 0 as `_tensorize_min_max` does."""
    lo, hi = np.percentile(np.asarray(a, dtype=np.float64), [lo_q, hi_q])
    lo, hi = min(float(lo), 0.0), max(float(hi), 1e-8)
    delta = (hi - lo) / 255.0
    return delta, -lo / delta + 0.0  # (+ 0: no -0 for lo == 0)


# ---- the fused feed-forward: an accumulator known to float64, the index interval its fp32-grade evaluations may fall in -----------------
def linear64(x, w, b):
    """(x W^T + b in float64, the rows' scale sum_k |x_k| |w_k| + |b|: the unit of a GEMM's accumulation error)."""
    x, w, b = (np.asarray(t, dtype=np.float64) for t in (x, w, b))
    return x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)


def ffn_index_interval(acc, row_scale, act: str, scale, zp, rel=1e-6):
    """The interval of a QuantLinear's output index when its fp32-grade accumulator lies within rel * row_scale of `acc` (the documented
    bound of oeh_proj_quant_i8, include/oeh.h) and the activation is evaluated in fp32 behind it."""
    t = rel * row_scale
    if act == "relu":
        lo, hi = relu(acc - t), relu(acc + t)
    elif act == "gelu":
        g = np.stack([gelu64(acc - t), gelu64(acc), gelu64(acc + t)])  # (not monotone below 0: the ends and the middle; the curvature term t^2 is far below delta)
        d = gelu_delta(np.abs(acc) + t, np.abs(g).max(axis=0))
        lo, hi = g.min(axis=0) - d, g.max(axis=0) + d
    else:
        lo, hi = acc - t, acc + t
    return index_interval(round_to(lo, "f32"), round_to(hi, "f32"), scale, zp)
