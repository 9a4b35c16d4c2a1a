"""float64 restatement of the cross-entropy formulas (include/oeh.h: oeh_xent_fwd / oeh_xent_bwd), the test inputs and the acceptance
rules the cross-entropy tests share.  numpy only; no GPU, no package import."""
import numpy as np

from tests._ln_ref import ulp_of

LOG2E = 1.4426950408889634


def inputs(kind: str, rows: int, V: int, seed: int):
    """(rows, V) float64 logits of one of the four kinds the accuracy bounds were derived on."""
    rng = np.random.default_rng(seed)
    if kind == "n1":
        return rng.standard_normal((rows, V))
    if kind == "n8":
        return 8.0 * rng.standard_normal((rows, V))
    if kind == "t3":  # Student-t(3), clipped so that max - min <= 64
        return np.clip(rng.standard_t(3, (rows, V)), -32.0, 32.0)
    if kind == "spike":  # one logit at +60
        x = rng.standard_normal((rows, V))
        x[np.arange(rows), rng.integers(0, V, rows)] = 60.0
        return x
    raise ValueError(kind)


def forward64(x, y, ignore_index=-100, eps=0.0):
    """x: (rows, V) values AS STORED (any float type), y: (rows,) integers.  Returns float64 (lse, loss, counted, sum_x / V); an ignored row
    has lse = loss = 0 and counted False, a label that is none has NaN and counted True."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    rows, V = x.shape
    m = x.max(axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
        ign = y == ignore_index
        bad = ~ign & ((y < 0) | (y >= V))
        xy = x[np.arange(rows), np.where(ign | bad, 0, y)]
        sxv = x.sum(axis=1) / V
        loss = (1.0 - eps) * (lse - xy) + (eps * (lse - sxv) if eps > 0 else 0.0)
    lse = np.where(ign, 0.0, np.where(bad, np.nan, lse))
    loss = np.where(ign, 0.0, np.where(bad, np.nan, loss))
    return lse, loss, ~ign, sxv


def backward64(x, y, g, ignore_index=-100, eps=0.0):
    """(dlogits64, p64): (softmax - (1 - eps) onehot - eps / V) * g[:, None] per row in float64; zeros for ignored rows, NaN for labels that are none."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    rows, V = x.shape
    lse = forward64(x, np.where((y < 0) | (y >= V), 0, y), ignore_index=-(1 << 62))[0]  # (every row's own lse, whatever its label)
    p = np.exp(x - lse[:, None])
    d = p.copy()
    ok = (y >= 0) & (y < V)
    d[np.arange(rows)[ok], y[ok]] -= 1.0 - eps
    if eps > 0:
        d -= eps / V
    d *= np.asarray(g, dtype=np.float64).reshape(rows, 1)
    ign = y == ignore_index
    d[ign] = 0.0
    d[~ign & ~ok] = np.nan
    return d, p


def lse_bound(lse64):
    """|lse - lse64| <= 4 ulp32(lse64).  Where the 4 comes from: the algorithm's emulation on the host (`emulate_lse32`: 256 lanes,
    sequential fp32 sums, fp32 exp2((x - m) * log2e)) measures at most 1.31 ulp32 on these inputs (tests/test_xent_cpu.py asserts 2, half
    the bound); the hardware exponential is one ulp worse than numpy's and the device logarithm is no better than numpy's, which the other
    half is left to."""
    return 4.0 * ulp_of(lse64, "float32")


def loss_bound(lse64, loss64):
    return lse_bound(lse64) + 0.5 * ulp_of(loss64, "float32")


def smoothing_sum_error(lse32, loss32, x, y, counted, eps):
    """The check of the smoothing term's sum(x) / V, which is no output: the kernel's own fp32 expression
        RN(RN((1 - eps) * RN(lse - x_y)) + RN(eps * RN(lse - RN(S / V))))
    evaluated on the RETURNED fp32 lse, the stored x_y and the float64 row sum S, against the returned fp32 row loss.  Every step is a
    monotone rounding, so an error d of sum(x) / V moves RN(S / V) by at most d + ulp, the second difference b by one ulp32(b) more, the
    product by eps times that plus ulp32(eps * b), the sum by one ulp32(loss) more.  With d = 2^-20 mean|x|, what the kernel is held to:
        tol = eps * (2^-20 mean|x| + ulp32(S / V) + ulp32(b)) + ulp32(eps * b) + ulp32(loss)
    Returns max |loss - expression| / tol over the counted rows (<= 1 passes).  lse32, loss32: the kernel's; x: float64 stored logits."""
    f = np.float32
    x = np.asarray(x, dtype=np.float64)
    rows, V = x.shape
    e32 = f(eps)
    xy = x[np.arange(rows), np.where(counted, np.asarray(y), 0)].astype(f)
    sv = (x.sum(axis=1) / V).astype(f)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (lse32 - xy).astype(f)
        b = (lse32 - sv).astype(f)
        t1 = ((f(1.0) - e32) * a).astype(f)
        t2 = (e32 * b).astype(f)
        want = (t1 + t2).astype(f)
    tol = eps * (2.0 ** -20 * np.abs(x).mean(axis=1) + ulp_of(sv, "float32") + ulp_of(b, "float32")) + ulp_of(t2, "float32") + ulp_of(want, "float32")
    err = np.abs(loss32.astype(np.float64) - want.astype(np.float64)) / tol
    return float(err[counted].max()) if counted.any() else 0.0


def grad_bound(d64, p64, g, dtype_name):
    """|dl - dl64| <= |g| (2^-15 p64 + 2^-24) + ulp_dtype(dl64) / 2: with a = (x - lse) * log2e and |a| <= 92, two fp32 roundings of a give a
    relative error of p below 2^-16; twice that is allowed."""
    g = np.abs(np.asarray(g, dtype=np.float64)).reshape(-1, 1)
    return g * (2.0 ** -15 * p64 + 2.0 ** -24) + 0.5 * ulp_of(d64, dtype_name)


def emulate_lse32(x, lanes=256, slots=4, nv=8):
    """The kernel's forward order on the host in fp32 (an aligned row): thread t takes slots k * lanes + t of every step, rescales once per
    step, the threads merge at the row maximum.  Sums inside a slot and over lanes are sequential fp32 sums (the kernel's trees are no
    worse).  Returns the fp32 lse of one row - what the factor-4 bound was derived from."""
    x = np.asarray(x, dtype=np.float32)
    V = x.shape[0]
    T = lanes * slots * nv
    pad = (-V) % T
    xp = np.concatenate([x, np.full(pad, -np.inf, np.float32)]).reshape(-1, slots, lanes, nv)  # step, k, t, e
    per = xp.transpose(2, 0, 1, 3).reshape(lanes, -1, slots * nv)  # t, step, values
    m = np.full(lanes, -np.inf, np.float32)
    l = np.zeros(lanes, np.float32)
    l2e = np.float32(LOG2E)
    with np.errstate(invalid="ignore", over="ignore"):
        for st in range(per.shape[1]):
            v = per[:, st, :]
            mn = np.maximum(m, v.max(axis=1))
            r = np.where(np.isneginf(mn), np.float32(0), mn)
            e = np.exp2(((v - r[:, None]).astype(np.float32) * l2e).astype(np.float32)).astype(np.float32)
            step = np.zeros(lanes, np.float32)
            for j in range(e.shape[1]):
                step = (step + e[:, j]).astype(np.float32)
            scale = np.exp2(((m - r).astype(np.float32) * l2e).astype(np.float32)).astype(np.float32)
            l = (np.where(np.isneginf(m), np.float32(0), l * scale) + step).astype(np.float32)
            m = mn
        M = m.max()
        r = np.float32(0) if np.isneginf(M) else M
        lt = np.where(np.isneginf(m), np.float32(0), l * np.exp2(((m - r).astype(np.float32) * l2e).astype(np.float32))).astype(np.float32)
        L = np.float32(0)
        for t in range(lanes):
            L = np.float32(L + lt[t])
        return np.float32(M + np.log(L, dtype=np.float32))
