"""NumPy float64 restatement of oeh_softmax_train_fwd / oeh_softmax_train_bwd (include/oeh.h) with the error bounds the tests use.

The constants of the call are the kernel's: `scale` (or `scale_div`), gamma and eta are fp32 values, the clip width is
w = RN32(eta - gamma) formed in double, inv = RN32(1 / RN32(1 - p)) and the keep threshold is floor(p_f32 * 2^32).  Everything behind them is
float64, so what is left between this file and the kernel is the kernel's own rounding.  u = 2^-24 below (half an fp32 ulp, relative).

Forward bound, counted per rounding of the kernel (none of it fitted to its output):
  z^   = RN(RN(x * s) + mask)                    |z^ - z| <= u * A,  A = |x s| + |z|      (two roundings; the clamp adds none)
  m^   = max z^                                   |m^ - m| <= u * Am, Am = max A over the elements within 1 of the row maximum
  d^   = RN(z^ - m^)                              |d^ - (z - m)| <= u * (A + Am + |z - m|)
  e^   = exp_acc(d^)   (2 ulp = 4 u relative)     e^ = e (1 + theta),  |theta| <= u * T,  T = 4 + |z - m| + A + Am
  den^ = sum e^ [+ exp_acc(-m^)]                  relative error <= u * (sum_k p_k T_k [+ p_0 (4 + Am)] + D),  D = Sk / 32 + 18: the most
                                                  additions any term goes through in any launch form (a lane's own elements, at most
                                                  2 Sk / 64 + 8, then 6 butterfly steps, 3 wave steps and the softmax_1 term)
  p^   = RN(e^ / den^)                            relative error <= u * R,  R = T + sum_k p_k T_k [+ ...] + D + 1
so with c0 = 4 + A + Am + (the row's den term) + D + 1 and c1 = 1 the fp32 error of p is (c0 + c1 |z - m|) u p.  The clip adds two
roundings, |w| u p R + u |p w| + u |t|, and is non-expansive behind them; the store adds half an ulp of y_dtype at |y| + that error.
Each fp32 rounding can also be a subnormal one (an absolute 2^-150 instead of a relative u): TINY = 8 * 2^-149 covers those of e, den, p,
the clip and the backward's products.

Backward bound: p^ carries u R p from above (the backward recomputes the same p), and
  g^   = RN(dy + RN(du * inv)) [* w: one more]    |g^ - g| <= 3 u G,  G = |w| (|dy| + |du inv|)   (+ |w| (|dy| + |du inv|) where the clip's
                                                  gate cannot be decided: t within its forward error of 0 or 1)
  dl^  = sum RN(p^ g^)                            |dl^ - dl| <= sum_k [p_k |g_k| u (R_k + 1 + D) + p_k |g^_k - g_k|]
  dz^  = RN(p^ RN(g^ - dl^))                      |dz^ - dz| <= p (|g| + sum p |g|) u (R + 2) + p (|g^ - g| + |dl^ - dl|)
  dx^  = RN_x(RN(dz^ * gate * s))                 one more fp32 rounding (the gate's 0, 1/2 and 1 are exact), then half an ulp of x_dtype
which is half an ulp of x_dtype plus c u |s| p_j (|g_j| + sum_k p_k |g_k|) with c the counted (data dependent) constant above.
"""
import numpy as np

U = 2.0 ** -24
TINY = 8.0 * 2.0 ** -149
F32_MAX = float(np.finfo(np.float32).max)
_U32 = np.uint64(0xFFFFFFFF)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 as outeffhop_amd/csrc/oeh_philox.h states it: broadcastable counter words, scalar key words -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & _U32 for x in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + np.uint64(W0)) & _U32, (k1 + np.uint64(W1)) & _U32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def keep_mask(B, H, Sq, Sk, p, seed):
    """(B,H,Sq,Sk) bool: the attention dropout stream - counter (j >> 2, i, b * H + h, 0), word j & 3, kept iff word >= floor(p_f32 * 2^32)."""
    if not p > 0:
        return np.ones((B, H, Sq, Sk), dtype=bool)
    nc = (Sk + 3) // 4
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    i = np.arange(Sq, dtype=np.uint64)[None, :, None]
    c = np.arange(nc, dtype=np.uint64)[None, None, :]
    w = philox4x32_10(c, i, bh, 0, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=-1).reshape(B * H, Sq, 4 * nc)[..., :Sk]
    thr = int(np.floor(float(np.float32(p)) * 2.0 ** 32))
    return (words >= np.uint32(thr)).reshape(B, H, Sq, Sk)


def inv_of(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def half_ulp(v, dtype):
    """Half an ulp of the storage type (\"f16\", \"bf16\", \"f32\") at magnitude v (subnormals included)."""
    mant, emin = {"f16": (10, -14), "bf16": (7, -126), "f32": (23, -126)}[dtype]
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** (emin - 1))))
    return 0.5 * 2.0 ** (np.maximum(e, emin) - mant)


class Call:
    """The constants of one call, as the kernel sees them."""

    def __init__(self, base=1, clip=False, gamma=0.0, eta=1.0, scale=1.0, scale_div=0.0, clamp_min=None, p=0.0, seed=0):
        self.base, self.clip = int(base), bool(clip)
        self.gamma = float(np.float32(gamma))
        self.w = float(np.float32(float(np.float32(eta)) - float(np.float32(gamma))))
        self.scale, self.scale_div = float(np.float32(scale)), float(np.float32(scale_div))
        self.clamp_min = None if clamp_min is None else float(np.float32(clamp_min))
        self.p, self.seed = float(p), int(seed)
        self.inv = inv_of(p) if p > 0 else 1.0

    def s(self):
        return 1.0 / self.scale_div if self.scale_div > 0 else self.scale


def forward(c: Call, x, mask=None):
    """x (B,H,Sq,Sk) float64 holding the stored values, mask float64 broadcastable or None.  Returns a dict: z_pre, z, m, den, p, t, y (float64,
    before the store's rounding), R (the relative fp32 error bound of p over u) and y_err (the absolute fp32 error bound of y)."""
    x = np.asarray(x, dtype=np.float64)
    xs = x / c.scale_div if c.scale_div > 0 else x * c.scale
    z_pre = xs + (0.0 if mask is None else np.asarray(mask, dtype=np.float64))
    z = z_pre if c.clamp_min is None else np.maximum(z_pre, c.clamp_min)
    m = z.max(axis=-1, keepdims=True)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        e = np.exp(z - m)
        e0 = np.exp(-m) if c.base == 1 else np.zeros_like(m)
        den = e.sum(axis=-1, keepdims=True) + e0
        dead = ~(den <= F32_MAX)  # fp32 den = inf (or a NaN row): p = 0
        p = np.where(dead, 0.0, e / np.where(dead, 1.0, den))
        p0 = np.where(dead, 0.0, e0 / np.where(dead, 1.0, den))
    A = np.abs(xs) + np.abs(z)
    near = z >= m - 1.0
    Am = np.where(near, A, 0.0).max(axis=-1, keepdims=True)
    d = np.abs(z - m)
    T = 4.0 + d + A + Am
    D = x.shape[-1] / 32.0 + 18.0
    with np.errstate(invalid="ignore", over="ignore"):
        row = np.where(p > 0, p * T, 0.0).sum(axis=-1, keepdims=True) + p0 * (4.0 + Am) + D
    R = T + row + 1.0
    if c.clip:
        t = p * c.w + c.gamma
        y = np.clip(t, 0.0, 1.0)
        t_err = U * (abs(c.w) * p * R + np.abs(p * c.w) + np.abs(t))
        y_err = t_err + TINY
    else:
        t, y, t_err = p, p, None
        y_err = U * p * R + TINY
    return dict(z_pre=z_pre, z=z, m=m, den=den, p=p, t=t, y=y, R=R, D=D, y_err=y_err, t_err=t_err)


def y_bound(f, y_dtype):
    return f["y_err"] + half_ulp(np.abs(f["y"]) + f["y_err"], y_dtype)


def dropped(c: Call, y_stored, keep):
    """u before its store: keep ? stored y * inv : 0, exact in float64 up to the product's one fp32 rounding (the test compares bits of
    RN_ydtype(RN32(y * inv)))."""
    return np.where(keep, np.asarray(y_stored, dtype=np.float64) * c.inv, 0.0)


def backward(c: Call, f, dy=None, du=None, keep=None):
    """dx (float64) and its absolute fp32 error bound (before the store's half ulp) from forward()'s dict and the gradients."""
    p, R, D = f["p"], f["R"], f["D"]
    g = np.zeros_like(p)
    G = np.zeros_like(p)
    if dy is not None:
        g = g + np.asarray(dy, dtype=np.float64)
        G = G + np.abs(dy)
    if du is not None:
        k = np.where(keep, np.asarray(du, dtype=np.float64) * c.inv, 0.0)
        g, G = g + k, G + np.abs(k)
    g_err = 3.0 * U * G
    if c.clip:
        t, t_err = f["t"], f["t_err"]
        inside = (t >= 0.0) & (t <= 1.0)
        unsure = (np.abs(t) <= t_err) | (np.abs(t - 1.0) <= t_err)
        g = np.where(inside, c.w * g, 0.0)
        g_err = np.where(inside | unsure, abs(c.w) * g_err, 0.0) + np.where(unsure, abs(c.w) * G, 0.0)
    pg = p * np.abs(g)
    delta = (p * g).sum(axis=-1, keepdims=True)
    spg = pg.sum(axis=-1, keepdims=True)
    delta_err = (pg * U * (R + 1.0 + D) + p * g_err).sum(axis=-1, keepdims=True)
    dz = p * (g - delta)
    dz_err = p * (np.abs(g) + spg) * U * (R + 2.0) + p * (g_err + delta_err)
    if c.clamp_min is not None:
        gate = np.where(f["z_pre"] > c.clamp_min, 1.0, np.where(f["z_pre"] == c.clamp_min, 0.5, 0.0))
        dz, dz_err = dz * gate, dz_err * gate
    s = abs(c.s())
    dx = dz / c.scale_div if c.scale_div > 0 else dz * c.scale
    dx_err = dz_err * s + U * np.abs(dx) + TINY * max(1.0, s)
    return dx, dx_err


def dx_bound(dx, dx_err, x_dtype):
    return dx_err + half_ulp(np.abs(dx) + dx_err, x_dtype)
