"""The training block tail (include/oeh.h: oeh_drop_resid_ln_fwd / oeh_drop_resid_ln_bwd) restated for its tests: the keep bit from the
published Philox4x32-10 algorithm (Salmon et al., SC 2011; Random123's constants - as tests/test_attn_dropout_cpu.py restates it for the
attention dropout) and the float64 forward and backward formulas.  numpy only; no GPU, no package import."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10: counter words and key words (broadcastable integer arrays) -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & _U32 for x in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    m0, m1, w0, w1, s32 = np.uint64(M0), np.uint64(M1), np.uint64(W0), np.uint64(W1), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # (exact: both factors < 2^32)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _U32, (p0 >> s32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + w0) & _U32, (k1 + w1) & _U32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def dropout_threshold(p):
    """thr = floor(p_f32 * 2^32): a word keeps its element iff word >= thr."""
    return int(np.floor(float(np.float32(p)) * 2.0 ** 32))


def inv_keep(p):
    """1 / (1 - p) as the kernels form it: once, in fp32."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(rows, cols, p, seed, row0=0):
    """The (rows, cols) bool keep mask of rows row0 .. row0 + rows - 1: key (seed & 0xffffffff, seed >> 32), counter
    (j >> 2, i & 0xffffffff, i >> 32, 1), word j & 3 of element (i, j), kept iff word >= floor(p * 2^32)."""
    nc = (cols + 3) // 4
    i = np.arange(row0, row0 + rows, dtype=np.uint64)[:, None]
    c = np.arange(nc, dtype=np.uint64)[None, :]
    w = philox4x32_10(c, i & _U32, i >> np.uint64(32), 1, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=-1).reshape(rows, 4 * nc)[:, :cols]
    return words >= np.uint32(dropout_threshold(p)) if p > 0 else np.ones((rows, cols), dtype=bool)


def stats64(s, eps):
    """(mean, rstd) of the rows of s, biased variance, float64."""
    s = np.asarray(s, dtype=np.float64)
    mean = s.mean(axis=-1)
    var = ((s - mean[:, None]) ** 2).mean(axis=-1)
    return mean, 1.0 / np.sqrt(var + np.float64(eps))


def forward64(s, gamma, beta, eps):
    """y of the stored sum s, float64."""
    mean, rstd = stats64(s, eps)
    y = (np.asarray(s, dtype=np.float64) - mean[:, None]) * rstd[:, None] * np.asarray(gamma, dtype=np.float64)
    return y if beta is None else y + np.asarray(beta, dtype=np.float64)


def backward64(dy, s, gamma, eps, keep, inv, dsum=None):
    """(dx, dr, dgamma, dbeta) in float64 from the stored sum s, the output gradient dy, the keep mask and inv = 1 / (1 - p); dsum: the
    gradient that arrived on the sum itself."""
    s, dy, gamma = (np.asarray(a, dtype=np.float64) for a in (s, dy, gamma))
    mean, rstd = stats64(s, eps)
    xhat = (s - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    c1 = g.mean(axis=-1, keepdims=True)
    c2 = (g * xhat).mean(axis=-1, keepdims=True)
    ds = rstd[:, None] * (g - c1 - xhat * c2)
    if dsum is not None:
        ds = ds + np.asarray(dsum, dtype=np.float64)
    dx = np.where(keep, ds * np.float64(inv), 0.0)
    return dx, ds, (dy * xhat).sum(axis=0), dy.sum(axis=0)
