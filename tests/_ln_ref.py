"""float64 restatement of the block-tail formula (include/oeh.h: oeh_resid_ln_quant) and the acceptance rules the LayerNorm tests share.
numpy only; no GPU, no package import."""
import numpy as np


def grid_from_minmax(lo: float, hi: float, n_bits: int = 8, eps: float = 1e-8):
    """(scale, zero_point, qmax) as AsymmetricUniformQuantizer.set_quant_range + the scale / zero_point properties derive them
    (uniform_quantizers.py:72-82) from a float32 (min, max) pair."""
    qmax = float(2 ** n_bits - 1)
    lo32, hi32 = np.float32(min(lo, 0.0)), np.float32(max(hi, eps))
    delta = np.float32((hi32 - lo32) / np.float32(qmax))
    zero_float = np.float32(-lo32 / delta)
    scale = float(np.float32(max(float(delta), eps)))
    zp = float(min(max(float(np.rint(np.float64(zero_float))), 0.0), qmax))
    return scale, zp, qmax


def fake_quant64(x, scale, zp, qmax):
    """(indices, values) of the asymmetric fake-quant in float64."""
    x = np.asarray(x, dtype=np.float64)
    idx = np.clip(np.rint(x / scale) + zp, 0.0, qmax)
    return idx, scale * (idx - zp)


def layer_norm64(s, gamma, beta, eps):
    """y = (s - mean) / sqrt(var + eps) * gamma + beta over the last axis, biased variance, float64."""
    s = np.asarray(s, dtype=np.float64)
    mean = s.mean(axis=-1, keepdims=True)
    var = ((s - mean) ** 2).mean(axis=-1, keepdims=True)
    y = (s - mean) / np.sqrt(var + np.float64(eps))
    y = y * np.asarray(gamma, dtype=np.float64)
    if beta is not None:
        y = y + np.asarray(beta, dtype=np.float64)
    return y


def ulp_of(a, dtype_name: str):
    """Spacing of the storage type at |a| (elementwise): float16, bfloat16 or float32."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    if dtype_name == "float32":
        return np.spacing(a.astype(np.float32)).astype(np.float64)
    if dtype_name == "float16":
        return np.spacing(np.minimum(a, 65504.0).astype(np.float16)).astype(np.float64)
    # bfloat16: 8 significand bits, float32's exponent range
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 7)


def check_values(y, y64, err64, dtype_name: str = "float32", factor: float = 4.0):
    """|y - y64| <= factor * err64 (+ half an ulp of a 16-bit storage type).  Returns the measured max |y - y64| / err64 (of the part the
    storage rounding does not explain), for the test to print."""
    y = np.asarray(y, dtype=np.float64)
    diff = np.abs(y - y64)
    lim = np.full_like(diff, factor * err64)
    slack = np.zeros_like(diff)
    if dtype_name != "float32":
        slack = 0.5 * ulp_of(np.abs(y64) + factor * err64, dtype_name)
    bad = diff > lim + slack
    ratio = float(np.max(np.maximum(diff - slack, 0.0)) / err64) if err64 > 0 else (0.0 if not bad.any() else float("inf"))
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} values beyond {factor} x err64 = {factor * err64:.3e}: max |y - f64| = {diff.max():.3e} (ratio {ratio:.2f})"
    return ratio


def check_indices(idx, y64, scale, zp, qmax, err64, max_band: float = 1e-3, factor: float = 4.0, ref_idx=None):
    """The tie-band rule for a quantised output.  With t = y64 / scale + zp: outside the band |frac(t) - 1/2| <= factor * err64 / scale every
    index equals clamp(rint(t)); inside it an index may differ by exactly one step; the band holds at most `max_band` of the elements (a
    condition on the inputs).  Returns (share of elements in the band, share of indices that differ)."""
    idx = np.asarray(idx, dtype=np.float64)
    t = np.asarray(y64, dtype=np.float64) / scale + zp
    want = np.clip(np.rint(t), 0.0, qmax)
    band = np.abs((t - np.floor(t)) - 0.5) <= factor * err64 / scale
    share = float(band.mean())
    assert share <= max_band, f"the tie band holds {share:.2e} of the elements (> {max_band:.0e}): not a usable case"
    off = idx != want
    assert not (off & ~band).any(), f"{int((off & ~band).sum())} indices differ outside the tie band"
    assert (np.abs(idx - want)[band] <= 1.0).all(), "an index inside the tie band moved by more than one step"
    if ref_idx is not None:  # another fp32 evaluation's indices (the reference's): the same outside the band, within one step inside it
        ref_idx = np.asarray(ref_idx, dtype=np.float64).reshape(idx.shape)
        assert not ((idx != ref_idx) & ~band).any(), f"{int(((idx != ref_idx) & ~band).sum())} indices differ from the reference's outside the tie band"
        assert (np.abs(idx - ref_idx)[band] <= 1.0).all(), "an index inside the tie band is more than one step from the reference's"
        off = idx != ref_idx
    return share, float(off.mean())


def check_on_grid(y, idx, scale, zp, round_storage=None):
    """Every written value is exactly fl32(scale * (idx - zp)) - rounded to the storage type by `round_storage` where that is 16-bit."""
    want = np.float32(scale) * (np.asarray(idx, dtype=np.float32) - np.float32(zp))
    if round_storage is not None:
        want = round_storage(want)
    got = np.asarray(y, dtype=np.float32)
    assert np.array_equal(got, want.astype(np.float32)), f"{int((got != want).sum())} values are not scale * (idx - zp)"


# ---- seeded inputs and weights of tests/golden/ln_tail.npz: tests/golden/make_ln_golden.py (next to the reference) and the tests (GPU box)
# regenerate the same bits from numpy's legacy RandomState streams; the fixture stores seeds, ranges, indices and error figures only
OUTLIER_CHANNELS = ((7, 40.0), (-3, -25.0))  # (channel, factor): the residual stream's outlier dimensions


def normal(seed: int, shape, scale: float = 1.0):
    return (np.random.RandomState(seed).standard_normal(size=tuple(shape)) * scale).astype(np.float32)


def with_outliers(x):
    x = np.array(x, dtype=np.float32, copy=True)
    for ch, f in OUTLIER_CHANNELS:
        x[..., ch] *= np.float32(f)
    return x


def tail_state_dict(shapes: dict, seed: int, w_std: float = 0.05):
    """name -> float32 array for every (name, shape), drawn in sorted-name order from one stream: LayerNorm weights 1 + N(0, 0.2), LayerNorm
    biases N(0, 0.1), everything else N(0, w_std)."""
    rs = np.random.RandomState(seed)
    out = {}
    for name in sorted(shapes):
        v = rs.standard_normal(size=tuple(shapes[name]))
        is_ln = "layer_norm" in name.lower() or "layernorm" in name.lower() or name in ("weight", "bias")
        if is_ln:
            v = 1.0 + 0.2 * v if name.endswith("weight") else 0.1 * v
        else:
            v = w_std * v
        out[name] = v.astype(np.float32)
    return out
