"""float64 restatement of the attention calibration chain (include/oeh.h: oeh_attn_calibrate), the exactly-known score inputs of the
selection tests, the cases both calibration test files run, and the acceptance helpers they share.
numpy only; no GPU, no package import."""
import itertools
import zlib

import numpy as np

FMIN32 = float(np.finfo(np.float32).min)
FMIN16 = float(np.finfo(np.float16).min)
MANT_BITS = {"fp32": 23, "fp16": 10, "bf16": 7}


# ---- storage types ------------------------------------------------------------------------------------------------------------
def round_storage(a, storage: str):
    """float32 array -> the nearest value of the storage type (ties to even), as float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if storage == "fp32":
        return a.copy()
    if storage == "fp16":
        return a.astype(np.float16).astype(np.float32)
    u = a.view(np.uint32).astype(np.uint64)  # bf16: the upper 16 bits, round to nearest even
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def next_representable(a, storage: str):
    """a + one spacing of the storage type at |a| (a: values of that type, away from its subnormals): again a value of the type,
    and one of the two neighbours of a."""
    a = np.asarray(a, dtype=np.float32)
    _, e = np.frexp(a)
    return (a.astype(np.float64) + np.ldexp(1.0, e - 1 - MANT_BITS[storage])).astype(np.float32)


# ---- the chain in float64 -----------------------------------------------------------------------------------------------------
def grid_from_range(x_min: float, x_max: float, n_bits: int = 8, eps: float = 1e-8):
    """(scale, zero_point, qmax) from a float64 (x_min, x_max) pair as set_quant_range derives them (uniform_quantizers.py:72-82) and
    the kernel's grid_from_range restates: the range is widened to hold 0 and eps, the scale is rounded to float32."""
    qmax = float(2 ** n_bits - 1)
    lo, hi = min(float(x_min), 0.0), max(float(x_max), eps)
    delta = (hi - lo) / qmax
    zero = -lo / delta
    scale = float(np.float32(max(delta, eps)))
    zp = float(min(max(float(np.rint(zero)), 0.0), qmax))
    return scale, zp, qmax


def fake_quant64(x, scale, zp, qmax):
    return scale * (np.clip(np.rint(np.asarray(x, dtype=np.float64) / scale) + zp, 0.0, qmax) - zp)


def causal_mask(Sq: int, Sk: int, mask_min: float):
    i = np.arange(Sq)[:, None] + (Sk - Sq)
    j = np.arange(Sk)[None, :]
    return np.where(j > i, float(mask_min), 0.0)


def attn64(q, k, v=None, *, scale=1.0, scale_div=0.0, scores_range=None, probs_range=None, n_bits=8, eps=1e-8, pad=None, full=None,
           causal=False, clamp_min=False, mask_min=FMIN32, base=1, clip=None, scores_grid=None, probs_grid=None):
    """The contract's chain in float64, in its order: q k^T; / scale_div or else * scale; [score fake-quant]; + pad; + full; + causal
    (Sk - Sq offset); [max(., mask_min)]; softmax (base 0 / 1); [clamp(p (eta - gamma) + gamma, 0, 1)]; [probability fake-quant]; P V.
    Scalars the kernel receives as float32 (scale, scale_div, mask_min, gamma, eta - gamma) enter as those float32 values.
    scores_grid / probs_grid: a quantiser given as its grid (scale, zero_point, qmax) instead of a range (tests/_attn_ref.py).
    Returns a dict: "scores" (scaled, before quantiser and masks - what CALIB_SCORES measures), "probs" (after the clip, before the
    probability quantiser - what CALIB_PROBS measures), "probs_q" (what multiplies V) and "ctx" (None without v)."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    Sq, Sk = q.shape[2], k.shape[2]
    s = np.matmul(q, np.swapaxes(k, -1, -2))
    if scale_div != 0.0:
        s = s / float(np.float32(scale_div))
    elif scale != 1.0:
        s = s * float(np.float32(scale))
    out = {"scores": s}
    if scores_grid is None and scores_range is not None:
        scores_grid = grid_from_range(scores_range[0], scores_range[1], n_bits, eps)
    if probs_grid is None and probs_range is not None:
        probs_grid = grid_from_range(probs_range[0], probs_range[1], n_bits, eps)
    x = s if scores_grid is None else fake_quant64(s, *scores_grid)
    mmin = float(np.float32(mask_min))
    if pad is not None:
        x = x + np.asarray(pad, dtype=np.float64)[:, None, None, :]
    if full is not None:
        x = x + np.asarray(full, dtype=np.float64)
    if causal:
        x = x + causal_mask(Sq, Sk, mmin)[None, None]
    if clamp_min:
        x = np.maximum(x, mmin)
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(over="ignore"):
        e = np.exp(x - m)
        den = e.sum(axis=-1, keepdims=True)
        if base != 0:
            den = den + np.exp(-m)
        p = e / den
    if clip is not None:
        gamma, eta = clip
        p = np.clip(p * float(np.float32(float(eta) - float(gamma))) + float(np.float32(gamma)), 0.0, 1.0)
    out["probs"] = p
    pq = p if probs_grid is None else fake_quant64(p, *probs_grid)
    out["probs_q"] = pq
    out["ctx"] = None if v is None else np.matmul(pq, np.asarray(v, dtype=np.float64))
    return out


def err64(a32, a64) -> float:
    """max |a32 - a64|: the distance of an fp32 evaluation from the float64 one, the unit of every tolerance here."""
    return float(np.max(np.abs(np.asarray(a32, dtype=np.float64) - np.asarray(a64, dtype=np.float64))))


def tie_band(p64, scale, zp, qmax, err_probs: float, factor: float = 4.0):
    """Boolean array like p64: the probabilities within factor * err_probs / scale (in grid steps) of a rounding boundary of the
    grid, which an fp32 evaluation may put on either neighbouring grid point.  The boundaries are j + 1/2 for j = 0 .. qmax - 1: beyond
    the saturated ends both sides clamp to the same point."""
    t = np.asarray(p64, dtype=np.float64) / scale + zp
    w = factor * err_probs / scale
    near = np.abs((t - np.floor(t)) - 0.5) <= w
    return near & (t >= 0.5 - w) & (t <= qmax - 0.5 + w)


# ---- percentile pairs ---------------------------------------------------------------------------------------------------------
def virtual_index(n: int, q: float):
    """np.percentile's ("linear") position of percent q among n sorted elements, as the entry point forms it: (i, frac)."""
    h = float(n - 1) * (float(q) / 100.0)
    return int(h), h - float(int(h))


def frac0_pair(n: int):
    """A percentile pair whose positions (n - 1) q / 100 are integers in floating point too (frac exactly 0), near 30 % and 80 %."""
    def find(m0):
        for m in itertools.chain(range(m0, n), range(m0 - 1, -1, -1)):
            qv = 100.0 * m / max(n - 1, 1)
            if 0.0 <= qv <= 100.0 and virtual_index(n, qv) == (m, 0.0):
                return qv
        return 0.0
    return find(int(0.3 * (n - 1))), find(int(0.8 * (n - 1)))


def pairs_for(n: int):
    return ((0.0, 100.0), (50.0, 50.0), (0.1, 99.9), (25.0, 75.0), frac0_pair(n))


# ---- inputs whose scores are known exactly ------------------------------------------------------------------------------------
def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def selector_inputs(seed: int, B: int, H: int, Sq: int, Sk: int, D: int, storage: str):
    """q, k (float32 arrays holding values of `storage`) and the exact q k^T (float32).  Every q row is zero except one head dim,
    which holds +-2^e, e in -2..2: every product with 0 is exact, so the score is k[key][dim] * +-2^e whatever the summation order.
    k: N(0,1) with Student-t tails, a block of exact duplicate rows, and rows one spacing of the storage type above their neighbour."""
    rs = np.random.RandomState(seed)
    k = (rs.standard_normal((B, H, Sk, D)) * (1.0 + 0.25 * np.abs(rs.standard_t(3, size=(B, H, Sk, D))))).astype(np.float32)
    k = round_storage(k, storage)
    k = np.where(np.abs(k) < 2.0 ** -10, np.float32(0.5), k).astype(np.float32)  # (keep clear of the fp16 subnormals)
    if Sk >= 8:
        a = Sk // 4
        k[:, :, a + 1:a + 1 + Sk // 8] = k[:, :, a:a + 1]        # exact duplicates
        src = np.arange(Sk // 2, Sk - 1, 2)
        k[:, :, src + 1] = next_representable(k[:, :, src], storage)  # one-spacing pairs
    dim = rs.randint(0, D, size=(B, H, Sq))
    val = (np.ldexp(1.0, rs.randint(-2, 3, size=(B, H, Sq))) * rs.choice([-1.0, 1.0], size=(B, H, Sq))).astype(np.float32)
    q = np.zeros((B, H, Sq, D), dtype=np.float32)
    bi, hi, si = np.meshgrid(np.arange(B), np.arange(H), np.arange(Sq), indexing="ij")
    q[bi, hi, si, dim] = val
    # gather: scores[b,h,i,j] = k[b,h,j,dim[b,h,i]] * val[b,h,i]
    kt = np.swapaxes(k, 2, 3)                                     # (B,H,D,Sk)
    scores = kt[bi, hi, dim] * val[..., None]                     # (B,H,Sq,Sk), exact: a power of two times a float32
    return q, k, scores.astype(np.float32)


def integer_inputs(seed: int, B: int, H: int, Sq: int, Sk: int, D: int):
    """q in {-1,0,1}, k in {-2..2}: integer scores (exact in every summation order and storage type), a few dozen distinct values."""
    rs = np.random.RandomState(seed)
    q = rs.randint(-1, 2, size=(B, H, Sq, D)).astype(np.float32)
    k = rs.randint(-2, 3, size=(B, H, Sk, D)).astype(np.float32)
    scores = np.matmul(q.astype(np.float64), np.swapaxes(k, -1, -2).astype(np.float64)).astype(np.float32)
    return q, k, scores


def scale_scores(scores32, scale: float, scale_div: float):
    """The entry point's scaling in float32 (a power of two here: exact)."""
    s = np.asarray(scores32, dtype=np.float32)
    if scale_div != 0.0:
        return (s / np.float32(scale_div)).astype(np.float32)
    if scale != 1.0:
        return (s * np.float32(scale)).astype(np.float32)
    return s


# ---- masks --------------------------------------------------------------------------------------------------------------------
def pad_vector(B: int, Sk: int, lens, low: float, dtype=np.float32):
    """(B,Sk) additive key padding: 0 for the first lens[b] keys of sample b, `low` beyond."""
    m = np.zeros((B, Sk), dtype=dtype)
    for b in range(B):
        m[b, int(lens[b % len(lens)]):] = low
    return m


def full_matrix(seed: int, B: int, Sq: int, Sk: int, low: float = FMIN32):
    """(B,1,Sq,Sk) additive mask: each key masked with probability 0.3, key 0 always kept (no row without a key)."""
    rs = np.random.RandomState(seed)
    m = np.where(rs.rand(B, 1, Sq, Sk) < 0.3, np.float32(low), np.float32(0.0)).astype(np.float32)
    m[..., 0] = 0.0
    return m


# ---- the cases ----------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 45), (16, 15), (63, 17), (64, 16), (65, 33), (150, 150), (17, 128))
HEAD_DIMS = (32, 64, 128)
STORAGES = ("fp32", "fp16", "bf16")
FAMILIES = ("selector", "integer")
LAYOUTS = ("contiguous", "fused")
MOMENTA = (0.0, 0.9, 1.0)


def batch_heads(Sq: int, Sk: int):
    return (1, 1) if (Sq, Sk) == (1, 1) else (3, 2)


def selection_cases(D: int, storage: str):
    """The selection cases of one template instance: family x shape x layout, with the scaling form, the masks / clip (which must not
    change the score statistics) and the momentum rotating over them."""
    out = []
    for ci, (family, (Sq, Sk), layout) in enumerate(itertools.product(FAMILIES, SHAPES, LAYOUTS)):
        B, H = batch_heads(Sq, Sk)
        c = dict(name=f"{family}-{Sq}x{Sk}-{layout}", family=family, B=B, H=H, Sq=Sq, Sk=Sk, D=D, storage=storage, layout=layout,
                 seed=_seed("sel", family, Sq, Sk, D, storage), momentum=MOMENTA[(ci // 2) % 3],
                 scale=0.5 if ci % 3 == 1 else 1.0, scale_div=2.0 if ci % 3 == 0 else 0.0, extras=("none", "opt", "bert", "none")[ci % 4])
        out.append(c)
    return out


def selection_inputs(c):
    """(q, k, the exactly known scaled scores) of a selection case."""
    if c["family"] == "selector":
        q, k, s = selector_inputs(c["seed"], c["B"], c["H"], c["Sq"], c["Sk"], c["D"], c["storage"])
    else:
        q, k, s = integer_inputs(c["seed"], c["B"], c["H"], c["Sq"], c["Sk"], c["D"])
    return q, k, scale_scores(s, c["scale"], c["scale_div"])


def selection_extras(c):
    """Masks / clip of a selection case as keyword values shared by attn64 and the entry point (numpy arrays for the masks)."""
    B, Sq, Sk = c["B"], c["Sq"], c["Sk"]
    if c["extras"] == "opt":
        return dict(pad=pad_vector(B, Sk, (Sk, max(1, Sk // 2), Sk), FMIN32), causal=True, clamp_min=True, base=1)
    if c["extras"] == "bert":
        return dict(full=full_matrix(c["seed"] + 1, B, Sq, Sk), clip=(-0.025, 1.0), base=0)
    return dict(base=1)


def _vc(name, Sq, Sk, **kw):
    d = dict(name=name, Sq=Sq, Sk=Sk, B=3, H=2, base=1, clip=None, scale=1.0, scale_div=0.0, sr=None, n_bits=8, pad=None, lens=None, full=None,
             causal=False, clamp_min=False)
    d.update(kw)
    return d


# probabilities and context: the integer-score family (no rounding boundary of the score quantiser to straddle: every range below has
# a power-of-two step), one or two ragged shapes per branch
VALUE_CASES = (
    _vc("vanilla", 65, 33, base=0),
    _vc("softmax1", 150, 150),
    _vc("single", 1, 1, B=1, H=1),
    _vc("scale-half", 16, 15, base=0, scale=0.5),
    _vc("clip-025-sat-below", 63, 17, base=0, clip=(-0.025, 1.0), sr=(-8.0, 247.0)),
    _vc("clip-003-sat-above", 65, 33, clip=(-0.003, 1.003), sr=(-250.0, 5.0)),
    _vc("pad-f32-4bit", 16, 15, pad="f32", lens=(15, 7, 1), sr=(-8.0, 7.0), n_bits=4),
    _vc("pad-f16-eighths", 1, 45, base=0, pad="f16", lens=(45, 20, 33), scale_div=8.0, sr=(-12.0, 19.875)),
    _vc("full-f32", 65, 33, full="f32"),
    _vc("full-strided", 17, 128, base=0, full="strided"),
    _vc("pad-and-full-eighths", 150, 150, pad="f32", lens=(150, 97, 16), full="f32", scale_div=8.0, sr=(-12.0, 19.875)),
    _vc("causal-pad-clamp-wide", 17, 128, pad="f32", lens=(128, 120, 64), causal=True, clamp_min=True, sr=(-8.0, 247.0)),
    _vc("causal-pad-clamp-tall", 63, 17, base=0, pad="f32", lens=(17, 9, 17), causal=True, clamp_min=True),
    _vc("masked-sample-clamp-vanilla", 64, 16, base=0, pad="f32", lens=(16, 0, 11), clamp_min=True),
    _vc("masked-sample-clamp-softmax1", 64, 16, pad="f32", lens=(16, 0, 11), clamp_min=True, sr=(-8.0, 247.0)),
)
VALUE_PAIRS = ((30.0, 99.9), (50.0, 90.0))
PROB_RANGES = ((0.0, 1.0), (0.0, 0.5))  # the full range, and a narrower one that saturates
MAX_BAND_ROWS = 0.05


def value_inputs(c, D: int, storage: str):
    """q, k (integer family), v ~ N(0,1) in the storage type, and the masks of a value case: dict(q, k, v, pad, full).  pad keeps the
    dtype the entry point is to read (float16 masks hold finfo(float16).min)."""
    B, H, Sq, Sk = c["B"], c["H"], c["Sq"], c["Sk"]
    seed = _seed("val", c["name"], D, storage)
    q, k, _ = integer_inputs(seed, B, H, Sq, Sk, D)
    v = round_storage(np.random.RandomState(seed + 1).standard_normal((B, H, Sk, D)).astype(np.float32), storage)
    pad = None
    if c["pad"] == "f32":
        pad = pad_vector(B, Sk, c["lens"], FMIN32, np.float32)
    elif c["pad"] == "f16":
        pad = pad_vector(B, Sk, c["lens"], FMIN16, np.float16)
    full = None if c["full"] is None else full_matrix(seed + 2, B, Sq, Sk)
    return dict(q=q, k=k, v=v, pad=pad, full=full)


def value_kwargs(c, probs_range=None):
    """attn64's keyword arguments of a value case (masks come from value_inputs)."""
    return dict(scale=c["scale"], scale_div=c["scale_div"], scores_range=c["sr"], probs_range=probs_range, n_bits=c["n_bits"],
                causal=c["causal"], clamp_min=c["clamp_min"], mask_min=FMIN32, base=c["base"], clip=c["clip"])


def value_refs(c, D: int, storage: str, oracle, probs_range=None):
    """(inputs, float64 results, the fp32 oracle's probabilities and context) of a value case.  `oracle`: the module
    oracle.oeh_oracle, passed in by the test files (this module imports numpy only)."""
    x = value_inputs(c, D, storage)
    kw = value_kwargs(c, probs_range)
    pad32 = None if x["pad"] is None else x["pad"].astype(np.float32)
    r64 = attn64(x["q"], x["k"], x["v"], pad=pad32, full=x["full"], **kw)
    okw = dict(base=c["base"], pad_mask=pad32, full_mask=x["full"], causal=c["causal"], clamp_min=c["clamp_min"], mask_min=FMIN32)
    if c["clip"] is not None:
        okw.update(gamma=c["clip"][0], eta=c["clip"][1], clip=True)
    if c["scale_div"] != 0.0:
        okw.update(scale=c["scale_div"], scale_is_divisor=True)
    else:
        okw.update(scale=c["scale"])
    if c["sr"] is not None:
        okw["fq_scores"] = oracle.quant_range_to_params(np.float64(c["sr"][0]), np.float64(c["sr"][1]), c["n_bits"]) + (c["n_bits"],)
    _, o = oracle.attn_core(x["q"], x["k"], x["v"], want=("probs",), **okw)
    p32 = o["probs"]
    if probs_range is not None:
        okw["fq_probs"] = oracle.quant_range_to_params(np.float64(probs_range[0]), np.float64(probs_range[1]), c["n_bits"]) + (c["n_bits"],)
    ctx32 = oracle.attn_core(x["q"], x["k"], x["v"], **okw)
    return x, r64, p32, ctx32


def band_rows(r64, p32, probs_range, n_bits: int, eps: float = 1e-8):
    """The tie band of a context case with the probability quantiser: (boolean (B,H,Sq) rows that hold a band probability, band
    probabilities per row, the grid's scale)."""
    scale, zp, qmax = grid_from_range(probs_range[0], probs_range[1], n_bits, eps)
    band = tie_band(r64["probs"], scale, zp, qmax, err64(p32, r64["probs"]))
    return band.any(axis=-1), band.sum(axis=-1), scale
