"""float64 restatement of the whole attention core (include/oeh.h: oeh_attn_fwd) on top of tests/_calib_ref.attn64 - the gate, the
context quantiser before or after it, ctx_emit_index, quantisers given as grids - with the fp32 oracle's distance from it per stage,
the cases tests/test_attn_fallback_cpu.py, tests/test_attn_small_gpu.py and tests/test_attn_generic_gpu.py share, the acceptance
checks, and the one routine that poses a case to the library.  numpy only: `oracle`, `ops` and `torch` are passed in by the test files.

Acceptance (the issue's "Tolerances"):
  exact kernels (small-shape, any-shape: fp32 arithmetic on the stored values, one rounding at the store)
      |got - want64| <= 4 err64 [+ half a 16-bit ulp of want64], err64 = max |fp32 oracle - float64| of the case's output over the
      elements the check covers; a quantiser's index equals the float64 index outside its tie band (_calib_ref.tie_band with err64
      of the stage feeding it, factor 4) and is within one of it inside; rows that hold a band element of an upstream quantiser are
      left out of everything downstream; a context element inside the context quantiser's band may sit one grid step off
  general kernel (fp16 matrix-core operands; operand pairs in fp32 storage) and the one-pass kernel
      the contract of tests/test_attn_gpu.py against float64: 1e-3 + half an fp16 ulp (fp16), 2e-2 absolute + relative (bf16),
      5e-4 absolute + relative (fp32 storage: dict(atol=5e-4, rtol=5e-4) wherever that file checks it - the probability operand is
      one fp16 number, 2^-11 relative, so the error grows with |p| |v|); with quantisers the same file's statement - an index is within one of the float64 index, such flips are
      rarer than 2e-3 of a dump (two elements always allowed), and rows without a flip upstream meet the contract
"""
import ctypes
import itertools

import numpy as np

from tests import _calib_ref as R

U = 2.0 ** -24
FACTOR = 4.0              # yardstick C of tests/test_attn_calibrate_gpu.py
MAX_BAND_ELEMENTS = 0.01  # of a dump
MAX_LEFT_OUT_ROWS = 0.10  # of a case
FLIP_SHARE = 2e-3         # general kernel: tests/test_attn_gpu.py's docstring
GENERIC_ONLY = (1 << 1) | (1 << 2) | (1 << 3) | (1 << 5) | (1 << 6) | (1 << 7)  # include/oeh_debug.h: every kernel but the any-shape one off
FORCE_SMALL = 1 << 10
DT_NAME = {"fp32": "f32", "fp16": "f16", "bf16": "bf16"}
CONTRACT = {"fp16": (1e-3, 0.0), "bf16": (2e-2, 2e-2), "fp32": (5e-4, 5e-4)}  # (absolute, relative) as tests/test_attn_gpu.py applies them; fp16 adds half an fp16 ulp


# ---- the chain ----------------------------------------------------------------------------------------------------------------
def index64(x, scale, zp, qmax):
    return np.clip(np.rint(np.asarray(x, dtype=np.float64) / scale) + zp, 0.0, qmax)


def chain64(q, k, v, *, gate=None, ctx_grid=None, ctx_before_gate=True, ctx_emit_index=False, scores_grid=None, probs_grid=None, **kw):
    """_calib_ref.attn64 (its keyword arguments pass through), then: [context fake-quant] ; * gate ; [context fake-quant] - before the
    gate in the OPT order, after it in the BERT order; ctx_emit_index: the integers idx - zp instead of scale * (idx - zp).  gate: fp32
    values broadcastable to (B,H,Sq,1).  Returns scores, scores_idx, probs, probs_idx, ctx_pre (what the context quantiser reads; the
    output itself without one), ctx_idx, ctx (the output); an index array is None without its quantiser."""
    r = R.attn64(q, k, v, scores_grid=scores_grid, probs_grid=probs_grid, **kw)
    out = dict(scores=r["scores"], probs=r["probs"], probs_q=r["probs_q"],
               scores_idx=None if scores_grid is None else index64(r["scores"], *scores_grid),
               probs_idx=None if probs_grid is None else index64(r["probs"], *probs_grid), ctx_idx=None)
    c = r["ctx"]
    g = None if gate is None else np.asarray(gate, dtype=np.float64)

    def quant(c):
        scale, zp, qmax = ctx_grid
        out["ctx_pre"], out["ctx_idx"] = c, index64(c, scale, zp, qmax)
        return (out["ctx_idx"] - zp) * (1.0 if ctx_emit_index else scale)
    if ctx_grid is not None and ctx_before_gate:
        c = quant(c)
    if g is not None:
        c = c * g
    if ctx_grid is not None and not ctx_before_gate:
        c = quant(c)
    if ctx_grid is None:
        out["ctx_pre"] = c
    out["ctx"] = c
    return out


def half_ulp(want64, storage: str):
    """Half a spacing of the 16-bit storage type at |want64| (0 for fp32): what storing the result adds."""
    if storage == "fp32":
        return np.zeros_like(want64)
    _, e = np.frexp(np.abs(want64))
    e = np.maximum(e - 1, -14 if storage == "fp16" else -126)
    return 0.5 * np.ldexp(1.0, e - R.MANT_BITS[storage])


# ---- cases --------------------------------------------------------------------------------------------------------------------
def _c(name, Sq, Sk, D, **kw):
    """A case.  clip: (gamma, eta); pad: "f32" / "f16" with lens (visible keys per sample); full: "f32" / "f16" / "strided"; gate:
    "token" (B,H,Sq,1) / "head" (1,H,1,1: zero strides); gs / gp / gc: the score / probability / context quantiser as (lo, hi, bits);
    before: the context quantiser before the gate; emit: ctx_emit_index; dumps: index dumps of every quantiser that is on; layout:
    see `pose`; qmul: q is N(0,1) * qmul; shift: a constant added to every score; hook: the off_mask of include/oeh_debug.h;
    via "prepared": launched through the prebuilt-call form (ops pads no head dim there); kernel: the variant name the library must give;
    seq_bound: see `check_exact`; out32: out_dtype=float32 on 16-bit storage; pv_pairs: the probability pairs (fp32 storage); pad_bool:
    key_pad_boolean; gate_units: the in-kernel gate predictor (ops.GatePredictor) with that many hidden units, 0 the linear one;
    mq: flash_mq_force of include/oeh_debug.h; ramp: ramp * (j - Sk) is added to the score of key j, so that the latest keys a causal row
    sees weigh most."""
    d = dict(name=name, B=2, H=2, Sq=Sq, Sk=Sk, D=D, storage="fp32", base=1, clip=None, scale=None, scale_div=0.0, pad=None, lens=None,
             full=None, causal=False, clamp_min=False, mask_min=R.FMIN32, gate=None, gs=None, gp=None, gc=None, before=True, emit=False,
             dumps=False, layout="contig", qmul=1.0, shift=None, hook=0, via="fwd", kernel=None, seq_bound=False, out32=False, pv_pairs=False, pad_bool=False,
             gate_units=None, mq=0, ramp=None)
    assert not set(kw) - set(d), set(kw) - set(d)
    d.update(kw)
    if d["scale"] is None:
        d["scale"] = 1.0 if d["scale_div"] != 0.0 else float(np.float32(D ** -0.5))
    return d


MODES = ((0, None), (1, None), (0, (-0.003, 1.003)), (1, (-0.025, 1.1)))  # vanilla, softmax_1, clipped, clipped softmax_1


def _small(name, Sq, Sk, D, **kw):
    c = _c("small-" + name, Sq, Sk, D, hook=FORCE_SMALL, **kw)
    c["kernel"] = f"small/ST{2 if Sk <= 32 else 4}/D{D}/{DT_NAME[c['storage']]}"
    return c


def _small_instances():
    """The 18 template instances (D x ST x storage), with every Sk and Sq of the issue's lists, H in 1 / 3 / 4, the three scalings and the
    four softmax modes rotating over them."""
    sk_short, sk_long, sqs = (1, 3, 5, 15, 16, 17, 31, 32, 5), (33, 48, 63, 64, 33, 48, 63, 64, 48), (1, 15, 16, 17, 32, 33, 49, 64)
    out = []
    for i, (D, st) in enumerate(itertools.product((16, 32, 64), R.STORAGES)):
        for j, sks in enumerate((sk_short, sk_long)):
            n = 2 * i + j
            base, clip = MODES[(n + i) % 4]
            scaling = (dict(), dict(scale=1.0, qmul=0.5), dict(scale_div=3.0))[n % 3]
            out.append(_small(f"inst{n}", sqs[(3 * n) % 8], sks[i], D, storage=st, B=(2, 3, 5)[(n // 3) % 3], H=(1, 3, 4)[(n + n // 3) % 3], base=base,
                              clip=clip, **scaling))
    return out


SMALL_CASES = tuple(_small_instances()) + (
    _small("form2-nqb2-one-problem", 17, 17, 32, B=1, H=1, base=0),
    _small("form2-nqb3-nine-waves", 33, 33, 16, B=1, H=3),
    _small("form2-nqb4", 64, 64, 64, B=2, H=4, storage="fp16", base=0),
    _small("form3-512x4-gamma-pos", 33, 5, 16, B=512, H=4, base=0, clip=(0.05, 1.0)),
    _small("form3-683x3-gate", 33, 5, 16, B=683, H=3, storage="fp16", gate="token"),
    _small("gamma-pos-17", 15, 17, 32, B=3, base=0, clip=(0.05, 1.0)),
    _small("gamma-pos-33", 17, 33, 64, B=3, storage="bf16", clip=(0.05, 1.05)),
    _small("gate-token-ragged", 17, 31, 32, B=3, H=3, storage="fp16", gate="token", base=0),
    _small("gate-head", 49, 48, 64, B=2, H=4, gate="head"),
    _small("layout-blhe", 28, 28, 64, B=3, H=4, layout="blhe", clip=(-0.025, 1.1)),
    _small("layout-longkv", 16, 15, 16, B=2, H=3, storage="fp16", layout="longkv"),
    _small("layout-outslice", 33, 32, 32, B=2, H=3, storage="bf16", layout="outslice", base=0),
    _small("layout-off4-f16", 15, 63, 16, B=2, H=3, storage="fp16", layout="off4"),
    _small("layout-off4-bf16", 33, 17, 64, B=2, H=1, storage="bf16", layout="off4", gate="head"),
    _small("layout-fused", 31, 31, 32, B=3, H=4, layout="fused", base=0, scale_div=3.0),
    _small("hot60", 17, 33, 16, B=3, H=3, scale=1.0, qmul=6.0),
    _small("cold30", 16, 16, 32, B=3, H=3, shift=-30.0),
)


def _gen(name, Sq, Sk, D, **kw):
    """An any-shape case: head dims the matrix-core kernels take are put there by the hooks, the others arrive by themselves."""
    if D in (16, 32, 64, 128) and Sk <= 512:
        kw.setdefault("hook", GENERIC_ONLY)
    if D < 128 and D not in (16, 32, 64):
        kw.setdefault("via", "prepared")
    return _c("generic-" + name, Sq, Sk, D, kernel="generic", **kw)


S8, P8, C8 = (-5.0, 5.0, 8), (0.0, 1.0, 8), (-2.0, 2.0, 8)
GENERIC_CASES = (
    # how the kernel is reached, storages, head dims (d loop: 200 > 128 threads), Sk on both sides of 128 threads
    _gen("d144-fwd", 5, 129, 144, storage="fp16"),
    _gen("d200-fwd-div", 3, 300, 200, base=0, scale_div=3.0),
    _gen("d8-prepared", 7, 5, 8, storage="bf16", clip=(-0.003, 1.003), base=0),
    _gen("d48-pad-f16", 4, 127, 48, storage="fp16", pad="f16", lens=(127, 50), clamp_min=True, mask_min=R.FMIN16),
    _gen("d80-pad-and-full", 6, 128, 80, pad="f32", lens=(128, 77), full="f32", clamp_min=True),
    _gen("d127-one-key", 3, 1, 127),
    _gen("d64-hook-causal-wide", 16, 64, 64, storage="fp16", causal=True),
    _gen("d64-hook-causal-square", 17, 17, 64, causal=True, clamp_min=True, base=0),
    _gen("d64-hook-causal-tall", 9, 5, 64, storage="bf16", causal=True, clamp_min=True),
    _gen("causal-tall-vanilla", 9, 5, 48, causal=True, clamp_min=True, base=0),
    _gen("full-f16", 5, 129, 144, storage="fp16", full="f16", mask_min=R.FMIN16, base=0),
    _gen("full-strided", 4, 300, 64, full="strided"),
    _gen("pad-f32-no-clamp", 5, 33, 48, pad="f32", lens=(33, 9), base=0),
    _gen("mask-min-1e4", 12, 40, 64, pad="f32", lens=(40, 25), causal=True, mask_min=-1.0e4),
    _gen("mask-min-100", 12, 40, 64, pad="f32", lens=(40, 25), causal=True, mask_min=-100.0, base=0),
    # seq_bound: 4.35 err64 at ONE element of the unmasked sample, 4 err64 missed by 5e-8.  The kernel's q k^T is one fma chain over D = 48
    # terms (partial sums up to 18.5) where the oracle's matmul sums in blocks: that chain alone, restated in numpy with everything after
    # it in float64, puts 6.0e-7 on this very element (measured 6.6e-7; the oracle 5.5e-8).  Bounded by the running-error bound instead.
    _gen("masked-sample-vanilla", 5, 20, 48, pad="f32", lens=(20, 0), clamp_min=True, base=0, seq_bound=True),
    _gen("masked-sample-softmax1", 5, 20, 48, pad="f32", lens=(20, 0), clamp_min=True),
    _gen("gamma-pos-513", 3, 513, 64, base=0, clip=(0.05, 1.0)),
    _gen("clipped-softmax1-bf16", 5, 45, 144, storage="bf16", clip=(-0.025, 1.1)),
    _gen("neg-scale-700", 3, 700, 64, scale=-0.125),
    _gen("lds-edge", 1, 16376, 8, B=1, H=2),  # D + Sk = 16384: all 64 KiB of dynamic LDS
    _gen("gate-token", 7, 33, 48, gate="token", storage="fp16"),
    _gen("gate-head", 7, 33, 144, gate="head", base=0),
    # quantisers
    _gen("q-scores", 12, 64, 48, gs=S8, dumps=True),
    _gen("q-probs-4bit", 12, 5, 64, gp=(0.0, 1.0, 4), dumps=True, base=0),
    _gen("q-ctx-before-gate", 12, 33, 48, gc=C8, gate="token", dumps=True),
    _gen("q-ctx-after-gate-emit", 12, 33, 144, gc=C8, gate="head", before=False, emit=True, dumps=True, storage="fp16"),
    _gen("q-scores-probs", 12, 129, 144, gs=S8, gp=P8, dumps=True, base=0),
    _gen("q-all-three", 12, 45, 64, gs=S8, gp=P8, gc=C8, dumps=True, storage="fp16", causal=True),
    _gen("q-all-three-bf16-4bit", 12, 17, 80, gs=(-4.0, 4.0, 4), gp=P8, gc=(-2.0, 2.0, 4), dumps=True, storage="bf16", before=False, gate="token"),
    _gen("q-saturating", 12, 64, 48, gs=(-1.0, 1.0, 8), gp=(0.0, 0.05, 8), gc=(-0.25, 0.25, 8), dumps=True),
    _gen("q-probs-12bit", 12, 5, 64, gs=S8, gp=(0.0, 1.0, 12)),
    _gen("q-long-peaked", 12, 700, 64, H=1, gs=(-256.0, 254.0, 8), gp=P8, gc=C8, dumps=True, qmul=8.0),
)


def _routes():
    """Part 4: what fast_can (csrc/oeh_api.hip) refuses, at D = 64 in fp16 and fp32 storage, once at 80 keys (general kernel) and once at
    513 (any-shape kernel).  Two rows follow the code where the issue's table generalises: a (B,1,Sq,Sk) mask on long rows belongs to the
    one-pass kernel, and a probability grid of more than 2047 levels is refused by the general kernel too (its integer-valued fp16
    probability operand would not be exact): the any-shape kernel at both lengths."""
    kinds = (
        ("gamma-pos", dict(clip=(0.05, 1.0))),
        ("neg-scale", dict(scale=-0.125, base=0)),
        ("mask-min-1e4", dict(causal=True, pad="f32", mask_min=-1.0e4)),
        ("causal-tall", dict(causal=True, clamp_min=True)),
        ("full-mask", dict(full="f32", base=0)),
        ("q-scores-only", dict(gs=S8)),
        ("q-probs-only", dict(gp=P8, base=0)),
        ("q-probs-ctx", dict(gp=P8, gc=C8)),
        ("q-dumps", dict(gs=S8, gp=P8, dumps=True)),
        ("q-div3", dict(gs=S8, gp=P8, scale_div=3.0, qmul=0.375)),
        ("q-probs-12bit", dict(gs=S8, gp=(0.0, 1.0, 12))),
    )
    out = []
    for (kind, kw), st, long in itertools.product(kinds, ("fp16", "fp32"), (False, True)):
        Sk = 513 if long else 80
        kw = dict(kw, storage=st)
        Sq = 12
        if kind == "causal-tall":
            Sq, kw["B"], kw["H"] = Sk + 2, 1, (1 if long else 2)
        if kw.get("pad"):
            kw["lens"] = (Sk, Sk // 2)
        quant = any(kw.get(g) for g in ("gs", "gp", "gc"))
        if long and quant:  # peaked rows (few probabilities off zero) and a coarser score grid: the issue's long-row form
            kw["qmul"] = kw.get("qmul", 1.0) * 8.0
            if kw.get("gs"):
                kw["gs"] = (-256.0, 254.0, 8)
        if kind == "full-mask" and long:
            kernel = f"flash16/MQ1/D64/{DT_NAME[st]}"
        elif long or kind == "q-probs-12bit":
            kernel = "generic"
        else:
            kernel = f"mfma16/NT8/D64/{DT_NAME[st]}" + ("/fq" if quant else "")
        out.append(_c(f"route-{kind}-{st}-{Sk}", Sq, Sk, 64, kernel=kernel, **kw))
    return tuple(out)


ROUTE_CASES = _routes()


def grid(c, key):
    return None if c[key] is None else R.grid_from_range(c[key][0], c[key][1], c[key][2])


def low_of(c, dtype16: bool):
    """The value a mask holds for a hidden key: mask_min, or finfo(float16).min in a float16 mask when mask_min lies below it."""
    return max(c["mask_min"], R.FMIN16) if dtype16 else c["mask_min"]


def inputs(c):
    """dict(q, k, v: float32 arrays of values of the storage type; pad: (B,Sk) in the dtype the library is to read; full: (B,1,Sq,Sk)
    likewise; gate: float32, (B,H,Sq,1) or (1,H,1,1)).  With gate_units: hidden (B,Sq,H D) in the storage type, the predictor's float32 weights
    w1, b1, w2, b2 (ops.gate_fwd's layout), gate64 - the predictor in float64, (B,H,Sq,1), without gate_scaling - and gate: gate64 times
    gate_scaling, which the chain applies until a kernel has written its own (GatePredictor.out)."""
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    seed = R._seed("attn", c["name"])
    rs = np.random.RandomState(seed)
    q = (rs.standard_normal((B, H, Sq, D)) * c["qmul"]).astype(np.float32)
    k, v = rs.standard_normal((B, H, Sk, D)).astype(np.float32), rs.standard_normal((B, H, Sk, D)).astype(np.float32)
    if c["shift"] is not None:  # head dim 0 carries the constant: q0 * 1 * scale = shift
        eff = 1.0 / c["scale_div"] if c["scale_div"] != 0.0 else c["scale"]
        q[..., 0], k[..., 0] = c["shift"] / eff, 1.0
    if c["ramp"] is not None:  # head dim 1 carries the ramp: 1 * k1 * scale = ramp (j - Sk)
        eff = 1.0 / c["scale_div"] if c["scale_div"] != 0.0 else c["scale"]
        q[..., 1], k[..., 1] = 1.0, ((np.arange(Sk) - Sk) * (c["ramp"] / eff)).astype(np.float32)[None, None, :]
    x = dict(q=R.round_storage(q, c["storage"]), k=R.round_storage(k, c["storage"]), v=R.round_storage(v, c["storage"]), pad=None, full=None, gate=None)
    if c["pad"] is not None:
        f16 = c["pad"] == "f16"
        x["pad"] = R.pad_vector(B, Sk, c["lens"], low_of(c, f16), np.float16 if f16 else np.float32)
    if c["full"] is not None:
        f16 = c["full"] == "f16"
        x["full"] = R.full_matrix(seed + 2, B, Sq, Sk, low_of(c, f16)).astype(np.float16 if f16 else np.float32)
    if c["gate"] is not None:
        x["gate"] = rs.rand(*((B, H, Sq, 1) if c["gate"] == "token" else (1, H, 1, 1))).astype(np.float32)
    if c["gate_units"] is not None:
        m = c["gate_units"]
        x["hidden"] = R.round_storage(rs.standard_normal((B, Sq, H * D)).astype(np.float32), c["storage"])
        x["w1"] = (rs.standard_normal((H, m, D) if m else (H, D)) * 0.2).astype(np.float32)
        x["b1"] = (rs.standard_normal((H, m) if m else (H,)) * 0.2).astype(np.float32)
        x["w2"] = (rs.standard_normal((H, m)) * 0.5).astype(np.float32) if m else None
        x["b2"] = rs.standard_normal((H,)).astype(np.float32) if m else None
        x["gate64"] = gate64(x["hidden"], H, x["w1"], x["b1"], x["w2"], x["b2"])
        x["gate"] = (x["gate64"] * gate_scaling(c)).astype(np.float32)
    return x


def gate_scaling(c) -> float:
    """gate_scaling of a case with the in-kernel predictor: 1 with the linear predictor, 2 with the hidden layer."""
    return 2.0 if c["gate_units"] else 1.0


def gate64(hidden, H, w1, b1, w2=None, b2=None):
    """The per-head gate predictor in float64 (oracle/oeh_oracle.py: gate_values, "linear" / "mlp"): (B,H,T,1) probabilities."""
    x = np.asarray(hidden, dtype=np.float64)
    B, T, E = x.shape
    xh = x.reshape(B, T, H, E // H).transpose(0, 2, 1, 3)
    if w2 is None:
        a = np.einsum("bhtd,hd->bht", xh, w1.astype(np.float64)) + b1.astype(np.float64)[None, :, None]
    else:
        h1 = np.maximum(np.einsum("bhtd,hmd->bhtm", xh, w1.astype(np.float64)) + b1.astype(np.float64)[None, :, None, :], 0.0)
        a = np.einsum("bhtm,hm->bht", h1, w2.astype(np.float64)) + b2.astype(np.float64)[None, :, None]
    return (1.0 / (1.0 + np.exp(-a)))[..., None]


def _f32(a):
    return None if a is None else np.asarray(a, dtype=np.float32)


def want64(c, x):
    return chain64(x["q"], x["k"], x["v"], gate=x["gate"], ctx_grid=grid(c, "gc"), ctx_before_gate=c["before"], ctx_emit_index=c["emit"],
                   scores_grid=grid(c, "gs"), probs_grid=grid(c, "gp"), scale=c["scale"], scale_div=c["scale_div"], pad=_f32(x["pad"]),
                   full=_f32(x["full"]), causal=c["causal"], clamp_min=c["clamp_min"], mask_min=c["mask_min"], base=c["base"], clip=c["clip"])


def oracle32(c, x, O, upto: int):
    """The fp32 oracle with the quantisers of the first `upto` stages (0: none, 1: scores, 2: + probabilities, 3: + context): dict(scores,
    probs: before their quantisers; ctx_pre; ctx: the output, integers under ctx_emit_index)."""
    def og(key, on):
        g = grid(c, key) if on else None
        return None if g is None else (g[0], g[1], c[key][2])
    kw = dict(base=c["base"], pad_mask=_f32(x["pad"]), full_mask=_f32(x["full"]), causal=c["causal"], clamp_min=c["clamp_min"], mask_min=c["mask_min"],
              gate=x["gate"], ctx_quant_before_gate=c["before"], fq_scores=og("gs", upto >= 1), fq_probs=og("gp", upto >= 2), fq_ctx=og("gc", upto >= 3))
    if c["clip"] is not None:
        kw.update(gamma=c["clip"][0], eta=c["clip"][1], clip=True)
    if c["scale_div"] != 0.0:
        kw.update(scale=c["scale_div"], scale_is_divisor=True)
    else:
        kw.update(scale=c["scale"])
    ctx, o = O.attn_core(x["q"], x["k"], x["v"], want=("scores", "probs", "ctx_prequant", "ctx_idx"), **kw)
    pre = o.get("ctx_prequant", ctx)
    if "ctx_idx" in o and c["emit"]:
        ctx = o["ctx_idx"].astype(np.float32) - np.float32(grid(c, "gc")[1])
    return dict(scores=o["scores"], probs=o["probs"], ctx_pre=pre, ctx=ctx)


_REFS = {}


def refs(c, O):
    """Everything the checks of a case need, computed once per process: x (inputs), w (float64 chain), the oracle's distance per stage
    (e_scores, e_probs, e_pre, e_out - each over the rows / elements the stage's check covers), the tie bands (band_s, band_p: (B,H,Sq,Sk);
    band_c: (B,H,Sq,D)) and the rows left out downstream of them (rows_s: of the probability checks; rows_p: of the context checks)."""
    if c["name"] in _REFS:
        return _REFS[c["name"]]
    x = inputs(c)
    w = want64(c, x)
    gs, gp, gc = grid(c, "gs"), grid(c, "gp"), grid(c, "gc")
    o0 = oracle32(c, x, O, 0)
    e_s = R.err64(o0["scores"], w["scores"])
    band_s = R.tie_band(w["scores"], *gs, e_s, FACTOR) if gs else np.zeros(w["scores"].shape, dtype=bool)
    rows_s = band_s.any(axis=-1)
    o1 = oracle32(c, x, O, 1) if gs else o0
    e_p = R.err64(o1["probs"][~rows_s], w["probs"][~rows_s])
    band_p = (R.tie_band(w["probs"], *gp, e_p, FACTOR) & ~rows_s[..., None]) if gp else np.zeros(w["probs"].shape, dtype=bool)
    rows_p = rows_s | band_p.any(axis=-1)
    o3 = oracle32(c, x, O, 3) if (gs or gp or gc) else o0
    e_pre = R.err64(o3["ctx_pre"][~rows_p], w["ctx_pre"][~rows_p])
    band_c = (R.tie_band(w["ctx_pre"], *gc, e_pre, FACTOR) & ~rows_p[..., None]) if gc else np.zeros(w["ctx"].shape, dtype=bool)
    clean = ~rows_p[..., None] & ~band_c
    e_out = R.err64(o3["ctx"][clean], w["ctx"][clean])
    r = dict(x=x, w=w, o=o3, e_scores=e_s, e_probs=e_p, e_pre=e_pre, e_out=e_out, band_s=band_s, band_p=band_p, band_c=band_c, rows_s=rows_s,
             rows_p=rows_p, grids=(gs, gp, gc))
    _REFS[c["name"]] = r
    return r


def conditions(c, r):
    """The issue's conditions on a quantiser case, on the references alone; returns the shares."""
    shares = dict(band_s=float(r["band_s"].mean()), band_p=float(r["band_p"].mean()), band_c=float(r["band_c"].mean()), rows=float(r["rows_p"].mean()))
    assert max(shares["band_s"], shares["band_p"], shares["band_c"]) <= MAX_BAND_ELEMENTS, (c["name"], shares)
    assert shares["rows"] <= MAX_LEFT_OUT_ROWS, (c["name"], shares)
    if c["dumps"]:
        if c["gs"]:
            assert len(np.unique(r["w"]["scores_idx"])) >= 8, c["name"]
        if c["gp"]:
            assert len(np.unique(r["w"]["probs_idx"])) >= 3, c["name"]
    return shares


def _ratio(diff, unit):
    """max of diff / unit over an array; 0 / 0 counts as 0, x / 0 as inf."""
    if diff.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(diff == 0, 0.0, diff / unit)
    return float(np.max(q))


def _check_indices(c, what, got, want, band, rows_out):
    """Outside the band equal, inside within one; rows_out are not looked at."""
    got, keep = got.astype(np.float64), ~rows_out[..., None]
    d = np.abs(got - want)
    assert not (d[keep & ~band] != 0).any(), (c["name"], what, "index off outside the tie band", int((d[keep & ~band] != 0).sum()), float(d[keep & ~band].max()))
    assert not (d[keep & band] > 1).any(), (c["name"], what, "index more than one off inside the tie band")


def check_exact(c, r, got, dumps=None):
    """The exact kernels' acceptance (module docstring).  got: the output as float64; dumps: dict(scores, probs, ctx) of uint8 arrays.
    c["seq_bound"]: the issue's fallback for a case whose only difference from the oracle is a longer sequential sum - the output is bounded
    by the running-error bound gamma_n sum |p| |v| (n = max(D, Sk), the longer of the kernel's two fma chains; u = 2^-24; times |gate|)
    instead of 4 err64.  Returns the largest
    |got - want64| / err64 over the checked elements (inf where err64 is 0 and got differs by more than the storage rounding)."""
    w, (gs, gp, gc) = r["w"], r["grids"]
    zero = np.zeros(r["rows_s"].shape, dtype=bool)
    if dumps:
        if gs:
            _check_indices(c, "scores", dumps["scores"], w["scores_idx"], r["band_s"], zero)
        if gp:
            _check_indices(c, "probs", dumps["probs"], w["probs_idx"], r["band_p"], r["rows_s"])
        if gc:
            _check_indices(c, "ctx", dumps["ctx"], w["ctx_idx"], r["band_c"], r["rows_p"])
    assert np.isfinite(got).all(), (c["name"], "non-finite output")
    keep = ~r["rows_p"][..., None] & np.ones(got.shape, dtype=bool)
    diff = np.abs(got - w["ctx"])
    store = half_ulp(w["ctx"], c["storage"])
    arith = FACTOR * r["e_out"]
    if c["seq_bound"]:
        n = max(c["D"], c["Sk"])
        gam = n * U / (1.0 - n * U)
        g = 1.0 if r["x"]["gate"] is None else np.abs(r["x"]["gate"].astype(np.float64))
        arith = gam * np.matmul(np.abs(w["probs_q"]), np.abs(r["x"]["v"].astype(np.float64))) * g
    lim = arith + store
    if gc:  # inside the context quantiser's band: either neighbouring grid point
        step = (1.0 if c["emit"] else gc[0]) * (1.0 if (r["x"]["gate"] is None or not c["before"]) else np.abs(r["x"]["gate"].astype(np.float64)))
        lim = lim + np.where(r["band_c"], step, 0.0) * (1.0 + 2.0 ** -R.MANT_BITS[c["storage"]])
    bad = keep & (diff > lim)
    clean = keep & ~r["band_c"]
    ratio = _ratio(np.maximum(diff - store, 0.0)[clean], r["e_out"])
    assert not bad.any(), (c["name"], "output", int(bad.sum()), "worst |got - want64|", float(diff[keep].max()), "err64", r["e_out"], "ratio", ratio)
    return ratio


def contract_limit(want, storage: str, gate_scale: float = 1.0):
    """gate_scale: gate_scaling of the in-kernel predictor, which multiplies the output - the arithmetic (absolute) term scales with it, as
    tests/test_attn_gpu.py: test_gate_predictor_fused_in_kernel writes it."""
    a, rel = CONTRACT[storage]
    return a * gate_scale + rel * np.abs(want) + (half_ulp(want, "fp16") if storage == "fp16" else 0.0)


def limit_of(c, r):
    """The limit on |got - want64| of a case of the matrix-core kernels: the contract - or, with the probability pairs, the bound
    tests/test_attn_pv_pairs_gpu.py applies (4 x the fp32 oracle's own distance from float64 + 2^-20 max(1, |V|max))."""
    if c["pv_pairs"]:
        return np.full(r["w"]["ctx"].shape, 4.0 * r["e_out"] + 2.0 ** -20 * max(1.0, float(np.abs(r["x"]["v"]).max())))
    return contract_limit(r["w"]["ctx"], c["storage"], gate_scaling(c) if c["gate_units"] is not None else 1.0)


def check_contract_long(c, r, got, dumps):
    """Quantised rows of more than 512 keys, where no kernel with fp16 operands writes dumps: `dumps` are the any-shape kernel's, held to
    check_exact's statement; rows that hold an element inside a tie band or an index that differs from float64 are left out of the output
    check (at most MAX_LEFT_OUT_ROWS of them), as are such elements of the context; the others meet the contract.  Returns the largest
    |got - want64| / limit."""
    w, (gs, gp, gc) = r["w"], r["grids"]
    zero = np.zeros(r["rows_s"].shape, dtype=bool)
    rows = r["rows_p"].copy()
    out_c = r["band_c"].copy()
    for key, g, band, up in (("scores", gs, r["band_s"], zero), ("probs", gp, r["band_p"], r["rows_s"]), ("ctx", gc, r["band_c"], r["rows_p"])):
        if not g:
            continue
        _check_indices(c, key, dumps[key], w[key + "_idx"], band, up)
        differs = dumps[key].astype(np.float64) != w[key + "_idx"]
        if key == "ctx":
            out_c |= differs
        else:
            rows |= (band | differs).any(axis=-1)
    assert rows.mean() <= MAX_LEFT_OUT_ROWS, (c["name"], "rows left out", float(rows.mean()))
    assert np.isfinite(got).all(), (c["name"], "non-finite output")
    keep = ~rows[..., None] & ~out_c
    q = np.abs(got - w["ctx"]) / limit_of(c, r)
    assert not (q[keep] > 1.0).any(), (c["name"], "output", int((q[keep] > 1.0).sum()), float(q[keep].max()))
    return float(q[keep].max())


def check_contract(c, r, got, dumps=None, leave_out=None):
    """The general / one-pass kernels' acceptance (module docstring).  Quantised cases come with the dumps of a second, bitwise equal run.
    leave_out: elements of the output that the dumps do not speak for (where the run that wrote them differs from `got`).
    Returns the largest |got - want64| / limit over the checked elements."""
    w, (gs, gp, gc) = r["w"], r["grids"]
    assert np.isfinite(got).all(), (c["name"], "non-finite output")
    rows = np.zeros(got.shape[:3], dtype=bool)
    flip_c = np.zeros(got.shape, dtype=bool)
    if gs or gp or gc:
        assert dumps is not None, c["name"]
        for key, g in (("scores", gs), ("probs", gp), ("ctx", gc)):
            if not g:
                continue
            d = np.abs(dumps[key].astype(np.float64) - w[key + "_idx"])
            if key != "scores":
                d = np.where(rows[..., None], 0.0, d)  # (downstream of a flip: nothing to compare)
            assert d.max() <= 1, (c["name"], key, "index more than one off", float(d.max()))
            assert (d != 0).sum() <= max(FLIP_SHARE * d.size, 2.0), (c["name"], key, "flips", int((d != 0).sum()), d.size)
            if key == "ctx":
                flip_c = d != 0
            else:
                rows |= (d != 0).any(axis=-1)
    keep = ~rows[..., None] & ~flip_c
    if leave_out is not None:
        keep = keep & ~leave_out
    q = np.abs(got - w["ctx"]) / limit_of(c, r)
    assert not (q[keep] > 1.0).any(), (c["name"], "output", int((q[keep] > 1.0).sum()), float(q[keep].max()))
    return float(q[keep].max())


# ---- posing a case to the library ---------------------------------------------------------------------------------------------
GUARD = 7.0


def pose(ops, torch, c, x, with_dumps=None, info=None):
    """Run case c on inputs x through ops.attn_fwd under its hook mask (and flash_mq_force).  Returns (variant name of the real descriptor,
    output as a float64 array, dumps or None).  Layouts: "contig"; "blhe" - (B,L,H,E) tensors viewed (B,H,L,E); "longkv" - k and v are the
    first Sk rows of a longer buffer whose other rows are NaN;
    "outslice" - the caller's `out` is the inside of a larger tensor that must keep its other
    elements; "off4" - rows of q, k, v and out start 4 elements into rows of D + 4 (8-byte, not 16-byte aligned in 16-bit storage);
    "fused" - q, k and v are the three slots of one (B,S,3 H D) tensor; "qslice" - q is the first Sq rows of a buffer of Sk rows (NaN beyond):
    q, k and v then have the same three strides.  info: a dict that receives desc / fqd (the real descriptors), raw (the output tensor as the
    library wrote it, on the host), gate_out (what the in-kernel predictor wrote, (B,H,Sq)) and hot (how many launches took the hot argument
    prefix)."""
    from outeffhop_amd import _lib

    DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    dt = DT[c["storage"]]
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    lay = c["layout"]

    def dev(a, dtype=None):
        t = torch.from_numpy(np.ascontiguousarray(a))
        return (t if dtype is None else t.to(dtype)).cuda()

    def heads(a, slot):
        S = a.shape[2]
        if lay == "blhe":
            return dev(a.transpose(0, 2, 1, 3), dt).permute(0, 2, 1, 3)
        if lay == "longkv" and slot > 0:
            buf = torch.full((B, H, S + 5, D), float("nan"), dtype=dt, device="cuda")
            buf[:, :, :S] = dev(a, dt)
            return buf[:, :, :S]
        if lay == "qslice" and slot == 0:
            buf = torch.full((B, H, Sk, D), float("nan"), dtype=dt, device="cuda")
            buf[:, :, :S] = dev(a, dt)
            return buf[:, :, :S]
        if lay == "off4":
            buf = torch.full((B, H, S, D + 4), float("nan"), dtype=dt, device="cuda")
            buf[..., 4:] = dev(a, dt)
            t = buf[..., 4:]
            assert t.data_ptr() % 8 == 0 and (dt == torch.float32 or t.data_ptr() % 16 == 8)
            return t
        return dev(a, dt)

    if lay == "fused":
        assert Sq == Sk
        fused = torch.cat([dev(x[n].transpose(0, 2, 1, 3).reshape(B, Sq, H * D), dt) for n in ("q", "k", "v")], dim=2)
        tq, tk, tv = [fused[:, :, i * H * D:(i + 1) * H * D].view(B, Sq, H, D).permute(0, 2, 1, 3) for i in range(3)]
        assert tq.stride(2) == 3 * H * D
    else:
        tq, tk, tv = heads(x["q"], 0), heads(x["k"], 1), heads(x["v"], 2)
    out, big = None, None
    odt = torch.float32 if c["out32"] else dt
    if lay == "outslice":
        big = torch.full((B, H, Sq + 2, D + 8), GUARD, dtype=dt, device="cuda")
        out = big[:, :, 1:Sq + 1, 4:D + 4]
    elif lay == "off4":
        big = torch.full((B, H, Sq, D + 4), GUARD, dtype=dt, device="cuda")
        out = big[..., 4:]
    sm = ops.SoftmaxSpec(base=c["base"]) if c["clip"] is None else ops.SoftmaxSpec(base=c["base"], clip=True, gamma=c["clip"][0], eta=c["clip"][1])
    kw = dict(softmax=sm, scale=c["scale"], scale_div=c["scale_div"], causal=c["causal"], clamp_min=c["clamp_min"], mask_min=c["mask_min"], out=out)
    if c["out32"]:
        kw["out_dtype"] = torch.float32
    if c["pv_pairs"]:
        kw["pv_pairs"] = True
    if x["pad"] is not None:
        kw["key_pad_mask"] = dev(x["pad"])
        kw["key_pad_boolean"] = c["pad_bool"]
    gate_out = None
    if c["gate_units"] is not None:
        gate_out = torch.full((B, H, Sq), float("nan"), dtype=torch.float32, device="cuda")
        w = {n: None if x[n] is None else dev(x[n]) for n in ("w1", "b1", "w2", "b2")}
        kw["gate_mlp"] = ops.GatePredictor(dev(x["hidden"], dt), w["w1"], w["b1"], w["w2"], w["b2"], scaling=gate_scaling(c), out=gate_out)
    if x["full"] is not None:
        if c["full"] == "strided":  # rows of a wider allocation, read in place through the row stride
            wide = torch.full((B, 1, Sq, Sk + 8), GUARD, device="cuda")
            wide[..., :Sk] = dev(x["full"])
            kw["full_mask"] = wide[..., :Sk]
            assert not kw["full_mask"].is_contiguous()
        else:
            kw["full_mask"] = dev(x["full"])
    if x["gate"] is not None and c["gate_units"] is None:
        kw["gate"] = dev(x["gate"])
    dumps = None
    if c["gs"] or c["gp"] or c["gc"]:
        want_dumps = c["dumps"] if with_dumps is None else with_dumps
        dumps = {} if want_dumps else None

        def spec(key, shape):
            g = grid(c, key)
            if g is None:
                return None
            t = None
            if want_dumps:
                t = dumps[key] = torch.full(shape, 201, dtype=torch.uint8, device="cuda")
            return ops.FakeQuantSpec(g[0], g[1], g[2], dump=t)
        kw["fq"] = ops.AttnFakeQuant(scores=spec("gs", (B, H, Sq, Sk)), probs=spec("gp", (B, H, Sq, Sk)), ctx=spec("gc", (B, H, Sq, D)),
                                     ctx_before_gate=c["before"], ctx_emit_index=c["emit"])
    lib = _lib.load()
    assert lib.oeh_debug_set_variant(c["hook"], c["mq"]) == 0
    try:
        box = []
        res = ops.attn_fwd(tq, tk, tv, _prepared=box, **kw)  # (builds the descriptor, launches nothing)
        fn, args, keep = box
        d, fqd = keep[0], keep[1]
        if c["pv_pairs"]:
            name = lib.oeh_attn_variant_ex(ctypes.byref(d), ctypes.byref(_lib.oeh_attn_opts(pv_pairs=1)), None if fqd is None else ctypes.byref(fqd))
        else:
            name = lib.oeh_attn_variant(ctypes.byref(d), None if fqd is None else ctypes.byref(fqd))
        name = None if name is None else name.decode()
        lib.oeh_debug_hot_launches.restype = ctypes.c_long
        hot0 = lib.oeh_debug_hot_launches()
        if c["via"] == "prepared":
            _lib.check(fn(*args, ops._stream()), "oeh_attn_fwd")
        else:
            res = ops.attn_fwd(tq, tk, tv, **kw)
        torch.cuda.synchronize()
        hot = lib.oeh_debug_hot_launches() - hot0
    finally:
        lib.oeh_debug_set_variant(0, 0)
    assert res.shape == (B, H, Sq, D) and res.dtype == odt
    if big is not None:  # nothing around the caller's view was written
        inside = torch.zeros(big.shape, dtype=torch.bool, device="cuda")
        if lay == "outslice":
            inside[:, :, 1:Sq + 1, 4:D + 4] = True
        else:
            inside[..., 4:] = True
        assert bool((big[~inside] == GUARD).all()), (c["name"], "the kernel wrote outside the caller's out")
    got = res.float().cpu().numpy().astype(np.float64)
    if info is not None:
        info.update(desc=d, fqd=fqd, raw=res.cpu(), hot=hot, gate_out=None if gate_out is None else gate_out.cpu().numpy().astype(np.float64))
    if dumps is not None:
        dumps = {{"gs": "scores", "gp": "probs", "gc": "ctx"}[k]: t.cpu().numpy() for k, t in dumps.items()}
    return name, got, dumps
