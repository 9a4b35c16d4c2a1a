"""GPU parity tests proper: the HIP path (through the C ABI, outeffhop_amd.ops) against the CPU oracle on the
same seeded inputs, and against golden fixtures captured from the reference.  Run with `-m gpu` on an MI355X.

Tolerances (written here once):
  * 16-bit storage (fp16) - north_star's "within 1e-3 fp16", ONE statement, no relative term: the oracle is the reference
    arithmetic in fp32 on the fp16-rounded inputs; the kernel's arithmetic (fp16 operands, fp32 accumulation)
    is within 1e-3 absolute of it, and storing the result in fp16 adds at most half an fp16 ulp of the reference value:
        |hip - oracle| <= 1e-3 + ulp16(oracle) / 2                      (`_check`, `_check_fp16_contract`)
    (4.9e-4 for 1 <= |oracle| < 2).  Where a gate scaling factor s > 1 multiplies the output, the arithmetic part scales
    with it: s * 1e-3 + ulp16 / 2, written at the call.
  * bf16 storage: 2e-2 (8-bit significand of the probability operand).  fp32 storage: 5e-4.
  * fake-quant indices: bit-exact at the quantiser boundary (same fp32 input -> same index, test_rows_gpu.py);
    end to end, index flips vs the oracle come only from fp32 summation order / 1-ulp exp differences:
    flips must be +-1 and rarer than 2e-3 per tensor, and outside flipped elements outputs agree to 1e-3.
"""
import math
import os

import numpy as np
import pytest

from oracle import oeh_oracle as O
from tests.conftest import load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FLIP_RATE = 1e-4   # share of a fused quantiser's indices that may sit one step from the oracle's (measured <= 4e-6 at full size; round 4: 2e-3)
OUT_OFF = 2e-4     # share of outputs that may sit one context-grid step off (round 4: 4e-3)
F16_TOL = None  # fp16 storage: the contract above (1e-3 + half an fp16 ulp of the reference), see `_check`
BF16_TOL = dict(atol=2e-2, rtol=2e-2)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _rand(shape, seed, scale=1.0, dtype=torch.float16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _np32(t):
    return t.detach().float().cpu().numpy()


def _le(value, limit, what, n=None):
    """`value <= limit` with the margin on record: OEH_TEST_REPORT=<file> appends "what value limit" per call - how the shares below were
    set in round 5 (bounds ~500x looser than what the kernels deliver let a 0.1 % regression pass): measured on the
    GPU box, then a bound a small factor above the measurement, never below one element of the smallest tensor."""
    if n is not None:  # a share of n elements: two of them may always differ (a tensor of 1 152 outputs has no share below 8.7e-4)
        limit = max(float(limit), 2.0 / float(n))
    rep = os.environ.get("OEH_TEST_REPORT")
    if rep:
        with open(rep, "a") as f:
            f.write(f"{what}\t{float(value):.3e}\t{float(limit):.3e}\n")
    return float(value) <= float(limit)


def _lib_of(ops):
    from outeffhop_amd import _lib

    return _lib.load()


def _f16_limit(want, arith=1e-3):
    """arith + half an fp16 ulp of the reference value (the rounding of the stored output)"""
    return np.float32(arith) + 0.5 * np.spacing(np.abs(want).astype(np.float16)).astype(np.float32)


def _check(got, want, tol=F16_TOL, msg="", arith=1e-3):
    """tol None: the fp16 contract (arith = 1e-3 unless a gate scaling factor multiplies the output); else atol + rtol |want|
    (bf16 / fp32 storage)."""
    got = _np32(got) if hasattr(got, "detach") else got
    err = np.abs(got - want)
    lim = _f16_limit(want, arith) if tol is None else tol["atol"] + tol["rtol"] * np.abs(want)
    assert np.isfinite(got).all(), f"{msg}: non-finite output"
    worst = float((err - lim).max())
    _le(float((err / lim).max()), 1.0, f"_check[{msg}]")
    assert worst <= 0, f"{msg}: max abs err {err.max():.3e} (limit exceeded by {worst:.3e}) at {np.unravel_index((err - lim).argmax(), err.shape)}"


SPECS = {
    "softmax1": dict(base=1, gamma=0.0, eta=1.0, clip=False),
    "vanilla": dict(base=0, gamma=0.0, eta=1.0, clip=False),
    "clippedsoftmax1(-.025:1)": dict(base=1, gamma=-0.025, eta=1.1, clip=True),
    "clipped(-.003:1.003)": dict(base=0, gamma=-0.003, eta=1.003, clip=True),
}


def _spec(ops, name):
    s = SPECS[name]
    return ops.SoftmaxSpec(base=s["base"], clip=s["clip"], gamma=s["gamma"], eta=s["eta"])


def _pad_mask(B, S, lengths, fmin):
    m = np.zeros((B, S), dtype=np.float32)
    for b, L in enumerate(lengths):
        m[b, L:] = fmin
    return m


@pytest.mark.parametrize("S,D", [(80, 64), (128, 64), (160, 64), (200, 32), (512, 64), (384, 128), (33, 32)])
@pytest.mark.parametrize("sm", list(SPECS))
def test_core_nomask(ops, S, D, sm):
    B, H = 2, 3
    q, k, v = _rand((B, H, S, D), 1, 1.0), _rand((B, H, S, D), 2, 1.0), _rand((B, H, S, D), 3, 1.0)
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=1.0 / math.sqrt(D), **SPECS[sm])
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm), scale=1.0 / math.sqrt(D))
    assert got.shape == (B, H, S, D) and got.permute(0, 2, 1, 3).is_contiguous()
    _check(got, want, msg=f"S={S} D={D} {sm}")


@pytest.mark.parametrize("sm", ["softmax1", "clippedsoftmax1(-.025:1)", "vanilla"])
def test_bert_order_padmask_strided(ops, sm):
    """BERT: (B,S,E) projections viewed as (B,H,S,d) by a permute (no copy), scores / sqrt(d), (B,1,1,S) mask."""
    B, H, S, D = 4, 12, 128, 64
    fmin = float(np.finfo(np.float32).min)
    q3, k3, v3 = _rand((B, S, H * D), 11), _rand((B, S, H * D), 12), _rand((B, S, H * D), 13)
    pad = _pad_mask(B, S, [128, 97, 64, 1], fmin)
    view = lambda t: t.view(B, S, H, D).permute(0, 2, 1, 3)  # noqa: E731
    want = O.attn_core(_np32(view(q3)), _np32(view(k3)), _np32(view(v3)), scale=8.0, scale_is_divisor=True, pad_mask=pad, **SPECS[sm])
    mask4 = torch.from_numpy(pad).view(B, 1, 1, S).cuda()
    got = ops.attn_fwd(view(q3.cuda()), view(k3.cuda()), view(v3.cuda()), softmax=_spec(ops, sm), scale_div=8.0,
                       key_pad_mask=mask4, mask_min=fmin)
    _check(got, want, msg=sm)
    merged = got.permute(0, 2, 1, 3).reshape(B, S, H * D)
    assert merged.data_ptr() == got.data_ptr()  # head merge is free


@pytest.mark.parametrize("S", [64, 160, 512])
@pytest.mark.parametrize("sm", ["softmax1", "clippedsoftmax1(-.025:1)", "vanilla"])
def test_opt_order_causal(ops, S, sm):
    """OPT: q pre-scaled and re-rounded to fp16, causal (+ right padding) mask, clamp to finfo.min."""
    B, H, D = 2, 4, 64
    fmin = float(np.finfo(np.float32).min)
    q = (_rand((B, H, S, D), 21).float() * D ** -0.5).half()
    k, v = _rand((B, H, S, D), 22), _rand((B, H, S, D), 23)
    lengths = [S, max(1, S - 37)]
    pad = _pad_mask(B, S, lengths, fmin)
    with np.errstate(over="ignore"):
        full = (O.causal_additive(S, S, fmin)[None, None] + pad[:, None, None, :]).astype(np.float32)  # may be -inf: clamped
    want = O.attn_core(_np32(q), _np32(k), _np32(v), full_mask=full, clamp_min=True, **SPECS[sm])
    # (a) analytic causal flag + key padding vector
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm), causal=True, clamp_min=True,
                       key_pad_mask=torch.from_numpy(pad).cuda(), mask_min=fmin)
    _check(got, want, msg=f"causal flag S={S} {sm}")
    # (b) the materialised (B,1,T,S) HF mask
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm), clamp_min=True,
                       full_mask=torch.from_numpy(full).cuda(), mask_min=fmin)
    _check(got, want, msg=f"full mask S={S} {sm}")
    # (c) pure causal, no padding: tile skipping path
    want = O.attn_core(_np32(q), _np32(k), _np32(v), causal=True, clamp_min=True, **SPECS[sm])
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=fmin)
    _check(got, want, msg=f"pure causal S={S} {sm}")


def test_fully_masked_rows(ops):
    """softmax1 zeroes a fully masked row, vanilla makes it uniform (SURVEY 7 hard part 3)."""
    B, H, S, D = 1, 2, 48, 64
    fmin = float(np.finfo(np.float32).min)
    q, k, v = _rand((B, H, S, D), 31), _rand((B, H, S, D), 32), _rand((B, H, S, D), 33)
    pad = np.full((B, S), fmin, dtype=np.float32)
    for sm in ("softmax1", "vanilla"):
        want = O.attn_core(_np32(q), _np32(k), _np32(v), pad_mask=pad, scale=0.125, **SPECS[sm])
        got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm), scale=0.125, key_pad_mask=torch.from_numpy(pad).cuda(), mask_min=fmin)
        _check(got, want, msg=sm)
        if sm == "softmax1":
            assert float(got.abs().max()) == 0.0


def test_cross_and_kv_cache_shapes(ops):
    """Sq != Sk: cross attention (no mask) and causal with a key/value cache offset."""
    B, H, D = 2, 2, 64
    fmin = float(np.finfo(np.float32).min)
    q, k, v = _rand((B, H, 40, D), 41), _rand((B, H, 200, D), 42), _rand((B, H, 200, D), 43)
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=0.125, **SPECS["softmax1"])
    _check(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), scale=0.125), want, msg="cross")
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=0.125, causal=True, clamp_min=True, **SPECS["softmax1"])
    _check(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), scale=0.125, causal=True, clamp_min=True, mask_min=fmin), want, msg="kv-cache causal")


def test_gate_epilogue(ops):
    B, H, S, D = 2, 3, 96, 64
    q, k, v = _rand((B, H, S, D), 51), _rand((B, H, S, D), 52), _rand((B, H, S, D), 53)
    g = torch.rand((B, H, S, 1), generator=torch.Generator().manual_seed(54))
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=0.125, gate=g.numpy(), **SPECS["softmax1"])
    _check(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), scale=0.125, gate=g.cuda()), want, msg="per token")
    gh = torch.rand((H, 1, 1), generator=torch.Generator().manual_seed(55))
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=0.125, gate=gh.numpy()[None], **SPECS["softmax1"])
    _check(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), scale=0.125, gate=gh.cuda()), want, msg="per head")


@pytest.mark.parametrize("dtype,tol", [(torch.float32, dict(atol=5e-4, rtol=5e-4)), (torch.bfloat16, dict(atol=2e-2, rtol=2e-2))])
def test_other_storage_dtypes(ops, dtype, tol):
    B, H, S, D = 2, 2, 144, 64
    q, k, v = _rand((B, H, S, D), 61, dtype=dtype), _rand((B, H, S, D), 62, dtype=dtype), _rand((B, H, S, D), 63, dtype=dtype)
    # fp32 storage: the oracle sees the fp32 values themselves (scores from fp16 operand PAIRS are fp32-accurate; what is left
    # is the probability operand's rounding to fp16, <= 2^-12 relative per key)
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=0.125, causal=True, clamp_min=True, **SPECS["clippedsoftmax1(-.025:1)"])
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, "clippedsoftmax1(-.025:1)"), scale=0.125, causal=True,
                       clamp_min=True, mask_min=float(np.finfo(np.float32).min))
    assert got.dtype == dtype
    _check(got, want, tol, msg=str(dtype))


@pytest.mark.filterwarnings("ignore:outeffhop_amd.*any-shape HIP kernel:RuntimeWarning")  # (deliberate: the test forces / poses shapes only that kernel takes)
def test_generic_kernel_shapes(ops):
    """Shapes outside the MFMA kernels (D = 160) run the any-shape HIP kernel; D = 16 with few rows has the small-shape kernel,
    clipped rows of more than 512 keys the two-pass kernel (16-bit and fp32 storage)."""
    for (B, H, Sq, Sk, D, dt, name) in [(3, 4, 7, 5, 16, torch.float16, "small/ST2/D16/f16"), (1, 2, 33, 33, 160, torch.float16, "generic"),
                                        (1, 1, 20, 700, 64, torch.float16, "flash16/MQ1/D64/f16/clip2p"), (1, 1, 20, 700, 64, torch.float32, "flash16/MQ1/D64/f32/clip2p")]:
        assert ops.attn_variant(B, H, Sq, Sk, D, dt, clip=True) == name
        q, k, v = _rand((B, H, Sq, D), 71, dtype=dt), _rand((B, H, Sk, D), 72, dtype=dt), _rand((B, H, Sk, D), 73, dtype=dt)
        want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=1 / math.sqrt(D), **SPECS["clippedsoftmax1(-.025:1)"])
        got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, "clippedsoftmax1(-.025:1)"), scale=1 / math.sqrt(D))
        _check(got, want, msg=f"{(B, H, Sq, Sk, D, dt)}")
    assert ops.attn_variant(16, 12, 512, 512, 64, clip=True) == "fast16/NT32/D64/f16/clip"
    assert ops.attn_variant(16, 12, 512, 512, 64) == "flash16/MQ2/D64/f16"


def test_reference_golden_core(ops):
    """Directly against outputs captured from the reference (fp32 math on fp16-rounded inputs)."""
    g = load_golden("core_attn.npz")
    q, k, v = (torch.from_numpy(g[n]).half().cuda() for n in ("q", "k", "v"))
    B = q.shape[0]
    fmin = float(np.finfo(np.float32).min)
    for sm in ("softmax1", "vanilla", "clippedsoftmax1(-.025:1)"):
        got = ops.attn_fwd(q, k, v, softmax=_spec(ops, sm), scale_div=8.0, key_pad_mask=torch.from_numpy(g["pad_mask"]).cuda().view(B, -1), mask_min=fmin)
        _check(got, g[f"bert[{sm}].ctx"], msg=f"bert {sm}")
        qs = (q.float() * 64 ** -0.5).half()
        got = ops.attn_fwd(qs, k, v, softmax=_spec(ops, sm), full_mask=torch.from_numpy(g["opt_mask"]).cuda(), clamp_min=True, mask_min=fmin)
        _check(got, g[f"opt[{sm}].ctx"], msg=f"opt {sm}")


def _flip_stats(got_idx, want_idx):
    d = np.abs(got_idx.astype(np.int32) - want_idx.astype(np.int32))
    return int(d.max()), float((d != 0).mean())


@pytest.mark.parametrize("order", ["opt", "bert"])
@pytest.mark.parametrize("sm", ["softmax1", "clippedsoftmax1(-.025:1)"])
@pytest.mark.parametrize("S", [96, 512])
def test_int8_fused(ops, order, sm, S):
    """The three activation quantisers fused into the kernel; index tensors dumped and compared."""
    B, H, D = 2, 2, 64
    fmin = float(np.finfo(np.float32).min)
    q, k, v = _rand((B, H, S, D), 81), _rand((B, H, S, D), 82), _rand((B, H, S, D), 83)
    if order == "opt":
        q = (q.float() * D ** -0.5).half()
    gate = torch.rand((B, H, S, 1), generator=torch.Generator().manual_seed(84))
    kw = dict(SPECS[sm])
    common = dict(causal=(order == "opt"), clamp_min=(order == "opt"), gate=gate.numpy(), **kw)
    if order == "bert":
        common.update(scale=8.0, scale_is_divisor=True)
    # calibrate the three ranges on the oracle's own FP intermediates (percentile 99.999 like validate_clm.py:450-454)
    _, fp = O.attn_core(_np32(q), _np32(k), _np32(v), want=("scores", "probs"), **common)
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    ctx_fp = O.attn_core(_np32(q), _np32(k), _np32(v), **{**common, "gate": None if order == "opt" else gate.numpy()})
    d_c = O.quant_range_to_params(*np.percentile(ctx_fp, (0.001, 99.999)))
    before = order == "opt"
    want, ex = O.attn_core(_np32(q), _np32(k), _np32(v), fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, ctx_quant_before_gate=before,
                           want=("scores_idx", "probs_idx", "ctx_idx"), **common)
    dump_s = torch.zeros((B, H, S, S), dtype=torch.uint8, device="cuda")
    dump_p = torch.zeros((B, H, S, S), dtype=torch.uint8, device="cuda")
    dump_c = torch.zeros((B, H, S, D), dtype=torch.uint8, device="cuda")
    FQ = ops.FakeQuantSpec.from_delta
    fq = ops.AttnFakeQuant(FQ(*d_s, dump=dump_s), FQ(*d_p, dump=dump_p), FQ(*d_c, dump=dump_c), ctx_before_gate=before)
    args = dict(softmax=_spec(ops, sm), causal=(order == "opt"), clamp_min=(order == "opt"), gate=gate.cuda(), mask_min=fmin)
    if order == "bert":
        args["scale_div"] = 8.0
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), fq=fq, **args)
    for name, dump in (("scores", dump_s), ("probs", dump_p), ("ctx", dump_c)):
        mx, rate = _flip_stats(dump.cpu().numpy(), ex[f"{name}_idx"])
        assert mx <= 1 and _le(rate, FLIP_RATE, f"int8_fused[{order},{sm},{S}] {name} flip rate", n=dump.numel()), f"{name}: max index diff {mx}, flip rate {rate:.2e}"
    step = float(np.float32(d_c[0])) * float(gate.max())
    err = np.abs(_np32(got) - want)
    flipped = err > 1e-3 + 1e-3 * np.abs(want)
    assert _le(flipped.mean(), OUT_OFF, f"int8_fused[{order},{sm},{S}] outputs off", n=flipped.size) and err.max() <= 1.05 * step + 2e-3, f"out: {flipped.mean():.2e} elements off, max err {err.max():.3e} (step {step:.3e})"
    # production form (no dumps -> causal tile skipping allowed) gives the same bits
    fq2 = ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c), ctx_before_gate=before)
    got2 = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), fq=fq2, **args)
    assert torch.equal(got, got2)
    # 16-bit storage runs the full-row kernel's FQ variant; the general kernel's FQ chain must give the same bits and indices
    from outeffhop_amd import _lib
    assert ops.attn_variant(B, H, S, S, D, fq=True).startswith("fast16/") and ops.attn_variant(B, H, S, S, D, fq=True).endswith("/fq")
    dumps2 = [torch.zeros_like(t) for t in (dump_s, dump_p, dump_c)]
    fq3 = ops.AttnFakeQuant(FQ(*d_s, dump=dumps2[0]), FQ(*d_p, dump=dumps2[1]), FQ(*d_c, dump=dumps2[2]), ctx_before_gate=before)
    _lib.load().oeh_debug_set_variant(4, 0)
    try:
        got3 = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), fq=fq3, **args)
    finally:
        _lib.load().oeh_debug_set_variant(0, 0)
    assert torch.equal(got, got3)
    for a, b_ in zip((dump_s, dump_p, dump_c), dumps2):
        assert torch.equal(a, b_)


def test_bit_reproducible_and_batch_shard_invariant(ops):
    """Same inputs -> same bits; a batch shard computes exactly the rows of the full batch."""
    B, H, S, D = 8, 12, 128, 64
    q, k, v = _rand((B, H, S, D), 91).cuda(), _rand((B, H, S, D), 92).cuda(), _rand((B, H, S, D), 93).cuda()
    a = ops.attn_fwd(q, k, v, scale=0.125)
    b = ops.attn_fwd(q, k, v, scale=0.125)
    assert torch.equal(a, b)
    for lo, hi in ((0, 4), (4, 8), (5, 6)):
        part = ops.attn_fwd(q[lo:hi], k[lo:hi], v[lo:hi], scale=0.125)
        assert torch.equal(part, a[lo:hi])


def test_full_size_properties(ops):
    """BASELINE sizes (OPT-125m B=16 H=12 S=512 d=64): size-independent properties instead of the O(S^2) oracle:
    (1) V = const c  =>  out = c * sum_j p_j, and for softmax1 sum_j p_j = 1 - 1/(1 + sum exp)  < 1;
    (2) linearity in V;  (3) causality: perturbing keys/values > i leaves row i bit-identical;
    plus (4) an oracle spot check on two (b,h) slices."""
    B, H, S, D = 16, 12, 512, 64
    fmin = float(np.finfo(np.float32).min)
    q = (_rand((B, H, S, D), 101).float() * 0.125).half().cuda()
    k, v = _rand((B, H, S, D), 102).cuda(), _rand((B, H, S, D), 103).cuda()
    kw = dict(causal=True, clamp_min=True, mask_min=fmin)
    out = ops.attn_fwd(q, k, v, **kw)
    ones = torch.ones_like(v)
    rowsum = ops.attn_fwd(q, k, ones, **kw).float()
    assert float(rowsum.max()) < 1.0 + 1e-3 and float(rowsum.min()) > 0.0
    assert float((rowsum - rowsum[..., :1]).abs().max()) <= 1e-3  # same for every d
    v2 = _rand((B, H, S, D), 104).cuda()
    lin = ops.attn_fwd(q, k, (v.float() + v2.float()).half(), **kw).float()
    sep = out.float() + ops.attn_fwd(q, k, v2, **kw).float()
    assert _le(float((lin - sep).abs().max()), 4e-3, "full_size linearity")
    k3, v3 = k.clone(), v.clone()
    k3[:, :, 300:] = 7.0
    v3[:, :, 300:] = -3.0
    out3 = ops.attn_fwd(q, k3, v3, **kw)
    assert torch.equal(out3[:, :, :300], out[:, :, :300])
    for (b, h) in ((0, 0), (15, 11)):
        want = O.attn_core(_np32(q[b:b + 1, h:h + 1]), _np32(k[b:b + 1, h:h + 1]), _np32(v[b:b + 1, h:h + 1]), causal=True, clamp_min=True)
        _check(out[b:b + 1, h:h + 1], want, msg=f"slice {(b, h)}")


@pytest.mark.parametrize("mq", [1, 2])
def test_one_pass_kernel_geometries(ops, mq):
    """The one-pass kernel (flash16) at both workgroup shapes, forced through the library's diagnostic hook: causal
    rows with even / odd / ragged 64-row slab counts, a key/value cache offset, rows longer than the full-row
    kernel's 512-key limit, left- and right-padded key masks (softmax_1), bf16, D in {32, 128}."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    fmin = float(np.finfo(np.float32).min)
    lib.oeh_debug_set_variant(256, mq)  # one-pass also for short rows; mq query blocks per wave
    try:
        cases = [  # (B, H, Sq, Sk, D, causal, softmax, pad?, dtype)
            (1, 2, 512, 512, 64, True, "softmax1", False, torch.float16),
            (1, 2, 320, 320, 64, True, "vanilla", False, torch.float16),   # 5 slabs: the last workgroup has one block
            (2, 1, 200, 200, 64, True, "softmax1", False, torch.float16),  # ragged last slab
            (1, 2, 192, 448, 64, True, "softmax1", False, torch.float16),  # kv-cache offset
            (1, 1, 70, 900, 64, False, "vanilla", False, torch.float16),   # Sk > 512, cross attention
            (1, 2, 130, 130, 32, True, "softmax1", False, torch.bfloat16),
            (1, 1, 150, 150, 128, True, "vanilla", False, torch.float16),
            (3, 2, 260, 260, 64, False, "softmax1", True, torch.float16),
        ]
        for n, (B, H, Sq, Sk, D, causal, sm, pad, dt) in enumerate(cases):
            assert ops.attn_variant(B, H, Sq, Sk, D, dt).startswith(f"flash16/MQ{mq}/")
            q = _rand((B, H, Sq, D), 900 + n, dtype=dt)
            k, v = _rand((B, H, Sk, D), 920 + n, dtype=dt), _rand((B, H, Sk, D), 940 + n, dtype=dt)
            padm = None
            if pad:
                padm = np.zeros((B, Sk), dtype=np.float32)
                padm[0, 200:] = fmin   # right padding
                padm[1, :70] = fmin    # left padding: the first 64-key tile is fully masked
                padm[2, :] = fmin      # everything masked: softmax_1 row must be exactly 0
            want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=D ** -0.5, causal=causal, clamp_min=causal, pad_mask=padm, **SPECS[sm])
            got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm), scale=D ** -0.5, causal=causal, clamp_min=causal,
                               key_pad_mask=None if padm is None else torch.from_numpy(padm).cuda(), mask_min=fmin)
            tol = F16_TOL if dt == torch.float16 else dict(atol=2e-2, rtol=2e-2)
            _check(got, want, tol=tol, msg=f"case {n} mq={mq}")
            if pad:
                assert float(got[2].abs().max()) == 0.0
    finally:
        lib.oeh_debug_set_variant(0, 0)


@pytest.mark.parametrize("mq", [1, 2])
def test_clipped_softmax_on_long_rows_two_pass(ops, mq):
    """Clipped softmax (softmax.py:10-19) on rows of more than 512 keys: the one-pass kernel's two-pass form (statistics pass,
    then the product against the final denominator) instead of the any-shape kernel.  Causal, cross attention with a ragged
    last tile, a key/value cache offset, bf16, D in {32, 128}; and, forced onto rows the full-row kernel takes, the two
    kernels agree to the fp16 contract."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    lib.oeh_debug_set_variant(0, mq)
    try:
        cases = [  # (B, H, Sq, Sk, D, causal, softmax, dtype)
            (1, 2, 640, 640, 64, True, "clippedsoftmax1(-.025:1)", torch.float16),
            (1, 1, 200, 1000, 64, False, "clipped(-.003:1.003)", torch.float16),
            (1, 2, 192, 704, 64, True, "clippedsoftmax1(-.025:1)", torch.float16),
            (1, 2, 576, 576, 128, True, "clippedsoftmax1(-.025:1)", torch.float16),
            (2, 1, 130, 700, 32, False, "clipped(-.003:1.003)", torch.bfloat16),
            (1, 2, 600, 600, 64, True, "clippedsoftmax1(-.025:1)", torch.float32),   # fp32 storage: operand pairs
            (1, 1, 90, 777, 128, False, "clipped(-.003:1.003)", torch.float32),
        ]
        for n, (B, H, Sq, Sk, D, causal, sm, dt) in enumerate(cases):
            sp = SPECS[sm]
            name = ops.attn_variant(B, H, Sq, Sk, D, dt, clip=True, base=sp["base"], gamma=sp["gamma"], causal=causal, scale=D ** -0.5)
            assert name.startswith("flash16/MQ1/" if (D == 128 and dt == torch.float32) else f"flash16/MQ{mq}/") and name.endswith("/clip2p"), name
            q = _rand((B, H, Sq, D), 4100 + n, dtype=dt)
            k, v = _rand((B, H, Sk, D), 4120 + n, dtype=dt), _rand((B, H, Sk, D), 4140 + n, dtype=dt)
            want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=D ** -0.5, causal=causal, clamp_min=causal, **sp)
            got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm), scale=D ** -0.5, causal=causal, clamp_min=causal)
            tol = F16_TOL if dt == torch.float16 else (dict(atol=5e-4, rtol=5e-4) if dt == torch.float32 else dict(atol=2e-2, rtol=2e-2))
            _check(got, want, tol=tol, msg=f"case {n} mq={mq}")
        # rows the full-row kernel takes: force the two-pass form over the same problem
        q, k, v = (_rand((2, 3, 512, 64), 4200 + i).cuda() for i in range(3))
        kw = dict(softmax=_spec(ops, "clippedsoftmax1(-.025:1)"), scale=0.125, causal=True, clamp_min=True)
        lib.oeh_debug_set_variant(0, 0)
        a = ops.attn_fwd(q, k, v, **kw)
        lib.oeh_debug_set_variant(256, mq)
        b = ops.attn_fwd(q, k, v, **kw)
        assert float((a.float() - b.float()).abs().max()) <= 1.5e-3
    finally:
        lib.oeh_debug_set_variant(0, 0)


@pytest.mark.parametrize("order", ["opt", "bert"])
@pytest.mark.parametrize("dt", [torch.float16, torch.float32])
def test_int8_chain_on_long_rows_two_pass(ops, dt, order):
    """The fused INT8 chain (quantized_opt.py:151-210: scores, probabilities and context on 8-bit grids) on rows of more than
    512 keys: the one-pass kernel's two-pass form of the grid chain instead of the any-shape kernel.  Against the oracle on
    640 causal keys (rare single steps of the context grid allowed, as for the full-row kernel), and, forced onto 512 keys,
    against the full-row kernel."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    fmin = float(np.finfo(np.float32).min)
    B, H, S, D = 1, 2, 640, 64
    q = _rand((B, H, S, D), 4301, dtype=dt)
    opt = order == "opt"   # OPT: q pre-scaled, causal, context quantised before the gate; BERT: scores / 8, no mask, after the gate
    if opt:
        q = (q.float() * D ** -0.5).to(dt)
    k, v = _rand((B, H, S, D), 4302, dtype=dt), _rand((B, H, S, D), 4303, dtype=dt)
    gate = torch.rand((B, H, S, 1), generator=torch.Generator().manual_seed(44))
    common = dict(causal=opt, clamp_min=opt, gate=gate.numpy(), **SPECS["softmax1"])
    if not opt:
        common.update(scale=8.0, scale_is_divisor=True)
    _, fp = O.attn_core(_np32(q), _np32(k), _np32(v), want=("scores", "probs"), **common)
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    ctx_fp = O.attn_core(_np32(q), _np32(k), _np32(v), **{**common, "gate": None if opt else gate.numpy()})
    d_c = O.quant_range_to_params(*np.percentile(ctx_fp, (0.001, 99.999)))
    want = O.attn_core(_np32(q), _np32(k), _np32(v), fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, ctx_quant_before_gate=opt, **common)
    FQ = ops.FakeQuantSpec.from_delta
    fq = ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c), ctx_before_gate=opt)
    name = ops.attn_variant(B, H, S, S, D, dt, fq=True, causal=opt, **({} if opt else {"scale_div": 8.0}))
    assert name.startswith("flash16/") and name.endswith("/fq2p"), name
    args = dict(softmax=_spec(ops, "softmax1"), causal=opt, clamp_min=opt, gate=gate.cuda(), mask_min=fmin)
    if not opt:
        args["scale_div"] = 8.0
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), fq=fq, **args)
    step = float(np.float32(d_c[0])) * (float(gate.max()) if opt else 1.0)
    err = np.abs(_np32(got) - want)
    flipped = err > 1e-3 + 1e-3 * np.abs(want)
    assert _le(flipped.mean(), OUT_OFF, "fq2p outputs off", n=flipped.size) and err.max() <= 1.05 * step + 2e-3, f"out: {flipped.mean():.2e} elements off, max err {err.max():.3e} (step {step:.3e})"
    # 512 keys: the full-row kernel's result against the two-pass form forced over the same problem
    q5, k5, v5, g5 = q[:, :, :512].cuda(), k[:, :, :512].cuda(), v[:, :, :512].cuda(), gate[:, :, :512].cuda()
    a = ops.attn_fwd(q5, k5, v5, fq=fq, **{**args, "gate": g5})
    lib.oeh_debug_set_variant(256, 0)
    try:
        b = ops.attn_fwd(q5, k5, v5, fq=fq, **{**args, "gate": g5})
    finally:
        lib.oeh_debug_set_variant(0, 0)
    d = (a.float() - b.float()).abs()
    assert float(d.max()) <= 1.05 * step + 2e-3 and _le(float((d > 1e-3).float().mean()), OUT_OFF, "fq2p vs full-row outputs apart", n=d.numel()), (float(d.max()), float((d > 1e-3).float().mean()))


def test_snake_block_order_changes_nothing_but_the_placement(ops):
    """The one-pass kernel walks every second row of 256 block ids backwards (CU load balance on causal
    shapes).  Same results bit for bit with the plain order, for grids of whole rows, a ragged last row and a head
    count that is not a multiple of 8."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    for n, (B, H, S) in enumerate([(16, 12, 512), (5, 12, 512), (3, 7, 1024), (9, 12, 384)]):
        q, k, v = (_rand((B, H, S, 64), 3100 + 3 * n + i).cuda() for i in range(3))
        assert ops.attn_variant(B, H, S, S, 64, torch.float16, causal=True).startswith("flash16/")
        a = ops.attn_fwd(q, k, v, causal=True, clamp_min=True)
        lib.oeh_debug_set_variant(512, 0)  # plain block order
        try:
            b = ops.attn_fwd(q, k, v, causal=True, clamp_min=True)
        finally:
            lib.oeh_debug_set_variant(0, 0)
        assert torch.equal(a, b), f"case {n}"
        want = O.attn_core(_np32(q[:1, :1]), _np32(k[:1, :1]), _np32(v[:1, :1]), causal=True, clamp_min=True)
        _check(a[:1, :1], want, msg=f"case {n}")


@pytest.mark.filterwarnings("ignore:outeffhop_amd.*any-shape HIP kernel:RuntimeWarning")  # (deliberate: the test forces / poses shapes only that kernel takes)
def test_randomised_kernel_sweep(ops):
    """Seeded random configurations through each 16-bit MFMA kernel that is eligible for them (the library's diagnostic
    hook disables variants: one-pass, full-row, general), against the oracle.  Shapes are ragged on purpose (Sq, Sk not
    multiples of 16/64, Sq != Sk with a causal offset), inputs are strided head views, gates and both softmax bases."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    fmin = float(np.finfo(np.float32).min)
    rng = np.random.default_rng(20240607)
    seen = set()
    try:
        for n in range(36):
            D = int(rng.choice([32, 64, 64, 128]))
            H = int(rng.integers(1, 4))
            B = int(rng.integers(1, 4))
            Sk = int(rng.integers(17, 400))
            causal = bool(rng.integers(0, 2))
            Sq = int(rng.integers(max(1, Sk - 150), Sk + 1)) if causal else int(rng.integers(1, 300))
            sm = ["softmax1", "vanilla"][int(rng.integers(0, 2))]
            pad = (not causal) and sm == "softmax1" and bool(rng.integers(0, 2))
            gated = bool(rng.integers(0, 2))
            dt = [torch.float16, torch.bfloat16][int(rng.integers(0, 4) == 0)]
            # (B,S,H*D) projections viewed as (B,H,S,D): the strided layout the modules pass
            q = _rand((B, Sq, H * D), 3000 + n, dtype=dt).view(B, Sq, H, D).permute(0, 2, 1, 3)
            k = _rand((B, Sk, H * D), 3100 + n, dtype=dt).view(B, Sk, H, D).permute(0, 2, 1, 3)
            v = _rand((B, Sk, H * D), 3200 + n, dtype=dt).view(B, Sk, H, D).permute(0, 2, 1, 3)
            padm = None
            if pad:
                padm = np.zeros((B, Sk), dtype=np.float32)
                for b in range(B):
                    padm[b, int(rng.integers(1, Sk + 1)):] = fmin
            gate = torch.rand((B, H, Sq, 1), generator=torch.Generator().manual_seed(3300 + n)) if gated else None
            want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=D ** -0.5, causal=causal, clamp_min=causal, pad_mask=padm,
                               gate=None if gate is None else gate.numpy(), **SPECS[sm])
            tol = F16_TOL if dt == torch.float16 else dict(atol=2e-2, rtol=2e-2)
            for off_mask in (256, 2, 2 | 4):   # one-pass forced; one-pass off (full-row if eligible); both off (general)
                if off_mask != 256 and Sk > 512:
                    continue
                lib.oeh_debug_set_variant(off_mask, 0)
                var = ops.attn_variant(B, H, Sq, Sk, D, dt)
                seen.add(var.split("/")[0])
                got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm), scale=D ** -0.5, causal=causal,
                                   clamp_min=causal, key_pad_mask=None if padm is None else torch.from_numpy(padm).cuda(),
                                   gate=None if gate is None else gate.cuda(), mask_min=fmin)
                _check(got, want, tol=tol, msg=f"cfg {n} {(B, H, Sq, Sk, D, causal, sm, pad, gated, dt)} via {var}")
    finally:
        lib.oeh_debug_set_variant(0, 0)
    assert {"flash16", "fast16", "mfma16"} <= seen


def test_one_pass_padding_trim_and_long_rows(ops):
    """Key padding on the one-pass kernel: trailing fully padded 64-key tiles are dropped from the stream (exact: a masked key
    contributes 0), the padding row is read from LDS up to 1024 keys and from global memory beyond."""
    fmin = float(np.finfo(np.float32).min)
    for n, (B, H, Sq, Sk, lens) in enumerate([(3, 2, 90, 700, (130, 700, 1)), (2, 1, 150, 1100, (1100, 333))]):
        q, k, v = _rand((B, H, Sq, 64), 4000 + n), _rand((B, H, Sk, 64), 4010 + n), _rand((B, H, Sk, 64), 4020 + n)
        padm = _pad_mask(B, Sk, list(lens), fmin)
        assert ops.attn_variant(B, H, Sq, Sk, 64).startswith("flash16/")
        want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=0.125, pad_mask=padm, **SPECS["softmax1"])
        got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), scale=0.125, key_pad_mask=torch.from_numpy(padm).cuda(), mask_min=fmin)
        _check(got, want, msg=f"case {n}")


@pytest.mark.parametrize("units,dtype", [(16, torch.float16), (0, torch.float16), (7, torch.bfloat16), (64, torch.float16), (40, torch.bfloat16), (65, torch.float16)])
def test_gate_predictor_fused_in_kernel(ops, units, dtype):
    """The conditional per-token gate evaluated inside the full-row kernel (include/oeh.h: gate_hidden ...): first layer on
    the matrix cores with weights rounded to the storage dtype, so it agrees with oeh_gate_fwd (fp32 weights) to ~1e-4 in
    the gate and to the usual output tolerance; up to 64 hidden units (attn_gate_mlp2: head_dim of them) as four 16-unit MFMA
    tiles, more are refused (callers fall back to gate_fwd)."""
    B, H, S, D = 3, 4, 100, 64
    fmin = float(np.finfo(np.float32).min)
    q, k, v = _rand((B, S, H * D), 5001, dtype=dtype), _rand((B, S, H * D), 5002, dtype=dtype), _rand((B, S, H * D), 5003, dtype=dtype)
    view = lambda t: t.cuda().view(B, S, H, D).permute(0, 2, 1, 3)  # noqa: E731
    hidden = _rand((B, S, H * D), 5004, dtype=dtype).cuda()
    g = torch.Generator().manual_seed(5005)
    mm = max(units, 1)
    w1 = (torch.randn((H, mm, D) if units else (H, D), generator=g) * 0.2).cuda()
    b1 = (torch.randn((H, mm) if units else (H,), generator=g) * 0.2).cuda()
    w2 = (torch.randn((H, mm), generator=g) * 0.5).cuda() if units else None
    b2 = torch.randn((H,), generator=g).cuda() if units else None
    pad = torch.from_numpy(_pad_mask(B, S, [100, 63, 1], fmin)).cuda()
    gp = ops.GatePredictor(hidden, w1, b1, w2, b2, scaling=4.0, out=torch.empty((B, H, S), dtype=torch.float32, device="cuda"))
    if units > 64:
        from outeffhop_amd._lib import OehError
        assert not ops.fused_gate_ok(B, H, S, S, D, dtype, units=units)
        with pytest.raises(OehError) as ei:
            ops.attn_fwd(view(q), view(k), view(v), scale_div=8.0, gate_mlp=gp)
        assert ei.value.code == -95
        return
    assert ops.fused_gate_ok(B, H, S, S, D, dtype, units=units)
    got = ops.attn_fwd(view(q), view(k), view(v), scale_div=8.0, key_pad_mask=pad, mask_min=fmin, gate_mlp=gp)
    # the gate itself against the ORACLE's predictor (fp32 weights, bert_attention.py:294-325) on the same layer input: the
    # kernel rounds the first-layer weights to the storage dtype (11 / 8 significant bits), as the reference's Linear in a
    # 16-bit model does
    if units:
        params = dict(w1=w1.cpu().numpy(), b1=b1.cpu().numpy(), w2=w2.cpu().numpy(), b2=b2.cpu().numpy())
        gate_o = O.gate_values(_np32(hidden), H, "mlp", params)
    else:
        gate_o = O.gate_values(_np32(hidden), H, "linear", dict(w=w1.cpu().numpy(), b=b1.cpu().numpy()))
    gtol = 2e-3 if dtype == torch.float16 else 1.5e-2
    gerr = float(np.abs(gp.out.cpu().numpy() - gate_o[..., 0]).max())
    assert gerr < gtol, f"in-kernel gate vs the oracle's predictor: {gerr:.3e}"
    sep_gate = ops.gate_fwd(hidden, H, w1, b1, w2, b2, scaling=1.0)
    assert float((sep_gate[..., 0].cpu() - torch.from_numpy(gate_o[..., 0])).abs().max()) < 1e-5  # the stand-alone kernel: fp32 weights
    # the output against the oracle with the ORACLE's gate (gate_scaling = 4 multiplies the output: the arithmetic part of the
    # fp16 contract scales with it, and the gate's own rounding error gtol * |context| comes on top)
    want_o = O.attn_core(_np32(view(q)), _np32(view(k)), _np32(view(v)), scale=8.0, scale_is_divisor=True, pad_mask=_pad_mask(B, S, [100, 63, 1], fmin),
                         gate=gate_o * 4.0, **SPECS["softmax1"])
    if dtype == torch.float16:
        ctx = np.abs(O.attn_core(_np32(view(q)), _np32(view(k)), _np32(view(v)), scale=8.0, scale_is_divisor=True,
                                 pad_mask=_pad_mask(B, S, [100, 63, 1], fmin), **SPECS["softmax1"]))
        lim = _f16_limit(want_o, 4e-3) + 4.0 * gerr * ctx
        err = np.abs(_np32(got) - want_o)
        assert (err <= lim).all(), f"fused gate vs oracle: max err {err.max():.3e}, worst excess {float((err - lim).max()):.3e}"
    else:
        _check(got, want_o, tol=dict(atol=8e-2, rtol=2e-2), msg="fused gate vs oracle")


@pytest.mark.parametrize("mq", [1, 2])
@pytest.mark.parametrize("units", [0, 12, 48])
def test_gate_predictor_fused_one_pass(ops, mq, units):
    """The in-kernel gate predictor on the one-pass kernel (both workgroup shapes): causal rows longer than one tile, with
    and without key padding, against gate_fwd + the `gate` argument and against the oracle."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    B, H, S, D = 2, 3, 330, 64
    fmin = float(np.finfo(np.float32).min)
    q = (_rand((B, S, H * D), 6001).float() * 0.125).half()
    k, v, hidden = _rand((B, S, H * D), 6002), _rand((B, S, H * D), 6003), _rand((B, S, H * D), 6004).cuda()
    view = lambda t: t.cuda().view(B, S, H, D).permute(0, 2, 1, 3)  # noqa: E731
    g = torch.Generator().manual_seed(6005)
    mm = max(units, 1)
    w1 = (torch.randn((H, mm, D) if units else (H, D), generator=g) * 0.2).cuda()
    b1 = (torch.randn((H, mm) if units else (H,), generator=g) * 0.2).cuda()
    w2 = (torch.randn((H, mm), generator=g) * 0.5).cuda() if units else None
    b2 = torch.randn((H,), generator=g).cuda() if units else None
    if units:
        gate_o = O.gate_values(_np32(hidden), H, "mlp", dict(w1=w1.cpu().numpy(), b1=b1.cpu().numpy(), w2=w2.cpu().numpy(), b2=b2.cpu().numpy()))
    else:
        gate_o = O.gate_values(_np32(hidden), H, "linear", dict(w=w1.cpu().numpy(), b=b1.cpu().numpy()))
    lib.oeh_debug_set_variant(0, mq)
    try:
        for pad in (None, torch.from_numpy(_pad_mask(B, S, [330, 170], fmin)).cuda()):
            assert ops.attn_variant(B, H, S, S, D).startswith(f"flash16/MQ{mq}/")
            gp = ops.GatePredictor(hidden, w1, b1, w2, b2, scaling=1.0, out=torch.empty((B, H, S), dtype=torch.float32, device="cuda"))
            kw = dict(causal=True, clamp_min=True, key_pad_mask=pad, mask_min=fmin)
            got = ops.attn_fwd(view(q), view(k), view(v), gate_mlp=gp, **kw)
            gerr = float(np.abs(gp.out.cpu().numpy() - gate_o[..., 0]).max())
            assert gerr < 2e-3, f"in-kernel gate vs the oracle's predictor: {gerr:.3e}"
            okw = dict(causal=True, clamp_min=True, pad_mask=None if pad is None else _pad_mask(B, S, [330, 170], fmin))
            want_o = O.attn_core(_np32(view(q)), _np32(view(k)), _np32(view(v)), gate=gate_o, **okw, **SPECS["softmax1"])
            ctx = np.abs(O.attn_core(_np32(view(q)), _np32(view(k)), _np32(view(v)), **okw, **SPECS["softmax1"]))
            err = np.abs(_np32(got) - want_o)
            lim = _f16_limit(want_o) + gerr * ctx  # the fp16 contract + the gate's own rounding (first-layer weights in fp16)
            assert (err <= lim).all(), f"fused gate vs oracle, pad={pad is not None}: max err {err.max():.3e}, worst excess {float((err - lim).max()):.3e}"
    finally:
        lib.oeh_debug_set_variant(0, 0)


def test_repeated_launches_under_a_concurrent_stream_are_bitwise_equal(ops):
    """Race detector (short form of tools/stress_determinism.py): the same padded launch 500 times while another stream runs
    a different attention shape.  Before `barrier_mem` waited for the wave's own LDS writes about 1 launch in 1000 differed."""
    fmin = float(np.finfo(np.float32).min)
    B, H, S, D = 16, 12, 512, 64
    g = torch.Generator(device="cuda").manual_seed(3)
    mk = lambda: torch.randn(B, S, H * D, device="cuda", generator=g).half().view(B, S, H, D).permute(0, 2, 1, 3)  # noqa: E731
    q, k, v = mk() * 0.3, mk(), mk()
    pad = torch.zeros(B, S, device="cuda")
    for b in range(B):
        pad[b, int(S * (0.5 + 0.5 * b / B)):] = fmin
    q2 = torch.randn(4, 8, 333, 64, device="cuda", generator=g).half()
    s2 = torch.cuda.Stream()
    for kw in (dict(scale_div=8.0, key_pad_mask=pad), dict(causal=True, clamp_min=True, key_pad_mask=pad), dict(causal=True, clamp_min=True)):
        ref = ops.attn_fwd(q, k, v, mask_min=fmin, **kw).clone()
        bad = 0
        for it in range(500):
            if it % 3 == 0:
                with torch.cuda.stream(s2):
                    ops.attn_fwd(q2, q2, q2, causal=True, clamp_min=True, mask_min=fmin)
            bad += 0 if torch.equal(ops.attn_fwd(q, k, v, mask_min=fmin, **kw), ref) else 1
        torch.cuda.synchronize()
        assert bad == 0, f"{bad} of 500 launches differ ({sorted(kw)})"


def test_fq_kernels_agree_bitwise_on_ragged_shapes(ops):
    """The full-row kernel's FQ variant against the general kernel's FQ chain (pinned to the reference by the golden INT8
    fixtures): random ragged shapes, quantiser subsets, zero points, masks, clipping, both softmax bases - same bits, same
    indices."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    fmin = float(np.finfo(np.float32).min)
    rng = np.random.default_rng(977)
    FQ = ops.FakeQuantSpec
    for n in range(24):
        D = int(rng.choice([32, 64, 64, 128]))
        B, H = int(rng.integers(1, 3)), int(rng.integers(1, 4))
        Sk = int(rng.integers(17, 513))
        causal = bool(rng.integers(0, 2))
        Sq = int(rng.integers(max(1, Sk - 150), Sk + 1)) if causal else int(rng.integers(1, 300))
        sm = ["softmax1", "vanilla", "clippedsoftmax1(-.025:1)"][int(rng.integers(0, 3))]
        dt = [torch.float16, torch.bfloat16][int(rng.integers(0, 4) == 0)]
        q = _rand((B, Sq, H * D), 5000 + n, dtype=dt).view(B, Sq, H, D).permute(0, 2, 1, 3).cuda()
        k = _rand((B, Sk, H * D), 5100 + n, dtype=dt).view(B, Sk, H, D).permute(0, 2, 1, 3).cuda()
        v = _rand((B, Sk, H * D), 5200 + n, dtype=dt).view(B, Sk, H, D).permute(0, 2, 1, 3).cuda()
        pad = None
        if not causal and bool(rng.integers(0, 2)):
            pad = torch.zeros(B, Sk)
            for b in range(B):
                pad[b, int(rng.integers(1, Sk + 1)):] = fmin
            pad = pad.cuda()
        gate = torch.rand((B, H, Sq, 1), generator=torch.Generator().manual_seed(5300 + n)).cuda() if rng.integers(0, 2) else None
        on = [True, True, bool(rng.integers(0, 4))]  # the FQ variant is compiled for scores + probabilities (context optional)
        grids = [(0.013 + 0.05 * float(rng.random()), float(rng.integers(0, 200))), (1.0 / 255.0, float(rng.integers(0, 3))),
                 (0.004 + 0.02 * float(rng.random()), float(rng.integers(60, 190)))]
        want_dump = bool(rng.integers(0, 2))
        res = []
        for off_mask in (1 << 11, 4):  # the full-row FQ variant (also at d = 128, where the library would pick the general kernel); full-row kernel disabled (general kernel)
            dumps = [torch.zeros((B, H, Sq, Sk), dtype=torch.uint8, device="cuda"), torch.zeros((B, H, Sq, Sk), dtype=torch.uint8, device="cuda"),
                     torch.zeros((B, H, Sq, D), dtype=torch.uint8, device="cuda")] if want_dump else [None] * 3
            specs = [FQ(g_[0], g_[1], dump=d_) if o_ else None for g_, d_, o_ in zip(grids, dumps, on)]
            lib.oeh_debug_set_variant(off_mask, 0)
            try:
                var = ops.attn_variant(B, H, Sq, Sk, D, dt, fq=True)
                got = ops.attn_fwd(q, k, v, softmax=_spec(ops, sm), scale=D ** -0.5, causal=causal, clamp_min=causal, key_pad_mask=pad, gate=gate,
                                   fq=ops.AttnFakeQuant(*specs, ctx_before_gate=bool(n & 1)), mask_min=fmin)
            finally:
                lib.oeh_debug_set_variant(0, 0)
            res.append((var, got, dumps))
        (var_a, got_a, dumps_a), (var_b, got_b, dumps_b) = res
        assert var_a.startswith("fast16/") and var_b.startswith("mfma16/"), (var_a, var_b)
        what = f"case {n}: {var_a} vs {var_b}, on={on} sm={sm} causal={causal} pad={pad is not None} gate={gate is not None}"
        assert torch.equal(got_a, got_b), what
        for i_, (da, db) in enumerate(zip(dumps_a, dumps_b)):
            if da is not None and on[i_]:
                assert torch.equal(da, db), what + f": index dump {i_} differs"


def test_fp32_storage_is_read_in_place_by_the_16bit_operand_kernels(ops):
    """fp32 q/k/v (the reference's validate_* scripts): the one-pass kernel (plain softmax / softmax_1) and the full-row kernel
    (clipped softmax, INT8 chain) stage fp32 tiles through registers; the diagnostic switch gives the general kernel (same
    arithmetic: fp32 storage, fp16 matrix-core operands).  All against the oracle; the INT8 chain must agree bit for bit."""
    from outeffhop_amd import _lib

    fmin = float(np.finfo(np.float32).min)
    FQ = ops.FakeQuantSpec
    tol32 = dict(atol=5e-4, rtol=5e-4)  # fp32 data as fp16 operand pairs: fp32-accurate scores; the probability operand is rounded to fp16
    for n, (B, H, Sq, Sk, D, causal, sm) in enumerate([(2, 3, 300, 300, 64, True, "softmax1"), (1, 2, 77, 290, 32, False, "vanilla"),
                                                        (2, 2, 400, 400, 128, True, "clippedsoftmax1(-.025:1)"), (1, 4, 512, 512, 64, True, "softmax1"),
                                                        (3, 2, 100, 100, 64, False, "clippedsoftmax1(-.025:1)"), (1, 2, 700, 700, 64, True, "softmax1")]):
        q = _rand((B, Sq, H * D), 7000 + n, dtype=torch.float32).view(B, Sq, H, D).permute(0, 2, 1, 3)
        k = _rand((B, Sk, H * D), 7100 + n, dtype=torch.float32).view(B, Sk, H, D).permute(0, 2, 1, 3)
        v = _rand((B, Sk, H * D), 7200 + n, dtype=torch.float32).view(B, Sk, H, D).permute(0, 2, 1, 3)
        pad = None
        if not causal:
            padm = np.zeros((B, Sk), dtype=np.float32)
            padm[:, Sk - 9:] = fmin
            pad = torch.from_numpy(padm).cuda()
        kw = dict(softmax=_spec(ops, sm), scale=D ** -0.5, causal=causal, clamp_min=causal, key_pad_mask=pad, mask_min=fmin)
        want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=D ** -0.5, causal=causal, clamp_min=causal,
                           pad_mask=None if pad is None else pad.cpu().numpy(), **SPECS[sm])
        var = ops.attn_variant(B, H, Sq, Sk, D, torch.float32, clip="clipped" in sm)
        assert (var.startswith("flash16/") or var.startswith("fast16/")) and "/f32" in var, var
        got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw)
        assert got.dtype == torch.float32
        _check(got, want, tol=tol32, msg=f"fp32 in place, case {n} ({var})")
        if Sk > 512:  # the full-row and general kernels stop at 512 keys: no pair for the comparisons below
            continue
        _lib.load().oeh_debug_set_variant((1 << 6) | (1 << 7), 0)  # fp32 forms of the one-pass / full-row kernels off
        try:
            got_gen = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw)
        finally:
            _lib.load().oeh_debug_set_variant(0, 0)
        _check(got_gen, want, tol=tol32, msg=f"general kernel case {n}")
        # INT8 chain: same bits from both kernels (same operand pairs, same per-element chain)
        fq = ops.AttnFakeQuant(FQ(0.05, 120.0), FQ(1.0 / 255.0, 0.0), FQ(0.01, 128.0), ctx_before_gate=bool(n & 1))
        a = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), fq=fq, **kw)
        _lib.load().oeh_debug_set_variant((1 << 6) | (1 << 7), 0)
        try:
            b_ = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), fq=fq, **kw)
        finally:
            _lib.load().oeh_debug_set_variant(0, 0)
        assert torch.equal(a, b_), f"INT8 fp32 case {n}: the full-row kernel differs from the general kernel"


@pytest.mark.parametrize("D", [32, 128])
def test_bert_order_with_a_divisor_that_is_not_a_power_of_two(ops, D):
    """scores / sqrt(d) with d = 32 / 128 (bert_attention.py:265): the 16-bit kernels multiply by RN(1/sqrt(d)); under
    fake-quant the general kernel divides."""
    B, H, S = 2, 3, 200
    fmin = float(np.finfo(np.float32).min)
    q, k, v = _rand((B, H, S, D), 910), _rand((B, H, S, D), 911), _rand((B, H, S, D), 912)
    padm = np.zeros((B, S), dtype=np.float32)
    padm[1, 150:] = fmin
    div = float(np.sqrt(D))
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=div, scale_is_divisor=True, pad_mask=padm, **SPECS["softmax1"])
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, "softmax1"), scale_div=div, key_pad_mask=torch.from_numpy(padm).cuda(), mask_min=fmin)
    _check(got, want, msg=f"divisor sqrt({D})")
    from outeffhop_amd import _lib
    d = _lib.oeh_attn_desc()
    d.B, d.H, d.Sq, d.Sk, d.D, d.dtype, d.scale, d.scale_div, d.mask_min, d.softmax_base = B, H, S, S, D, 0, 1.0, div, fmin, 1
    assert _lib.load().oeh_attn_variant(d, None).decode().startswith("flash16/")
    fqd = _lib.oeh_fq_desc()
    for f in (fqd.scores, fqd.probs):
        f.enable, f.scale, f.qmax = 1, 0.05, 255.0
    assert _lib.load().oeh_attn_variant(d, fqd).decode().startswith("mfma16/")


def test_fp32_storage_out_of_range_values_saturate(ops):
    """fp32 q / k / v are carried as fp16 operand pairs; a value beyond the fp16 range must not turn into inf
    (and the row into NaN).  The pair saturates: exact up to 65504 + 32, finite beyond; every other row is untouched."""
    B, H, S, D = 1, 2, 192, 64
    q, k, v = (_rand((B, H, S, D), 5100 + i, dtype=torch.float32).cuda() for i in range(3))
    base = ops.attn_fwd(q, k, v, causal=True, clamp_min=True, scale=0.125)
    q2, v2 = q.clone(), v.clone()
    q2[0, 0, 17, 3] = 65520.0      # inside hi + lo 2^-11: still exact to 2^-22
    q2[0, 1, 40, 9] = 3.0e5        # beyond: saturates
    v2[0, 1, 5, 0] = -1.0e6
    out = ops.attn_fwd(q2, k, v2, causal=True, clamp_min=True, scale=0.125)
    assert bool(torch.isfinite(out).all())
    want = O.attn_core(_np32(q2[:, :1]), _np32(k[:, :1]), _np32(v[:, :1]), causal=True, clamp_min=True, scale=0.125)
    _check(out[:, :1], want, tol=dict(atol=5e-4, rtol=5e-4), msg="head 0 (65520 in q)")
    untouched = torch.ones(S, dtype=torch.bool, device="cuda")
    untouched[40] = False
    assert torch.equal(out[0, 1, untouched, 1:], base[0, 1, untouched, 1:])  # v's column 0 and q's row 40 are the only places the big values reach


@pytest.mark.filterwarnings("ignore:outeffhop_amd.*any-shape HIP kernel:RuntimeWarning")  # (deliberate: the test forces / poses shapes only that kernel takes)
def test_randomised_sweep_fp32_storage(ops):
    """The same kind of sweep on fp32 tensors: the register-staged fp32 forms of the one-pass and the full-row kernel and
    the general kernel, ragged shapes, strided head views, masks, gates, clipped and plain softmax, against the oracle."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    fmin = float(np.finfo(np.float32).min)
    rng = np.random.default_rng(424242)
    tol32 = dict(atol=5e-4, rtol=5e-4)
    seen = set()
    try:
        for n in range(30):
            D = int(rng.choice([32, 64, 64, 128]))
            H, B = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            Sk = int(rng.integers(17, 600))
            causal = bool(rng.integers(0, 2))
            Sq = int(rng.integers(max(1, Sk - 150), Sk + 1)) if causal else int(rng.integers(1, 300))
            sm = ["softmax1", "vanilla", "clippedsoftmax1(-.025:1)"][int(rng.integers(0, 3))]
            pad = (not causal) and bool(rng.integers(0, 2))
            gated = bool(rng.integers(0, 2))
            q = _rand((B, Sq, H * D), 8000 + n, dtype=torch.float32).view(B, Sq, H, D).permute(0, 2, 1, 3)
            k = _rand((B, Sk, H * D), 8100 + n, dtype=torch.float32).view(B, Sk, H, D).permute(0, 2, 1, 3)
            v = _rand((B, Sk, H * D), 8200 + n, dtype=torch.float32).view(B, Sk, H, D).permute(0, 2, 1, 3)
            padm = None
            if pad:
                padm = np.zeros((B, Sk), dtype=np.float32)
                for b in range(B):
                    padm[b, int(rng.integers(1, Sk + 1)):] = fmin
            gate = torch.rand((B, H, Sq, 1), generator=torch.Generator().manual_seed(8300 + n)) if gated else None
            want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=D ** -0.5, causal=causal, clamp_min=causal, pad_mask=padm,
                               gate=None if gate is None else gate.numpy(), **SPECS[sm])
            for off_mask in (0, 1 << 6, (1 << 6) | (1 << 7)):   # as picked; fp32 one-pass off; both fp32 forms off (general / generic)
                lib.oeh_debug_set_variant(off_mask, 0)
                var = ops.attn_variant(B, H, Sq, Sk, D, torch.float32, clip="clipped" in sm)
                if var is None:
                    continue
                seen.add(var.split("/")[0])
                got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm), scale=D ** -0.5, causal=causal, clamp_min=causal,
                                   key_pad_mask=None if padm is None else torch.from_numpy(padm).cuda(),
                                   gate=None if gate is None else gate.cuda(), mask_min=fmin)
                _check(got, want, tol=tol32, msg=f"cfg {n} {(B, H, Sq, Sk, D, causal, sm, pad, gated)} via {var}")
    finally:
        lib.oeh_debug_set_variant(0, 0)
    assert {"flash16", "fast16", "mfma16"} <= seen


def test_fp32_storage_indices_match_the_reference_capture(ops):
    """VERDICT r1 J1 / north_star "bit-exact INT8 indices": the reference's validate path runs fp32 models
    (accelerate_configs/1gpu_no_mp.yaml:14), `quantized_opt.py:151` is an fp32 bmm.  The reference's own captured fp32
    projections (tests/golden/int8_attn.npz: q_lin / k_lin / v_lin, calibrated quantiser ranges) go through oeh_attn_fwd with
    index dumps; the three index tensors are compared with the ones captured inside the reference modules.  Operands rounded
    to fp16 (round 1) flipped 0.5-0.7 % of the score indices; carried as fp16 pairs (hi, lo) they must not flip more than
    1e-4 of any tensor kind, and never by more than one step."""
    g = load_golden("int8_attn.npz")
    import json

    fmin = float(np.finfo(np.float32).min)
    B, T, H, D = 2, 32, 2, 64
    FQ = ops.FakeQuantSpec.from_delta
    totals = {"scores": [0, 0], "probs": [0, 0], "ctx": [0, 0]}
    worst = 0

    def heads(name):
        return torch.from_numpy(g[name]).cuda().view(B, T, H, D).permute(0, 2, 1, 3)

    def grids(pre, dumps):
        out = []
        for n, d in zip(("attn_scores_act_quantizer", "attn_probs_act_quantizer", "context_act_quantizer"), dumps):
            out.append(FQ(float(g[f"{pre}.q.{n}.activation_quantizer.delta"]), float(g[f"{pre}.q.{n}.activation_quantizer.zero_float"]), dump=d))
        return out

    def tally(kind, got, want):
        nonlocal worst
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        totals[kind][0] += int((d != 0).sum())
        totals[kind][1] += d.size
        worst = max(worst, int(d.max()))

    for meta in json.loads(str(g["meta_json"])):
        sm = _spec(ops, meta["softmax"])
        gated = meta["gate"] != "nogate"
        # ---- OPT order: q scaled after the projection (opt_attention.py:167), causal + padding mask tensor, context quantised before the gate
        pre = f"opt{meta['tag']}"
        q, k, v = heads(f"{pre}.q_lin") * (D ** -0.5), heads(f"{pre}.k_lin"), heads(f"{pre}.v_lin")
        dumps = [torch.zeros((B, H, T, T), dtype=torch.uint8, device="cuda"), torch.zeros((B, H, T, T), dtype=torch.uint8, device="cuda"),
                 torch.zeros((B, H, T, D), dtype=torch.uint8, device="cuda")]
        fq = ops.AttnFakeQuant(*grids(pre, dumps), ctx_before_gate=True)
        mask = torch.from_numpy(g["opt_mask"]).cuda()
        out = ops.attn_fwd(q, k, v, softmax=sm, full_mask=mask, clamp_min=True, mask_min=fmin, fq=fq)
        for kind, dmp in zip(("scores", "probs", "ctx"), dumps):
            tally(kind, dmp.cpu().numpy().reshape(g[f"{pre}.{kind}.idx"].shape), g[f"{pre}.{kind}.idx"])
        if not gated:  # the dequantised context is the kernel's output
            ref = g[f"{pre}.ctx.out"].reshape(B, H, T, D)
            step = float(np.float32(g[f"{pre}.q.context_act_quantizer.activation_quantizer.delta"]))
            err = np.abs(_np32(out) - ref)
            assert err.max() <= 1.01 * step and (err > 1e-6).mean() <= 2e-3, (pre, err.max(), step, (err > 1e-6).mean())
        # the production kernels on the sample without padding (batch 0): analytic causal flag, fp32 forms of the full-row
        # kernel (no dumps) and of the general kernel (dumps) - on the quantiser grid when the softmax is not clipped
        q0, k0, v0 = q[:1], k[:1], v[:1]
        d0 = [torch.zeros((1, H, T, T), dtype=torch.uint8, device="cuda"), torch.zeros((1, H, T, T), dtype=torch.uint8, device="cuda"),
              torch.zeros((1, H, T, D), dtype=torch.uint8, device="cuda")]
        kw = dict(softmax=sm, causal=True, clamp_min=True, mask_min=fmin)
        o_dump = ops.attn_fwd(q0, k0, v0, fq=ops.AttnFakeQuant(*grids(pre, d0), ctx_before_gate=True), **kw)
        o_prod = ops.attn_fwd(q0, k0, v0, fq=ops.AttnFakeQuant(*grids(pre, [None] * 3), ctx_before_gate=True), **kw)
        assert torch.equal(o_dump, o_prod), pre + ": the production kernel and the index-dump run differ"
        for kind, dmp in zip(("scores", "probs", "ctx"), d0):
            want = g[f"{pre}.{kind}.idx"].reshape((B, H) + dmp.shape[2:])[:1]
            tally(kind, dmp.cpu().numpy(), want)
        # ---- BERT order: scores / sqrt(d), key-padding mask, context quantised AFTER the gate and the head merge
        pre = f"bert{meta['tag']}"
        q, k, v = heads(f"{pre}.q_lin"), heads(f"{pre}.k_lin"), heads(f"{pre}.v_lin")
        dumps = [torch.zeros((B, H, T, T), dtype=torch.uint8, device="cuda"), torch.zeros((B, H, T, T), dtype=torch.uint8, device="cuda"),
                 torch.zeros((B, H, T, D), dtype=torch.uint8, device="cuda")]
        sp = grids(pre, dumps)
        fq = ops.AttnFakeQuant(sp[0], sp[1], None if gated else sp[2], ctx_before_gate=False)  # (the gate values are not part of the capture)
        pad = torch.from_numpy(g["bert_mask"]).cuda()
        ops.attn_fwd(q, k, v, softmax=sm, scale_div=math.sqrt(D), key_pad_mask=pad, mask_min=fmin, fq=fq)
        kinds = ("scores", "probs") if gated else ("scores", "probs", "ctx")
        for kind, dmp in zip(kinds, dumps):
            got = dmp.cpu().numpy()
            if kind == "ctx":
                got = got.transpose(0, 2, 1, 3).reshape(B, T, H * D)
            tally(kind, got, g[f"{pre}.{kind}.idx"])
    rates = {kind: n / max(tot, 1) for kind, (n, tot) in totals.items()}
    print("fp32-storage index flips vs the reference capture:", {kind: f"{n}/{tot}" for kind, (n, tot) in totals.items()})
    assert worst <= 1 and all(r <= 1e-4 for r in rates.values()), (totals, worst)


@pytest.mark.filterwarnings("ignore:outeffhop_amd.*any-shape HIP kernel:RuntimeWarning")  # (deliberate: its last case poses unaligned rows)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_small_shape_kernel_stanhop(ops, dtype):
    """SURVEY 8f-4 / VERDICT r1 #8: STanHop's Association (cross_models/hopfield.py:42-51) - B*data_dim problems of L, S ~ 28
    rows, H = 4, E in {16, 32, 64}, (B,L,H,E) layout - one wave per (batch, head) with K and V in registers and fp32
    matrix-core products.  All four modes, ragged L / S (cross attention between segment and router axes), a gate; against
    the oracle.  fp32 storage: the products are exact fmaf chains, so the tolerance is fp32 rounding, not an fp16 contract."""
    tol = {torch.float32: dict(atol=3e-6, rtol=1e-5), torch.float16: F16_TOL, torch.bfloat16: dict(atol=2e-2, rtol=2e-2)}[dtype]
    modes = [("softmax1", 1.0), ("vanilla", 1.0), ("clippedsoftmax1(-.025:1)", 1.0), ("clipped(-.003:1.003)", 1.0)]
    n = 0
    # what the library picks by itself (round 3, measured): the small-shape kernel for fp32 problems (exact fp32 products) when there
    # are enough of them to fill the chip, and for d = 16; 16-bit problems take the full-row kernel (S = 64: 7.1 us against 19.9)
    assert ops.attn_variant(224, 4, 28, 28, 64, torch.float32).startswith("small/") and ops.attn_variant(64, 4, 10, 28, 16, torch.float16).startswith("small/")
    assert ops.attn_variant(224, 4, 28, 28, 64, torch.float16).startswith("fast16/") and ops.attn_variant(80, 4, 64, 64, 64, torch.float32).startswith("fast16/")
    from outeffhop_amd import _lib
    forced = _lib.load().oeh_debug_set_variant(1 << 10, 0) == 0  # the kernel under test wherever it can run (hooks off: the library's own picks)
    try:
        _small_shape_cases(ops, dtype, tol, modes, n, forced)
    finally:
        _lib.load().oeh_debug_set_variant(0, 0)


def _small_shape_cases(ops, dtype, tol, modes, n, forced):
    for (B, L, S, H, E) in [(32 * 7, 28, 28, 4, 64), (70, 28, 10, 4, 32), (64, 10, 28, 4, 16), (300, 1, 64, 1, 16), (80, 64, 64, 4, 64), (96, 33, 17, 3, 32)]:
        for sm, _ in modes[n % 2::2]:
            n += 1
            q, k, v = _rand((B, L, H, E), 900 + n, dtype=dtype), _rand((B, S, H, E), 950 + n, dtype=dtype), _rand((B, S, H, E), 990 + n, dtype=dtype)
            qv, kv, vv = q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)  # (B,H,L,E) views of the (B,L,H,E) layout
            assert not forced or ops.attn_variant(B, H, L, S, E, dtype, clip="clipped" in sm).startswith("small/"), (B, L, S, H, E)
            scale = 1.0 / math.sqrt(E)
            gate = torch.rand((B, H, L, 1), generator=torch.Generator().manual_seed(n)) if n % 3 == 0 else None
            want = O.attn_core(_np32(qv), _np32(kv), _np32(vv), scale=scale, gate=None if gate is None else gate.numpy(), **SPECS[sm])
            got = ops.attn_fwd(qv.cuda(), kv.cuda(), vv.cuda(), softmax=_spec(ops, sm), scale=scale, gate=None if gate is None else gate.cuda())
            assert got.dtype == dtype and got.permute(0, 2, 1, 3).is_contiguous()
            exact = forced or dtype != torch.float32 or ops.attn_variant(B, H, L, S, E, dtype, clip="clipped" in sm).startswith("small/")
            _check(got, want, tol if exact else dict(atol=5e-4, rtol=5e-4), msg=f"{(B, L, S, H, E)} {sm} {dtype}")  # (not this kernel: fp16 probability operand)
    # BERT-order division and a single problem with D = 16 (no other matrix-core kernel takes D = 16)
    q, k, v = _rand((2, 3, 20, 16), 1, dtype=dtype), _rand((2, 3, 40, 16), 2, dtype=dtype), _rand((2, 3, 40, 16), 3, dtype=dtype)
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=4.0, scale_is_divisor=True, **SPECS["softmax1"])
    _check(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), scale_div=4.0), want, tol, msg="divisor")
    # unaligned rows (3-element offset) fall back to the any-shape kernel and still agree
    buf = _rand((300, 28, 4 * 16 + 3), 4, dtype=dtype).cuda()
    qu = buf[:, :, 3:].view(300, 28, 4, 16).permute(0, 2, 1, 3)
    want = O.attn_core(_np32(qu), _np32(qu), _np32(qu), scale=0.25, **SPECS["softmax1"])
    _check(ops.attn_fwd(qu, qu, qu, scale=0.25), want, tol, msg="unaligned")


def _check_fp16_contract(got, want, msg):
    """north_star: "within 1e-3 fp16", stated without a relative fudge.  The kernel's ARITHMETIC (fp16 operands, fp32
    accumulation) is within 1e-3 of the reference - checked on its own by `_check_arithmetic_1e3` through the fp32-output form
    of the same kernels - and storing the result in fp16 adds at most half an fp16 ulp of the reference value (4.9e-4 for
    1 <= |ref| < 2): |hip - ref| <= 1e-3 + ulp16(ref) / 2."""
    got = _np32(got) if hasattr(got, "detach") else got
    lim = _f16_limit(want)
    err = np.abs(got - want)
    assert np.isfinite(got).all() and (err <= lim).all(), f"{msg}: max abs err {err.max():.3e}, worst excess {float((err - lim).max()):.3e}"
    return float(err.max())


def _check_arithmetic_1e3(ops, q, k, v, want, msg, **kw):
    """The fp16 kernel that SHIPS, with its output taken from the fp32 accumulators (`out_dtype=torch.float32`, include/oeh.h:
    o_dtype - the same instantiation, the same instruction stream up to the epilogue's store): what it computes before the output is
    rounded to fp16 must be within 1e-3 of the reference, everywhere.  (Rounds 1-3 measured this through the fp32-STORAGE
    instantiation on the same values - a proxy; VERDICT r3 weak #1.)  The stored fp16 output must be that value rounded once."""
    got = ops.attn_fwd(q, k, v, out_dtype=torch.float32, **kw)
    err = float(np.abs(_np32(got) - want).max())
    assert err <= 1e-3, f"{msg}: arithmetic error {err:.3e} > 1e-3"
    stored = ops.attn_fwd(q, k, v, **kw)
    assert torch.equal(stored, got.to(q.dtype)), f"{msg}: the stored output is not the accumulator rounded once"
    return err


def test_long_rows_against_the_reference_itself(ops):
    """Round 6 (VERDICT r5 next #2a): the kernels that serve LONG rows - the one-pass multi-tile loop (softmax1 / vanilla at S = 512 causal,
    704 padded keys), the full-row NT = 32 kernel (clippedsoftmax1 at 512 keys), their fp32-storage forms - against outputs captured from
    the REFERENCE at those shapes (tests/golden/core_attn_long.npz; inputs regenerated from tests/golden/synth.py), not only against the
    oracle.  fp16 storage: the stated contract (1e-3 before the output rounding, + half an fp16 ulp stored); fp32 storage: 5e-4."""
    from tests.golden import synth as sy

    g = load_golden("core_attn_long.npz")
    fmin = float(np.finfo(np.float32).min)
    q, k, v = (torch.from_numpy(a) for a in sy.long_causal_qkv())
    seen = set()
    for sm in ("softmax1", "clippedsoftmax1(-.025:1)", "vanilla"):
        want = g[f"opt512[{sm}].ctx"]
        kw = dict(softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=fmin)
        q16, k16, v16 = q.half().cuda(), k.half().cuda(), v.half().cuda()
        assert torch.equal(q16.float().cpu(), q)   # (the fixture's inputs are fp16 values)
        seen.add(ops.attn_variant(1, sy.LONG_H, sy.LONG_S, sy.LONG_S, sy.LONG_D, torch.float16, clip=SPECS[sm]["clip"], causal=True).split("/")[0])
        e16 = _check_fp16_contract(ops.attn_fwd(q16, k16, v16, **kw), want, f"reference S=512 causal {sm} fp16")
        ea = _check_arithmetic_1e3(ops, q16, k16, v16, want, f"reference S=512 causal {sm}", **kw)
        got32 = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw)
        _check(got32, want, dict(atol=5e-4, rtol=5e-4), f"reference S=512 causal {sm} fp32 storage")
        gotb = ops.attn_fwd(q.bfloat16().cuda(), k.bfloat16().cuda(), v.bfloat16().cuda(), **kw)
        wantb = O.attn_core(_np32(q.bfloat16()), _np32(k.bfloat16()), _np32(v.bfloat16()), causal=True, clamp_min=True, **SPECS[sm])
        _check(gotb, wantb, BF16_TOL, f"S=512 causal {sm} bf16 (oracle on the bf16-rounded inputs)")
        print(f"reference fixture S=512 causal {sm}: fp16 stored {e16:.2e}, before output rounding {ea:.2e}, fp32 storage {float(np.abs(_np32(got32) - want).max()):.2e}")
    assert {"flash16", "fast16"} <= seen, seen   # both fast families were the ones measured
    q, k, v = (torch.from_numpy(a) for a in sy.long_padded_qkv())
    pad = torch.from_numpy(sy.key_padding(sy.LONG_PAD_B, sy.LONG_PAD_S, sy.LONG_PAD_LEFT, sy.LONG_PAD_RIGHT)).cuda()
    for sm in ("softmax1", "vanilla"):
        want = g[f"bert704[{sm}].ctx"]
        kw = dict(softmax=_spec(ops, sm), scale_div=8.0, key_pad_mask=pad, mask_min=fmin)
        e16 = _check_fp16_contract(ops.attn_fwd(q.half().cuda(), k.half().cuda(), v.half().cuda(), **kw), want, f"reference 704 padded keys {sm} fp16")
        got32 = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw)
        _check(got32, want, dict(atol=5e-4, rtol=5e-4), f"reference 704 padded keys {sm} fp32 storage")
        print(f"reference fixture 704 padded keys {sm}: fp16 stored {e16:.2e}, fp32 storage {float(np.abs(_np32(got32) - want).max()):.2e}")


def test_full_size_bert_softmax1_cfg2(ops):
    """BASELINE config 2 at full size: BERT-base B=32 S=128 H=12 d=64 fp16, key-padding mask, softmax1.  Properties: a padded
    key never matters (bitwise), a sample's rows do not depend on its batch neighbours (bitwise), row sums < 1; oracle slices."""
    B, H, S, D = 32, 12, 128, 64
    fmin = float(np.finfo(np.float32).min)
    view = lambda t: t.cuda().view(B, S, H, D).permute(0, 2, 1, 3)  # noqa: E731
    q, k, v = view(_rand((B, S, H * D), 1234)), view(_rand((B, S, H * D), 1235)), view(_rand((B, S, H * D), 1236))
    lens = torch.randint(64, 129, (B,), generator=torch.Generator().manual_seed(1237)).tolist()
    padm = _pad_mask(B, S, lens, fmin)
    pad = torch.from_numpy(padm).cuda()
    kw = dict(scale_div=8.0, key_pad_mask=pad, mask_min=fmin)
    out = ops.attn_fwd(q, k, v, **kw)
    k2, v2 = k.clone(), v.clone()
    for b, n in enumerate(lens):
        k2[b, :, n:] = 9.0
        v2[b, :, n:] = -5.0
    assert torch.equal(ops.attn_fwd(q, k2, v2, **kw), out)
    assert torch.equal(ops.attn_fwd(q[5:9], k[5:9], v[5:9], scale_div=8.0, key_pad_mask=pad[5:9], mask_min=fmin), out[5:9])
    rowsum = ops.attn_fwd(q, k, torch.ones_like(v), **kw).float()
    assert 0.0 < float(rowsum.min()) and float(rowsum.max()) < 1.0 + 1e-3
    worst = 0.0
    for (b, h) in ((0, 0), (17, 5), (31, 11)):
        want = O.attn_core(_np32(q[b:b + 1, h:h + 1]), _np32(k[b:b + 1, h:h + 1]), _np32(v[b:b + 1, h:h + 1]), scale=8.0, scale_is_divisor=True,
                           pad_mask=padm[b:b + 1], **SPECS["softmax1"])
        worst = max(worst, _check_fp16_contract(out[b:b + 1, h:h + 1], want, f"cfg2 slice {(b, h)}"))
    print(f"cfg2 full size: max abs err on oracle slices {worst:.2e}")


@pytest.mark.parametrize("sm", ["softmax1", "clippedsoftmax1(-.025:1)"])
def test_full_size_opt_cfg3(ops, sm):
    """BASELINE config 3 (and the headline) at full size: OPT-125m B=16 S=512 fp16 causal, clippedsoftmax1(-.025:1) / softmax1:
    causality (bitwise), batch-shard invariance (bitwise), V = 1 gives row sums in [0, 1]; oracle slices under the stated
    1e-3 fp16 contract (no relative term below |ref| = 2)."""
    B, H, S, D = 16, 12, 512, 64
    fmin = float(np.finfo(np.float32).min)
    q = (_rand((B, H, S, D), 201).float() * 0.125).half().cuda()
    k, v = _rand((B, H, S, D), 202).cuda(), _rand((B, H, S, D), 203).cuda()
    kw = dict(softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=fmin)
    out = ops.attn_fwd(q, k, v, **kw)
    k3, v3 = k.clone(), v.clone()
    k3[:, :, 257:] = 7.0
    v3[:, :, 257:] = -3.0
    assert torch.equal(ops.attn_fwd(q, k3, v3, **kw)[:, :, :257], out[:, :, :257])
    assert torch.equal(ops.attn_fwd(q[2:4], k[2:4], v[2:4], **kw), out[2:4])
    rowsum = ops.attn_fwd(q, k, torch.ones_like(v), **kw).float()
    top = 1.0 if "clipped" not in sm else SPECS[sm]["eta"] - SPECS[sm]["gamma"]  # a stretched row sums to at most (eta - gamma) * 1 + S * gamma clipped at 0
    assert float(rowsum.min()) >= 0.0 and float(rowsum.max()) < top + 2e-3
    worst, arith = 0.0, 0.0
    for (b, h) in ((0, 0), (7, 3), (15, 11)):
        sl = (slice(b, b + 1), slice(h, h + 1))
        want = O.attn_core(_np32(q[sl]), _np32(k[sl]), _np32(v[sl]), causal=True, clamp_min=True, **SPECS[sm])
        worst = max(worst, _check_fp16_contract(out[sl], want, f"cfg3 {sm} slice {(b, h)}"))
        arith = max(arith, _check_arithmetic_1e3(ops, q[sl], k[sl], v[sl], want, f"cfg3 {sm} slice {(b, h)}", **kw))
    print(f"cfg3 {sm} full size: max abs err on oracle slices {worst:.2e} (before the output is rounded to fp16: {arith:.2e})")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_full_size_opt_int8_cfg4(ops, dtype):
    """BASELINE config 4 at full size, fp16 and fp32 storage: OPT-125m softmax1 + the three 8-bit activation quantisers.
    Properties: every output sits exactly on the context quantiser's grid and inside its range; causality and batch-shard
    invariance bitwise; the production kernel equals the index-dump kernel bitwise on a slice; index dumps of that slice
    against the oracle (<= 1 step, <= 1e-4 of a tensor)."""
    B, H, S, D = 16, 12, 512, 64
    fmin = float(np.finfo(np.float32).min)
    q = (_rand((B, H, S, D), 301, dtype=torch.float32) * 0.125).to(dtype).cuda()
    k, v = _rand((B, H, S, D), 302, dtype=torch.float32).to(dtype).cuda(), _rand((B, H, S, D), 303, dtype=torch.float32).to(dtype).cuda()
    common = dict(base=1, causal=True, clamp_min=True)
    sl = (slice(3, 4), slice(5, 7))  # calibrate on the oracle's FP intermediates of one slice (percentile 99.999, validate_clm.py:450-454)
    qs, ks, vs = q[sl], k[sl], v[sl]
    ctx_fp, fp = O.attn_core(_np32(qs), _np32(ks), _np32(vs), want=("scores", "probs"), **common)
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    d_c = O.quant_range_to_params(*np.percentile(ctx_fp, (0.001, 99.999)))
    FQ = ops.FakeQuantSpec.from_delta
    fq = ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c), ctx_before_gate=True)
    kw = dict(causal=True, clamp_min=True, mask_min=fmin)
    assert ops.attn_variant(B, H, S, S, D, dtype, fq=True, causal=True).startswith("fast16/")
    out = ops.attn_fwd(q, k, v, fq=fq, **kw)
    grid = FQ(*d_c)
    idx = out.float() / grid.scale + grid.zero_point
    off_grid = float((idx - idx.round()).abs().max())  # fp16 storage: the grid value itself is rounded to fp16 (half an ulp of |out| <= 2 is 5e-4 = 0.04 steps)
    assert off_grid < (6e-2 if dtype == torch.float16 else 1e-4), off_grid
    assert float(idx.round().min()) >= 0.0 and float(idx.round().max()) <= 255.0
    k3, v3 = k.clone(), v.clone()
    k3[:, :, 300:] = 7.0
    v3[:, :, 300:] = -3.0
    assert torch.equal(ops.attn_fwd(q, k3, v3, fq=fq, **kw)[:, :, :300], out[:, :, :300])
    assert torch.equal(ops.attn_fwd(q[8:10], k[8:10], v[8:10], fq=fq, **kw), out[8:10])
    dumps = [torch.zeros((1, 2, S, S), dtype=torch.uint8, device="cuda"), torch.zeros((1, 2, S, S), dtype=torch.uint8, device="cuda"),
             torch.zeros((1, 2, S, D), dtype=torch.uint8, device="cuda")]
    fqd = ops.AttnFakeQuant(FQ(*d_s, dump=dumps[0]), FQ(*d_p, dump=dumps[1]), FQ(*d_c, dump=dumps[2]), ctx_before_gate=True)
    assert torch.equal(ops.attn_fwd(qs, ks, vs, fq=fqd, **kw), out[sl])
    want, ex = O.attn_core(_np32(qs), _np32(ks), _np32(vs), fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, ctx_quant_before_gate=True,
                           want=("scores_idx", "probs_idx", "ctx_idx"), **common)
    tri = np.tril(np.ones((S, S), dtype=bool))[None, None]
    rates = {}
    for name, dmp in zip(("scores", "probs", "ctx"), dumps):
        a, b_ = dmp.cpu().numpy().astype(np.int32), ex[f"{name}_idx"].astype(np.int32)
        sel = np.broadcast_to(tri, a.shape) if name != "ctx" else np.ones_like(a, dtype=bool)
        d = np.abs(a[sel] - b_[sel])
        rates[name] = float((d != 0).mean())
        assert d.max() <= 1 and rates[name] <= 1e-4, f"{name}: max index diff {d.max()}, flip rate {rates[name]:.2e}"
    err = np.abs(_np32(out[sl]) - want)
    assert err.max() <= 1.01 * float(grid.scale) + 1e-3
    print(f"cfg4 {dtype} full size: index flip rates vs the oracle {rates}, max abs err {err.max():.2e}")


def test_full_size_bert_gated_cfg5(ops):
    """BASELINE config 5, one GPU's share at full size: BERT-base gated (conditional per-token gate, per-head MLP 64->16->1 on
    the layer input, evaluated inside the kernel), B=256 split 8 x 32: the shard of 32 samples.  Properties: a shard's rows
    are bit-identical whichever batch they are computed in (what makes the 8-GPU split exact), the gate the kernel reports
    is a probability and agrees with the stand-alone gate kernel; oracle slices with the oracle's own gate."""
    B, H, S, D = 32, 12, 128, 64
    fmin = float(np.finfo(np.float32).min)
    view = lambda t: t.cuda().view(B, S, H, D).permute(0, 2, 1, 3)  # noqa: E731
    q, k, v = view(_rand((B, S, H * D), 1240)), view(_rand((B, S, H * D), 1241)), view(_rand((B, S, H * D), 1242))
    hidden = _rand((B, S, H * D), 1243).cuda()
    g = torch.Generator().manual_seed(1244)
    w1, b1 = (torch.randn((H, 16, D), generator=g) * 0.1).cuda(), (torch.randn((H, 16), generator=g) * 0.1).cuda()
    w2, b2 = (torch.randn((H, 16), generator=g) * 0.5).cuda(), torch.full((H,), float(O.logit(0.25))).cuda()
    lens = torch.randint(64, 129, (B,), generator=g).tolist()
    padm = _pad_mask(B, S, lens, fmin)
    pad = torch.from_numpy(padm).cuda()
    gp = ops.GatePredictor(hidden, w1, b1, w2, b2, scaling=1.0, out=torch.empty((B, H, S), dtype=torch.float32, device="cuda"))
    out = ops.attn_fwd(q, k, v, scale_div=8.0, key_pad_mask=pad, mask_min=fmin, gate_mlp=gp)
    assert ops.fused_gate_ok(B, H, S, S, D, torch.float16, units=16, key_pad=True, scale_div=8.0)
    gate = gp.out.clone()
    assert 0.0 < float(gate.min()) and float(gate.max()) < 1.0
    # the gate against the ORACLE's predictor on the same layer input (bert_attention.py:314-320; fp32 weights there, first-layer
    # weights rounded to fp16 in the kernel - what the reference's Linear does in an fp16 model)
    params = dict(w1=w1.cpu().numpy(), b1=b1.cpu().numpy(), w2=w2.cpu().numpy(), b2=b2.cpu().numpy())
    gate_o = O.gate_values(_np32(hidden), H, "mlp", params)  # (B,H,S,1)
    gerr = float(np.abs(gate.cpu().numpy() - gate_o[..., 0]).max())
    assert gerr < 2e-3, f"in-kernel gate vs the oracle's predictor: {gerr:.3e}"
    # shard invariance: samples 8..15 computed alone
    gp2 = ops.GatePredictor(hidden[8:16], w1, b1, w2, b2, scaling=1.0, out=torch.empty((8, H, S), dtype=torch.float32, device="cuda"))
    out2 = ops.attn_fwd(q[8:16], k[8:16], v[8:16], scale_div=8.0, key_pad_mask=pad[8:16], mask_min=fmin, gate_mlp=gp2)
    assert torch.equal(out2, out[8:16]) and torch.equal(gp2.out, gate[8:16])
    worst = 0.0
    for (b, h) in ((0, 0), (20, 7)):
        sl = (slice(b, b + 1), slice(h, h + 1))
        okw = dict(scale=8.0, scale_is_divisor=True, pad_mask=padm[b:b + 1])
        want = O.attn_core(_np32(q[sl]), _np32(k[sl]), _np32(v[sl]), gate=gate_o[sl], **okw, **SPECS["softmax1"])  # the ORACLE's gate
        ctx = np.abs(O.attn_core(_np32(q[sl]), _np32(k[sl]), _np32(v[sl]), **okw, **SPECS["softmax1"]))
        err = np.abs(_np32(out[sl]) - want)
        lim = _f16_limit(want) + gerr * ctx  # the fp16 contract + the gate's own rounding
        assert (err <= lim).all(), f"cfg5 slice {(b, h)}: max err {err.max():.3e}, worst excess {float((err - lim).max()):.3e}"
        worst = max(worst, float(err.max()))
    print(f"cfg5 full size (one GPU's 32 samples): max abs err on oracle slices {worst:.2e}, in-kernel gate vs the oracle's predictor {gerr:.2e}")


def _quantise_to_grid(x, pct=99.999):
    """numpy: a per-tensor 8-bit asymmetric grid from percentiles (as the reference calibrates), indices and dequantised values."""
    lo, hi = np.percentile(x, (100 - pct, pct))
    delta, zero = O.quant_range_to_params(lo, hi)
    scale, zp, qmax = O.fq_grid(delta, zero)
    idx = O.fq_index(x, scale, zp, qmax)
    return idx.astype(np.uint8), O.fq_dequant(idx, scale, zp).astype(np.float32), (float(scale), float(zp))


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("S,causal,base", [(512, True, 1), (200 - 200 % 16, False, 0), (96, True, 1)])
def test_int8_storage_on_the_integer_matrix_cores(ops, S, causal, base, out_dtype):
    """SURVEY 8f-3 / VERDICT r1 #3: q, k, v as the 8-bit indices the reference's QuantLinear projections put them on
    (hijacker.py:78-127, quantized_opt.py:67-75), both products on v_mfma_i32_16x16x64_i8.  Against the oracle run on the
    DEQUANTISED values (what the reference's fp32 bmm sees): the integer products are exact where the reference rounds every
    fp32 product, so an output may sit one context-grid step away where a quantiser input was within an ulp of a rounding
    boundary - a few in 1e4 outputs (each output depends on hundreds of quantised scores and probabilities) - and nowhere else.  Also against the fake-quant kernel on the dequantised fp32 values."""
    from outeffhop_amd._lib import OehError

    B, H, D = 2, 3, 64
    fmin = float(np.finfo(np.float32).min)
    g = torch.Generator().manual_seed(77 + S)
    x = [torch.randn((B, S, H * D), generator=g).numpy() * s_ for s_ in (1.0, 1.3, 0.8)]
    (qi, qd, qg), (ki, kd, kg), (vi, vd, vg) = (_quantise_to_grid(t) for t in x)
    heads = lambda t: np.ascontiguousarray(t.reshape(B, S, H, D).transpose(0, 2, 1, 3))  # noqa: E731
    scaling = D ** -0.5
    qdh, kdh, vdh = heads(qd) * np.float32(scaling), heads(kd), heads(vd)
    common = dict(base=base, causal=causal, clamp_min=causal)
    ctx_fp, fp = O.attn_core(qdh, kdh, vdh, want=("scores", "probs"), **common)
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    d_c = O.quant_range_to_params(*np.percentile(ctx_fp, (0.001, 99.999)))
    gate = torch.rand((B, H, S, 1), generator=g)
    want = O.attn_core(qdh, kdh, vdh, fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, ctx_quant_before_gate=True, gate=gate.numpy(), **common)
    FQ = ops.FakeQuantSpec.from_delta
    fq = ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c), ctx_before_gate=True)
    # INT8 storage: centred indices; q, k as (B,H,S,D) views of (B,S,E), v transposed to (B,H,D,S)
    dev = lambda t: torch.from_numpy(t).cuda()  # noqa: E731
    qc = ops.centre_indices(dev(qi)).view(B, S, H, D).permute(0, 2, 1, 3)
    kc = ops.centre_indices(dev(ki)).view(B, S, H, D).permute(0, 2, 1, 3)
    vt = ops.centre_indices(dev(vi)).view(B, S, H, D).permute(0, 2, 3, 1).contiguous()
    grids = (ops.QuantGrid(qg[0], qg[1]), ops.QuantGrid(*kg), ops.QuantGrid(*vg))
    got = ops.attn_fwd_i8(qc, kc, vt, grids, fq=fq, out_dtype=out_dtype, softmax=ops.SoftmaxSpec(base, False, 0.0, 1.0), scale=scaling,
                          causal=causal, clamp_min=causal, mask_min=fmin, gate=gate.cuda())
    assert got.dtype == out_dtype and got.shape == (B, H, S, D) and got.permute(0, 2, 1, 3).is_contiguous()
    step = float(np.float32(d_c[0]))
    err = np.abs(_np32(got) - want)
    tol = 1e-6 if out_dtype == torch.float32 else 1e-3
    off = float((err > tol + (0 if out_dtype == torch.float32 else 1e-3) * np.abs(want)).mean())
    assert err.max() <= 1.01 * step + tol and off <= 3e-4, f"max err {err.max():.3e} (step {step:.3e}), {off:.2e} of the outputs off their grid point"
    # the fake-quant kernel of the fp32-storage path on the dequantised values: the same results up to those rare steps
    ref = ops.attn_fwd(dev(qdh), dev(kdh), dev(vdh), softmax=ops.SoftmaxSpec(base, False, 0.0, 1.0), causal=causal, clamp_min=causal,
                       mask_min=fmin, gate=gate.cuda(), fq=fq)
    d2 = (got.float() - ref).abs()
    assert float(d2.max()) <= 1.01 * step + tol and float((d2 > tol + 1e-3 * ref.abs()).float().mean()) <= 3e-4
    # clipped softmax (gamma <= 0: the reference's registry) on the integer cores since round 3: against the oracle, same bounds
    csm = SPECS["clippedsoftmax1(-.025:1)"]
    ccommon = dict(causal=causal, clamp_min=causal, **csm)
    cctx, cfp = O.attn_core(qdh, kdh, vdh, want=("scores", "probs"), **ccommon)
    c_p = O.quant_range_to_params(*np.percentile(cfp["probs"], (0.001, 99.999)))
    c_c = O.quant_range_to_params(*np.percentile(cctx, (0.001, 99.999)))
    cwant = O.attn_core(qdh, kdh, vdh, fq_scores=d_s, fq_probs=c_p, fq_ctx=c_c, ctx_quant_before_gate=True, gate=gate.numpy(), **ccommon)
    cgot = ops.attn_fwd_i8(qc, kc, vt, grids, fq=ops.AttnFakeQuant(FQ(*d_s), FQ(*c_p), FQ(*c_c)), out_dtype=out_dtype,
                           softmax=ops.SoftmaxSpec(1, True, csm["gamma"], csm["eta"]), scale=scaling, causal=causal, clamp_min=causal, mask_min=fmin, gate=gate.cuda())
    cstep = float(np.float32(c_c[0]))
    cerr = np.abs(_np32(cgot) - cwant)
    coff = float((cerr > tol + (0 if out_dtype == torch.float32 else 1e-3) * np.abs(cwant)).mean())
    assert cerr.max() <= 1.01 * cstep + tol and coff <= 1e-3, f"clipped: max err {cerr.max():.3e} (step {cstep:.3e}), {coff:.2e} off their grid point"
    # not this path: gamma > 0, a 7-bit probability grid, another head dim -> refused, never silently something else
    with pytest.raises(OehError) as ei:
        ops.attn_fwd_i8(qc, kc, vt, grids, fq=fq, softmax=ops.SoftmaxSpec(1, True, 0.01, 1.1), scale=scaling)
    assert ei.value.code == -95
    with pytest.raises(OehError):
        ops.attn_fwd_i8(qc, kc, vt, grids, fq=ops.AttnFakeQuant(FQ(*d_s), ops.FakeQuantSpec(1 / 127.0, 0.0, 127.0), None), scale=scaling)


@pytest.mark.parametrize("order,causal,base", [("bert", False, 1), ("bert", False, 0), ("opt", True, 1), ("opt", True, 0)])
def test_int8_storage_key_padding_and_bert_order(ops, order, causal, base):
    """the integer-matrix-core kernel with a key-padding vector (its PAD variants), in BERT order (scores
    divided by sqrt(d), `quantized_bert.py:363`; context quantised AFTER the gate, `:434`) and in OPT order with padded keys on
    top of the causal mask (HF's decoder mask for a padded batch) - against the oracle on the dequantised values, incl. a
    right-padded, a left-padded and a fully padded sample (softmax_1: exactly the zero point's value; vanilla softmax: uniform
    over all keys, as the reference gives)."""
    B, H, D, S = 4, 3, 64, 176
    fmin = float(np.finfo(np.float32).min)
    g = torch.Generator().manual_seed(91 + base)
    x = [torch.randn((B, S, H * D), generator=g).numpy() * s_ for s_ in (1.0, 1.2, 0.9)]
    (qi, qd, qg), (ki, kd, kg), (vi, vd, vg) = (_quantise_to_grid(t) for t in x)
    heads = lambda t: np.ascontiguousarray(t.reshape(B, S, H, D).transpose(0, 2, 1, 3))  # noqa: E731
    padm = _pad_mask(B, S, [S, 121, S, 0], fmin)
    padm[2, :37] = fmin  # left padding
    if order == "bert":
        okw = dict(scale=8.0, scale_is_divisor=True)
        qdh = heads(qd)
        kkw = dict(scale_div=8.0)
    else:
        okw = dict()
        qdh = heads(qd) * np.float32(D ** -0.5)
        kkw = dict(scale=D ** -0.5)
    kdh, vdh = heads(kd), heads(vd)
    common = dict(base=base, causal=causal, clamp_min=True, pad_mask=padm, **okw)
    ctx_fp, fp = O.attn_core(qdh, kdh, vdh, want=("scores", "probs"), **common)
    vis = padm[:, None, None, :] == 0
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"][np.broadcast_to(vis, fp["scores"].shape)], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    d_c = O.quant_range_to_params(*np.percentile(ctx_fp, (0.001, 99.999)))
    gate = torch.rand((B, H, S, 1), generator=g)
    before = order == "opt"
    want = O.attn_core(qdh, kdh, vdh, fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, ctx_quant_before_gate=before, gate=gate.numpy(), **common)
    FQ = ops.FakeQuantSpec.from_delta
    fq = ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c), ctx_before_gate=before)
    dev = lambda t: torch.from_numpy(t).cuda()  # noqa: E731
    qc = ops.centre_indices(dev(qi)).view(B, S, H, D).permute(0, 2, 1, 3)
    kc = ops.centre_indices(dev(ki)).view(B, S, H, D).permute(0, 2, 1, 3)
    vt = ops.centre_indices(dev(vi)).view(B, S, H, D).permute(0, 2, 3, 1).contiguous()
    grids = (ops.QuantGrid(*qg), ops.QuantGrid(*kg), ops.QuantGrid(*vg))
    got = ops.attn_fwd_i8(qc, kc, vt, grids, fq=fq, out_dtype=torch.float32, softmax=ops.SoftmaxSpec(base, False, 0.0, 1.0), causal=causal,
                          clamp_min=True, mask_min=fmin, gate=gate.cuda(), key_pad_mask=dev(padm), **kkw)
    step = float(np.float32(d_c[0])) * (1.0 if before else 1.0)
    err = np.abs(_np32(got) - want)
    off = float((err > 1e-6).mean())
    assert err.max() <= 1.01 * step + 1e-6 and off <= 5e-4, f"max err {err.max():.3e} (step {step:.3e}), {off:.2e} of the outputs off their grid point"
    # the fake-quant kernels on the dequantised fp32 values: the same results up to those rare steps
    ref = ops.attn_fwd(dev(qdh), dev(kdh), dev(vdh), softmax=ops.SoftmaxSpec(base, False, 0.0, 1.0), causal=causal, clamp_min=True, mask_min=fmin,
                       gate=gate.cuda(), fq=fq, key_pad_mask=dev(padm), **({"scale_div": 8.0} if order == "bert" else {}))
    d2 = (got - ref).abs()
    assert float(d2.max()) <= 1.01 * step + 1e-6 and float((d2 > 1e-6 + 1e-3 * ref.abs()).float().mean()) <= 5e-4
    # a mask value that is neither 0 nor <= -1e4 is the caller's to keep away (attention.pad_is_boolean); a full additive mask is refused
    from outeffhop_amd._lib import OehError
    with pytest.raises((OehError, TypeError)):
        ops.attn_fwd_i8(qc, kc, vt, grids, fq=fq, softmax=ops.SoftmaxSpec(1, True, 0.01, 1.1), key_pad_mask=dev(padm), **kkw)   # (gamma > 0)


def test_int8_storage_indices_match_the_reference_capture(ops):
    """VERDICT r2 next #3a / missing #4: the reference's captured QuantLinear outputs (tests/golden/int8_attn.npz: q_lin / k_lin /
    v_lin of `quantized_opt.py:67-75`, on the captured q_proj / k_proj / v_proj activation grids) are turned into the 8-bit indices
    they are, and go through the integer-matrix-core kernel with its index dumps on; the three index tensors are compared with the
    ones captured inside the reference module (`quantized_opt.py:154,182,210`).  The integer products are exact where the
    reference's fp32 bmm rounds, so an index may sit one step away where the reference's quantiser input was within an ulp of
    a rounding boundary - per tensor kind at most 1e-4 of the indices, never more than one step (the bound of the fp32-storage
    path, `test_fp32_storage_indices_match_the_reference_capture`).  OPT order (q scaled after the projection, causal mask,
    context quantised before the gate), unclipped softmaxes, the sample without padded keys: what `oeh_attn_i8_kernel` takes."""
    g = load_golden("int8_attn.npz")
    import json

    fmin = float(np.finfo(np.float32).min)
    B, T, H, D = 2, 32, 2, 64
    FQ = ops.FakeQuantSpec.from_delta
    totals = {"scores": [0, 0], "probs": [0, 0], "ctx": [0, 0]}
    worst = 0
    ran = 0
    for meta in json.loads(str(g["meta_json"])):
        sm = _spec(ops, meta["softmax"])
        if sm.clip:
            continue
        pre = f"opt{meta['tag']}"
        cent, grids = [], []
        for nm in ("q", "k", "v"):
            spec = FQ(float(g[f"{pre}.q.{nm}_proj.activation_quantizer.delta"]), float(g[f"{pre}.q.{nm}_proj.activation_quantizer.zero_float"]))
            x = g[f"{pre}.{nm}_lin"][:1]  # (1, T, E) fp32, already on its grid
            idx = np.rint(x.astype(np.float64) / np.float64(np.float32(spec.scale))) + spec.zero_point
            assert idx.min() >= 0 and idx.max() <= 255
            assert np.array_equal((np.float32(spec.scale) * (idx - spec.zero_point).astype(np.float32)).astype(np.float32), x), "captured projections are on their grid"
            cent.append(ops.centre_indices(torch.from_numpy(idx.astype(np.uint8)).cuda()))
            grids.append(ops.QuantGrid.of(spec))
        qc = cent[0].view(1, T, H, D).permute(0, 2, 1, 3)
        kc = cent[1].view(1, T, H, D).permute(0, 2, 1, 3)
        vt = cent[2].view(1, T, H, D).permute(0, 2, 3, 1).contiguous()
        dumps = [torch.zeros((1, H, T, T), dtype=torch.uint8, device="cuda"), torch.zeros((1, H, T, T), dtype=torch.uint8, device="cuda"),
                 torch.zeros((1, H, T, D), dtype=torch.uint8, device="cuda")]
        sp = [FQ(float(g[f"{pre}.q.{n}.activation_quantizer.delta"]), float(g[f"{pre}.q.{n}.activation_quantizer.zero_float"]), dump=d)
              for n, d in zip(("attn_scores_act_quantizer", "attn_probs_act_quantizer", "context_act_quantizer"), dumps)]
        kw = dict(out_dtype=torch.float32, softmax=sm, scale=D ** -0.5, causal=True, clamp_min=True, mask_min=fmin)
        o_dump = ops.attn_fwd_i8(qc, kc, vt, grids, fq=ops.AttnFakeQuant(*sp, ctx_before_gate=True), **kw)
        sp_nd = [ops.FakeQuantSpec(x.scale, x.zero_point, x.qmax) for x in sp]
        o_prod = ops.attn_fwd_i8(qc, kc, vt, grids, fq=ops.AttnFakeQuant(*sp_nd, ctx_before_gate=True), **kw)
        assert torch.equal(o_dump, o_prod), pre + ": the production kernel and its index-dump variant differ"
        for kind, dmp in zip(("scores", "probs", "ctx"), dumps):
            want = g[f"{pre}.{kind}.idx"].reshape((B, H) + dmp.shape[2:])[:1]
            d = np.abs(dmp.cpu().numpy().astype(np.int32) - want.astype(np.int32))
            totals[kind][0] += int((d != 0).sum())
            totals[kind][1] += d.size
            worst = max(worst, int(d.max()))
        if meta["gate"] == "nogate":  # the dequantised context is the kernel's output
            ref = g[f"{pre}.ctx.out"].reshape(B, H, T, D)[:1]
            step = float(np.float32(sp[2].scale))
            err = np.abs(_np32(o_prod) - ref)
            assert err.max() <= 1.01 * step and (err > 1e-6).mean() <= 1e-3, (pre, err.max(), step)
        ran += 1
    rates = {kind: n / max(tot, 1) for kind, (n, tot) in totals.items()}
    print("INT8-storage index flips vs the reference capture:", {kind: f"{n}/{tot}" for kind, (n, tot) in totals.items()}, "worst step", worst)
    assert ran >= 3
    assert worst <= 1 and all(r <= 1e-4 for r in rates.values()), (totals, worst)


def test_int8_storage_randomised_sweep(ops):
    """The integer-matrix-core kernel over ragged shapes: key counts that are not multiples of 64 (multiples of 16: its
    alignment), cross attention (Sq != Sk, causal with a key/value cache offset), all three row-length variants (NT 8/16/32),
    zero points on both sides of 128 (and exactly 128: no offsets), context quantiser before / after the gate / off, bf16
    output, strided (B,S,H*64) layouts.  Against the fake-quant kernels on the dequantised fp32 values (pinned to the oracle
    and to the reference capture by the tests above): equal up to rare single steps of the output grid."""
    rng = np.random.default_rng(2024)
    fmin = float(np.finfo(np.float32).min)
    for n in range(14):
        B, H = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        Sk = int(rng.choice([16, 48, 64, 112, 128, 144, 256, 272, 400, 512]))
        causal = bool(rng.integers(0, 2))
        Sq = Sk if (causal and rng.integers(0, 2)) else int(rng.integers(1, Sk + 1)) if causal else int(rng.integers(1, 300))
        base = int(rng.integers(0, 2))
        out_dtype = [torch.float32, torch.float16, torch.bfloat16][n % 3]
        g = torch.Generator().manual_seed(5000 + n)
        zq, zk, zv = (float(z) for z in rng.choice([128.0, 97.0, 131.0, 160.0, 120.0], 3))
        if n in (3, 9):
            zq = 0.0 if n == 3 else 255.0  # the ends of the range: 128 - zp = 128 does not fit a signed byte (the kernel's CQ2 variant), -127 does
        if n == 6:
            zk, zv = 0.0, 255.0
        sq, sk_, sv = 0.031, 0.027, 0.035
        if n in (3, 9):
            sq *= 0.2  # (one-sided q below: keep the scores inside their grid - saturated rows are all ties, which either kernel may break either way)
        # centred indices, strided (B,S,H*D) storage
        qi = torch.randint(0, 256, (B, Sq, H * 64), generator=g, dtype=torch.int64).to(torch.uint8)
        ki = torch.randint(0, 256, (B, Sk, H * 64), generator=g, dtype=torch.int64).to(torch.uint8)
        vi = torch.randint(0, 256, (B, Sk, H * 64), generator=g, dtype=torch.int64).to(torch.uint8)
        deq = lambda idx, s_, z_: ((idx.float() - z_) * s_)  # noqa: E731
        hv = lambda t, S_: t.view(B, S_, H, 64).permute(0, 2, 1, 3)  # noqa: E731
        scaling = 0.125
        qd, kd, vd = hv(deq(qi, sq, zq), Sq) * scaling, hv(deq(ki, sk_, zk), Sk), hv(deq(vi, sv, zv), Sk)
        FQ = ops.FakeQuantSpec
        before = bool(n & 1)
        fq = ops.AttnFakeQuant(FQ(0.09, float(rng.choice([128.0, 100.0, 140.0]))), FQ(1.0 / 255.0, 0.0),
                               None if n % 5 == 4 else FQ(0.03, 126.0), ctx_before_gate=before)
        gate = torch.rand((B, H, Sq, 1), generator=g).cuda() if n % 3 != 2 else None
        sm = ops.SoftmaxSpec(base, False, 0.0, 1.0)
        kw = dict(softmax=sm, causal=causal, clamp_min=causal, mask_min=fmin, gate=gate, fq=fq)
        ref = ops.attn_fwd(qd.cuda(), kd.cuda(), vd.cuda(), **kw)
        qc = hv(ops.centre_indices(qi.cuda()), Sq)
        kc = hv(ops.centre_indices(ki.cuda()), Sk)
        vt = ops.centre_indices(vi.cuda()).view(B, Sk, H, 64).permute(0, 2, 3, 1).contiguous()
        got = ops.attn_fwd_i8(qc, kc, vt, (ops.QuantGrid(sq, zq), ops.QuantGrid(sk_, zk), ops.QuantGrid(sv, zv)), out_dtype=out_dtype, scale=scaling, **kw)
        assert got.dtype == out_dtype
        step = 0.03 * (float(gate.max()) if gate is not None else 1.0) if fq.ctx is not None else 0.0
        tol = {torch.float32: 2e-5, torch.float16: 2e-3, torch.bfloat16: 2e-2}[out_dtype]
        d = (got.float() - ref).abs()
        lim = tol + tol * ref.abs()
        frac_off = float((d > lim).float().mean())
        assert float(d.max()) <= 1.05 * step + float(lim.max()) and _le(frac_off, OUT_OFF, f"i8 storage case {n} outputs off", n=d.numel()), \
            f"case {n} {(B, H, Sq, Sk, causal, base, out_dtype)}: max diff {float(d.max()):.3e} (step {step:.3e}), {frac_off:.2e} off"


@pytest.mark.parametrize("order,dtype", [("opt", torch.float32), ("bert", torch.float32), ("opt", torch.float16)])
def test_attn_calibrate_without_the_score_tensors(ops, order, dtype):
    """VERDICT r2 missing #3 / next #8: `oeh_attn_calibrate` - the percentile ranges of the score and probability quantisers from
    values recomputed tile by tile inside the kernel (nothing of size Sq x Sk is stored) - against np.percentile on the tensors
    the oracle materialises (range_estimators.py:83-106), through the running average over two batches, and the context with
    both quantisers applied against the oracle's.  OPT order: causal + a padded sample (HF's decoder mask as flag + vector);
    BERT order: key padding, scores / sqrt(d).  Ragged sizes (Sq = 150: the last 64-row block is partial; 150 keys: not a
    multiple of 16)."""
    B, H, S, D = 3, 2, 150, 64
    fmin = float(np.finfo(np.float32).min)
    P = 99.9  # (a 135 000-element tensor: the 99.999th percentile would interpolate between its top two values only)
    st_s = torch.zeros(2, dtype=torch.float64, device="cuda")
    st_p = torch.zeros(2, dtype=torch.float64, device="cuda")
    ref_s = ref_p = None
    for batch in range(2):
        q = _rand((B, H, S, D), 9100 + batch, scale=1.3 if order == "bert" else 0.16, dtype=dtype)
        k, v = _rand((B, H, S, D), 9110 + batch, dtype=dtype), _rand((B, H, S, D), 9120 + batch, dtype=dtype)
        padm = _pad_mask(B, S, [S, 97, S], fmin)
        okw = dict(base=1, pad_mask=padm, **(dict(scale=8.0, scale_is_divisor=True) if order == "bert" else dict(causal=True, clamp_min=True)))
        kw = dict(key_pad_mask=torch.from_numpy(padm).cuda(), mask_min=fmin, q_lo=100 - P, q_hi=P, momentum=0.9,
                  **(dict(scale_div=8.0) if order == "bert" else dict(causal=True, clamp_min=True)))
        qn, kn, vn = _np32(q), _np32(k), _np32(v)
        # scores: the oracle's tensor, its percentiles, the running average
        _, fp = O.attn_core(qn, kn, vn, want=("scores",), **okw)
        lo, hi = np.percentile(fp["scores"], (100 - P, P))
        ref_s = (lo, hi) if ref_s is None else (0.1 * lo + 0.9 * ref_s[0], 0.1 * hi + 0.9 * ref_s[1])
        ops.attn_calibrate(q.cuda(), k.cuda(), None, ops.CALIB_SCORES, state=st_s, first=batch == 0, **kw)
        got = st_s.cpu().numpy()
        assert np.allclose(got, ref_s, rtol=3e-6, atol=1e-6), (order, batch, got, ref_s)
        # probabilities: scores quantised on the grid of the (device-resident) running range
        d_s = O.quant_range_to_params(float(got[0]), float(got[1]))
        _, fp = O.attn_core(qn, kn, vn, fq_scores=d_s, want=("probs",), **okw)
        lo, hi = np.percentile(fp["probs"], (100 - P, P))
        ref_p = (lo, hi) if ref_p is None else (0.1 * lo + 0.9 * ref_p[0], 0.1 * hi + 0.9 * ref_p[1])
        ops.attn_calibrate(q.cuda(), k.cuda(), None, ops.CALIB_PROBS, scores_range=st_s, state=st_p, first=batch == 0, **kw)
        gotp = st_p.cpu().numpy()
        assert np.allclose(gotp, ref_p, rtol=2e-5, atol=1e-7), (order, batch, gotp, ref_p)
        # the context with both quantisers on their running ranges
        d_p = O.quant_range_to_params(float(gotp[0]), float(gotp[1]))
        want = O.attn_core(qn, kn, vn, fq_scores=d_s, fq_probs=d_p, **okw)
        ctx = ops.attn_calibrate(q.cuda(), k.cuda(), v.cuda(), ops.CALIB_CONTEXT, scores_range=st_s, probs_range=st_p, **kw)
        assert ctx.dtype == torch.float32 and ctx.shape == (B, H, S, D)
        err = np.abs(_np32(ctx) - want)
        # a score or probability within an ulp of a rounding boundary may land on the neighbouring grid point: rare, small
        assert (err > 2e-5).mean() <= 2e-3 and err.max() <= 2e-2, (order, batch, float(err.max()), float((err > 2e-5).mean()))


@pytest.mark.gpu
def test_context_quantiser_emits_its_integers(ops):
    """include/oeh.h ctx_emit_index: the output is idx - zp of the context quantiser (what a QuantLinear consumer multiplies as
    integers, quantized_opt.py:271) - on the int8-storage core and on the fake-quant kernels: scale * integers reproduces the
    ordinary output bit for bit, in fp16 the integers are exact; refused (EINVAL) when a gate follows the quantiser."""
    import dataclasses
    from outeffhop_amd import _lib

    torch.manual_seed(5)
    B, H, S, D = 2, 3, 128, 64
    dev = torch.device("cuda:0")
    q = torch.randn(B, H, S, D, device=dev) * 0.5
    k, v = torch.randn(B, H, S, D, device=dev), torch.randn(B, H, S, D, device=dev)
    fq = ops.AttnFakeQuant(scores=ops.FakeQuantSpec(0.11, 130.0), probs=ops.FakeQuantSpec(1.0 / 255, 0.0), ctx=ops.FakeQuantSpec(0.021, 121.0))
    fqi = dataclasses.replace(fq, ctx_emit_index=True)
    kw = dict(softmax=ops.SoftmaxSpec(base=1), causal=True, clamp_min=True, mask_min=float(np.finfo(np.float32).min))
    for dt in (torch.float32, torch.float16):
        val = ops.attn_fwd(q.to(dt), k.to(dt), v.to(dt), fq=fq, **kw)
        rel = ops.attn_fwd(q.to(dt), k.to(dt), v.to(dt), fq=fqi, **kw)
        assert torch.equal(rel, rel.round()) and float(rel.min()) >= -121.0 and float(rel.max()) <= 134.0
        assert torch.equal((rel.float() * np.float32(0.021)).to(dt), val)
    grids = [ops.QuantGrid(0.02, 128.0), ops.QuantGrid(0.03, 125.0), ops.QuantGrid(0.025, 131.0)]
    qc, kc = [torch.randint(-128, 128, (B, S, H * D), device=dev, dtype=torch.int8).view(B, S, H, D).permute(0, 2, 1, 3) for _ in range(2)]
    vt = torch.randint(-128, 128, (B, H, D, S), device=dev, dtype=torch.int8)
    val = ops.attn_fwd_i8(qc, kc, vt, grids, fq=fq, out_dtype=torch.float32, **kw)
    rel = ops.attn_fwd_i8(qc, kc, vt, grids, fq=fqi, out_dtype=torch.float16, **kw)
    assert torch.equal(rel, rel.round()) and torch.equal(rel.float() * np.float32(0.021), val)
    # (round 4) ... and as int8 CENTRED indices idx - 128 (o_dtype OEH_I8: what an int8 consumer GEMM takes, oeh_proj_quant_i8 pairs == 3),
    # with and without a key-padding vector, on row lengths of all three kernel variants; refused without ctx_emit_index
    for S_ in (128, 48, 512):
        qs, ks = [torch.randint(-128, 128, (B, S_, H * D), device=dev, dtype=torch.int8).view(B, S_, H, D).permute(0, 2, 1, 3) for _ in range(2)]
        vs = torch.randint(-128, 128, (B, H, D, S_), device=dev, dtype=torch.int8)
        for pad in (None, torch.tensor([[0.0] * (S_ - 7) + [float(np.finfo(np.float32).min)] * 7] * B, device=dev)):
            kw_ = dict(kw, key_pad_mask=pad)
            r16 = ops.attn_fwd_i8(qs, ks, vs, grids, fq=fqi, out_dtype=torch.float16, **kw_)
            c8 = ops.attn_fwd_i8(qs, ks, vs, grids, fq=fqi, out_dtype=torch.int8, **kw_)
            assert c8.dtype == torch.int8 and c8.shape == r16.shape and torch.equal(c8.float() + (128.0 - 121.0), r16.float())
    with pytest.raises(_lib.OehError):
        ops.attn_fwd_i8(qc, kc, vt, grids, fq=fq, out_dtype=torch.int8, **kw)
    gate = torch.rand(B, H, S, 1, device=dev)
    with pytest.raises(_lib.OehError):
        ops.attn_fwd(q, k, v, fq=fqi, gate=gate, **kw)
    relg = ops.attn_fwd(q, k, v, fq=dataclasses.replace(fqi, ctx_before_gate=False), gate=gate, **kw)  # BERT order: the quantiser is last
    valg = ops.attn_fwd(q, k, v, fq=dataclasses.replace(fq, ctx_before_gate=False), gate=gate, **kw)
    assert torch.equal(relg * np.float32(0.021), valg)


@pytest.mark.gpu
@pytest.mark.parametrize("D,S,dt", [(80, 200, torch.float16), (96, 640, torch.float16), (48, 33, torch.float32), (16, 100, torch.float16), (8, 40, torch.float32),
                                    (72, 130, torch.bfloat16)])
def test_head_dims_between_the_kernels_are_zero_padded(ops, D, S, dt):
    """OPT-2.7b / ViT-H have head dim 80, others 96 or 48: `ops.attn_fwd` runs them zero-padded at the next matrix-core head dim
    (the library alone would pick the any-shape kernel: one workgroup per query row) - same result, no any-shape warning; with a
    key-padding mask, a gate, an `out` tensor and the fused INT8 chain."""
    import warnings

    B, H = 2, 3
    assert ops.attn_variant(B, H, S, S, D, dt, causal=True) == "generic"
    q, k, v = _rand((B, H, S, D), 171, dtype=dt), _rand((B, H, S, D), 172, dtype=dt), _rand((B, H, S, D), 173, dtype=dt)
    fmin = float(np.finfo(np.float32).min)
    pad = _pad_mask(B, S, [S, S - 9], fmin)
    gate = np.random.default_rng(3).random((B, H, S, 1), dtype=np.float32)
    tol = None if dt == torch.float16 else (dict(atol=5e-4, rtol=5e-4) if dt == torch.float32 else BF16_TOL)  # (fp32: the probability operand is fp16)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=1 / math.sqrt(D), base=1, causal=True, clamp_min=True, mask_min=fmin)
        got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), scale=1 / math.sqrt(D), causal=True, clamp_min=True, mask_min=fmin)
        assert got.shape == (B, H, S, D)
        _check(got, want, tol=tol, msg=f"causal D={D}")
        want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=math.sqrt(D), scale_is_divisor=True, base=1, pad_mask=pad, mask_min=fmin, gate=gate)
        out = torch.empty((B, S, H, D), dtype=dt, device="cuda").permute(0, 2, 1, 3)
        got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), scale_div=math.sqrt(D), key_pad_mask=torch.from_numpy(pad).cuda(), mask_min=fmin,
                           gate=torch.from_numpy(gate).cuda(), out=out)
        assert got is out
        _check(got, want, tol=tol, msg=f"padded + gated D={D}")


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["bert", "opt"])
@pytest.mark.parametrize("base", [1, 0])
@pytest.mark.parametrize("S,dt", [(96, torch.float16), (512, torch.float16), (176, torch.float32)])
def test_int8_grid_chain_with_key_padding(ops, order, base, S, dt):
    """include/oeh.h key_pad_boolean: with a key-padding vector of 0 / finfo.min entries the fused INT8 chain stays on the quantiser
    grid (full-row kernel's grid form: a flag per key, one instruction per element) instead of the reference's op order on
    dequantised values - BERT order and OPT order with padded keys on top of the causal mask, right- and left-padded samples and one
    without a visible key (softmax_1: zeros; vanilla: uniform over all keys): against the oracle, and against the literal form
    (the same call without the promise) up to rare single steps."""
    B, H, D = 4, 2, 64
    fmin = float(np.finfo(np.float32).min)
    q, k, v = _rand((B, H, S, D), 181, dtype=dt), _rand((B, H, S, D), 182, dtype=dt), _rand((B, H, S, D), 183, dtype=dt)
    if order == "opt":
        q = (q.float() * D ** -0.5).to(dt)
    padm = _pad_mask(B, S, [S, S - 37, S, 0], fmin)
    padm[2, :21] = fmin   # a left-padded sample
    common = dict(base=base, causal=(order == "opt"), clamp_min=True, pad_mask=padm, mask_min=fmin)
    if order == "bert":
        common.update(scale=8.0, scale_is_divisor=True)
    vis = dict(common, pad_mask=None)
    _, fp = O.attn_core(_np32(q), _np32(k), _np32(v), want=("scores", "probs"), **vis)
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    d_c = O.quant_range_to_params(*np.percentile(O.attn_core(_np32(q), _np32(k), _np32(v), **vis), (0.001, 99.999)))
    want = O.attn_core(_np32(q), _np32(k), _np32(v), fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, **common)
    FQ = ops.FakeQuantSpec.from_delta
    fq = ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c))
    args = dict(softmax=ops.SoftmaxSpec(base), causal=(order == "opt"), clamp_min=True, mask_min=fmin, key_pad_mask=torch.from_numpy(padm).cuda(), fq=fq)
    if order == "bert":
        args["scale_div"] = 8.0
    grid = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), key_pad_boolean=True, **args)
    literal = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **args)
    step = float(np.float32(d_c[0]))
    for name, got in (("grid", grid), ("literal", literal)):
        err = np.abs(_np32(got) - want)
        off = float((err > 0.5 * step).mean())
        assert np.isfinite(_np32(got)).all() and _le(off, OUT_OFF, f"grid-vs-literal {name} outputs off", n=err.size) and err.max() <= 2.05 * step + 2e-3, f"{name}: {off:.2e} off, max {err.max() / step:.2f} steps"
    d = (grid.float() - literal.float()).abs()
    assert _le(float((d > 0.5 * step).float().mean()), OUT_OFF, "grid vs literal apart", n=d.numel()) and float(d.max()) <= 2.05 * step + 2e-3
    if base == 1:
        assert float(grid[3].abs().max()) <= abs(float(np.float32(d_c[0])) * 0.51) + abs(want[3]).max()  # the sample without a visible key


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.float32])
@pytest.mark.parametrize("kind", ["clip", "fq"])
@pytest.mark.parametrize("order", ["opt", "bert"])
def test_long_rows_with_key_padding_two_pass(ops, order, kind, dt):
    """VERDICT r2 missing #6: clipped softmax and the fused INT8 chain with a key-padding vector on rows of more than 512 keys -
    the two-pass forms of the one-pass kernel (PAD variants; softmax_1; the INT8 chain with include/oeh.h key_pad_boolean)
    instead of the any-shape kernel: right- and left-padded samples and one without a visible key, against the oracle."""
    B, H, S, D = 3, 2, 704, 64
    fmin = float(np.finfo(np.float32).min)
    opt = order == "opt"
    q, k, v = _rand((B, H, S, D), 5101, dtype=dt), _rand((B, H, S, D), 5102, dtype=dt), _rand((B, H, S, D), 5103, dtype=dt)
    if opt:
        q = (q.float() * D ** -0.5).to(dt)
    padm = _pad_mask(B, S, [S - 150, S, 0], fmin)
    padm[1, :70] = fmin   # a left-padded sample
    sm = "clippedsoftmax1(-.025:1)" if kind == "clip" else "softmax1"
    common = dict(causal=opt, clamp_min=True, pad_mask=padm, mask_min=fmin, **SPECS[sm])
    if not opt:
        common.update(scale=8.0, scale_is_divisor=True)
    args = dict(softmax=_spec(ops, sm), causal=opt, clamp_min=True, mask_min=fmin, key_pad_mask=torch.from_numpy(padm).cuda(), key_pad_boolean=True)
    if not opt:
        args["scale_div"] = 8.0
    vkw = dict(fq=(kind == "fq"), clip=(kind == "clip"), base=1, gamma=SPECS[sm]["gamma"], causal=opt, key_pad=True, key_pad_boolean=True, mask_min=fmin,
               **({} if opt else {"scale_div": 8.0}))
    name = ops.attn_variant(B, H, S, S, D, dt, **vkw)
    assert name.startswith("flash16/") and name.endswith("/fq2p" if kind == "fq" else "/clip2p"), name
    if kind == "clip":
        want = O.attn_core(_np32(q), _np32(k), _np32(v), **common)
        got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **args)
        _check(got, want, tol=F16_TOL if dt == torch.float16 else dict(atol=5e-4, rtol=5e-4), msg=f"{order} clip2p + pad")
        assert float(got[2].abs().max()) == 0.0   # no visible key: softmax_1 gives zeros, the clip keeps them
        return
    vis = dict(common, pad_mask=None)
    _, fp = O.attn_core(_np32(q), _np32(k), _np32(v), want=("scores", "probs"), **vis)
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    d_c = O.quant_range_to_params(*np.percentile(O.attn_core(_np32(q), _np32(k), _np32(v), **vis), (0.001, 99.999)))
    want = O.attn_core(_np32(q), _np32(k), _np32(v), fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, **common)
    FQ = ops.FakeQuantSpec.from_delta
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), fq=ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c)), **args)
    step = float(np.float32(d_c[0]))
    err = np.abs(_np32(got) - want)
    off = float((err > 0.5 * step).mean())
    assert np.isfinite(_np32(got)).all() and _le(off, OUT_OFF, "fused chain outputs off", n=err.size) and err.max() <= 2.05 * step + 2e-3, f"{off:.2e} off, max {err.max() / step:.2f} steps"


@pytest.mark.gpu
@pytest.mark.parametrize("S", [384, 704])
@pytest.mark.parametrize("dt", [torch.float16, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("causal", [False, True])
def test_vanilla_softmax_with_key_padding_on_the_one_pass_kernel(ops, S, dt, causal):
    """Key padding under the VANILLA softmax on the one-pass kernel (round 3; before: full-row kernel up to 512 keys, any-shape kernel
    beyond): a row without a visible key - a fully padded sample, the first rows of a left-padded one under the causal mask - is
    uniform over ALL keys in the reference (models/softmax.py: every score is the same finfo.min), i.e. the mean of V: the PAD
    variant's epilogue forms it for such rows."""
    B, H, D = 4, 2, 64
    fmin = float(np.finfo(np.float32).min)
    q, k, v = _rand((B, H, S, D), 6101, dtype=dt), _rand((B, H, S, D), 6102, dtype=dt), _rand((B, H, S, D), 6103, dtype=dt)
    padm = _pad_mask(B, S, [S - 90, S, 0, S], fmin)
    padm[1, :70] = fmin    # left-padded
    padm[3, 5:] = fmin     # five visible keys
    gate = np.random.default_rng(4).random((B, H, S, 1), dtype=np.float32)
    name = ops.attn_variant(B, H, S, S, D, dt, base=0, key_pad=True, causal=causal, scale=0.125, mask_min=fmin)
    assert name.startswith("flash16/"), name
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=0.125, base=0, causal=causal, clamp_min=True, pad_mask=padm, mask_min=fmin, gate=gate)
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=ops.SoftmaxSpec(0), scale=0.125, causal=causal, clamp_min=True, mask_min=fmin,
                       key_pad_mask=torch.from_numpy(padm).cuda(), gate=torch.from_numpy(gate).cuda())
    tol = F16_TOL if dt == torch.float16 else (dict(atol=5e-4, rtol=5e-4) if dt == torch.float32 else BF16_TOL)
    _check(got, want, tol=tol, msg=f"vanilla + pad S={S} causal={causal}")
    mean_v = _np32(v)[2].mean(axis=1, keepdims=True) * gate[2]
    assert np.abs(_np32(got)[2] - mean_v).max() < (2e-2 if dt == torch.bfloat16 else 2e-3)   # the sample without a visible key: the mean of V


@pytest.mark.gpu
@pytest.mark.parametrize("units", [0, 16, 64])
@pytest.mark.parametrize("S,clip", [(100, False), (128, True), (384, False)])
def test_gate_predictor_fused_on_fp32_storage(ops, units, S, clip):
    """VERDICT r2 missing #5: the conditional per-token gate evaluated inside the attention kernel on fp32 data (the reference's
    validate precision) - full-row kernel, weights and layer input as fp16 operand pairs, so the gate is the fp32 Linear's
    (against the oracle's predictor to 2e-6, where the 16-bit kernels round the weights: 2e-3) - instead of a separate
    oeh_gate_fwd launch; key padding, clipped softmax, rows up to 512 keys."""
    B, H, D = 3, 4, 64
    fmin = float(np.finfo(np.float32).min)
    dt = torch.float32
    q, k, v = _rand((B, S, H * D), 7001, dtype=dt), _rand((B, S, H * D), 7002, dtype=dt), _rand((B, S, H * D), 7003, dtype=dt)
    view = lambda t: t.cuda().view(B, S, H, D).permute(0, 2, 1, 3)  # noqa: E731
    hidden = _rand((B, S, H * D), 7004, dtype=dt).cuda()
    g = torch.Generator().manual_seed(7005)
    mm = max(units, 1)
    w1 = (torch.randn((H, mm, D) if units else (H, D), generator=g) * 0.2).cuda()
    b1 = (torch.randn((H, mm) if units else (H,), generator=g) * 0.2).cuda()
    w2 = (torch.randn((H, mm), generator=g) * 0.5).cuda() if units else None
    b2 = torch.randn((H,), generator=g).cuda() if units else None
    lens = [S, S - 37, 1]
    pad = torch.from_numpy(_pad_mask(B, S, lens, fmin)).cuda()
    sm = "clippedsoftmax1(-.025:1)" if clip else "softmax1"
    gp = ops.GatePredictor(hidden, w1, b1, w2, b2, scaling=2.0, out=torch.empty((B, H, S), dtype=torch.float32, device="cuda"))
    # (round 5: the host takes the fused form only where it is the faster one - not where the problem without the predictor runs the one-pass fp32 kernel:
    # that kernel + one gate launch wins there; the library call itself, below, works either way)
    plain = ops.attn_variant(B, H, S, S, D, dt, clip=clip, key_pad=True, scale_div=8.0, mask_min=fmin)
    assert ops.fused_gate_ok(B, H, S, S, D, dt, units=units, clip=clip, key_pad=True, scale_div=8.0, mask_min=fmin) == (not plain.startswith("flash16/"))
    assert ops.attn_variant(B, H, S, S, D, dt, clip=clip, key_pad=True, scale_div=8.0, mask_min=fmin, gate_hidden=True).startswith("fast16/")
    got = ops.attn_fwd(view(q), view(k), view(v), softmax=_spec(ops, sm), scale_div=8.0, key_pad_mask=pad, mask_min=fmin, gate_mlp=gp)
    if units:
        gate_o = O.gate_values(_np32(hidden), H, "mlp", dict(w1=w1.cpu().numpy(), b1=b1.cpu().numpy(), w2=w2.cpu().numpy(), b2=b2.cpu().numpy()))
    else:
        gate_o = O.gate_values(_np32(hidden), H, "linear", dict(w=w1.cpu().numpy(), b=b1.cpu().numpy()))
    gerr = float(np.abs(gp.out.cpu().numpy() - gate_o[..., 0]).max())
    assert gerr < 2e-6, f"in-kernel fp32 gate vs the oracle's predictor: {gerr:.3e}"
    want = O.attn_core(_np32(view(q)), _np32(view(k)), _np32(view(v)), scale=8.0, scale_is_divisor=True, pad_mask=_pad_mask(B, S, lens, fmin), mask_min=fmin,
                       gate=gate_o * 2.0, **SPECS[sm])
    _check(got, want, tol=dict(atol=1e-3, rtol=5e-4), msg=f"fp32 fused gate units={units} S={S} clip={clip}")
    # and the separate gate kernel + the `gate` argument (another attention kernel takes that call: the one-pass form, whose
    # probability operand is rounded at other points - both within the fp32-storage tolerance of the oracle)
    sep = ops.gate_fwd(hidden, H, w1, b1, w2, b2, scaling=2.0)
    assert float((sep[..., 0] / 2.0 - gp.out).abs().max()) < 2e-6
    ref = ops.attn_fwd(view(q), view(k), view(v), softmax=_spec(ops, sm), scale_div=8.0, key_pad_mask=pad, mask_min=fmin, gate=sep)
    assert float((got - ref).abs().max()) < 1.5e-3


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("base", [1, 0])
def test_full_masks_on_long_rows_run_the_one_pass_kernel(ops, dt, base):
    """VERDICT r2 missing #6: a (B,1,Sq,Sk) additive mask on rows of more than 512 keys (opt_attention.py:215-224 takes arbitrary
    masks) - the one-pass kernel's PAD variant reads it per block instead of the any-shape kernel: a random mask of finfo.min
    entries and moderate additive values, alone and on top of a key-padding vector, rows without a visible key under both
    softmax bases, cross attention with a ragged last tile."""
    B, H, Sq, Sk, D = 2, 2, 200, 715, 64
    fmin = float(np.finfo(np.float32).min)
    q, k, v = _rand((B, H, Sq, D), 8101, dtype=dt), _rand((B, H, Sk, D), 8102, dtype=dt), _rand((B, H, Sk, D), 8103, dtype=dt)
    rng = np.random.default_rng(8)
    full = np.zeros((B, 1, Sq, Sk), dtype=np.float32)
    full[rng.random(full.shape) < 0.3] = fmin
    full[rng.random(full.shape) < 0.1] = -1.5      # an additive bias, not a mask
    full[0, 0, 7, :] = fmin                         # a row without a visible key
    padm = _pad_mask(B, Sk, [Sk, Sk - 200], fmin)
    tol = F16_TOL if dt == torch.float16 else (dict(atol=1e-3, rtol=5e-4) if dt == torch.float32 else BF16_TOL)
    for pad in (None, padm):
        name = ops.attn_variant(B, H, Sq, Sk, D, dt, base=base, full_mask=True, key_pad=pad is not None, scale=0.125, mask_min=fmin)
        assert name.startswith("flash16/"), name
        want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=0.125, base=base, full_mask=full, pad_mask=pad, clamp_min=True, mask_min=fmin)
        got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=ops.SoftmaxSpec(base), scale=0.125, full_mask=torch.from_numpy(full).cuda(),
                           key_pad_mask=None if pad is None else torch.from_numpy(pad).cuda(), clamp_min=True, mask_min=fmin)
        _check(got, want, tol=tol, msg=f"full mask, pad={pad is not None}, base={base}")
    assert ops.attn_variant(B, H, Sq, 512, D, dt, base=base, full_mask=True, scale=0.125, mask_min=fmin).startswith("mfma16/")


@pytest.mark.gpu
@pytest.mark.parametrize("S,dt", [(512, torch.float16), (704, torch.float16), (640, torch.float32), (128, torch.float16)])
@pytest.mark.parametrize("pad", [False, True])
def test_clipped_int8_chain_on_the_quantiser_grid(ops, S, dt, pad):
    """Clipped softmax together with the three fake-quantisers (the reference's `--attn_softmax clipped...` with `--quantize`,
    quantized_opt.py:151-210 around models/softmax.py:16-19): since round 3 on the quantiser grid too - the clip as one clamped fma
    between the exponential and the probability's index - in the full-row kernel and, for rows of more than 512 keys, in the two-pass
    form (before: the literal chain, 38 against 27 us on the OPT shape; the any-shape kernel on long rows).  Against the oracle."""
    B, H, D = 2, 2, 64
    fmin = float(np.finfo(np.float32).min)
    sm = "clippedsoftmax1(-.025:1)"
    q = (_rand((B, H, S, D), 9101, dtype=dt).float() * D ** -0.5).to(dt)
    k, v = _rand((B, H, S, D), 9102, dtype=dt), _rand((B, H, S, D), 9103, dtype=dt)
    padm = _pad_mask(B, S, [S, S - 41], fmin) if pad else None
    common = dict(causal=True, clamp_min=True, pad_mask=padm, mask_min=fmin, **SPECS[sm])
    vis = dict(common, pad_mask=None)
    _, fp = O.attn_core(_np32(q), _np32(k), _np32(v), want=("scores", "probs"), **vis)
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    d_c = O.quant_range_to_params(*np.percentile(O.attn_core(_np32(q), _np32(k), _np32(v), **vis), (0.001, 99.999)))
    want = O.attn_core(_np32(q), _np32(k), _np32(v), fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, **common)
    name = ops.attn_variant(B, H, S, S, D, dt, fq=True, clip=True, base=1, gamma=-0.025, causal=True, key_pad=pad, key_pad_boolean=pad, mask_min=fmin)
    assert name.startswith("flash16/" if S > 512 else "fast16/") and name.endswith("/fq2p" if S > 512 else "/fq"), name
    FQ = ops.FakeQuantSpec.from_delta
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=fmin,
                       key_pad_mask=None if padm is None else torch.from_numpy(padm).cuda(), key_pad_boolean=pad,
                       fq=ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c)))
    step = float(np.float32(d_c[0]))
    err = np.abs(_np32(got) - want)
    off = float((err > 0.5 * step).mean())
    assert np.isfinite(_np32(got)).all() and _le(off, OUT_OFF, "fused chain outputs off", n=err.size) and err.max() <= 2.05 * step + 2e-3, f"{off:.2e} off, max {err.max() / step:.2f} steps"


# ---------------------------------------------------------------------------------------------------------------------------------
# Round 4
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["i8", "fast_fq3", "flash_fq2p"])
def test_padding_masks_of_exactly_minus_1e4_hide_their_keys(ops, path):
    """HF's classic extended mask `(1 - mask) * -10000.0` holds EXACTLY -1e4; include/oeh.h (key_pad_boolean) and
    `attention.pad_is_boolean` call such an entry hidden (<= -1e4), and the three kernels that read the promise tested `< -1e4`:
    the padded keys attended.  The integer core's PAD variant, the full-row kernel's grid form with padding (FQ == 3) and the one-pass
    kernel's two-pass grid form with padding: a -1e4 mask must give bit for bit what a finfo.min mask gives (both mean "not there";
    every row keeps a visible key), and both must agree with the oracle run with the -1e4 mask literally (the reference's op order)."""
    B, H, D = 3, 2, 64
    S = 640 if path == "flash_fq2p" else 208
    fmin = float(np.finfo(np.float32).min)
    lens = [S, S - 75, 19]
    pad_hf = _pad_mask(B, S, lens, -10000.0)      # HF: (1 - mask) * -10000.0
    pad_min = _pad_mask(B, S, lens, fmin)
    assert (pad_hf[pad_hf != 0] == np.float32(-10000.0)).all()
    FQ = ops.FakeQuantSpec.from_delta
    dev = lambda t: torch.from_numpy(t).cuda()  # noqa: E731
    if path == "i8":
        g = torch.Generator().manual_seed(4101)
        x = [torch.randn((B, S, H * D), generator=g).numpy() * s_ for s_ in (1.0, 1.2, 0.9)]
        (qi, qd, qg), (ki, kd, kg), (vi, vd, vg) = (_quantise_to_grid(t) for t in x)
        heads = lambda t: np.ascontiguousarray(t.reshape(B, S, H, D).transpose(0, 2, 1, 3))  # noqa: E731
        qdh, kdh, vdh = heads(qd), heads(kd), heads(vd)
        common = dict(base=1, scale=8.0, scale_is_divisor=True)
    else:
        q, k, v = _rand((B, H, S, D), 4102), _rand((B, H, S, D), 4103), _rand((B, H, S, D), 4104)
        qdh, kdh, vdh = _np32(q), _np32(k), _np32(v)
        common = dict(base=1, scale=8.0, scale_is_divisor=True)
    ctx_fp, fp = O.attn_core(qdh, kdh, vdh, want=("scores", "probs"), **common)
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    d_c = O.quant_range_to_params(*np.percentile(ctx_fp, (0.001, 99.999)))
    want = O.attn_core(qdh, kdh, vdh, fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, pad_mask=pad_hf, **common)
    fq = ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c))
    sm = ops.SoftmaxSpec(1, False, 0.0, 1.0)
    if path == "i8":
        qc = ops.centre_indices(dev(qi)).view(B, S, H, D).permute(0, 2, 1, 3)
        kc = ops.centre_indices(dev(ki)).view(B, S, H, D).permute(0, 2, 1, 3)
        vt = ops.centre_indices(dev(vi)).view(B, S, H, D).permute(0, 2, 3, 1).contiguous()
        grids = (ops.QuantGrid(*qg), ops.QuantGrid(*kg), ops.QuantGrid(*vg))
        run = lambda pm: ops.attn_fwd_i8(qc, kc, vt, grids, fq=fq, out_dtype=torch.float32, softmax=sm, scale_div=8.0, mask_min=fmin, key_pad_mask=dev(pm))  # noqa: E731
    else:
        name = ops.attn_variant(B, H, S, S, D, torch.float16, fq=True, key_pad=True, key_pad_boolean=True, scale_div=8.0, mask_min=fmin)
        assert name.startswith("fast16/") if path == "fast_fq3" else (name.startswith("flash16/") and name.endswith("fq2p")), name
        run = lambda pm: ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=sm, scale_div=8.0, mask_min=fmin, key_pad_mask=dev(pm), key_pad_boolean=True, fq=fq)  # noqa: E731
    got_hf, got_min = run(pad_hf), run(pad_min)
    assert torch.equal(got_hf, got_min), f"{path}: a -1e4 entry is read differently from a finfo.min entry ({float((got_hf.float() - got_min.float()).abs().max()):.3e})"
    step = float(np.float32(d_c[0]))
    err = np.abs(_np32(got_hf) - want)
    off = float((err > 0.5 * step + 1e-3).mean())
    assert err.max() <= 2.05 * step + 2e-3 and _le(off, OUT_OFF, f"{path} outputs off", n=err.size), f"{path}: max {err.max() / step:.2f} steps, {off:.2e} off (padded keys attending?)"


@pytest.mark.gpu
@pytest.mark.parametrize("S", [256, 640])
def test_vanilla_softmax_with_non_absorbing_padding_and_very_negative_scores(ops, S):
    """the one-pass kernel's PAD variant under the VANILLA softmax.  (a) A fully padded sample whose mask entries are
    NOT absorbing (-1e4): every score is s - 1e4, the reference's probabilities are softmax(s), not uniform - the kernel must not
    take the "no visible key: mean of V" shortcut.  (b) A left-padded sample (finfo.min: first tile absorbed) whose visible scores
    are all below -100: against the initial reference 0 every exponential underflows; the first VISIBLE tile must set the row's
    reference (the row used to pass for one without a visible key).  Against the oracle."""
    B, H, D = 3, 2, 64
    fmin = float(np.finfo(np.float32).min)
    g = torch.Generator().manual_seed(4200 + S)
    q = (1.5 + 0.05 * torch.randn((B, H, S, D), generator=g)).half()
    k = (-1.5 + 0.05 * torch.randn((B, H, S, D), generator=g)).half()   # scores around -144
    v = _rand((B, H, S, D), 4201)
    padm = np.zeros((B, S), dtype=np.float32)
    padm[0, :] = -10000.0          # (a) fully padded, non-absorbing
    padm[1, :100] = fmin           # (b) left-padded: more than one 64-key tile absorbed
    padm[2, S - 50:] = -10000.0    # right-padded, non-absorbing entries
    assert ops.attn_variant(B, H, S, S, D, torch.float16, base=0, key_pad=True, mask_min=fmin).startswith("flash16/")
    want = O.attn_core(_np32(q), _np32(k), _np32(v), base=0, pad_mask=padm, mask_min=fmin)
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=ops.SoftmaxSpec(0), mask_min=fmin, key_pad_mask=torch.from_numpy(padm).cuda())
    assert np.isfinite(_np32(got)).all()
    _check(got, want, msg=f"vanilla + non-absorbing / left padding S={S}")
    mean_v = _np32(v)[0].mean(axis=1, keepdims=True)
    assert np.abs(want[0] - mean_v).max() > 1e-2   # (the case is not degenerate: the reference is NOT the mean of V there)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_fp32_output_of_the_16bit_kernels(ops, dt):
    """VERDICT r3 next #4a: `out_dtype=torch.float32` (include/oeh.h: o_dtype = OEH_F32 with 16-bit q / k / v) stores the one-pass
    and full-row kernels' fp32 accumulators - the arithmetic of the kernel that ships, before the output rounding.  The 16-bit
    output of the same call must be exactly that value rounded once; kernels without the switch refuse (no silent fallback)."""
    from outeffhop_amd._lib import OehError

    B, H, D = 2, 3, 64
    fmin = float(np.finfo(np.float32).min)
    cases = [("flash16/", 512, dict(softmax=ops.SoftmaxSpec(1), causal=True, clamp_min=True, mask_min=fmin), dict(base=1, causal=True, clamp_min=True)),
             ("fast16/", 256, dict(softmax=ops.SoftmaxSpec(1, True, -0.025, 1.1), causal=True, clamp_min=True, mask_min=fmin),
              dict(base=1, clip=True, gamma=-0.025, eta=1.1, causal=True, clamp_min=True)),
             ("fast16/", 128, dict(softmax=ops.SoftmaxSpec(1), scale_div=8.0, mask_min=fmin), dict(base=1, scale=8.0, scale_is_divisor=True))]
    for prefix, S, kw, okw in cases:
        q = (_rand((B, H, S, D), 4301 + S, dtype=torch.float32) * (D ** -0.5 if "scale_div" not in kw else 1.0)).to(dt)
        k, v = _rand((B, H, S, D), 4302 + S, dtype=dt), _rand((B, H, S, D), 4303 + S, dtype=dt)
        name = ops.attn_variant(B, H, S, S, D, dt, clip=kw["softmax"].clip, causal=kw.get("causal", False), scale_div=kw.get("scale_div", 0.0), mask_min=fmin)
        assert name.startswith(prefix), name
        acc = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), out_dtype=torch.float32, **kw)
        out = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw)
        assert acc.dtype == torch.float32 and acc.permute(0, 2, 1, 3).is_contiguous()
        assert torch.equal(out, acc.to(dt)), f"{name}: the stored output is not the accumulator rounded once"
        want = O.attn_core(_np32(q), _np32(k), _np32(v), **okw)
        err = float(np.abs(_np32(acc) - want).max())
        assert err <= (1e-3 if dt == torch.float16 else 8e-3), f"{name}: arithmetic error {err:.3e}"
    # a (B,1,Sq,Sk) mask on short rows runs the general kernel: no fp32-output form there
    q, k, v = _rand((1, 2, 64, D), 1, dtype=dt).cuda(), _rand((1, 2, 64, D), 2, dtype=dt).cuda(), _rand((1, 2, 64, D), 3, dtype=dt).cuda()
    with pytest.raises(OehError) as ei:
        ops.attn_fwd(q, k, v, full_mask=torch.zeros(1, 1, 64, 64, device="cuda"), out_dtype=torch.float32)
    assert ei.value.code == -95
    with pytest.raises(ValueError):
        ops.attn_fwd(q.float(), k.float(), v.float(), out_dtype=torch.float16)


@pytest.mark.gpu
def test_fp32_output_siblings_of_the_gated_padded_and_d128_kernels(ops):
    """the `O32` equality - the stored fp16 output IS the fp32 accumulator rounded once, and the
    accumulator is within 1e-3 of the reference - existed for the d = 64 plain / clipped forms only.  Now also: the in-kernel gate
    predictor (full-row kernel, BERT cfg5's shape class; one-pass kernel on 320-key rows), key padding on the one-pass kernel, and
    head dim 128 (both kernels).  Gated cases are held against the oracle run with the gate probabilities the kernel itself formed and
    wrote out (their own error against the fp32 predictor is bounded in test_gate_predictor_fused_*): this isolates the attention
    arithmetic, which is what the 1e-3 is about."""
    fmin = float(np.finfo(np.float32).min)
    dt = torch.float16

    def run(name_prefix, q, k, v, want_kw, kw, gate_mlp=None, arith=1e-3, variant_kw=None):
        B, H, Sq, D = q.shape
        Sk = k.shape[2]
        name = ops.attn_variant(B, H, Sq, Sk, D, dt, mask_min=fmin, **(variant_kw or {}))
        assert name.startswith(name_prefix), name
        mk = (lambda: dict(gate_mlp=ops.GatePredictor(gate_mlp.hidden, gate_mlp.w1, gate_mlp.b1, gate_mlp.w2, gate_mlp.b2, scaling=gate_mlp.scaling,
                                                       out=torch.empty_like(gate_mlp.out)))) if gate_mlp is not None else (lambda: {})
        a_kw = mk()
        acc = ops.attn_fwd(q, k, v, out_dtype=torch.float32, mask_min=fmin, **kw, **a_kw)
        o_kw = mk()
        out = ops.attn_fwd(q, k, v, mask_min=fmin, **kw, **o_kw)
        assert acc.dtype == torch.float32 and torch.equal(out, acc.to(dt)), f"{name}: the stored output is not the accumulator rounded once"
        if gate_mlp is not None:
            assert torch.equal(a_kw["gate_mlp"].out, o_kw["gate_mlp"].out)
            want_kw = dict(want_kw, gate=(a_kw["gate_mlp"].out.cpu().numpy() * np.float32(gate_mlp.scaling))[..., None])
        want = O.attn_core(_np32(q), _np32(k), _np32(v), **want_kw)
        err = float(np.abs(_np32(acc) - want).max())
        assert _le(err, arith, f"O32 arithmetic {name}"), f"{name}: arithmetic error {err:.3e} > {arith:.1e}"

    # (1) BERT order, key padding, per-token gate from per-head MLPs 64 -> 16 -> 1 evaluated in the kernel: the full-row kernel (cfg5's class)
    B, H, S, D = 4, 12, 128, 64
    view = lambda t: t.cuda().view(B, S, H, D).permute(0, 2, 1, 3)  # noqa: E731
    q, k, v = view(_rand((B, S, H * D), 6101)), view(_rand((B, S, H * D), 6102)), view(_rand((B, S, H * D), 6103))
    hidden = _rand((B, S, H * D), 6104).cuda()
    g = torch.Generator().manual_seed(6105)
    w1, b1 = (torch.randn((H, 16, D), generator=g) * 0.2).cuda(), (torch.randn((H, 16), generator=g) * 0.2).cuda()
    w2, b2 = (torch.randn((H, 16), generator=g) * 0.5).cuda(), torch.randn((H,), generator=g).cuda()
    padm = _pad_mask(B, S, [128, 97, 64, 33], fmin)
    gp = ops.GatePredictor(hidden, w1, b1, w2, b2, scaling=1.0, out=torch.empty((B, H, S), dtype=torch.float32, device="cuda"))
    run("fast16/", q, k, v, dict(scale=8.0, scale_is_divisor=True, pad_mask=padm, **SPECS["softmax1"]),
        dict(scale_div=8.0, key_pad_mask=torch.from_numpy(padm).cuda()), gate_mlp=gp, variant_kw=dict(scale_div=8.0, key_pad=True, gate_hidden=True))
    # (2) the one-pass kernel with the in-kernel gate predictor (OPT order, causal, 512-key rows)
    B, H, S = 2, 4, 512
    view = lambda t: t.cuda().view(B, S, H, D).permute(0, 2, 1, 3)  # noqa: E731
    q = view((_rand((B, S, H * D), 6111, dtype=torch.float32) * D ** -0.5).half())
    k, v = view(_rand((B, S, H * D), 6112)), view(_rand((B, S, H * D), 6113))
    hidden = _rand((B, S, H * D), 6114).cuda()
    w1h, b1h, w2h, b2h = w1[:H].contiguous(), b1[:H].contiguous(), w2[:H].contiguous(), b2[:H].contiguous()
    gp = ops.GatePredictor(hidden, w1h, b1h, w2h, b2h, scaling=1.0, out=torch.empty((B, H, S), dtype=torch.float32, device="cuda"))
    run("flash16/", q, k, v, dict(causal=True, clamp_min=True, **SPECS["softmax1"]), dict(causal=True, clamp_min=True), gate_mlp=gp,
        variant_kw=dict(causal=True, gate_hidden=True))
    # (3) key padding on the one-pass kernel (softmax_1, left- and right-padded samples)
    padm = np.zeros((B, S), dtype=np.float32)
    padm[0, 400:] = fmin
    padm[1, :70] = fmin
    run("flash16/", q, k, v, dict(pad_mask=padm, **SPECS["softmax1"]), dict(key_pad_mask=torch.from_numpy(padm).cuda()), variant_kw=dict(key_pad=True))
    # (4) head dim 128: the one-pass kernel ...
    B2, H2, S2, D2 = 2, 2, 512, 128
    q2 = (_rand((B2, H2, S2, D2), 6121, dtype=torch.float32) * D2 ** -0.5).half().cuda()
    k2, v2 = _rand((B2, H2, S2, D2), 6122).cuda(), _rand((B2, H2, S2, D2), 6123).cuda()
    run("flash16/", q2, k2, v2, dict(causal=True, clamp_min=True, **SPECS["softmax1"]), dict(causal=True, clamp_min=True), variant_kw=dict(causal=True))
    # ... and the full-row kernel (short rows)
    q3, k3, v3 = q2[:, :, :96].contiguous(), k2[:, :, :96].contiguous(), v2[:, :, :96].contiguous()
    run("fast16/", q3, k3, v3, dict(**SPECS["vanilla"]), dict(softmax=_spec(ops, "vanilla")))


@pytest.mark.gpu
def test_int8_storage_randomised_sweep_against_the_oracle(ops):
    """VERDICT r3 weak #3 / next #4b: the ragged shapes of `test_int8_storage_randomised_sweep` (cross attention with a cache offset,
    zero points at 0 and 255 - the CQ2 variant -, zero points on both sides of 128, context quantiser before / after the gate / off,
    strided (B,S,H*64) storage, NT = 8 / 16 / 32) against `O.attn_core` on the DEQUANTISED values - the reference's op chain, not this
    repository's own fake-quant kernels: an output may sit one context-grid step away where a quantiser input was within an ulp of a
    rounding boundary (the integer products are exact where the reference rounds every product), in at most 1e-4 ... 5e-4 of the
    outputs, never further; with the context quantiser off the outputs agree to 2e-5 + 2e-5 |ref|."""
    rng = np.random.default_rng(2025)
    fmin = float(np.finfo(np.float32).min)
    cases = [  # (B, H, Sq, Sk, causal, base, zq, zk, zv, ctx quantiser: "before" | "after" | None, gate)
        (2, 3, 144, 144, True, 1, 0.0, 131.0, 120.0, "before", True),      # zero point 0: 128 - zp = 128 (CQ2)
        (1, 4, 77, 272, True, 0, 255.0, 97.0, 160.0, "after", True),       # zero point 255; cross attention with a cache offset
        (3, 2, 200, 48, False, 1, 128.0, 0.0, 255.0, "before", False),     # k / v grids at the ends; cross attention, NT = 8
        (2, 2, 33, 512, True, 1, 120.0, 160.0, 131.0, None, True),         # decoder step block against a 512-key cache, no context quantiser
        (1, 3, 256, 256, False, 0, 97.0, 128.0, 100.0, "after", True),     # NT = 16, vanilla
        (2, 1, 400, 400, True, 1, 131.0, 120.0, 97.0, "before", False),    # ragged NT = 32
    ]
    worst_off = 0.0
    for n, (B, H, Sq, Sk, causal, base, zq, zk, zv, cq, gated) in enumerate(cases):
        g = torch.Generator().manual_seed(7000 + n)
        sq, sk_, sv = (0.031 * (0.2 if zq in (0.0, 255.0) else 1.0)), 0.027, 0.035
        qi = torch.randint(0, 256, (B, Sq, H * 64), generator=g, dtype=torch.int64).to(torch.uint8)
        ki = torch.randint(0, 256, (B, Sk, H * 64), generator=g, dtype=torch.int64).to(torch.uint8)
        vi = torch.randint(0, 256, (B, Sk, H * 64), generator=g, dtype=torch.int64).to(torch.uint8)
        deq = lambda idx, s_, z_: ((idx.float() - z_) * np.float32(s_))  # noqa: E731
        hv = lambda t, S_: t.view(B, S_, H, 64).permute(0, 2, 1, 3)  # noqa: E731
        scaling = 0.125
        qd, kd, vd = hv(deq(qi, sq, zq), Sq) * scaling, hv(deq(ki, sk_, zk), Sk), hv(deq(vi, sv, zv), Sk)
        s_grid, p_grid, c_grid = (0.09, float(rng.choice([128.0, 100.0, 140.0]))), (1.0 / 255.0, 0.0), (0.03, 126.0)
        gate = torch.rand((B, H, Sq, 1), generator=g) if gated else None
        okw = dict(base=base, causal=causal, clamp_min=causal, fq_scores=s_grid, fq_probs=p_grid, fq_ctx=c_grid if cq else None,
                   ctx_quant_before_gate=(cq == "before"), gate=None if gate is None else gate.numpy())
        want = O.attn_core(qd.numpy(), kd.numpy(), vd.numpy(), **okw)
        FQ = ops.FakeQuantSpec
        fq = ops.AttnFakeQuant(FQ(*s_grid), FQ(*p_grid), FQ(*c_grid) if cq else None, ctx_before_gate=(cq == "before"))
        qc, kc = hv(ops.centre_indices(qi.cuda()), Sq), hv(ops.centre_indices(ki.cuda()), Sk)
        vt = ops.centre_indices(vi.cuda()).view(B, Sk, H, 64).permute(0, 2, 3, 1).contiguous()
        got = ops.attn_fwd_i8(qc, kc, vt, (ops.QuantGrid(sq, zq), ops.QuantGrid(sk_, zk), ops.QuantGrid(sv, zv)), out_dtype=torch.float32, scale=scaling,
                              softmax=ops.SoftmaxSpec(base, False, 0.0, 1.0), causal=causal, clamp_min=causal, mask_min=fmin,
                              gate=None if gate is None else gate.cuda(), fq=fq)
        err = np.abs(_np32(got) - want)
        if cq:
            step = 0.03 * (float(gate.max()) if (gate is not None and cq == "before") else 1.0)
            off = float((err > 1e-5 + 1e-5 * np.abs(want)).mean())
            worst_off = max(worst_off, off)
            assert err.max() <= 1.01 * step + 1e-5 and off <= 5e-4, f"case {n}: max err {err.max():.3e} (step {step:.3e}), {off:.2e} of the outputs off their grid point"
        else:
            assert (err <= 2e-5 + 2e-5 * np.abs(want)).all(), f"case {n}: max err {err.max():.3e} without a context quantiser"
    print(f"int8 storage vs the oracle on ragged shapes: at most {worst_off:.2e} of the outputs one step off")


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["flash_mq", "short_rows", "ragged_causal", "clip_two_pass", "int8_two_pass", "fp32_short_rows", "small_shape"])
def test_both_sides_of_every_dispatch_rule_meet_the_contract(ops, rule):
    """`pick_variant`'s size thresholds (profiles/r04_dispatch_ab.txt times both sides of each) only choose between
    kernels that compute the same thing - so a rule can move after a re-measurement without a correctness review.  At a boundary shape
    of every rule both sides are forced through `oeh_debug_set_variant` and checked against the ORACLE under the storage dtype's
    contract; where the two kernels share their arithmetic (one-pass MQ1 / MQ2) the outputs are bitwise equal."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    fmin = float(np.finfo(np.float32).min)
    H, D = 4, 64
    # rule: (B, S, dtype, causal, clip, int8, pad, side A (off, mq), side B (off, mq), bitwise)
    table = {
        "flash_mq": (2, 512, torch.float16, True, False, False, False, (0, 1), (0, 2), True),
        "short_rows": (3, 128, torch.float16, False, False, False, True, (2, 0), (256, 0), False),
        "ragged_causal": (2, 320, torch.float16, True, False, False, False, (2, 0), (256, 0), False),
        "clip_two_pass": (2, 512, torch.float16, True, True, False, False, (0, 0), (256, 0), False),
        "int8_two_pass": (2, 512, torch.float16, True, False, True, False, (0, 0), (256, 0), False),
        "fp32_short_rows": (3, 128, torch.float32, False, False, False, True, (64, 0), (256, 0), False),
        "small_shape": (70, 28, torch.float32, False, False, False, False, (1 << 5, 0), (1 << 10, 0), False),
    }
    B, S, dt, causal, clip, int8, pad, side_a, side_b, bitwise = table[rule]
    q = (_rand((B, H, S, D), 4401, dtype=torch.float32) * D ** -0.5).to(dt)
    k, v = _rand((B, H, S, D), 4402, dtype=dt), _rand((B, H, S, D), 4403, dtype=dt)
    padm = _pad_mask(B, S, [S - 11 * (b + 1) for b in range(B)], fmin) if pad else None
    okw = dict(base=1, causal=causal, clamp_min=causal, pad_mask=padm, mask_min=fmin)
    if clip:
        okw.update(clip=True, gamma=-0.025, eta=1.1)
    fq = None
    if int8:
        _, fp = O.attn_core(_np32(q), _np32(k), _np32(v), want=("scores", "probs"), **okw)
        d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
        d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
        d_c = O.quant_range_to_params(*np.percentile(O.attn_core(_np32(q), _np32(k), _np32(v), **okw), (0.001, 99.999)))
        okw.update(fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c)
        FQ = ops.FakeQuantSpec.from_delta
        fq = ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c))
    want = O.attn_core(_np32(q), _np32(k), _np32(v), **okw)
    kw = dict(softmax=ops.SoftmaxSpec(1, clip, -0.025 if clip else 0.0, 1.1 if clip else 1.0), causal=causal, clamp_min=causal, mask_min=fmin,
              key_pad_mask=None if padm is None else torch.from_numpy(padm).cuda(), fq=fq)
    outs, names = [], []
    try:
        for side in (side_a, side_b):
            lib.oeh_debug_set_variant(*side)
            names.append(ops.attn_variant(B, H, S, S, D, dt, fq=int8, clip=clip, causal=causal, key_pad=pad, mask_min=fmin))
            outs.append(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw))
    finally:
        lib.oeh_debug_set_variant(0, 0)
    assert names[0] != names[1] or rule == "flash_mq", f"{rule}: both sides ran {names[0]}"
    for name, got in zip(names, outs):
        if int8:
            step = float(np.float32(d_c[0]))
            err = np.abs(_np32(got) - want)
            assert err.max() <= 2.05 * step + 2e-3 and _le(float((err > 0.5 * step + 1e-3).mean()), OUT_OFF, f"{rule} {name} outputs off", n=err.size), f"{rule} {name}: {err.max() / step:.2f} steps"
        elif dt == torch.float32:
            _check(got, want, tol=dict(atol=5e-4, rtol=5e-4), msg=f"{rule} {name}")
        else:
            _check(got, want, msg=f"{rule} {name}")
    if bitwise:
        assert torch.equal(outs[0], outs[1]), f"{rule}: {names} differ"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.float32])
@pytest.mark.parametrize("kind", ["full_mask", "vanilla_pad"])
def test_clipped_softmax_on_long_rows_with_masks_two_pass(ops, kind, dt):
    """two cliffs to the any-shape kernel (one workgroup per query row, ~100x slower) on rows of more than 512 keys,
    closed on the one-pass kernel's two-pass clipped form (PAD variants): a (B,1,Sq,Sk) additive mask (read per block, like the plain
    one-pass form does), and key padding under the VANILLA clipped softmax - where a sample without a visible key is uniform over all
    Sk keys in the reference, i.e. clip(w / Sk + gamma, 0, 1) times the sum of V (models/softmax.py:10-13).  Against the oracle."""
    B, H, S, D = 3, 2, 704, 64
    fmin = float(np.finfo(np.float32).min)
    q = (_rand((B, H, S, D), 4801, dtype=torch.float32) * 0.125).to(dt)
    k, v = _rand((B, H, S, D), 4802, dtype=dt), _rand((B, H, S, D), 4803, dtype=dt)
    tol = F16_TOL if dt == torch.float16 else dict(atol=5e-4, rtol=5e-4)
    for sm_name, base in (("clippedsoftmax1(-.025:1)", 1), ("clipped(-.003:1.003)", 0)):
        if kind == "vanilla_pad" and base == 1:
            continue
        sp = SPECS[sm_name]
        if kind == "full_mask":
            full = np.zeros((B, 1, S, S), dtype=np.float32)
            full[:, 0] = np.triu(np.full((S, S), fmin, dtype=np.float32), 1)      # causal ...
            full[1, 0, :, 600:] = fmin                                               # ... with padded keys in one sample
            full[2, 0, 5, :] = fmin                                                  # ... and one row without any visible key
            okw = dict(full_mask=full, clamp_min=True)
            kw = dict(full_mask=torch.from_numpy(full).cuda(), clamp_min=True)
            name = ops.attn_variant(B, H, S, S, D, dt, clip=True, base=base, full_mask=True, mask_min=fmin)
        else:
            padm = _pad_mask(B, S, [S, S - 130, 0], fmin)                            # the last sample has no visible key at all
            okw = dict(pad_mask=padm)
            kw = dict(key_pad_mask=torch.from_numpy(padm).cuda())
            name = ops.attn_variant(B, H, S, S, D, dt, clip=True, base=base, key_pad=True, mask_min=fmin)
        assert name.startswith("flash16/") and name.endswith("clip2p"), name
        want = O.attn_core(_np32(q), _np32(k), _np32(v), mask_min=fmin, **okw, **sp)
        got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), softmax=_spec(ops, sm_name), mask_min=fmin, **kw)
        assert np.isfinite(_np32(got)).all()
        _check(got, want, tol=tol, msg=f"{kind} {sm_name} {dt}")


@pytest.mark.gpu
@pytest.mark.parametrize("sm_name", ["clipped(-.003:1.003)", "clippedsoftmax1(-.025:1)", "vanilla"])
def test_left_padded_rows_with_strongly_negative_scores_on_long_rows(ops, sm_name):
    """a LEFT-padded sample whose visible scores are all below about -87.  The statistics pass of the two-pass clipped
    form kept its initial reference 0 behind the fully masked first tile(s): every exponential underflowed, the row sum came out 0 and
    under the vanilla clipped softmax the row was taken for one without a visible key (a uniform row times the clip) instead of the
    real softmax.  It now moves the reference at a row's first VISIBLE tile, like the plain one-pass form (checked here too).  Rows of
    704 keys (beyond the full-row kernels), the first 200 padded; q . k around -150 for the visible keys."""
    B, H, S, D = 2, 2, 704, 64
    fmin = float(np.finfo(np.float32).min)
    rng = np.random.default_rng(77)
    u = rng.standard_normal(D).astype(np.float32)
    u /= np.linalg.norm(u)
    q = (0.05 * rng.standard_normal((B, H, S, D)).astype(np.float32) + 12.5 * u).astype(np.float16)
    k = (0.05 * rng.standard_normal((B, H, S, D)).astype(np.float32) - 12.0 * u).astype(np.float16)   # q . k ~ -150 +- 1
    v = rng.standard_normal((B, H, S, D)).astype(np.float16)
    padm = np.zeros((B, S), dtype=np.float32)
    padm[0, :200] = fmin   # left padding over three whole 64-key tiles and a part of the fourth
    padm[1, :64] = fmin
    sp = SPECS[sm_name]
    name = ops.attn_variant(B, H, S, S, D, torch.float16, clip=bool(sp["clip"]), base=sp["base"], key_pad=True, mask_min=fmin)
    assert name.startswith("flash16/") and (name.endswith("clip2p") == bool(sp["clip"])), name
    want = O.attn_core(q.astype(np.float32), k.astype(np.float32), v.astype(np.float32), pad_mask=padm, mask_min=fmin, **sp)
    got = ops.attn_fwd(torch.from_numpy(q).cuda(), torch.from_numpy(k).cuda(), torch.from_numpy(v).cuda(), softmax=_spec(ops, sm_name),
                       key_pad_mask=torch.from_numpy(padm).cuda(), mask_min=fmin)
    assert np.isfinite(_np32(got)).all()
    if sp["base"] == 0:  # the reference's rows are real softmax rows over the visible keys, far from the uniform row the bug produced
        uniform = v.astype(np.float32).mean(axis=2, keepdims=True)
        assert np.abs(want - uniform).max() > 0.05
    _check(got, want, tol=F16_TOL, msg=f"left padding, scores ~ -150, {sm_name}")


@pytest.mark.gpu
def test_repeated_calls_reuse_a_prebuilt_descriptor(ops):
    """Round 5: `ops.attn_fwd` keeps the C descriptor of a plain call (no fused quantisers, no in-kernel predictor, no (B,1,Sq,Sk) mask) per geometry and
    option set and, on the next call of that kind, only patches the data / mask / gate pointers (13 -> ~5 us of host time per call; the fp16 BERT-base
    layer is host-bound in eager mode).  The reused descriptor must give the bits of a freshly built one: other data, another mask of the same geometry,
    another gate tensor, strided (B,S,H*d) views, and no cross-talk between option sets that share a geometry."""
    fmin = float(np.finfo(np.float32).min)
    B, H, S, D = 4, 6, 128, 64

    def fresh(*a, **k):
        ops.FAST_CALLS = False
        try:
            return ops.attn_fwd(*a, **k)
        finally:
            ops.FAST_CALLS = True

    view = lambda t: t.cuda().view(B, S, H, D).permute(0, 2, 1, 3)  # noqa: E731
    table = ops._fast_tls.table
    table.clear()
    sets = [tuple(view(_rand((B, S, H * D), 9000 + 10 * i + j)) for j in range(3)) for i in range(3)]
    pads = [torch.from_numpy(_pad_mask(B, S, lens, fmin)).cuda() for lens in ([128, 97, 64, 1], [5, 128, 33, 100], [128, 128, 128, 128])]
    gates = [torch.rand((B, H, S, 1), generator=torch.Generator().manual_seed(9100 + i)).cuda() for i in range(3)]
    g_head = torch.rand((1, H, 1, 1), generator=torch.Generator().manual_seed(9200)).cuda()   # a broadcast gate (unconditional per head)
    variants = [
        dict(scale_div=8.0, mask_min=fmin),
        dict(scale_div=8.0, mask_min=fmin, softmax=ops.SoftmaxSpec(0)),
        dict(scale=0.125, causal=True, clamp_min=True, mask_min=fmin),
        dict(scale=0.125, causal=True, clamp_min=True, mask_min=fmin, softmax=ops.SoftmaxSpec(1, True, -0.025, 1.1)),
    ]
    for kw in variants:
        for i, (q, k, v) in enumerate(sets):
            for extra in (dict(), dict(key_pad_mask=pads[i]), dict(gate=gates[i]), dict(key_pad_mask=pads[(i + 1) % 3], gate=g_head)):
                if "key_pad_mask" in extra and kw.get("causal"):
                    extra = dict(extra, key_pad_boolean=False)
                got = ops.attn_fwd(q, k, v, **kw, **extra)
                want = fresh(q, k, v, **kw, **extra)
                assert torch.equal(got, want), (kw, list(extra), i)
    assert 8 <= len(table) <= 16   # one descriptor per (options, mask / gate presence and geometry), reused across data sets
    # a mask in another dtype or layout, a caller's `out`, fused quantisers: the full path (and correct)
    q, k, v = sets[0]
    n0 = len(table)
    assert torch.equal(ops.attn_fwd(q, k, v, scale_div=8.0, mask_min=fmin, key_pad_mask=pads[0].double()), fresh(q, k, v, scale_div=8.0, mask_min=fmin, key_pad_mask=pads[0]))
    assert torch.equal(ops.attn_fwd(q, k, v, scale_div=8.0, mask_min=fmin, key_pad_mask=pads[0].view(B, 1, 1, S)), fresh(q, k, v, scale_div=8.0, mask_min=fmin, key_pad_mask=pads[0]))
    assert len(table) == n0
    with torch.enable_grad():   # autograd on: never the cached call (and a grad-requiring input still raises)
        from outeffhop_amd._lib import OehError
        with pytest.raises(OehError, match="forward-only"):
            ops.attn_fwd(q.clone().requires_grad_(True), k, v, scale_div=8.0, mask_min=fmin)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Round 6: the OUTLIER regime - what the reference exists to measure (kurtosis / inf-norm of attention activations:
# transformers_language/utils.py:9-20, validate_clm.py:596-621).  Every parity test above draws q, k, v from N(0, 1); here they are
# heavy-tailed, carry outlier channels, saturate the 8-bit grids, or put a row's maximum in its LAST key tile by far more than the lazy
# reference's 2^8 threshold.
#
# Contract for 16-bit storage in this regime, stated once and asserted below (measured on MI355X: margins of 3x ... 18x, printed per case):
#     |hip - oracle| <= A * max(1, |V|max) + ulp_storage(oracle) / 2,     A = 1e-3 (fp16), 8e-3 (bf16);  fp32 storage: 5e-4 * max(1, |V|max) + 5e-4 |oracle|
# with |V|max the largest |v| of the (b, h) slice.  Why it scales with V: the probabilities enter the second product rounded to the storage
# dtype (2^-11 relative for fp16), so the absolute error of sum_j p_j v_j is at most 2^-11 * sum_j p_j |v_j| <= 2^-11 * |V|max - an ABSOLUTE
# 1e-3 cannot hold once |V| > 2, by construction.  With N(0, 1) inputs the factor is 1 and this is north_star's 1e-3.
# Large scores (|s| up to 180 here) cost nothing extra: the kernels subtract the row reference in fp32 before the exponential, as the
# reference does.  The float64 evaluation of the same formula is printed beside each case: with outlier channels the reference's own fp32
# arithmetic (the oracle) sits 1e-3 ... 2e-3 from it - the same order as the kernels' distance to the oracle.
def _outlier_qkv(kind, B, H, S, D, seed):
    """float32 (q already multiplied by D ** -0.5: OPT order), k, v for one outlier flavour."""
    rs = np.random.RandomState(seed)
    sh = (B, H, S, D)
    if kind == "normal":         # unit variance (the baseline the other flavours are compared with)
        q, k, v = rs.standard_normal(sh), rs.standard_normal(sh), rs.standard_normal(sh)
    elif kind == "student_t3":   # heavy tails everywhere (kurtosis -> infinity)
        q, k, v = rs.standard_t(3, sh), rs.standard_t(3, sh), rs.standard_t(3, sh)
    elif kind == "channel":      # outlier channels of the hidden state show up in q, k and v alike (x6 / x20 / x60 on 2 of the 64 head channels)
        q, k, v = rs.standard_normal(sh), rs.standard_normal(sh), rs.standard_normal(sh)
        q[..., [5, 41]] *= 6.0
        k[..., [5]] *= 20.0
        v[..., [5, 41]] *= 60.0
    elif kind == "last_tile_jump":   # the last 64 keys score ~ +25 (natural units) above everything before: the reference moves in the LAST tile, alpha ~ e^-25
        q, k, v = rs.standard_normal(sh), rs.standard_normal(sh), rs.standard_normal(sh) * 3.0
        u = rs.standard_normal(D)
        u /= np.linalg.norm(u)
        q += 8.0 * u
        k[:, :, S - 64:] += 25.0 * u
    elif kind == "ascending":    # scores grow ~0.25 per key: every 64-key tile lifts the row maximum by ~16 (23 in log2 units): the reference moves every tile
        q, k, v = rs.standard_normal(sh) * 0.3, rs.standard_normal(sh) * 0.3, rs.standard_t(3, sh)
        u = rs.standard_normal(D)
        u /= np.linalg.norm(u)
        q += 8.0 * u
        k += (0.25 * np.arange(S))[None, None, :, None] * u
    else:
        raise ValueError(kind)
    return (q * D ** -0.5).astype(np.float32), k.astype(np.float32), v.astype(np.float32)


def _attn_f64(q, k, v, *, base, clip, gamma, eta, causal):
    """the reference formula in float64 on the same (storage-rounded) inputs: how far the fp32 oracle itself is from exact arithmetic"""
    s = np.matmul(q.astype(np.float64), np.swapaxes(k.astype(np.float64), -1, -2))
    if causal:
        S_ = s.shape[-1]
        s = np.where(np.triu(np.ones((S_, S_), bool), 1), -np.inf, s)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    p = e / (e.sum(-1, keepdims=True) + (np.exp(-m) if base else 0.0))
    if clip:
        p = np.clip(p * (eta - gamma) + gamma, 0, 1)
    return np.matmul(p, v.astype(np.float64)), np.abs(np.where(np.isfinite(s), s, 0.0)).max(axis=(-1, -2))


def _outlier_limit(want, vmax, dt):
    scale = np.maximum(1.0, vmax)[..., None, None]
    if dt == torch.float32:
        return 5e-4 * scale + 5e-4 * np.abs(want), scale
    if dt == torch.float16:
        return 1e-3 * scale + 0.5 * np.spacing(np.abs(want).astype(np.float16)).astype(np.float32), scale
    return 8e-3 * scale + np.abs(want) * 2.0 ** -8, scale


@pytest.mark.parametrize("kind", ["normal", "student_t3", "channel", "last_tile_jump", "ascending"])
@pytest.mark.parametrize("path", ["one_pass", "one_pass_bf16", "full_row_clip", "vanilla", "fp32"])
def test_outlier_inputs_16bit_and_fp32_storage(ops, kind, path):
    """one-pass (softmax1, fp16 / bf16), full-row clipped, vanilla softmax, fp32 storage - S = 512 causal, the headline geometry."""
    B, H, S, D = 2, 3, 512, 64
    fmin = float(np.finfo(np.float32).min)
    dt = {"one_pass_bf16": torch.bfloat16, "fp32": torch.float32}.get(path, torch.float16)
    sm = {"full_row_clip": "clippedsoftmax1(-.025:1)", "vanilla": "vanilla"}.get(path, "softmax1")
    q, k, v = (torch.from_numpy(a).to(dt) for a in _outlier_qkv(kind, B, H, S, D, 4000 + len(kind)))
    qn, kn, vn = _np32(q), _np32(k), _np32(v)
    want = O.attn_core(qn, kn, vn, causal=True, clamp_min=True, **SPECS[sm])
    exact, smax = _attn_f64(qn, kn, vn, causal=True, **SPECS[sm])
    vmax = np.abs(vn).max(axis=(-1, -2))
    kw = dict(softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=fmin)
    var = ops.attn_variant(B, H, S, S, D, dt, clip=SPECS[sm]["clip"], causal=True)
    got = _np32(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw))
    assert np.isfinite(got).all(), f"{kind}/{path}: non-finite output"
    err = np.abs(got - want)
    lim, scale = _outlier_limit(want, vmax, dt)
    rel = err / np.maximum(np.abs(want), 1e-3 * scale)
    e_hip64, e_or64 = np.abs(got - exact).max(), np.abs(want - exact).max()
    print(f"outlier {kind:15s} {path:14s} [{var}] |V|max {vmax.max():6.1f} |s|max {smax.max():6.1f}: abs err {err.max():.2e} (worst err/limit {float((err / lim).max()):.2f}), "
          f"rel err {rel.max():.2e}; vs float64: kernel {e_hip64:.2e}, fp32 oracle {e_or64:.2e}")
    _le(float((err / lim).max()), 1.0, f"outlier[{kind},{path}] err/limit")
    assert (err <= lim).all(), f"{kind}/{path}: max abs err {err.max():.3e}, worst excess {float((err - lim).max()):.3e} (|V|max {vmax.max():.1f})"
    if dt == torch.float16 and path in ("one_pass", "full_row_clip"):   # the arithmetic before the output rounding: the same scaled bound without the ulp term
        a32 = _np32(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), out_dtype=torch.float32, **kw))
        assert (np.abs(a32 - want) <= 1e-3 * scale).all(), f"{kind}/{path}: arithmetic error {np.abs(a32 - want).max():.3e}"
        print(f"        before the output rounding: abs err {np.abs(a32 - want).max():.2e} = {float((np.abs(a32 - want) / scale).max()):.2e} x max(1, |V|max)")


@pytest.mark.parametrize("kind", ["student_t3", "channel", "scores_x4"])
@pytest.mark.parametrize("dt", [torch.float16, torch.float32])
def test_outlier_inputs_fused_int8_chain(ops, kind, dt):
    """The fused fake-quant chain (fp16 and fp32 storage) on heavy-tailed / outlier-channel inputs and on SURVEY 8d cfg4's "scores x 4" variant
    (the grids are calibrated on the unscaled data, then q is multiplied by 4: both ends of the score grid and the top of the probability grid
    saturate).  Index dumps against the oracle: differences of one step only, rarer than FLIP_RATE; outputs on the oracle's grid point outside
    flipped elements."""
    B, H, S, D = 2, 2, 512, 64
    fmin = float(np.finfo(np.float32).min)
    base_kind = "normal" if kind == "scores_x4" else kind
    q, k, v = (torch.from_numpy(a).to(dt) for a in _outlier_qkv(base_kind, B, H, S, D, 4100 + len(kind)))
    common = dict(base=1, causal=True, clamp_min=True)
    ctx_fp, fp = O.attn_core(_np32(q), _np32(k), _np32(v), want=("scores", "probs"), **common)
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    d_c = O.quant_range_to_params(*np.percentile(ctx_fp, (0.001, 99.999)))
    if kind == "scores_x4":
        q = (q.float() * 4.0).to(dt)
    want, ex = O.attn_core(_np32(q), _np32(k), _np32(v), fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, ctx_quant_before_gate=True,
                           want=("scores_idx", "probs_idx", "ctx_idx"), **common)
    dumps = [torch.zeros((B, H, S, S), dtype=torch.uint8, device="cuda"), torch.zeros((B, H, S, S), dtype=torch.uint8, device="cuda"),
             torch.zeros((B, H, S, D), dtype=torch.uint8, device="cuda")]
    FQ = ops.FakeQuantSpec.from_delta
    fq = ops.AttnFakeQuant(FQ(*d_s, dump=dumps[0]), FQ(*d_p, dump=dumps[1]), FQ(*d_c, dump=dumps[2]), ctx_before_gate=True)
    kw = dict(causal=True, clamp_min=True, mask_min=fmin)
    got = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), fq=fq, **kw)
    rates = []
    for name, dump in zip(("scores", "probs", "ctx"), dumps):
        want_idx = ex[f"{name}_idx"]
        mx, rate = _flip_stats(dump.cpu().numpy(), want_idx)
        rates.append(f"{name} flips {rate:.1e} (at 0 / 255: {float((want_idx == 0).mean()):.1%} / {float((want_idx == 255).mean()):.2%})")
        assert mx <= 1 and _le(rate, FLIP_RATE, f"outlier_int8[{kind},{dt}] {name} flip rate", n=dump.numel()), f"{kind} {name}: max index diff {mx}, flip rate {rate:.2e}"
    step = float(np.float32(d_c[0]))
    err = np.abs(_np32(got) - want)
    tol = 1e-3 + 1e-3 * np.abs(want) if dt == torch.float16 else 1e-5 + 1e-6 * np.abs(want)
    off = float((err > tol).mean())
    print(f"outlier int8 chain {kind:11s} {str(dt)[6:]:8s}: {', '.join(rates)}; outputs off their grid point {off:.1e}, max err {err.max() / step:.2f} steps")
    assert _le(off, OUT_OFF, f"outlier_int8[{kind},{dt}] outputs off", n=err.size) and err.max() <= 1.05 * step + 2e-3
    # the production form (no dumps) gives the same bits
    got2 = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), fq=ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c), ctx_before_gate=True), **kw)
    assert torch.equal(got, got2)


@pytest.mark.parametrize("kind", ["student_t3", "channel", "scores_x4"])
def test_outlier_inputs_int8_storage(ops, kind):
    """The integer-matrix-core kernel (INT8 storage) with q / k / v grids calibrated on heavy-tailed / outlier-channel activations - the
    percentile range clips the tails, so many indices sit at 0 / 255 - and with the score grid saturated ("scores x 4": the q grid's scale
    multiplied by 4 after calibration).  Against the oracle on the dequantised values: at most one context-grid step, rarely."""
    B, H, S, D = 2, 3, 512, 64
    fmin = float(np.finfo(np.float32).min)
    base_kind = "normal" if kind == "scores_x4" else kind
    qf, kf, vf = _outlier_qkv(base_kind, B, H, S, D, 4200 + len(kind))
    flat = lambda t: np.ascontiguousarray(t.transpose(0, 2, 1, 3).reshape(B, S, H * D))  # noqa: E731
    scaling = D ** -0.5
    # grids from the 99th percentile: ~2 % of the indices clip to 0 / 255 (a range estimator that ignores the tails, or a stale range)
    (qi, qd, qg), (ki, kd, kg), (vi, vd, vg) = (_quantise_to_grid(flat(t), pct=99.0) for t in (qf / np.float32(scaling), kf, vf))
    heads = lambda t: np.ascontiguousarray(t.reshape(B, S, H, D).transpose(0, 2, 1, 3))  # noqa: E731
    qdh, kdh, vdh = heads(qd) * np.float32(scaling), heads(kd), heads(vd)
    common = dict(base=1, causal=True, clamp_min=True)
    ctx_fp, fp = O.attn_core(qdh, kdh, vdh, want=("scores", "probs"), **common)
    d_s = O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999)))
    d_p = O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999)))
    d_c = O.quant_range_to_params(*np.percentile(ctx_fp, (0.001, 99.999)))
    if kind == "scores_x4":
        qg = (qg[0] * 4.0, qg[1])
        qdh = qdh * np.float32(4.0)
    want = O.attn_core(qdh, kdh, vdh, fq_scores=d_s, fq_probs=d_p, fq_ctx=d_c, ctx_quant_before_gate=True, **common)
    FQ = ops.FakeQuantSpec.from_delta
    fq = ops.AttnFakeQuant(FQ(*d_s), FQ(*d_p), FQ(*d_c), ctx_before_gate=True)
    dev = lambda t: torch.from_numpy(t).cuda()  # noqa: E731
    qc = ops.centre_indices(dev(qi)).view(B, S, H, D).permute(0, 2, 1, 3)
    kc = ops.centre_indices(dev(ki)).view(B, S, H, D).permute(0, 2, 1, 3)
    vt = ops.centre_indices(dev(vi)).view(B, S, H, D).permute(0, 2, 3, 1).contiguous()
    grids = (ops.QuantGrid(*qg), ops.QuantGrid(*kg), ops.QuantGrid(*vg))
    got = ops.attn_fwd_i8(qc, kc, vt, grids, fq=fq, out_dtype=torch.float32, softmax=ops.SoftmaxSpec(1, False, 0.0, 1.0), scale=scaling,
                          causal=True, clamp_min=True, mask_min=fmin)
    step = float(np.float32(d_c[0]))
    err = np.abs(_np32(got) - want)
    off = float((err > 1e-6 + 1e-6 * np.abs(want)).mean())
    sat = [float(((t == 0) | (t == 255)).mean()) for t in (qi, ki, vi)]
    print(f"outlier int8 storage {kind:11s}: q/k/v indices saturated {sat[0]:.2%} / {sat[1]:.2%} / {sat[2]:.2%}; outputs off their grid point {off:.1e}, max err {err.max() / step:.2f} steps")
    assert err.max() <= 1.01 * step + 1e-6 and _le(off, 1e-3, f"outlier_i8[{kind}] outputs off", n=err.size)
