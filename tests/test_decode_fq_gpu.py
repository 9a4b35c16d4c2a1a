"""Split-key decode attention with the fused INT8 chain (ops.attn_decode(fq=...) / oeh_attn_decode_fq) on the GPU against the CPU oracle on the
16-bit-rounded inputs - index dumps and outputs -, against ops.attn_decode / ops.attn_fwd, and the quantised OPT module's generation steps.
`-m gpu`.

Bounds - the project's (tests/test_attn_gpu.py): an index is never more than one step from the oracle's, at a share <= FLIP_RATE; outputs off by
more than 1e-3 + 1e-3 |want| at a share <= OUT_OFF and never by more than 1.05 context-grid steps + 2e-3; each share floored at 2 / n elements.
bf16 storage: the same bounds on the fp32 output (out_dtype=float32, the same arithmetic) - a bf16 store alone rounds by up to 2^-9 |want|, more
than the 1e-3 |want| of the bound."""
import functools

import numpy as np
import pytest

from oracle import oeh_oracle as O
from tests.test_attn_gpu import FLIP_RATE, OUT_OFF, SPECS, _flip_stats, _le, _np32, _rand, _spec
from tests.test_decode_gpu import FMIN, MODULE_TOL, _hf_mask, _pad_vector

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

D = 64
GRID = [(2, 3, 1, 77, 4), (1, 2, 5, 333, 7), (2, 2, 16, 2049, 32), (2, 2, 16, 2049, 0), (2, 2, 3, 130, 64), (1, 1, 1, 1, 0)]
FORMS = ["softmax1", "vanilla", "clippedsoftmax1(-.025:1)"]
ALL = ("scores", "probs", "ctx")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


@functools.lru_cache(maxsize=None)
def _inputs(B, H, Sq, Sk, dt_name, order):
    dt = getattr(torch, dt_name)
    q = _rand((B, H, Sq, D), 201, dtype=torch.float32)
    # scores of standard deviation 3 (BERT order: 8 / 8 x 3): peaked rows, so that the clipped softmax keeps probabilities above its threshold
    # even over 2049 keys and the probability grid has many occupied points
    q = (q * (3.0 * D ** -0.5)).to(dt) if order == "opt" else (q * 3.0).to(dt)
    k, v = _rand((B, H, Sk, D), 202, dtype=dt), _rand((B, H, Sk, D), 203, dtype=dt)
    gate = torch.rand((B, H, Sq, 1), generator=torch.Generator().manual_seed(204))
    return q, k, v, gate


@functools.lru_cache(maxsize=None)
def _reference(B, H, Sq, Sk, dt_name, sm, order, subset=ALL, gated=True):
    """The oracle's side of one case, computed once: ranges from its own float intermediates at percentiles (0.001, 99.999), then the chain with
    the quantisers of `subset`.  OPT order: q pre-scaled, causal, clamp_min, key padding with finfo.min entries, context quantised before the
    gate; BERT order: / 8, no mask, context quantised after the gate."""
    q, k, v, gate = _inputs(B, H, Sq, Sk, dt_name, order)
    qn, kn, vn = _np32(q), _np32(k), _np32(v)
    g = gate.numpy() if gated else None
    if order == "opt":
        common = dict(causal=True, clamp_min=True, pad_mask=_pad_vector(B, Sk), mask_min=FMIN, gate=g, **SPECS[sm])
    else:
        common = dict(scale=8.0, scale_is_divisor=True, gate=g, **SPECS[sm])
    before = order == "opt"
    _, fp = O.attn_core(qn, kn, vn, want=("scores", "probs"), **common)
    ctx_fp = O.attn_core(qn, kn, vn, **{**common, "gate": None if before else g})
    d = {"scores": O.quant_range_to_params(*np.percentile(fp["scores"], (0.001, 99.999))),
         "probs": O.quant_range_to_params(*np.percentile(fp["probs"], (0.001, 99.999))),
         "ctx": O.quant_range_to_params(*np.percentile(ctx_fp, (0.001, 99.999)))}
    fqkw = {f"fq_{n}": d[n] for n in subset}
    want, ex = O.attn_core(qn, kn, vn, ctx_quant_before_gate=before, want=tuple(f"{n}_idx" for n in subset), **fqkw, **common)
    want.setflags(write=False)
    return d, want, ex


def _run(ops, B, H, Sq, Sk, dt_name, sm, order, splits, subset=ALL, gated=True, dumps=True, out_dtype=None, d=None):
    q, k, v, gate = _inputs(B, H, Sq, Sk, dt_name, order)
    if d is None:
        d = _reference(B, H, Sq, Sk, dt_name, sm, order, subset, gated)[0]
    shapes = {"scores": (B, H, Sq, Sk), "probs": (B, H, Sq, Sk), "ctx": (B, H, Sq, D)}
    dump = {n: torch.full(shapes[n], 77, dtype=torch.uint8, device="cuda") for n in subset} if dumps else {}
    FQ = ops.FakeQuantSpec.from_delta
    fq = ops.AttnFakeQuant(**{n: FQ(*d[n], dump=dump.get(n)) for n in subset}, ctx_before_gate=order == "opt")
    kw = dict(softmax=_spec(ops, sm), gate=gate.cuda() if gated else None, splits=splits, fq=fq, out_dtype=out_dtype)
    if order == "opt":
        kw.update(causal=True, clamp_min=True, mask_min=FMIN, key_pad_mask=torch.from_numpy(_pad_vector(B, Sk)).cuda())
    else:
        kw.update(scale_div=8.0)
    got = ops.attn_decode(q.cuda(), k.cuda(), v.cuda(), **kw)
    return got, dump


def _compare(tag, got, dump, want, ex, step):
    """`step`: the largest output change of one context-grid step (0 without the context quantiser)"""
    for n, t in dump.items():
        mx, rate = _flip_stats(t.cpu().numpy(), ex[f"{n}_idx"])
        print(f"decode fq {tag} {n}: max index diff {mx}, flip rate {rate:.2e} of {t.numel()}")
        assert mx <= 1 and _le(rate, FLIP_RATE, f"decode_fq[{tag}] {n} flip rate", n=t.numel()), f"{tag} {n}: max index diff {mx}, flip rate {rate:.2e}"
    err = np.abs(_np32(got) - want)
    assert np.isfinite(_np32(got)).all()
    flipped = err > 1e-3 + 1e-3 * np.abs(want)
    print(f"decode fq {tag} out: {flipped.mean():.2e} of {flipped.size} off, max err {err.max():.3e} (step {step:.3e})")
    assert _le(flipped.mean(), OUT_OFF, f"decode_fq[{tag}] outputs off", n=flipped.size) and err.max() <= 1.05 * step + 2e-3, \
        f"{tag} out: {flipped.mean():.2e} elements off, max err {err.max():.3e} (step {step:.3e})"


BF16_SHAPES = {(1, 2, 5, 333, 7), (2, 2, 16, 2049, 0)}
PARITY = [(g, "float16") for g in GRID] + [(g, "bfloat16") for g in GRID if g in BF16_SHAPES]


@pytest.mark.parametrize("sm", FORMS)
@pytest.mark.parametrize("shape,dt_name", PARITY)
def test_parity_grid(ops, shape, dt_name, sm):
    """OPT order with all three quantisers against oracle.attn_core: the three index dumps and the output.  Measured on MI355X (OEH_TEST_REPORT
    records each share against its limit): no index and no output off in any of the 24 cases."""
    B, H, Sq, Sk, splits = shape
    d, want, ex = _reference(B, H, Sq, Sk, dt_name, sm, "opt")
    if Sk >= 77:  # the probability check is not vacuous, and the score grid is not saturated
        assert len(np.unique(ex["probs_idx"])) >= 8
        assert float(np.isin(ex["scores_idx"], (0, 255)).mean()) < 0.2
    got, dump = _run(ops, B, H, Sq, Sk, dt_name, sm, "opt", splits, out_dtype=torch.float32 if dt_name == "bfloat16" else None)
    assert got.shape == (B, H, Sq, D) and got.permute(0, 2, 1, 3).is_contiguous()
    step = float(np.float32(d["ctx"][0])) * float(_inputs(B, H, Sq, Sk, dt_name, "opt")[3].max())  # (quantised, then multiplied by the gate)
    _compare(f"{shape},{dt_name},{sm}", got, dump, want, ex, step)


@pytest.mark.parametrize("subset", [ALL, ("scores",), ("probs",), ("ctx",), ("scores", "probs")])
@pytest.mark.parametrize("sm", ["softmax1", "clippedsoftmax1(-.025:1)"])
def test_bert_order_and_subsets(ops, subset, sm):
    """scale_div = 8, no mask, the context quantised AFTER the gate; every subset of quantisers against the oracle with the same subset.
    Measured on MI355X: one context index of 640 one step off in {ctx only} with the clipped softmax (the probabilities reach the second
    product rounded to fp16 there), nothing off elsewhere."""
    B, H, Sq, Sk, splits = 1, 2, 5, 333, 7
    d, want, ex = _reference(B, H, Sq, Sk, "float16", sm, "bert", subset)
    got, dump = _run(ops, B, H, Sq, Sk, "float16", sm, "bert", splits, subset)
    step = float(np.float32(d["ctx"][0])) if "ctx" in subset else 0.0  # (quantised after the gate: a step of the grid is a step of the output)
    _compare(f"bert,{'+'.join(subset)},{sm}", got, dump, want, ex, step)


@pytest.mark.parametrize("subset", [ALL, ("scores",), ("ctx",)])
def test_bf16_output_store_and_two_launch_forms(ops, subset):
    """bf16 storage with the bf16 output store of the fq combine / sum kernels, the three-launch form and both two-launch forms (scores only, ctx
    only), no gate.  Indices against the oracle with the project's bounds.  With the context quantiser the stored output must be
    bf16(scale (i - zp)) of the dumped index i, bit for bit; without it the output is within the bf16 contract of tests/test_decode_gpu.py:
    8e-3 max(1, |V|max) + half a bf16 ulp of the reference."""
    B, H, Sq, Sk, splits = 1, 2, 5, 333, 7
    sm = "softmax1"
    d, want, ex = _reference(B, H, Sq, Sk, "bfloat16", sm, "opt", subset, False)
    got, dump = _run(ops, B, H, Sq, Sk, "bfloat16", sm, "opt", splits, subset, gated=False)
    assert got.dtype == torch.bfloat16
    for n, t in dump.items():
        mx, rate = _flip_stats(t.cpu().numpy(), ex[f"{n}_idx"])
        print(f"decode fq bf16 {'+'.join(subset)} {n}: max index diff {mx}, flip rate {rate:.2e} of {t.numel()}")
        assert mx <= 1 and _le(rate, FLIP_RATE, f"decode_fq_bf16[{'+'.join(subset)}] {n} flip rate", n=t.numel())
    if "ctx" in subset:
        scale, zp, _ = O.fq_grid(*d["ctx"])
        vals = np.float32(scale) * (dump["ctx"].cpu().numpy().astype(np.float32) - np.float32(zp))
        assert torch.equal(got.cpu(), torch.from_numpy(vals.astype(np.float32)).to(torch.bfloat16))
    else:
        vn = _np32(_inputs(B, H, Sq, Sk, "bfloat16", "opt")[2])
        err = np.abs(_np32(got) - want)
        lim = 8e-3 * max(1.0, float(np.abs(vn).max())) + 0.5 * np.spacing(np.abs(want).astype(np.float32)) * 65536.0
        print(f"decode fq bf16 {'+'.join(subset)} out: max err {err.max():.3e}, worst err / limit {float((err / lim).max()):.2f}")
        assert (err <= lim).all()


@pytest.mark.parametrize("sm", FORMS)
def test_outputs_sit_on_the_context_grid(ops, sm):
    """out_dtype = float32, no gate: every output is scale * (i - zp) for an integer i in [0, 255], bit for bit."""
    B, H, Sq, Sk, splits = 1, 2, 5, 333, 7
    d = _reference(B, H, Sq, Sk, "float16", sm, "opt")[0]  # (OPT order: the context range is that of the ungated context)
    got, dump = _run(ops, B, H, Sq, Sk, "float16", sm, "opt", splits, gated=False, out_dtype=torch.float32, d=d)
    scale, zp, qmax = O.fq_grid(*d["ctx"])
    out = got.cpu().numpy()
    i = dump["ctx"].cpu().numpy().astype(np.float32)
    assert qmax == 255.0 and i.min() >= 0 and i.max() <= 255
    assert np.array_equal(out, (np.float32(scale) * (i - np.float32(zp)).astype(np.float32)).astype(np.float32))
    assert len(np.unique(i)) >= 8


def test_identities(ops):
    """No quantiser: ops.attn_decode's bits; repeated calls and NaN-filled scratch: the same bits; the score indices do not depend on the split
    count; one graph capture + replay equals the eager call; the production form (no dumps) equals the dumping form."""
    B, H, Sq, Sk, splits = 1, 2, 5, 333, 7
    q, k, v, gate = (t.cuda() for t in _inputs(B, H, Sq, Sk, "float16", "opt"))
    pad = torch.from_numpy(_pad_vector(B, Sk)).cuda()
    for sm in ("softmax1", "clippedsoftmax1(-.025:1)"):
        kw = dict(softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=FMIN, key_pad_mask=pad, gate=gate, splits=splits)
        plain = ops.attn_decode(q, k, v, **kw)
        assert torch.equal(ops.attn_decode(q, k, v, fq=None, **kw), plain)
        assert torch.equal(ops.attn_decode(q, k, v, fq=ops.AttnFakeQuant(), **kw), plain)
        first, dump = _run(ops, B, H, Sq, Sk, "float16", sm, "opt", splits)
        again, dump2 = _run(ops, B, H, Sq, Sk, "float16", sm, "opt", splits)
        assert torch.equal(first, again) and all(torch.equal(dump[n], dump2[n]) for n in ALL)
        work = ops._decode_scratch(q.device, 16)
        work.view(torch.float32).fill_(float("nan"))
        with_nan, _ = _run(ops, B, H, Sq, Sk, "float16", sm, "opt", splits)
        assert ops._decode_scratch(q.device, 16) is work and torch.equal(first, with_nan)
        production, none = _run(ops, B, H, Sq, Sk, "float16", sm, "opt", splits, dumps=False)
        assert not none and torch.equal(production, first)
        for other in (1, 2, 3, 6, 0):
            _, dump_o = _run(ops, B, H, Sq, Sk, "float16", sm, "opt", other)
            assert torch.equal(dump_o["scores"], dump["scores"]), (sm, other)
        d = _reference(B, H, Sq, Sk, "float16", sm, "opt")[0]
        FQ = ops.FakeQuantSpec.from_delta
        fq = ops.AttnFakeQuant(FQ(*d["scores"]), FQ(*d["probs"]), FQ(*d["ctx"]), ctx_before_gate=True)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = ops.attn_decode(q, k, v, fq=fq, **kw)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, first), sm


@pytest.mark.parametrize("shape", [(2, 2, 16, 2049, 0), (1, 2, 5, 333, 0)])
@pytest.mark.parametrize("sm", ["softmax1", "clippedsoftmax1(-.025:1)"])
def test_against_the_general_forward(ops, shape, sm):
    """ops.attn_fwd(fq=...) on the same tensors (what a generation step runs with the switch off): the context indices - read back from the fp16
    outputs, no gate: |i - zp| <= 255 is exact to 0.07 of a step in fp16 - differ by at most one step at a share <= OUT_OFF."""
    B, H, Sq, Sk, splits = shape
    d = _reference(B, H, Sq, Sk, "float16", sm, "opt")[0]
    got, _ = _run(ops, B, H, Sq, Sk, "float16", sm, "opt", splits, gated=False, dumps=False, d=d)
    q, k, v, _ = (t.cuda() for t in _inputs(B, H, Sq, Sk, "float16", "opt"))
    FQ = ops.FakeQuantSpec.from_delta
    fq = ops.AttnFakeQuant(FQ(*d["scores"]), FQ(*d["probs"]), FQ(*d["ctx"]), ctx_before_gate=True)
    ref = ops.attn_fwd(q, k, v, softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=FMIN,
                       key_pad_mask=torch.from_numpy(_pad_vector(B, Sk)).cuda(), key_pad_boolean=True, fq=fq)  # (as attention_core passes it)
    scale = float(O.fq_grid(*d["ctx"])[0])
    ia, ib = np.rint(_np32(got) / scale), np.rint(_np32(ref) / scale)
    diff = np.abs(ia - ib)
    print(f"decode fq vs attn_fwd {shape} {sm}: max index diff {diff.max():.0f}, share {float((diff != 0).mean()):.2e} of {diff.size}")
    assert diff.max() <= 1 and _le(float((diff != 0).mean()), OUT_OFF, f"decode_fq_vs_fwd[{shape},{sm}] ctx indices apart", n=diff.size)


@pytest.fixture
def split_decode_on():
    from outeffhop_amd import attention

    before = attention.SPLIT_DECODE
    attention.set_split_decode(True)
    yield attention
    attention.set_split_decode(before)


@pytest.mark.parametrize("form", ["softmax1", "tok_linear"])
def test_quantised_opt_module_generation_steps(ops, form, split_decode_on):
    """QuantizedOPTAttentionWithExtras (2 heads of 64, fp16, ranges fixed after a short calibration): prefill 40 tokens, 6 single-token steps and one
    3-token step with past_key_value and HF's causal + left-padding mask.  With the switch on every step runs the decode kernels; outputs agree
    with the switch off within MODULE_TOL, plus one context-grid step on a share <= OUT_OFF * E: one context value of a token that lands on the
    neighbouring grid point moves all E outputs of that token through out_proj.  The returned cache is identical.
    Measured on MI355X: the outputs of the two routes were bit-identical in both forms (share 0; OEH_TEST_REPORT records it)."""
    import outeffhop_amd as oa
    from tests.test_modules_gpu import _qparams

    attention = split_decode_on
    torch.manual_seed(17)
    B, T0, E, H = 2, 40, 128, 2
    chunks = [1] * 6 + [3]
    total = T0 + sum(chunks)
    kw = dict(softmax_fn=oa.SOFTMAX_MAPPING["softmax1"])
    if form == "tok_linear":
        kw.update(attn_gate_type=oa.AttentionGateType.conditional_per_token, attn_gate_init=0.25)
    org = oa.OPTAttentionWithExtras(E, H, is_decoder=True, **kw)
    qm = oa.QuantizedOPTAttentionWithExtras(org.cuda().half(), **_qparams(oa)).cuda().eval()
    qm.set_quant_state(weight_quant=True, act_quant=True)
    full = _hf_mask(B, total, total, [0, 7], torch.float16)
    with torch.no_grad():
        for _ in range(3):
            qm(torch.randn(B, T0, E).half().cuda(), attention_mask=full[:, :, :T0, :T0].cuda())
        qm.fix_ranges()
    hc = torch.randn(B, total, E).half().cuda()

    def run():
        outs = []
        with torch.no_grad():
            out, _, past = qm(hc[:, :T0], attention_mask=full[:, :, :T0, :T0].cuda())
            outs.append(out)
            t = T0
            for n in chunks:
                out, _, past = qm(hc[:, t:t + n], past_key_value=past, attention_mask=full[:, :, t:t + n, :t + n].contiguous().cuda())
                t += n
                assert past[0].shape == (B, H, t, E // H)
                outs.append(out)
        return torch.cat(outs, dim=1), past

    calls = ops.DECODE_CALLS
    got, past_on = run()
    assert ops.DECODE_CALLS == calls + len(chunks)
    try:
        attention.set_split_decode(False)
        calls = ops.DECODE_CALLS
        ref, past_off = run()
        assert ops.DECODE_CALLS == calls
    finally:
        attention.set_split_decode(True)
    assert torch.equal(past_on[0], past_off[0]) and torch.equal(past_on[1], past_off[1])
    assert torch.equal(got[:, :T0], ref[:, :T0])  # (the prefill is the same call either way)
    g, r = _np32(got[:, T0:]), _np32(ref[:, T0:])
    assert np.isfinite(g).all()
    diff = np.abs(g - r)
    lim = MODULE_TOL["atol"] + MODULE_TOL["rtol"] * np.abs(r)
    step = float(qm.context_act_quantizer.activation_quantizer.quantizer.delta)
    off = diff > lim
    print(f"quantised opt generation steps {form}: decode on / off differ by {diff.max():.2e} (limit {lim.min():.2e} + step {step:.2e}), {off.mean():.2e} beyond the limit")
    assert (diff <= lim + step).all()
    assert _le(off.mean(), OUT_OFF * E, f"decode_fq_module[{form}] outputs beyond MODULE_TOL", n=off.size)
