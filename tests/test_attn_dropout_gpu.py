"""Attention dropout inside the fused training kernels (include/oeh.h: oeh_attn_fwd_train_dropout / oeh_attn_bwd_dropout /
oeh_attn_dropout_mask; outeffhop_amd.fused_attention(dropout_p=...)) on the MI355X.

The device's keep mask is compared bit for bit with the numpy restatement of the generator (tests/test_attn_dropout_cpu.py).  The
gradients are calibrated as in tests/test_attn_bwd_gpu.py with that mask injected: the reference is float64 autograd of the op chain
with z = y keep / (1 - p) before the product with V, the yardstick the torch-op path (attention.unfused_core with
dropout = t -> t keep / (1 - p)) in the storage dtype:  max|fused - ref64| <= 2 max|torch_op - ref64| + 1e-3 max|ref64|."""
import numpy as np
import pytest
import torch

from tests.test_attn_bwd_gpu import SOFTMAX, _bert, _bert_pad_mask, _check, _grads, _problem, _spec
from tests.test_attn_dropout_cpu import keep_mask

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 0x9E3779B97F4A7C15, 2 ** 64 - 1)


def _ref_chain_drop(q, k, v, spec, scale, scale_div, add_mask, clamp, mask_min, keep, p):
    """tests/test_attn_bwd_gpu.py's reference chain with the dropout multiply where nn.Dropout sits (after the clip, before .V)."""
    s = torch.matmul(q, k.transpose(-1, -2))
    s = s / scale_div if scale_div else s * scale
    if add_mask is not None:
        s = s + add_mask
        if clamp:
            s = torch.max(s, torch.tensor(mask_min, dtype=s.dtype, device=s.device))
    if spec.base == 1:
        m = s.max(dim=-1, keepdim=True).values.clamp(min=0)
        e = torch.exp(s - m)
        pr = e / (e.sum(dim=-1, keepdim=True) + torch.exp(-m))
    else:
        pr = torch.softmax(s, dim=-1)
    if spec.clip:
        pr = torch.clip(pr * (spec.eta - spec.gamma) + spec.gamma, 0, 1)
    return torch.matmul(pr * keep.to(pr.dtype) / (1.0 - p), v)


# ---------------------------------------------------------------- the mask
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_matches_the_restatement(p):
    from outeffhop_amd import ops

    B, H, Sq = 2, 3, 70
    for seed in SEEDS:
        m256 = ops.attn_dropout_mask(B, H, Sq, 256, p, seed, "cuda")
        m200 = ops.attn_dropout_mask(B, H, Sq, 200, p, seed, "cuda")
        assert m256.dtype == torch.bool and m256.shape == (B, H, Sq, 256)
        ref = keep_mask(B, H, Sq, 256, p, seed)
        assert np.array_equal(m256.cpu().numpy(), ref), seed
        assert torch.equal(m200, m256[..., :200]), seed
        assert not torch.equal(m256[0, 0], m256[0, 1]) and not torch.equal(m256[0, 0], m256[1, 0])  # each (b, h) its own stream
    assert not torch.equal(ops.attn_dropout_mask(B, H, Sq, 256, p, 1, "cuda"), ops.attn_dropout_mask(B, H, Sq, 256, p, 2, "cuda"))


def test_mask_keep_rate():
    from outeffhop_amd import ops

    for p in (0.1, 0.5):
        m = ops.attn_dropout_mask(4, 12, 512, 512, p, 12345, "cuda")
        n = m.numel()
        assert n >= 10 ** 7
        rate = float(m.sum(dtype=torch.float64)) / n
        assert abs(rate - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n), (p, rate)
    assert bool(ops.attn_dropout_mask(1, 2, 33, 45, 0.0, 9, "cuda").all())


# ---------------------------------------------------------------- gradients
def _run_case(sm, mask, S, dt, p, seed, B=1, H=2):
    from outeffhop_amd import fused_attention
    from outeffhop_amd.attention import unfused_core
    from outeffhop_amd.softmax import softmax_autograd

    spec = _spec(sm)
    q, k, v, do, pad, fm, causal, add, clamp, mask_min = _problem(B, H, S, dt, mask, seed)
    keep = torch.from_numpy(keep_mask(B, H, S, S, p, seed))
    ref = _grads(lambda a, b, c: _ref_chain_drop(a, b, c, spec, 1.0, 0.0, add, clamp, mask_min, keep, p), q.double(), k.double(), v.double(),
                 do.double())
    dev = "cuda"
    fused = _grads(lambda a, b, c: fused_attention(a, b, c, softmax=spec, key_pad_mask=None if pad is None else pad.to(dev),
                                                 full_mask=None if fm is None else fm.to(dev), causal=causal, clamp_min=clamp,
                                                 mask_min=mask_min, dropout_p=p, dropout_seed=seed),
                   q.to(dev), k.to(dev), v.to(dev), do.to(dev))
    am = None if add is None else add.clamp(min=-3.0e38).to(dt).to(dev)
    fn = lambda x, dim=-1: softmax_autograd(x.float(), spec, dim).to(dt)  # noqa: E731
    kd = keep.to(dt).to(dev)
    top = _grads(lambda a, b, c: unfused_core(a, b, c, softmax_fn=fn, scale=1.0, attention_mask=am, clamp_min=clamp,
                                              dropout=lambda t: t * kd / (1.0 - p))[0],
                 q.to(dev), k.to(dev), v.to(dev), do.to(dev))
    rep = []
    _check(f"{sm}/{mask}/S{S}/{dt}/p{p}", fused, top, ref, rep)
    return rep


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("S", [128, 200, 512])
@pytest.mark.parametrize("mask", ["none", "causal", "key_pad", "full"])
@pytest.mark.parametrize("sm", list(SOFTMAX))
def test_gradient_parity_with_dropout(sm, mask, S, dt, p):
    for name, tag, ef, et, rel in _run_case(sm, mask, S, dt, p, seed=S + int(p * 10)):
        print(f"{name} {tag}: fused {ef:.2e} torch-op {et:.2e} rel {rel:.2e}")


@pytest.mark.parametrize("sm", list(SOFTMAX))
def test_fully_masked_rows_with_dropout(sm):
    """Rows with every key at the mask floor, with dropout: finite, close to float64 autograd (the bound of tests/test_attn_bwd_gpu.py's
    fully-masked test - the torch-op path itself is NaN on such softmax_1 rows, so it cannot calibrate them); softmax_1 rows give p = 0."""
    from outeffhop_amd import fused_attention

    spec = _spec(sm)
    B, H, S, dt, p, seed = 1, 2, 96, torch.float16, 0.1, 21
    q, k, v, do, _, _, _, _, _, mask_min = _problem(B, H, S, dt, "none", 11)
    full = torch.zeros(B, 1, S, S)
    full[:, :, 5] = mask_min
    full[:, :, 70:73] = mask_min
    keep = torch.from_numpy(keep_mask(B, H, S, S, p, seed))
    ref = _grads(lambda a, b, c: _ref_chain_drop(a, b, c, spec, 1.0, 0.0, full.double(), True, mask_min, keep, p), q.double(), k.double(),
                 v.double(), do.double())
    fused = _grads(lambda a, b, c: fused_attention(a, b, c, softmax=spec, full_mask=full.cuda(), clamp_min=True, mask_min=mask_min, dropout_p=p,
                                                 dropout_seed=seed), q.cuda(), k.cuda(), v.cuda(), do.cuda())
    for f, r, tag in zip(fused, ref, ("o", "dq", "dk", "dv")):
        f = f.double().cpu()
        assert torch.isfinite(f).all(), tag
        assert float((f - r).abs().max()) <= 2e-2 * float(r.abs().max()) + 1e-3, (tag, float((f - r).abs().max()))
    if spec.base == 1 and not spec.clip:
        assert float(fused[0][:, :, 5].abs().max()) == 0.0 and float(fused[1][:, :, 5].abs().max()) == 0.0


def test_multi_batch_bert_shape_with_dropout():
    """Several batches and heads (the counter's b * H + h word), key padding, p = 0.1."""
    _run_case("clippedsoftmax1", "key_pad", 128, torch.float16, 0.1, seed=5, B=3, H=4)


def test_same_seed_same_bits():
    """A seed fixes o, dq, dk, dv bit for bit; another seed changes them; p = 0 is the path without dropout."""
    from outeffhop_amd import fused_attention

    B, H, S = 4, 12, 512
    g = torch.Generator(device="cuda").manual_seed(1)
    q, k, v, do = (torch.randn(B, H, S, 64, generator=g, device="cuda", dtype=torch.float16) for _ in range(4))
    q = q * 0.125

    def run(**kw):
        return _grads(lambda a, b, c: fused_attention(a, b, c, softmax=_spec("softmax1"), causal=True, clamp_min=True, **kw), q, k, v, do)

    a, b, c = run(dropout_p=0.1, dropout_seed=77), run(dropout_p=0.1, dropout_seed=77), run(dropout_p=0.1, dropout_seed=78)
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y)
        assert not torch.equal(x, z)
    for x, y in zip(run(), run(dropout_p=0.0, dropout_seed=77)):
        assert torch.equal(x, y)


# ---------------------------------------------------------------- module level
def _bert_step(m, x, mask):
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(True)
    m(x, attention_mask=mask)[0].float().sum().backward()
    return [x.grad] + [p.grad for p in m.parameters()]


def test_bert_dropout_routes_to_the_fused_kernels(monkeypatch):
    """BERT with attention_probs_dropout_prob = 0.1 in .train(): with both switches on the fused op runs (forward and backward) and
    unfused_core never; with FUSED_DROPOUT off it is the torch-op path.  torch.manual_seed reproduces a fused step exactly."""
    import outeffhop_amd.bert_attention as BA
    from outeffhop_amd import attention as A
    from outeffhop_amd import autograd_attention as AA

    calls = []
    orig = BA.unfused_core
    monkeypatch.setattr(BA, "unfused_core", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    torch.manual_seed(0)
    m = _bert(0.1).cuda().half().train()
    x = torch.randn(2, 128, 768, device="cuda").half()
    mask = _bert_pad_mask(2, 128, torch.float16)
    prev = A.FUSED_BACKWARD, A.FUSED_DROPOUT
    try:
        A.set_fused_backward(True)
        A.set_fused_dropout(True)
        n0 = dict(AA.CALLS)
        torch.manual_seed(42)
        g1 = _bert_step(m, x, mask)
        torch.manual_seed(42)
        g2 = _bert_step(m, x, mask)
        ran = AA.CALLS["forward"] - n0["forward"], AA.CALLS["backward"] - n0["backward"]
        assert ran == (2, 2) and calls == [], (ran, calls)
        for a, b in zip(g1, g2):
            assert torch.isfinite(a).all() and torch.equal(a, b)
        g3 = _bert_step(m, x, mask)  # next draw of the generator: another mask
        assert not torch.equal(g1[0], g3[0])
        A.set_fused_dropout(False)
        n1 = AA.CALLS["forward"]
        _bert_step(m, x, mask)
        assert AA.CALLS["forward"] == n1 and len(calls) == 1
        m.eval()  # no dropout in eval: the differentiable path without dropout still takes the fused kernels
        A.set_fused_dropout(True)
        _bert_step(m, x, mask)
        assert AA.CALLS["forward"] == n1 + 1 and len(calls) == 1
    finally:
        A.set_fused_backward(prev[0])
        A.set_fused_dropout(prev[1])


def test_opt_dropout_routes_to_the_fused_kernels(monkeypatch):
    import outeffhop_amd.opt_attention as OA
    from outeffhop_amd import SOFTMAX_MAPPING, OPTAttentionWithExtras
    from outeffhop_amd import attention as A
    from outeffhop_amd import autograd_attention as AA

    calls = []
    orig = OA.unfused_core
    monkeypatch.setattr(OA, "unfused_core", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    torch.manual_seed(0)
    m = OPTAttentionWithExtras(768, 12, dropout=0.1, is_decoder=True, softmax_fn=SOFTMAX_MAPPING["softmax1"]).cuda().half().train()
    S = 256
    mask = torch.triu(torch.full((S, S), torch.finfo(torch.float16).min, device="cuda", dtype=torch.float16), 1)[None, None].expand(2, 1, S, S)
    x = torch.randn(2, S, 768, device="cuda").half().requires_grad_(True)
    prev = A.FUSED_BACKWARD, A.FUSED_DROPOUT
    try:
        A.set_fused_backward(True)
        A.set_fused_dropout(True)
        n0 = AA.CALLS["forward"]
        m(x, attention_mask=mask)[0].float().sum().backward()
        assert AA.CALLS["forward"] == n0 + 1 and calls == []
        assert torch.isfinite(x.grad).all()
    finally:
        A.set_fused_backward(prev[0])
        A.set_fused_dropout(prev[1])


def test_memory_has_no_sxs_term_with_dropout():
    """tests/test_attn_bwd_gpu.py's memory shape with dropout: peak memory beyond the inputs does not grow with S."""
    from outeffhop_amd import fused_attention

    peaks = []
    for B, S in ((8, 512), (2, 2048)):
        q, k, v = (torch.randn(B, 12, S, 64, device="cuda", dtype=torch.float16).requires_grad_(True) for _ in range(3))
        do = torch.randn(B, 12, S, 64, device="cuda", dtype=torch.float16)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fused_attention(q, k, v, softmax=_spec("softmax1"), causal=True, dropout_p=0.1).backward(do)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        del q, k, v, do
    assert peaks[1] <= 1.25 * peaks[0], peaks
