"""The fused training path of the attention core (include/oeh.h: oeh_attn_fwd_train / oeh_attn_bwd; outeffhop_amd.fused_attention) on
the MI355X.  The gradient reference is float64 CPU autograd of the reference op chain (opt_attention.py:204-263: matmul, scale, mask,
clamp, softmax_n_shifted_zeros / softmax, clip, matmul) on the 16-bit-rounded inputs.  The bound for every tensor is calibrated by
the path the fused one replaces - the torch-op path (attention.unfused_core under autograd) in the same storage dtype:
    max|fused - ref64| <= 2 max|torch_op - ref64| + 1e-3 max|ref64|."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SOFTMAX = {  # the four --attn_softmax values of the reference's pre-training scripts
    "vanilla": (0, False, 0.0, 1.0),
    "softmax1": (1, False, 0.0, 1.0),
    "clipped": (0, True, -0.025, 1.0),
    "clippedsoftmax1": (1, True, -0.025, 1.0),
}
MASKS = ("none", "causal", "key_pad", "causal_key_pad", "full")


def _spec(name):
    from outeffhop_amd.ops import SoftmaxSpec

    return SoftmaxSpec(*SOFTMAX[name])


def _ref_chain(q, k, v, spec, scale, scale_div, add_mask, clamp, mask_min):
    """The reference's op chain (any dtype / device): returns the context."""
    s = torch.matmul(q, k.transpose(-1, -2))
    s = s / scale_div if scale_div else s * scale
    if add_mask is not None:
        s = s + add_mask
        if clamp:
            s = torch.max(s, torch.tensor(mask_min, dtype=s.dtype, device=s.device))
    if spec.base == 1:  # vutils/softmax_1.py:11-21, shifted by max(m, 0): the same function, and autograd stays finite on a fully
        # masked row (the literal form's exp(-m) overflows there even in float64 and its gradient is NaN)
        m = s.max(dim=-1, keepdim=True).values.clamp(min=0)
        e = torch.exp(s - m)
        p = e / (e.sum(dim=-1, keepdim=True) + torch.exp(-m))
    else:
        p = torch.softmax(s, dim=-1)
    if spec.clip:
        p = torch.clip(p * (spec.eta - spec.gamma) + spec.gamma, 0, 1)
    return torch.matmul(p, v)


def _problem(B, H, S, dt, mask, seed, outlier=False):
    g = torch.Generator().manual_seed(seed)
    if outlier:  # the outlier family: heavy tails (Student-t with 3 degrees of freedom)
        t = torch.distributions.StudentT(3.0)
        torch.manual_seed(seed)
        mk = lambda: t.sample((B, H, S, 64)).clamp(-30, 30)  # noqa: E731
    else:
        mk = lambda: torch.randn(B, H, S, 64, generator=g)  # noqa: E731
    q, k, v = (mk() * 0.125).to(dt), mk().to(dt), mk().to(dt)
    do = torch.randn(B, H, S, 64, generator=g).to(dt)
    mask_min = float(torch.finfo(dt).min)
    pad = full = None
    causal = mask in ("causal", "causal_key_pad")
    if mask in ("key_pad", "causal_key_pad"):
        pad = torch.zeros(B, S)
        for b in range(B):
            pad[b, S - (S // 5) * (b + 1) // B - 1:] = mask_min  # a padded tail per sequence
    if mask == "full":
        full = torch.where(torch.rand(B, 1, S, S, generator=g) < 0.2, torch.tensor(mask_min), torch.zeros(()))
    add = torch.zeros(B, 1, S, S, dtype=torch.float64)
    if causal:
        add = add + torch.triu(torch.full((S, S), mask_min, dtype=torch.float64), 1)
    if pad is not None:
        add = add + pad.double()[:, None, None, :]
    if full is not None:
        add = add + full.double()
    add = None if mask == "none" else add
    clamp = mask in ("causal", "full", "causal_key_pad")  # OPT clamps at finfo.min, BERT's key padding does not
    return q, k, v, do, pad, full, causal, add, clamp, mask_min


def _grads(fn, q, k, v, do):
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = fn(q, k, v)
    o.backward(do)
    return [o.detach(), q.grad, k.grad, v.grad]


def _check(name, fused, torch_op, ref, report):
    errs = []
    for tag, f, t, r in zip(("o", "dq", "dk", "dv"), fused, torch_op, ref):
        f, t, r = f.double().cpu(), t.double().cpu(), r.double().cpu()
        assert torch.isfinite(f).all(), f"{name} {tag}: non-finite values"
        ef, et, mr = float((f - r).abs().max()), float((t - r).abs().max()), float(r.abs().max())
        report.append((name, tag, ef, et, ef / max(mr, 1e-30)))
        errs.append((tag, ef, et, mr))
    for tag, ef, et, mr in errs:
        assert ef <= 2 * et + 1e-3 * mr, f"{name} {tag}: fused {ef:.3e} vs torch-op {et:.3e} (max|ref| {mr:.3e})"


def _run_case(sm, mask, S, dt, seed=0, outlier=False, B=1, H=2):
    from outeffhop_amd import fused_attention
    from outeffhop_amd.attention import unfused_core
    from outeffhop_amd.softmax import softmax_autograd

    spec = _spec(sm)
    q, k, v, do, pad, full, causal, add, clamp, mask_min = _problem(B, H, S, dt, mask, seed, outlier)
    scale = 1.0  # OPT: q pre-scaled
    ref = _grads(lambda a, b, c: _ref_chain(a, b, c, spec, scale, 0.0, add, clamp, mask_min), q.double(), k.double(), v.double(), do.double())
    dev = "cuda"
    fused = _grads(lambda a, b, c: fused_attention(a, b, c, softmax=spec, scale=scale, key_pad_mask=None if pad is None else pad.to(dev),
                                                 full_mask=None if full is None else full.to(dev), causal=causal, clamp_min=clamp,
                                                 mask_min=mask_min),
                   q.to(dev), k.to(dev), v.to(dev), do.to(dev))
    am = None if add is None else add.clamp(min=-3.0e38).to(dt).to(dev)  # (the summed masks in the storage dtype, as a model holds them)
    fn = lambda x, dim=-1: softmax_autograd(x.float(), spec, dim).to(dt)  # noqa: E731  (OPT's upcast branch, opt_attention.py:227-230)
    top = _grads(lambda a, b, c: unfused_core(a, b, c, softmax_fn=fn, scale=scale, attention_mask=am, clamp_min=clamp)[0],
                 q.to(dev), k.to(dev), v.to(dev), do.to(dev))
    rep = []
    _check(f"{sm}/{mask}/S{S}/{dt}", fused, top, ref, rep)
    return rep


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("S", [80, 197, 512, 704])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("sm", list(SOFTMAX))
def test_gradient_parity(sm, mask, S, dt):
    for name, tag, ef, et, rel in _run_case(sm, mask, S, dt, seed=S):
        print(f"{name} {tag}: fused {ef:.2e} torch-op {et:.2e} rel {rel:.2e}")


@pytest.mark.parametrize("sm", list(SOFTMAX))
def test_gradient_parity_outliers(sm):
    _run_case(sm, "causal", 256, torch.float16, seed=7, outlier=True)


def test_gradient_parity_bert_scaling_and_batches():
    """scale_div (BERT's / sqrt(d)), several batches and heads, key padding without the clamp."""
    from outeffhop_amd import fused_attention
    from outeffhop_amd.attention import unfused_core
    from outeffhop_amd.softmax import softmax_autograd

    spec = _spec("clippedsoftmax1")
    q, k, v, do, pad, full, causal, add, clamp, mask_min = _problem(3, 4, 128, torch.float16, "key_pad", 3)
    q = (q.float() * 8).half()
    ref = _grads(lambda a, b, c: _ref_chain(a, b, c, spec, 1.0, 8.0, add, False, mask_min), q.double(), k.double(), v.double(), do.double())
    fused = _grads(lambda a, b, c: fused_attention(a, b, c, softmax=spec, scale_div=8.0, key_pad_mask=pad.cuda()), q.cuda(), k.cuda(), v.cuda(),
                   do.cuda())
    fn = lambda x, dim=-1: softmax_autograd(x.float(), spec, dim).half()  # noqa: E731
    top = _grads(lambda a, b, c: unfused_core(a, b, c, softmax_fn=fn, scale_div=8.0, attention_mask=add.half().cuda())[0], q.cuda(), k.cuda(),
                 v.cuda(), do.cuda())
    _check("bert", fused, top, ref, [])


@pytest.mark.parametrize("sm", ["vanilla", "softmax1"])
def test_fully_masked_rows(sm):
    """Rows with every key at the mask floor: softmax_1 gives p = 0 and zero gradients, vanilla a uniform row; finite, no NaN."""
    _fully_masked_rows(sm, torch.float16)


@pytest.mark.parametrize("sm", ["vanilla", "softmax1"])
def test_fully_masked_rows_bf16(sm):
    """test_fully_masked_rows in bf16: x + finfo.min IS the floor (in fp32 and in float64), so the clamp ties and passes half the
    gradient, as autograd's max does; and the vanilla row's fp32 lse = m + log(den) rounds to m (the saturated rows of the kernels)."""
    _fully_masked_rows(sm, torch.bfloat16)


def _fully_masked_rows(sm, dt):
    from outeffhop_amd import fused_attention

    spec = _spec(sm)
    B, H, S = 1, 2, 96
    q, k, v, do, _, _, _, _, _, mask_min = _problem(B, H, S, dt, "none", 11)
    full = torch.zeros(B, 1, S, S)
    full[:, :, 5] = mask_min
    full[:, :, 70:73] = mask_min
    ref = _grads(lambda a, b, c: _ref_chain(a, b, c, spec, 1.0, 0.0, full.double(), True, mask_min), q.double(), k.double(), v.double(),
                 do.double())
    fused = _grads(lambda a, b, c: fused_attention(a, b, c, softmax=spec, full_mask=full.cuda(), clamp_min=True, mask_min=mask_min),
                   q.cuda(), k.cuda(), v.cuda(), do.cuda())
    for f, r, tag in zip(fused, ref, ("o", "dq", "dk", "dv")):
        f = f.double().cpu()
        assert torch.isfinite(f).all(), tag
        assert float((f - r).abs().max()) <= 2e-2 * float(r.abs().max()) + 1e-3, (tag, float((f - r).abs().max()))
    if sm == "softmax1":  # p = 0 exactly on those rows: no output, no gradient to q
        assert float(fused[0][:, :, 5].abs().max()) == 0.0 and float(fused[1][:, :, 5].abs().max()) == 0.0


def test_clip_boundaries():
    """Sharp rows whose clipped probabilities saturate at 0 and at 1: the gradient gate of the clip matches torch's."""
    from outeffhop_amd import fused_attention
    from outeffhop_amd.ops import SoftmaxSpec

    for base in (0, 1):
        spec = SoftmaxSpec(base, True, -0.3, 1.5)
        q, k, v, do, _, _, _, _, _, mask_min = _problem(1, 2, 128, torch.float16, "none", 5)
        q = (q.float() * 24).half()  # peaked rows: p near 1 (u > 1) and many p near 0 (u < 0)
        u = (torch.softmax((q.double() @ k.double().transpose(-1, -2)), -1) * 1.8 - 0.3)
        assert bool((u >= 1).any()) and bool((u <= 0).any())
        ref = _grads(lambda a, b, c: _ref_chain(a, b, c, spec, 1.0, 0.0, None, False, mask_min), q.double(), k.double(), v.double(), do.double())
        fused = _grads(lambda a, b, c: fused_attention(a, b, c, softmax=spec), q.cuda(), k.cuda(), v.cuda(), do.cuda())
        for f, r, tag in zip(fused, ref, ("o", "dq", "dk", "dv")):
            err = float((f.double().cpu() - r).abs().max())
            assert err <= 1e-2 * float(r.abs().max()) + 1e-3, (base, tag, err)


def test_backward_is_deterministic():
    """Two backward calls give bitwise-identical dq / dk / dv (no atomics, fixed summation order): OPT-125m training shape."""
    from outeffhop_amd import ops

    B, H, S = 16, 12, 512
    g = torch.Generator(device="cuda").manual_seed(1)
    q, k, v, do = (torch.randn(B, H, S, 64, generator=g, device="cuda", dtype=torch.float16) for _ in range(4))
    q = q * 0.125
    kw = dict(softmax=_spec("softmax1"), causal=True, clamp_min=True)
    o, lse = ops.attn_fwd_train(q, k, v, **kw)
    a = ops.attn_bwd(q, k, v, o, do, lse, **kw)
    b = ops.attn_bwd(q, k, v, o, do, lse, **kw)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
        assert torch.isfinite(x).all()


def test_forward_matches_inference_kernel():
    """The training forward's output agrees with the shipped inference kernel on the same problem."""
    from outeffhop_amd import ops

    q, k, v, *_ = _problem(2, 12, 512, torch.float16, "none", 2)
    q, k, v = q.cuda(), k.cuda(), v.cuda()
    kw = dict(softmax=_spec("clippedsoftmax1"), causal=True, clamp_min=True)
    o, lse = ops.attn_fwd_train(q, k, v, **kw)
    with torch.no_grad():
        o_inf = ops.attn_fwd(q, k, v, **kw)
    assert float((o.float() - o_inf.float()).abs().max()) < 2e-3
    assert torch.isfinite(lse).all()


# ---------------------------------------------------------------- module level
def _copy_params(dst, src):
    with torch.no_grad():
        for p, q in zip(dst.parameters(), src.parameters()):
            p.copy_(q.to(p.dtype))


def _module_grads(mod, x, mask, dout):
    x = x.detach().clone().requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    out = mod(x, attention_mask=mask)[0]
    out.backward(dout.to(out.dtype))
    return [out.detach(), x.grad] + [p.grad for p in mod.parameters()]


def _module_case(make, mask_of, fused_expected=True):
    from outeffhop_amd import attention as A
    from outeffhop_amd import autograd_attention as AA

    torch.manual_seed(0)
    m16 = make().cuda().half().train()
    m32 = make().cuda().float().train()
    _copy_params(m32, m16)
    B, S, E = 2, 256, 768
    x = torch.randn(B, S, E, device="cuda").half()
    dout = torch.randn(B, S, E, device="cuda").half()
    mask16, mask32 = mask_of(B, S, torch.float16), mask_of(B, S, torch.float32)
    prev = A.FUSED_BACKWARD
    try:
        A.set_fused_backward(False)
        ref = _module_grads(m32, x.float(), mask32, dout)  # fp32 storage, torch-op path: the high-precision reference
        off = _module_grads(m16, x, mask16, dout)
        A.set_fused_backward(True)
        n0 = dict(AA.CALLS)
        on = _module_grads(m16, x, mask16, dout)
        ran = AA.CALLS["forward"] - n0["forward"], AA.CALLS["backward"] - n0["backward"]
    finally:
        A.set_fused_backward(prev)
    assert ran == ((1, 1) if fused_expected else (0, 0)), ran
    for i, (f, t, r) in enumerate(zip(on, off, ref)):
        f, t, r = f.double(), t.double(), r.double()
        ef, et, mr = float((f - r).abs().max()), float((t - r).abs().max()), float(r.abs().max())
        assert torch.isfinite(f).all()
        assert ef <= 2 * et + 1e-3 * mr, (i, ef, et, mr)


def _decoder_mask(B, S, dt):
    fmin = torch.finfo(dt).min
    m = torch.triu(torch.full((S, S), fmin, dtype=dt, device="cuda"), 1)[None, None].expand(B, 1, S, S).clone()
    m[1, :, :, S - 40:] = fmin  # second sequence padded
    return m


def _bert_pad_mask(B, S, dt):
    m = torch.zeros(B, 1, 1, S, dtype=dt, device="cuda")
    m[0, ..., S - 17:] = torch.finfo(dt).min
    return m


def _opt():
    from outeffhop_amd import OPTAttentionWithExtras, SOFTMAX_MAPPING
    from outeffhop_amd.attention import AttentionGateType

    return OPTAttentionWithExtras(768, 12, dropout=0.0, is_decoder=True, softmax_fn=SOFTMAX_MAPPING["softmax1"],
                                  attn_gate_type=AttentionGateType.conditional_per_token, attn_gate_init=0.25)


def _bert(p_drop=0.0):
    from types import SimpleNamespace

    from outeffhop_amd import SOFTMAX_MAPPING, BertSelfAttentionWithExtras

    cfg = SimpleNamespace(hidden_size=768, num_attention_heads=12, attention_probs_dropout_prob=p_drop, position_embedding_type="absolute",
                          max_position_embeddings=512, is_decoder=False)
    return BertSelfAttentionWithExtras(cfg, softmax_fn=SOFTMAX_MAPPING["clippedsoftmax1(-.025:1)"])


def test_opt_module_trains_on_the_fused_kernels(monkeypatch):
    import outeffhop_amd.opt_attention as OA

    calls = []
    orig = OA.unfused_core
    monkeypatch.setattr(OA, "unfused_core", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    _module_case(_opt, _decoder_mask)
    assert len(calls) == 2  # the two switch-off runs (fp32 reference, fp16); none with the switch on


def test_bert_module_trains_on_the_fused_kernels(monkeypatch):
    import outeffhop_amd.bert_attention as BA

    calls = []
    orig = BA.unfused_core
    monkeypatch.setattr(BA, "unfused_core", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    _module_case(_bert, _bert_pad_mask)
    assert len(calls) == 2


def test_dropout_keeps_the_torch_op_path(monkeypatch):
    """BERT with attention dropout in training: the observable path runs even with the switch on (no fused call)."""
    import outeffhop_amd.bert_attention as BA
    from outeffhop_amd import attention as A
    from outeffhop_amd import autograd_attention as AA

    calls = []
    orig = BA.unfused_core
    monkeypatch.setattr(BA, "unfused_core", lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1])
    m = _bert(0.1).cuda().half().train()
    x = torch.randn(2, 64, 768, device="cuda").half().requires_grad_(True)
    prev = A.FUSED_BACKWARD
    n0 = AA.CALLS["forward"]
    try:
        A.set_fused_backward(True)
        m(x, attention_mask=_bert_pad_mask(2, 64, torch.float16))[0].float().sum().backward()
    finally:
        A.set_fused_backward(prev)
    assert AA.CALLS["forward"] == n0 and len(calls) == 1


def test_memory_has_no_sxs_term():
    """fwd + bwd of the fused core at S = 512 and 2048 (same B*H*S): peak memory beyond the inputs does not grow with S."""
    from outeffhop_amd import fused_attention

    peaks = []
    for B, S in ((8, 512), (2, 2048)):
        q, k, v = (torch.randn(B, 12, S, 64, device="cuda", dtype=torch.float16).requires_grad_(True) for _ in range(3))
        do = torch.randn(B, 12, S, 64, device="cuda", dtype=torch.float16)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fused_attention(q, k, v, softmax=_spec("softmax1"), causal=True).backward(do)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        del q, k, v, do
    assert peaks[1] <= 1.25 * peaks[0], peaks  # an S x S term would make the second 4x the first
