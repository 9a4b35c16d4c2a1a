"""Split-key decode attention (ops.attn_decode / oeh_attn_decode) on the GPU against the CPU oracle on the 16-bit-rounded inputs, and the
OPT module's generation steps against the oracle on the whole sequence.  `-m gpu`.

Limits - the project's contract, per (batch, head) with s = max(1, |V|max):
  fp32 output (the accumulators, out_dtype=float32): 1e-3 s;  fp16 output: that plus half an fp16 ulp of the reference value;
  bf16 storage: 8e-3 s plus half a bf16 ulp of the reference value.
"""

import numpy as np
import pytest

from oracle import oeh_oracle as O
from tests.test_attn_gpu import SPECS, _np32, _outlier_qkv, _rand, _spec

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FMIN = float(np.finfo(np.float32).min)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _limit(want, v, out_dtype):
    s = np.maximum(1.0, np.abs(v).max(axis=(-1, -2)))[..., None, None]
    if out_dtype == torch.float32:
        return 1e-3 * s
    if out_dtype == torch.float16:
        return 1e-3 * s + 0.5 * np.spacing(np.abs(want).astype(np.float16)).astype(np.float32)
    return 8e-3 * s + 0.5 * np.spacing(np.abs(want).astype(np.float32)) * 65536.0  # (a bf16 ulp is 2^16 fp32 ulps)


def _check(got, want, v, msg):
    out_dtype = got.dtype
    got = _np32(got)
    assert np.isfinite(got).all(), f"{msg}: non-finite output"
    err = np.abs(got - want)
    lim = _limit(want, v, out_dtype)
    print(f"decode {msg} [{str(out_dtype)[6:]}]: max abs err {err.max():.2e}, worst err / limit {float((err / lim).max()):.2f}")
    assert (err <= lim).all(), f"{msg}: max abs err {err.max():.3e}, worst excess {float((err - lim).max()):.3e}"


def _pad_vector(B, Sk):
    """sample 0: the first 40 keys padded (left padding); sample 1 (when there is one): no visible key at all"""
    pad = np.zeros((B, Sk), dtype=np.float32)
    pad[0, :40] = FMIN
    if B > 1:
        pad[1, :] = FMIN
    return pad


GRID = [(2, 3, 1, 77, 4), (2, 3, 1, 1000, 16), (1, 2, 5, 333, 7), (2, 2, 16, 2049, 32), (2, 2, 16, 2049, 0), (3, 2, 1, 16, 4), (2, 2, 3, 130, 64), (1, 1, 1, 1, 0)]


@pytest.mark.parametrize("B,H,Sq,Sk,splits", GRID)
def test_parity_grid(ops, B, H, Sq, Sk, splits):
    """Ragged last chunks, one key in the last chunk, all 16 rows real, one tile, more splits asked than chunks, a single key; fully padded
    chunks in front of visible ones and rows without a visible key under both bases (softmax_1: exactly 0; vanilla: uniform over all keys)."""
    D = 64
    pad = _pad_vector(B, Sk)
    pad_t = torch.from_numpy(pad).cuda()
    for dt in (torch.float16, torch.bfloat16):
        q = (_rand((B, H, Sq, D), 101, dtype=torch.float32) * D ** -0.5).to(dt)
        k, v = _rand((B, H, Sk, D), 102, dtype=dt), _rand((B, H, Sk, D), 103, dtype=dt)
        qn, kn, vn = _np32(q), _np32(k), _np32(v)
        qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
        for sm in SPECS:
            for causal in (False, True):
                want = O.attn_core(qn, kn, vn, pad_mask=pad, causal=causal, clamp_min=causal, mask_min=FMIN, **SPECS[sm])
                kw = dict(softmax=_spec(ops, sm), key_pad_mask=pad_t, causal=causal, clamp_min=causal, mask_min=FMIN, splits=splits)
                msg = f"{(B, H, Sq, Sk, splits)} {sm} causal={causal}"
                got = ops.attn_decode(qc, kc, vc, **kw)
                assert got.shape == (B, H, Sq, D) and got.dtype == dt and got.permute(0, 2, 1, 3).is_contiguous()
                _check(got, want, vn, msg)
                if dt == torch.float16:
                    a32 = ops.attn_decode(qc, kc, vc, out_dtype=torch.float32, **kw)
                    assert a32.dtype == torch.float32
                    _check(a32, want, vn, msg)
                if B > 1 and SPECS[sm]["base"] == 1:
                    assert float(got[1].abs().max()) == 0.0, f"{msg}: a softmax_1 row without a visible key must be exactly 0"


@pytest.mark.parametrize("kind", ["last_tile_jump", "ascending"])
def test_cross_split_dynamics(ops, kind):
    """The running maximum moves from split to split: the last 64 keys score +25 above everything before / the scores ascend by 0.25 per key."""
    B, H, Sq, Sk, D, splits = 1, 2, 1, 512, 64, 8
    qf, kf, vf = _outlier_qkv(kind, B, H, Sk, D, 4000 + len(kind))
    for dt in (torch.float16, torch.bfloat16):
        q, k, v = (torch.from_numpy(a).to(dt) for a in (qf[:, :, -1:], kf, vf))
        qn, kn, vn = _np32(q), _np32(k), _np32(v)
        assert ops.attn_decode_variant(B, H, Sq, Sk, dtype=dt, splits=splits) == f"decode16/SP8/D64/{'f16' if dt == torch.float16 else 'bf16'}"
        for sm in SPECS:
            want = O.attn_core(qn, kn, vn, causal=True, clamp_min=True, **SPECS[sm])
            kw = dict(softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=FMIN, splits=splits)
            _check(ops.attn_decode(q.cuda(), k.cuda(), v.cuda(), **kw), want, vn, f"{kind} {sm}")
            if dt == torch.float16:
                _check(ops.attn_decode(q.cuda(), k.cuda(), v.cuda(), out_dtype=torch.float32, **kw), want, vn, f"{kind} {sm}")


def test_layouts(ops):
    """k / v as slices of a longer preallocated cache and as permuted (B,S,H*64) views; q from (B,Sq,H*64)."""
    B, H, Sq, Sk, D = 2, 3, 2, 300, 64
    q3 = (_rand((B, Sq, H * D), 111, dtype=torch.float32) * D ** -0.5).half()
    cache_k, cache_v = _rand((B, H, 512, D), 112), _rand((B, H, 512, D), 113)
    q = q3.view(B, Sq, H, D).permute(0, 2, 1, 3)
    want = O.attn_core(_np32(q), _np32(cache_k[:, :, :Sk]), _np32(cache_v[:, :, :Sk]), causal=True, clamp_min=True, **SPECS["softmax1"])
    kw = dict(causal=True, clamp_min=True, mask_min=FMIN, splits=4)
    qc = q3.cuda().view(B, Sq, H, D).permute(0, 2, 1, 3)
    ck, cv = cache_k.cuda(), cache_v.cuda()
    got = ops.attn_decode(qc, ck[:, :, :Sk], cv[:, :, :Sk], **kw)
    _check(got, want, _np32(cache_v[:, :, :Sk]), "cache slices")
    k3 = cache_k[:, :, :Sk].permute(0, 2, 1, 3).reshape(B, Sk, H * D).contiguous().cuda()
    v3 = cache_v[:, :, :Sk].permute(0, 2, 1, 3).reshape(B, Sk, H * D).contiguous().cuda()
    got2 = ops.attn_decode(qc, k3.view(B, Sk, H, D).permute(0, 2, 1, 3), v3.view(B, Sk, H, D).permute(0, 2, 1, 3), **kw)
    assert torch.equal(got, got2)  # the same numbers through other strides: the same bits
    assert got.permute(0, 2, 1, 3).reshape(B, Sq, H * D).data_ptr() == got.data_ptr()  # head merge is free


def test_gate_scale_div_and_f16_mask(ops):
    B, H, Sq, Sk, D = 2, 3, 4, 200, 64
    q, k, v = _rand((B, H, Sq, D), 121), _rand((B, H, Sk, D), 122), _rand((B, H, Sk, D), 123)
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    g = torch.rand((B, H, Sq, 1), generator=torch.Generator().manual_seed(124))
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=8.0, scale_is_divisor=True, gate=g.numpy(), **SPECS["softmax1"])
    _check(ops.attn_decode(qc, kc, vc, scale_div=8.0, gate=g.cuda(), splits=3), want, _np32(v), "gate per token")
    gh = torch.rand((H, 1, 1), generator=torch.Generator().manual_seed(125))
    for sm in ("vanilla", "clippedsoftmax1(-.025:1)"):
        want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=0.125, gate=gh.numpy()[None], **SPECS[sm])
        _check(ops.attn_decode(qc, kc, vc, softmax=_spec(ops, sm), scale=0.125, gate=gh.cuda(), splits=3), want, _np32(v), f"gate per head {sm}")
    # HF's (B,1,1,Sk) fp16 extended mask, finfo(fp16).min entries
    f16min = float(np.finfo(np.float16).min)
    pad = np.zeros((B, Sk), dtype=np.float32)
    pad[1, 150:] = f16min
    want = O.attn_core(_np32(q), _np32(k), _np32(v), scale=0.125, pad_mask=pad, clamp_min=True, mask_min=f16min, **SPECS["softmax1"])
    got = ops.attn_decode(qc, kc, vc, scale=0.125, key_pad_mask=torch.from_numpy(pad).half().view(B, 1, 1, Sk).cuda(), clamp_min=True, mask_min=f16min)
    _check(got, want, _np32(v), "fp16 mask")


def test_reproducible_scratch_independent_and_graph_safe(ops):
    """Two calls give the same bits; the scratch's contents before the call do not matter (NaN against zeros); one graph capture and a single
    replay match the eager call bit for bit."""
    B, H, Sq, Sk, D = 2, 4, 1, 1000, 64
    q, k, v = _rand((B, H, Sq, D), 131).cuda(), _rand((B, H, Sk, D), 132).cuda(), _rand((B, H, Sk, D), 133).cuda()
    for sm in ("softmax1", "clippedsoftmax1(-.025:1)"):
        kw = dict(softmax=_spec(ops, sm), scale=0.125, causal=True, clamp_min=True, mask_min=FMIN, splits=16)
        first = ops.attn_decode(q, k, v, **kw)
        work = ops._decode_scratch(q.device, 16)
        work.view(torch.float32).fill_(float("nan"))
        with_nan = ops.attn_decode(q, k, v, **kw)
        assert ops._decode_scratch(q.device, 16) is work
        work.zero_()
        with_zeros = ops.attn_decode(q, k, v, **kw)
        assert torch.equal(first, with_nan) and torch.equal(with_nan, with_zeros), sm
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = ops.attn_decode(q, k, v, **kw)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, first), sm


def test_captured_call_owns_its_scratch(ops):
    """A call under graph capture gets scratch of its own (the graph's pool), never the cached buffer an eager call may later replace."""
    q, k, v = _rand((1, 2, 1, 64), 141).cuda(), _rand((1, 2, 300, 64), 142).cuda(), _rand((1, 2, 300, 64), 143).cuda()
    eager = ops.attn_decode(q, k, v, splits=4)
    cached = ops._decode_scratch(q.device, 16)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert ops._decode_scratch(q.device, 16) is not cached
        captured = ops.attn_decode(q, k, v, splits=4)
    ops._decode_work.clear()  # the eager buffers go away; the graph's do not
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)


@pytest.fixture
def split_decode_on():
    """the modules' opt-in routing of generation steps (attention.SPLIT_DECODE), restored afterwards"""
    from outeffhop_amd import attention

    before = attention.SPLIT_DECODE
    attention.set_split_decode(True)
    yield attention
    attention.set_split_decode(before)


def _hf_mask(B, tgt, src, left_pad, dtype):
    """HF's decoder mask (B,1,tgt,src): causal with the cache offset, plus left padding of sample b by left_pad[b] keys"""
    fmin = torch.finfo(dtype).min
    m = torch.full((tgt, src), fmin, dtype=torch.float32).triu(1 + src - tgt)[None, None].repeat(B, 1, 1, 1)
    for b, n in enumerate(left_pad):
        m[b, :, :, :n] = fmin
    return m.clamp(min=fmin).to(dtype)


def _state_np(mod):
    return {k_: v_.detach().float().cpu().numpy() for k_, v_ in mod.state_dict().items()}


# fp16 OPTAttentionWithExtras(128, 2) against the fp32 oracle: the tolerance tests/test_modules_gpu.py::test_opt_module_all_cases sets for this
# very module geometry in fp16 ("fp16 softmax1": atol = rtol = 6e-3; its 4e-3 belongs to the 12-head, E = 768 case)
MODULE_TOL = dict(atol=6e-3, rtol=6e-3)


@pytest.mark.parametrize("form", ["softmax1", "alpha"])
def test_opt_module_generation_steps(ops, form, split_decode_on):
    """Prefill 40 tokens, then 3 steps of one token with an HF (B,1,1,src) mask that left-pads one sample: each step equals the matching row of
    the oracle on the whole sequence; the steps run the decode kernels (DECODE_CALLS), and with the switch off the general forward."""
    import outeffhop_amd as oa

    attention = split_decode_on
    torch.manual_seed(7)
    B, T0, steps, E, H = 2, 40, 3, 128, 2
    kw = dict(softmax_fn=oa.SOFTMAX_MAPPING["softmax1"]) if form == "softmax1" else dict(alpha=12.0, max_seq_length=64, attn_softmax="softmax1")
    m = oa.OPTAttentionWithExtras(E, H, is_decoder=True, **kw).cuda().half().eval()
    spec = oa.spec_of(m.softmax_fn)
    total = T0 + steps
    hidden = torch.randn(B, total, E).half()
    left = [0, 7]
    full = _hf_mask(B, total, total, left, torch.float16)
    want = O.opt_attention(_state_np(m), _np32(hidden), H, mask=_np32(full), base=spec.base, gamma=spec.gamma, eta=spec.eta, clip=bool(spec.clip))
    hc = hidden.cuda()

    def run():
        outs = []
        with torch.no_grad():
            out, _, past = m(hc[:, :T0], attention_mask=full[:, :, :T0, :T0].cuda())
            outs.append(out)
            for t in range(T0, total):
                step_mask = full[:, :, t:t + 1, :t + 1].contiguous().cuda()  # (B,1,1,src)
                out, _, past = m(hc[:, t:t + 1], past_key_value=past, attention_mask=step_mask)
                assert past[0].shape == (B, H, t + 1, E // H)
                outs.append(out)
        return torch.cat(outs, dim=1), past[1]

    calls = ops.DECODE_CALLS
    got, past_v = run()
    assert ops.DECODE_CALLS == calls + steps
    err = np.abs(_np32(got) - want)
    lim = MODULE_TOL["atol"] + MODULE_TOL["rtol"] * np.abs(want)
    print(f"opt generation steps {form}: max abs err prefill {err[:, :T0].max():.2e}, steps {err[:, T0:].max():.2e}")
    assert (err <= lim).all(), f"{form}: max err {err.max():.3e}"
    try:
        attention.set_split_decode(False)
        calls = ops.DECODE_CALLS
        ref, _ = run()
        assert ops.DECODE_CALLS == calls
    finally:
        attention.set_split_decode(True)
    # the two differ by at most twice the contract limit (1e-3 max(1, |V|max) + half an fp16 ulp of the value)
    vmax = max(1.0, float(past_v.float().abs().max()))
    lim2 = 2.0 * (1e-3 * vmax + 0.5 * np.spacing(np.abs(_np32(ref)).astype(np.float16)).astype(np.float32))
    diff = np.abs(_np32(got) - _np32(ref))
    print(f"opt generation steps {form}: decode on / off differ by {diff.max():.2e} (worst diff / limit {float((diff / lim2).max()):.2f})")
    assert (diff <= lim2).all()


def test_opt_module_head_dim_32_falls_back(ops, split_decode_on):
    """E = 128, H = 4 (head dim 32): outside the decode kernels - the module runs ops.attn_fwd silently and is still right."""
    import outeffhop_amd as oa

    torch.manual_seed(8)
    B, T0, E, H = 2, 40, 128, 4
    m = oa.OPTAttentionWithExtras(E, H, is_decoder=True, softmax_fn=oa.SOFTMAX_MAPPING["softmax1"]).cuda().half().eval()
    hidden = torch.randn(B, T0 + 1, E).half()
    full = _hf_mask(B, T0 + 1, T0 + 1, [0, 7], torch.float16)
    want = O.opt_attention(_state_np(m), _np32(hidden), H, mask=_np32(full), base=1)
    calls = ops.DECODE_CALLS
    with torch.no_grad():
        _, _, past = m(hidden[:, :T0].cuda(), attention_mask=full[:, :, :T0, :T0].cuda())
        out, _, _ = m(hidden[:, T0:].cuda(), past_key_value=past, attention_mask=full[:, :, T0:, :].contiguous().cuda())
    assert ops.DECODE_CALLS == calls
    err = np.abs(_np32(out) - want[:, T0:])
    assert (err <= MODULE_TOL["atol"] + MODULE_TOL["rtol"] * np.abs(want[:, T0:])).all(), f"max err {err.max():.3e}"


def test_opt_module_library_refusal_falls_back(ops, split_decode_on, monkeypatch):
    """A clipped softmax with gamma > 0 (alpha < 0) passes the module's routing conditions and is refused by the library (-95): the step runs
    ops.attn_fwd silently and is still right."""
    import outeffhop_amd as oa
    from outeffhop_amd._lib import OehError

    torch.manual_seed(9)
    B, T0, E, H = 2, 40, 128, 2
    m = oa.OPTAttentionWithExtras(E, H, is_decoder=True, alpha=-4.0, max_seq_length=64, attn_softmax="softmax1").cuda().half().eval()
    spec = oa.spec_of(m.softmax_fn)
    assert spec.clip and spec.gamma > 0
    hidden = torch.randn(B, T0 + 1, E).half()
    full = _hf_mask(B, T0 + 1, T0 + 1, [0, 7], torch.float16)
    want = O.opt_attention(_state_np(m), _np32(hidden), H, mask=_np32(full), base=spec.base, gamma=spec.gamma, eta=spec.eta, clip=True)
    refused = []
    real = ops.attn_decode

    def spy(*a, **kw):
        try:
            return real(*a, **kw)
        except OehError as e:
            refused.append(e.code)
            raise

    monkeypatch.setattr(ops, "attn_decode", spy)
    calls = ops.DECODE_CALLS
    with torch.no_grad():
        _, _, past = m(hidden[:, :T0].cuda(), attention_mask=full[:, :, :T0, :T0].cuda())
        out, _, _ = m(hidden[:, T0:].cuda(), past_key_value=past, attention_mask=full[:, :, T0:, :].contiguous().cuda())
    assert refused == [-95] and ops.DECODE_CALLS == calls
    err = np.abs(_np32(out) - want[:, T0:])
    assert (err <= MODULE_TOL["atol"] + MODULE_TOL["rtol"] * np.abs(want[:, T0:])).all(), f"max err {err.max():.3e}"
