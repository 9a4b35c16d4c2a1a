"""Which core every drop-in attention module runs, and with which arguments, checked without a GPU: the real modules
(outeffhop_amd/bert_attention.py, opt_attention.py, vit_attention.py and the two quantised wrappers of quantization.py) run on CPU
tensors, everything that touches a device is replaced, and the `ops` entry points the modules call - and
`autograd_attention.fused_attention` - are recorders that return a tensor of the right shape.  A case's result is the ordered list
of recorded calls; an attention call is written with the arguments that encode the decision (the shapes of q / k / v, which of
key_pad_mask / full_mask / causal is set, clamp_min and mask_min, scale / scale_div, gate values or the in-kernel predictor, the
decode entry point, fq.ctx_before_gate), a gate call with its pooling, and `-> ctx` is the merged context the module hands on
(its value where it is uniform: the recorders return ones, so a differentiable core's context shows the gate times its scaling).

The expected lists are the literal table ROUTES, produced by running this file on the tree before the modules shared their
mask / K-V / gate helpers.  One difference to that tree is deliberate and marked in the table with `Twice(now, before)`: a
quantised forward whose INT8 route declined evaluated its gate a second time.

Routes that open only for `is_cuda` inputs cannot be reached this way: `attention.fused_qkv`, the triple GEMM (`linear_fp32`),
`_QuantAttnBase._calibrate_fused` and `_int8_storage_core` (which here declines at its first line - that is the Twice case).  The
GPU suite covers them: tests/test_modules_gpu.py, test_quantised_opt_uses_the_int8_storage_core through
test_frozen_int8_layers_replay_a_prebuilt_plan, and test_fused_qkv_projection_matches_three_linears."""
import contextlib
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import outeffhop_amd as oa
from outeffhop_amd import _lib, attention, autograd_attention, ops
from outeffhop_amd.attention import AttentionGateType as G

B, H, D, S = 2, 2, 64, 16  # the smallest sizes at which every branch exists; the decode step meets a cache of S keys
E = H * D
FMIN = {float(torch.finfo(dt).min): name for dt, name in ((torch.float32, "f32"), (torch.float16, "f16"), (torch.bfloat16, "bf16"))}
BEFORE = not hasattr(attention, "module_gate")  # this file running on the tree the table was produced on


class Twice(tuple):
    """(the calls now, the calls with the gate evaluated a second time after the INT8 route declined)."""

    def __new__(cls, now, before):
        return super().__new__(cls, (now, before))


# ---- recorders
def _shape(t):
    return "x".join(str(n) for n in t.shape)


def _uniform(t):
    t = t.detach().float()
    return f"{float(t.flatten()[0]):g}" if bool((t == t.flatten()[0]).all()) else "var"


def _attn_args(q, k, v, kw):
    out = [f"q{_shape(q)} k{_shape(k)} v{_shape(v)}"]
    out += [name for name, key in (("pad", "key_pad_mask"), ("full", "full_mask")) if kw.get(key) is not None]
    out += [name for name, key in (("causal", "causal"), ("pad_bool", "key_pad_boolean"), ("clamp", "clamp_min"), ("pv_pairs", "pv_pairs")) if kw.get(key)]
    mm = kw.get("mask_min")
    out.append("min=" + ("None" if mm is None else FMIN.get(float(mm), f"{mm:g}")))
    out.append(f"scale={kw.get('scale', 1.0):g} div={kw.get('scale_div', 0.0):g}")
    if kw.get("gate") is not None:
        out.append(f"gate={_shape(kw['gate'])}:{_uniform(kw['gate'])}")
    if kw.get("gate_mlp") is not None:
        gp = kw["gate_mlp"]
        out.append(f"gate_mlp[units={0 if gp.w1.dim() == 2 else gp.w1.shape[1]} scaling={gp.scaling:g}]")
    if kw.get("fq") is not None:
        out.append(f"fq[ctx_before_gate={kw['fq'].ctx_before_gate}]")
    if kw.get("dropout_p"):
        out.append(f"dropout_p={kw['dropout_p']:g}")
    return " ".join(out)


def recorders(monkeypatch):
    """Replace what touches a device; returns the list the recorders append to."""
    log = []

    def core(name):
        def fn(q, k, v, **kw):
            log.append(f"{name}({_attn_args(q, k, v, kw)})")
            if kw.get("gate_mlp") is not None and kw["gate_mlp"].out is not None:
                kw["gate_mlp"].out.fill_(0.5)
            Bq, Hq, Sq, Dq = q.shape
            return torch.ones(Bq, Sq, Hq, Dq, dtype=q.dtype).permute(0, 2, 1, 3)
        return fn

    def gate_fwd(hidden, nh, w1, b1, w2=None, b2=None, per_head_pool=False, scaling=1.0):
        log.append(f"gate_fwd(units={0 if w1.dim() == 2 else w1.shape[1]} pool={per_head_pool} scaling={scaling:g})")
        return torch.full((hidden.shape[0], nh, 1 if per_head_pool else hidden.shape[1], 1), 0.5)

    def softmax_rows(x, spec=None, dim=-1, out=None):
        log.append("softmax_rows")
        return torch.softmax(x.float(), dim=dim).to(x.dtype)

    def named(name, result):
        def fn(*a, **kw):
            log.append(name)
            return result(*a, **kw)
        return fn

    def no_library():
        raise AssertionError("a module reached the library past the recorders")

    monkeypatch.setattr(ops, "_need_gpu", lambda *ts, allow_grad=False: torch.device("cpu"))
    monkeypatch.setattr(ops, "_on_device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(ops, "_stream", lambda: C.c_void_p(0))
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(ops, "attn_fwd", core("attn_fwd"))
    monkeypatch.setattr(ops, "attn_decode", core("attn_decode"))
    monkeypatch.setattr(ops, "attn_calibrate", named("attn_calibrate", lambda q, *a, **kw: torch.ones(q.shape[0], q.shape[2], q.shape[1], q.shape[3]).permute(0, 2, 1, 3)))
    monkeypatch.setattr(ops, "fused_gate_ok", lambda *a, **kw: True)  # (the host-only probe: the in-kernel predictor is taken where it is offered)
    monkeypatch.setattr(ops, "gate_fwd", gate_fwd)
    monkeypatch.setattr(ops, "softmax_rows", softmax_rows)
    monkeypatch.setattr(ops, "fake_quant", named("fake_quant", lambda x, spec, want_idx=False: x))
    monkeypatch.setattr(ops, "fake_quant_range", named("fake_quant_range", lambda x, *a, **kw: x))
    monkeypatch.setattr(ops, "minmax", named("minmax", lambda x: torch.stack([x.min(), x.max()]).float()))
    monkeypatch.setattr(autograd_attention, "fused_supported", lambda q, k, v, softmax: True)
    monkeypatch.setattr(autograd_attention, "fused_attention", core("fused_attention"))
    monkeypatch.setattr(attention, "_warned_autograd", [True])
    for switch in ("FUSED_BACKWARD", "FUSED_DROPOUT", "SPLIT_DECODE", "COMPENSATED_PV"):
        monkeypatch.setattr(attention, switch, False)
    attention._causal_cache.clear()
    return log


@pytest.fixture
def calls(monkeypatch):
    return recorders(monkeypatch)


# ---- the cases: module x scenario x gate
GATES = {
    "none": {},
    "uncond": dict(attn_gate_type=G.unconditional_per_head),
    "head": dict(attn_gate_type=G.conditional_per_head),
    "token": dict(attn_gate_type=G.conditional_per_token),
    "token_mlp": dict(attn_gate_type=G.conditional_per_token, attn_gate_mlp=True),
    "allfeat": dict(attn_gate_type=G.conditional_per_token, attn_gate_linear_all_features=True),
}
FT = dict(fine_tuning=True, attn_gate_init=0.25)  # gate_scaling_factor = 4
# scenario -> (mask, cross, cached, head mask, output_attentions, tap hook, training with dropout, autograd, FUSED_BACKWARD, SPLIT_DECODE)
_S = lambda mask=None, cross=False, cached=False, hm=False, oa_=False, hook=False, drop=False, grad=False, fb=False, sd=False: SimpleNamespace(  # noqa: E731
    mask=mask, cross=cross, cached=cached, hm=hm, oa=oa_, hook=hook, drop=drop, grad=grad, fb=fb, sd=sd)
SCENARIOS = {
    "nomask": _S(), "pad": _S(mask="pad"), "causal": _S(mask="causal"), "leftpad": _S(mask="leftpad"), "full": _S(mask="full"),
    "wrongsize": _S(mask="wrong"), "cross": _S(cross=True, mask="pad"), "cross_cached": _S(cross=True, cached=True, mask="pad"),
    "step": _S(cached=True, mask="step"), "step_split": _S(cached=True, mask="step", sd=True), "head_mask": _S(hm=True),
    "output_attentions": _S(oa_=True), "hook": _S(hook=True), "dropout": _S(drop=True), "autograd": _S(grad=True),
    "autograd_fused": _S(grad=True, fb=True), "autograd_fused_pad": _S(grad=True, fb=True, mask="pad"),
}
FAMILY = {"bert": "bert", "opt": "opt", "vit": "vit", "qbert_est": "bert", "qbert_fix": "bert", "qopt_est": "opt", "qopt_fix": "opt"}
APPLIES = {
    "bert": ("nomask", "pad", "cross", "cross_cached", "step", "head_mask", "output_attentions", "hook", "dropout", "autograd", "autograd_fused",
             "autograd_fused_pad"),
    "opt": ("nomask", "causal", "leftpad", "full", "wrongsize", "cross", "cross_cached", "step", "step_split", "head_mask", "output_attentions", "hook",
            "dropout", "autograd", "autograd_fused"),
    "vit": ("nomask", "hook", "dropout", "autograd", "autograd_fused"),
}


def case_ids():
    for mod, fam in FAMILY.items():
        for sc in APPLIES[fam]:
            if sc == "hook" and mod.startswith("q"):  # (the quantised modules have no taps)
                continue
            for gate in ("none", "token+ft"):
                yield f"{mod}/{sc}/{gate}"
        for gate in GATES:
            for ft in ("", "+ft"):
                if f"{gate}{ft}" not in ("none", "token+ft"):
                    yield f"{mod}/nomask/{gate}{ft}"


def _mask(kind, Sk):
    fmin = torch.finfo(torch.float32).min
    if kind is None:
        return None
    if kind in ("pad", "wrong"):  # (B,1,1,S): BERT's key padding; not a size OPT takes for S query rows
        m = torch.zeros(B, 1, 1, Sk)
        m[1, :, :, -3:] = fmin
        return m
    if kind == "step":  # one query row against the cache and itself
        return torch.zeros(B, 1, 1, Sk)
    if kind == "full":  # (B,1,S,S), not causal
        m = torch.zeros(B, 1, S, Sk)
        m[:, :, :, 2] = fmin
        return m
    m = torch.full((S, Sk), fmin).triu(1)[None, None].repeat(B, 1, 1, 1)  # HF's decoder mask
    if kind == "leftpad":
        m[1, :, :, :3] = fmin
    return m


def run_case(cid, log, monkeypatch):
    mod, sc_name, gate_name = cid.split("/")
    fam, sc = FAMILY[mod], SCENARIOS[sc_name]
    gate_kw = dict(GATES[gate_name.replace("+ft", "")], **(FT if gate_name.endswith("+ft") else {}))
    monkeypatch.setattr(attention, "FUSED_BACKWARD", sc.fb)
    monkeypatch.setattr(attention, "SPLIT_DECODE", sc.sd)
    dt = torch.float16 if sc.sd else torch.float32  # (the decode kernels take 16-bit storage only)
    p_drop = 0.1 if sc.drop else 0.0
    sm = oa.SOFTMAX_MAPPING["softmax1"]
    torch.manual_seed(0)
    if fam == "bert":
        cfg = SimpleNamespace(hidden_size=E, num_attention_heads=H, attention_probs_dropout_prob=p_drop, max_position_embeddings=64,
                              is_decoder=sc.cached or sc.cross, position_embedding_type="absolute")
        m = oa.BertSelfAttentionWithExtras(cfg, softmax_fn=sm, **gate_kw)
        last = None
    elif fam == "opt":
        m = oa.OPTAttentionWithExtras(E, H, dropout=p_drop, is_decoder=True, softmax_fn=sm, **gate_kw)
        last = "out_proj"
    else:
        m = oa.ViTSelfAttentionWithExtras(E, num_heads=H, qkv_bias=True, attn_drop=p_drop, softmax_fn=sm, **gate_kw)
        last = "proj"
    m = m.to(dt)
    if sc.hook:
        m.attn_probs_before_dropout.register_forward_hook(lambda *a: None)
    x = torch.randn(B, 1 if sc.cached and not sc.cross else S, E, dtype=dt)
    past = (torch.randn(B, H, S, D, dtype=dt), torch.randn(B, H, S, D, dtype=dt)) if sc.cached else None
    enc = torch.randn(B, S, E, dtype=dt) if sc.cross else None
    Sk = S + 1 if sc.cached and not sc.cross else S
    mask = _mask(sc.mask, Sk)
    mask = None if mask is None else mask.clamp(min=torch.finfo(dt).min).to(dt)
    if fam == "bert":
        kw = dict(attention_mask=None if sc.cross else mask, head_mask=torch.ones(1, H, 1, 1) if sc.hm else None, encoder_hidden_states=enc,
                  encoder_attention_mask=mask if sc.cross else None, past_key_value=past, output_attentions=sc.oa)
    elif fam == "opt":
        kw = dict(key_value_states=enc, past_key_value=past, attention_mask=None if sc.cross else mask,
                  layer_head_mask=torch.ones(H) if sc.hm else None, output_attentions=sc.oa)
    else:
        kw = {}
    if mod.startswith("q"):
        qp = oa.get_quant_config()
        qp.act_quant.options = dict(percentile=99.999)
        wrap = oa.QuantizedBertSelfAttentionWithExtras if fam == "bert" else oa.QuantizedOPTAttentionWithExtras
        m = wrap(m, **{**oa.val_qparams(qp), "quant_dict": {}})
        m.set_quant_state(weight_quant=True, act_quant=True)
        if mod.endswith("_fix"):  # ranges estimated on one batch of the same kind, then frozen
            with torch.no_grad():
                with contextlib.suppress(ValueError):
                    m.eval()(x, **kw)
            m.fix_ranges()
            del log[:]
    m.train(sc.drop)
    seen = []
    if last is not None:
        getattr(m, last).register_forward_pre_hook(lambda _m, args: seen.append(args[0]))
    with torch.enable_grad() if sc.grad else torch.no_grad():
        try:
            out = m(x, **kw)
        except ValueError as e:
            return log + [f"ValueError: {e}"]
    ctx = seen[0] if seen else (out[0] if isinstance(out, tuple) else out)
    return log + [f"-> ctx {_shape(ctx)}:{_uniform(ctx)}"]


def fold(calls):
    """The call list as one line; a run of the same call as `call xN`."""
    out = []
    for c in calls:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return " | ".join(c if n == 1 else f"{c} x{n}" for c, n in out)


@pytest.mark.parametrize("cid", list(case_ids()))
def test_module_route(cid, calls, monkeypatch):
    want = ROUTES[cid]
    if isinstance(want, Twice):
        want = want[1] if BEFORE else want[0]
    assert fold(run_case(cid, calls, monkeypatch)) == want


def test_the_table_has_no_other_cases():
    assert set(ROUTES) == set(case_ids())


# fmt: off
ROUTES = {
    "bert/nomask/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8) | -> ctx 2x16x128:1",
    "bert/nomask/token+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate_mlp[units=0 scaling=4]) | -> ctx 2x16x128:1",
    "bert/pad/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad min=f32 scale=1 div=8) | -> ctx 2x16x128:1",
    "bert/pad/token+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad min=f32 scale=1 div=8 gate_mlp[units=0 scaling=4]) | -> ctx 2x16x128:1",
    "bert/cross/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad min=f32 scale=1 div=8) | -> ctx 2x16x128:1",
    "bert/cross/token+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad min=f32 scale=1 div=8 gate_mlp[units=0 scaling=4]) | -> ctx 2x16x128:1",
    "bert/cross_cached/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad min=f32 scale=1 div=8) | -> ctx 2x16x128:1",
    "bert/cross_cached/token+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad min=f32 scale=1 div=8 gate_mlp[units=0 scaling=4]) | -> ctx 2x16x128:1",
    "bert/step/none": "attn_fwd(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad min=f32 scale=1 div=8) | -> ctx 2x1x128:1",
    "bert/step/token+ft": "attn_fwd(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad min=f32 scale=1 div=8 gate_mlp[units=0 scaling=4]) | -> ctx 2x1x128:1",
    "bert/head_mask/none": "softmax_rows | -> ctx 2x16x128:var",
    "bert/head_mask/token+ft": "gate_fwd(units=0 pool=False scaling=1) | softmax_rows | -> ctx 2x16x128:var",
    "bert/output_attentions/none": "softmax_rows | -> ctx 2x16x128:var",
    "bert/output_attentions/token+ft": "gate_fwd(units=0 pool=False scaling=1) | softmax_rows | -> ctx 2x16x128:var",
    "bert/hook/none": "softmax_rows | -> ctx 2x16x128:var",
    "bert/hook/token+ft": "gate_fwd(units=0 pool=False scaling=1) | softmax_rows | -> ctx 2x16x128:var",
    "bert/dropout/none": "softmax_rows | -> ctx 2x16x128:var",
    "bert/dropout/token+ft": "gate_fwd(units=0 pool=False scaling=1) | softmax_rows | -> ctx 2x16x128:var",
    "bert/autograd/none": "-> ctx 2x16x128:var",
    "bert/autograd/token+ft": "-> ctx 2x16x128:var",
    "bert/autograd_fused/none": "fused_attention(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8) | -> ctx 2x16x128:1",
    "bert/autograd_fused/token+ft": "fused_attention(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8) | -> ctx 2x16x128:var",
    "bert/autograd_fused_pad/none": "fused_attention(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad min=f32 scale=1 div=8) | -> ctx 2x16x128:1",
    "bert/autograd_fused_pad/token+ft": "fused_attention(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad min=f32 scale=1 div=8) | -> ctx 2x16x128:var",
    "bert/nomask/none+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8) | -> ctx 2x16x128:1",
    "bert/nomask/uncond": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=1x2x1x1:0.5) | -> ctx 2x16x128:1",
    "bert/nomask/uncond+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=1x2x1x1:0.5) | -> ctx 2x16x128:1",
    "bert/nomask/head": "gate_fwd(units=0 pool=True scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x1x1:0.5) | -> ctx 2x16x128:1",
    "bert/nomask/head+ft": "gate_fwd(units=0 pool=True scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x1x1:2) | -> ctx 2x16x128:1",
    "bert/nomask/token": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate_mlp[units=0 scaling=1]) | -> ctx 2x16x128:1",
    "bert/nomask/token_mlp": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate_mlp[units=16 scaling=1]) | -> ctx 2x16x128:1",
    "bert/nomask/token_mlp+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate_mlp[units=16 scaling=4]) | -> ctx 2x16x128:1",
    "bert/nomask/allfeat": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:var) | -> ctx 2x16x128:1",
    "bert/nomask/allfeat+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:var) | -> ctx 2x16x128:1",
    "opt/nomask/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0) | -> ctx 2x16x128:1",
    "opt/nomask/token+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate_mlp[units=0 scaling=4]) | -> ctx 2x16x128:1",
    "opt/causal/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 causal clamp min=f32 scale=1 div=0) | -> ctx 2x16x128:1",
    "opt/causal/token+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 causal clamp min=f32 scale=1 div=0 gate_mlp[units=0 scaling=4]) | -> ctx 2x16x128:1",
    "opt/leftpad/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad causal clamp min=f32 scale=1 div=0) | -> ctx 2x16x128:1",
    "opt/leftpad/token+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad causal clamp min=f32 scale=1 div=0 gate_mlp[units=0 scaling=4]) | -> ctx 2x16x128:1",
    "opt/full/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 full clamp min=f32 scale=1 div=0) | -> ctx 2x16x128:1",
    "opt/full/token+ft": "gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 full clamp min=f32 scale=1 div=0 gate=2x2x16x1:2) | -> ctx 2x16x128:1",
    "opt/wrongsize/none": "ValueError: Attention mask should be of size (2, 1, 16, 16), but is torch.Size([2, 1, 1, 16])",
    "opt/wrongsize/token+ft": "ValueError: Attention mask should be of size (2, 1, 16, 16), but is torch.Size([2, 1, 1, 16])",
    "opt/cross/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0) | -> ctx 2x16x128:1",
    "opt/cross/token+ft": "gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:2) | -> ctx 2x16x128:1",
    "opt/cross_cached/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0) | -> ctx 2x16x128:1",
    "opt/cross_cached/token+ft": "gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:2) | -> ctx 2x16x128:1",
    "opt/step/none": "attn_fwd(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad clamp min=f32 scale=1 div=0) | -> ctx 2x1x128:1",
    "opt/step/token+ft": "gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad clamp min=f32 scale=1 div=0 gate=2x2x1x1:2) | -> ctx 2x1x128:1",
    "opt/step_split/none": "attn_decode(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad clamp min=f16 scale=1 div=0) | -> ctx 2x1x128:1",
    "opt/step_split/token+ft": "gate_fwd(units=0 pool=False scaling=1) | attn_decode(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad clamp min=f16 scale=1 div=0 gate=2x2x1x1:2) | -> ctx 2x1x128:1",
    "opt/head_mask/none": "softmax_rows | -> ctx 2x16x128:var",
    "opt/head_mask/token+ft": "gate_fwd(units=0 pool=False scaling=1) | softmax_rows | -> ctx 2x16x128:var",
    "opt/output_attentions/none": "softmax_rows | -> ctx 2x16x128:var",
    "opt/output_attentions/token+ft": "gate_fwd(units=0 pool=False scaling=1) | softmax_rows | -> ctx 2x16x128:var",
    "opt/hook/none": "softmax_rows | -> ctx 2x16x128:var",
    "opt/hook/token+ft": "gate_fwd(units=0 pool=False scaling=1) | softmax_rows | -> ctx 2x16x128:var",
    "opt/dropout/none": "softmax_rows | -> ctx 2x16x128:var",
    "opt/dropout/token+ft": "gate_fwd(units=0 pool=False scaling=1) | softmax_rows | -> ctx 2x16x128:var",
    "opt/autograd/none": "-> ctx 2x16x128:var",
    "opt/autograd/token+ft": "-> ctx 2x16x128:var",
    "opt/autograd_fused/none": "fused_attention(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0) | -> ctx 2x16x128:1",
    "opt/autograd_fused/token+ft": "fused_attention(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0) | -> ctx 2x16x128:var",
    "opt/nomask/none+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0) | -> ctx 2x16x128:1",
    "opt/nomask/uncond": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=1x2x1x1:0.5) | -> ctx 2x16x128:1",
    "opt/nomask/uncond+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=1x2x1x1:0.5) | -> ctx 2x16x128:1",
    "opt/nomask/head": "gate_fwd(units=0 pool=True scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x1x1:0.5) | -> ctx 2x16x128:1",
    "opt/nomask/head+ft": "gate_fwd(units=0 pool=True scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x1x1:2) | -> ctx 2x16x128:1",
    "opt/nomask/token": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate_mlp[units=0 scaling=1]) | -> ctx 2x16x128:1",
    "opt/nomask/token_mlp": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate_mlp[units=16 scaling=1]) | -> ctx 2x16x128:1",
    "opt/nomask/token_mlp+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate_mlp[units=16 scaling=4]) | -> ctx 2x16x128:1",
    "opt/nomask/allfeat": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:var) | -> ctx 2x16x128:1",
    "opt/nomask/allfeat+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:var) | -> ctx 2x16x128:1",
    "vit/nomask/none": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0) | -> ctx 2x16x128:1",
    "vit/nomask/token+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0 gate_mlp[units=0 scaling=4]) | -> ctx 2x16x128:1",
    "vit/hook/none": "softmax_rows | -> ctx 2x16x128:var",
    "vit/hook/token+ft": "gate_fwd(units=0 pool=False scaling=1) | softmax_rows | -> ctx 2x16x128:var",
    "vit/dropout/none": "softmax_rows | -> ctx 2x16x128:var",
    "vit/dropout/token+ft": "gate_fwd(units=0 pool=False scaling=1) | softmax_rows | -> ctx 2x16x128:var",
    "vit/autograd/none": "-> ctx 2x16x128:var",
    "vit/autograd/token+ft": "-> ctx 2x16x128:var",
    "vit/autograd_fused/none": "fused_attention(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0) | -> ctx 2x16x128:1",
    "vit/autograd_fused/token+ft": "fused_attention(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0) | -> ctx 2x16x128:var",
    "vit/nomask/none+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0) | -> ctx 2x16x128:1",
    "vit/nomask/uncond": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0 gate=1x2x1x1:0.5) | -> ctx 2x16x128:1",
    "vit/nomask/uncond+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0 gate=1x2x1x1:0.5) | -> ctx 2x16x128:1",
    "vit/nomask/head": "gate_fwd(units=0 pool=True scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0 gate=2x2x1x1:0.5) | -> ctx 2x16x128:1",
    "vit/nomask/head+ft": "gate_fwd(units=0 pool=True scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0 gate=2x2x1x1:2) | -> ctx 2x16x128:1",
    "vit/nomask/token": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0 gate_mlp[units=0 scaling=1]) | -> ctx 2x16x128:1",
    "vit/nomask/token_mlp": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0 gate_mlp[units=16 scaling=1]) | -> ctx 2x16x128:1",
    "vit/nomask/token_mlp+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0 gate_mlp[units=16 scaling=4]) | -> ctx 2x16x128:1",
    "vit/nomask/allfeat": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0 gate=2x2x16x1:var) | -> ctx 2x16x128:1",
    "vit/nomask/allfeat+ft": "attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=0.125 div=0 gate=2x2x16x1:var) | -> ctx 2x16x128:1",
    "qbert_est/nomask/none": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/nomask/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/pad/none": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/pad/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/cross/none": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/cross/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/cross_cached/none": "fake_quant x2 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/cross_cached/token+ft": "fake_quant | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/step/none": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x1x128:var",
    "qbert_est/step/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x1x128:var",
    "qbert_est/head_mask/none": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/head_mask/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/output_attentions/none": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/output_attentions/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/dropout/none": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/dropout/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/autograd/none": "fake_quant x6 | -> ctx 2x16x128:var",
    "qbert_est/autograd/token+ft": "fake_quant x6 | -> ctx 2x16x128:var",
    "qbert_est/autograd_fused/none": "fake_quant x6 | -> ctx 2x16x128:var",
    "qbert_est/autograd_fused/token+ft": "fake_quant x6 | -> ctx 2x16x128:var",
    "qbert_est/autograd_fused_pad/none": "fake_quant x6 | -> ctx 2x16x128:var",
    "qbert_est/autograd_fused_pad/token+ft": "fake_quant x6 | -> ctx 2x16x128:var",
    "qbert_est/nomask/none+ft": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/nomask/uncond": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/nomask/uncond+ft": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/nomask/head": "fake_quant x3 | gate_fwd(units=0 pool=True scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/nomask/head+ft": "fake_quant x3 | gate_fwd(units=0 pool=True scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/nomask/token": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/nomask/token_mlp": "fake_quant x3 | gate_fwd(units=16 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/nomask/token_mlp+ft": "fake_quant x3 | gate_fwd(units=16 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/nomask/allfeat": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_est/nomask/allfeat+ft": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_fix/nomask/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/nomask/token+ft": Twice("gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
                                       "gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1"),
    "qbert_fix/pad/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad pad_bool min=f32 scale=1 div=8 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/pad/token+ft": Twice("gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad pad_bool min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
                                    "gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad pad_bool min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1"),
    "qbert_fix/cross/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad pad_bool min=f32 scale=1 div=8 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/cross/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad pad_bool min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/cross_cached/none": "fake_quant | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad pad_bool min=f32 scale=1 div=8 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/cross_cached/token+ft": "fake_quant | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad pad_bool min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/step/none": "fake_quant x3 | attn_fwd(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad pad_bool min=f32 scale=1 div=8 fq[ctx_before_gate=False]) | -> ctx 2x1x128:1",
    "qbert_fix/step/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad pad_bool min=f32 scale=1 div=8 gate=2x2x1x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x1x128:1",
    "qbert_fix/head_mask/none": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_fix/head_mask/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_fix/output_attentions/none": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_fix/output_attentions/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_fix/dropout/none": "fake_quant x4 | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_fix/dropout/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x2 | -> ctx 2x16x128:var",
    "qbert_fix/autograd/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/autograd/token+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:var fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/autograd_fused/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/autograd_fused/token+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:var fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/autograd_fused_pad/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad pad_bool min=f32 scale=1 div=8 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/autograd_fused_pad/token+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad pad_bool min=f32 scale=1 div=8 gate=2x2x16x1:var fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/nomask/none+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/nomask/uncond": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=1x2x1x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/nomask/uncond+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=1x2x1x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/nomask/head": Twice("gate_fwd(units=0 pool=True scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x1x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
                                   "gate_fwd(units=0 pool=True scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=True scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x1x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1"),
    "qbert_fix/nomask/head+ft": Twice("gate_fwd(units=0 pool=True scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x1x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
                                      "gate_fwd(units=0 pool=True scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=True scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x1x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1"),
    "qbert_fix/nomask/token": Twice("gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
                                    "gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1"),
    "qbert_fix/nomask/token_mlp": Twice("gate_fwd(units=16 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
                                        "gate_fwd(units=16 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=16 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1"),
    "qbert_fix/nomask/token_mlp+ft": Twice("gate_fwd(units=16 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
                                           "gate_fwd(units=16 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=16 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:0.5 fq[ctx_before_gate=False]) | -> ctx 2x16x128:1"),
    "qbert_fix/nomask/allfeat": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:var fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qbert_fix/nomask/allfeat+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=8 gate=2x2x16x1:var fq[ctx_before_gate=False]) | -> ctx 2x16x128:1",
    "qopt_est/nomask/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/nomask/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/causal/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/causal/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/leftpad/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/leftpad/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/full/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/full/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/wrongsize/none": "fake_quant x3 | ValueError: Attention mask should be of size (2, 1, 16, 16), but is torch.Size([2, 1, 1, 16])",
    "qopt_est/wrongsize/token+ft": "fake_quant x3 | ValueError: Attention mask should be of size (2, 1, 16, 16), but is torch.Size([2, 1, 1, 16])",
    "qopt_est/cross/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/cross/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/cross_cached/none": "fake_quant x2 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/cross_cached/token+ft": "fake_quant | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/step/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x1x128:var",
    "qopt_est/step/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x1x128:var",
    "qopt_est/step_split/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x1x128:var",
    "qopt_est/step_split/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x1x128:var",
    "qopt_est/head_mask/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/head_mask/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/output_attentions/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/output_attentions/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/dropout/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/dropout/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/autograd/none": "fake_quant x7 | -> ctx 2x16x128:var",
    "qopt_est/autograd/token+ft": "fake_quant x7 | -> ctx 2x16x128:var",
    "qopt_est/autograd_fused/none": "fake_quant x7 | -> ctx 2x16x128:var",
    "qopt_est/autograd_fused/token+ft": "fake_quant x7 | -> ctx 2x16x128:var",
    "qopt_est/nomask/none+ft": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/nomask/uncond": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/nomask/uncond+ft": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/nomask/head": "fake_quant x3 | gate_fwd(units=0 pool=True scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/nomask/head+ft": "fake_quant x3 | gate_fwd(units=0 pool=True scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/nomask/token": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/nomask/token_mlp": "fake_quant x3 | gate_fwd(units=16 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/nomask/token_mlp+ft": "fake_quant x3 | gate_fwd(units=16 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/nomask/allfeat": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_est/nomask/allfeat+ft": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_fix/nomask/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/nomask/token+ft": Twice("gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
                                      "gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1"),
    "qopt_fix/causal/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 causal clamp min=f32 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/causal/token+ft": Twice("gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 causal clamp min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
                                      "gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 causal clamp min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1"),
    "qopt_fix/leftpad/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad causal pad_bool clamp min=f32 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/leftpad/token+ft": Twice("gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad causal pad_bool clamp min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
                                       "gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 pad causal pad_bool clamp min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1"),
    "qopt_fix/full/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 full clamp min=f32 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/full/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 full clamp min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/wrongsize/none": "fake_quant x3 | ValueError: Attention mask should be of size (2, 1, 16, 16), but is torch.Size([2, 1, 1, 16])",
    "qopt_fix/wrongsize/token+ft": "fake_quant x3 | ValueError: Attention mask should be of size (2, 1, 16, 16), but is torch.Size([2, 1, 1, 16])",
    "qopt_fix/cross/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/cross/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/cross_cached/none": "fake_quant | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/cross_cached/token+ft": "fake_quant | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/step/none": "fake_quant x3 | attn_fwd(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad pad_bool clamp min=f32 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x1x128:1",
    "qopt_fix/step/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad pad_bool clamp min=f32 scale=1 div=0 gate=2x2x1x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x1x128:1",
    "qopt_fix/step_split/none": "fake_quant x3 | attn_decode(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad clamp min=f16 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x1x128:1",
    "qopt_fix/step_split/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_decode(q2x2x1x64 k2x2x17x64 v2x2x17x64 pad clamp min=f16 scale=1 div=0 gate=2x2x1x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x1x128:1",
    "qopt_fix/head_mask/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_fix/head_mask/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_fix/output_attentions/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_fix/output_attentions/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_fix/dropout/none": "fake_quant x4 | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_fix/dropout/token+ft": "fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | fake_quant | softmax_rows | fake_quant x3 | -> ctx 2x16x128:var",
    "qopt_fix/autograd/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/autograd/token+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:var fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/autograd_fused/none": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/autograd_fused/token+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:var fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/nomask/none+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/nomask/uncond": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=1x2x1x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/nomask/uncond+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=1x2x1x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/nomask/head": Twice("gate_fwd(units=0 pool=True scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x1x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
                                  "gate_fwd(units=0 pool=True scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=True scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x1x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1"),
    "qopt_fix/nomask/head+ft": Twice("gate_fwd(units=0 pool=True scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x1x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
                                     "gate_fwd(units=0 pool=True scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=True scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x1x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1"),
    "qopt_fix/nomask/token": Twice("gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
                                   "gate_fwd(units=0 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=0 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1"),
    "qopt_fix/nomask/token_mlp": Twice("gate_fwd(units=16 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
                                       "gate_fwd(units=16 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=16 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1"),
    "qopt_fix/nomask/token_mlp+ft": Twice("gate_fwd(units=16 pool=False scaling=1) | fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
                                          "gate_fwd(units=16 pool=False scaling=1) | fake_quant x3 | gate_fwd(units=16 pool=False scaling=1) | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:0.5 fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1"),
    "qopt_fix/nomask/allfeat": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:var fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
    "qopt_fix/nomask/allfeat+ft": "fake_quant x3 | attn_fwd(q2x2x16x64 k2x2x16x64 v2x2x16x64 min=f32 scale=1 div=0 gate=2x2x16x1:var fq[ctx_before_gate=True]) | fake_quant | -> ctx 2x16x128:1",
}
