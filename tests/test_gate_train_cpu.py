"""CPU-side checks of the fused gate training path (include/oeh.h: oeh_gate_apply_fwd / oeh_gate_apply_bwd; attention.FUSED_GATE_TRAIN):
the float64 restatement of tests/_gate_train_ref.py against torch's float64 autograd of the reference's per-head loop, the route predicate,
the entry points' refusals in their stated order without a GPU, and the launch plans `ops.gate_apply_variant` names."""
import ctypes as C

import numpy as np
import pytest

from tests import _gate_train_ref as G

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("units", (0, 1, 5, 16))
def test_float64_restatement_is_torchs_float64_autograd(units):
    B, T, H, d = 2, 7, 3, 32
    c = G.make_case(B, T, H, d, units, torch.float32, 11 + units, dead_unit=(1, 0) if units > 1 else None, zero_tokens=((1, 2),))
    assert G.kink_clear(c, H)
    args = (c["dout"], c["ctx"], c["hidden"], c["w1"], c["b1"], c["w2"], c["b2"], c["s"])
    t64 = G.torch_chain(*args, dtype=torch.float64)
    n = lambda t: None if t is None else t.double().numpy()  # noqa: E731
    out64, pi64 = G.forward64(*map(n, args[1:7]), c["s"])
    got = G.backward64(*map(n, args[:7]), c["s"])
    got.update(out=out64, pi=pi64)
    for k, v in got.items():
        if v is None:
            assert t64[k] is None
            continue
        want = t64[k].numpy()
        assert v.shape == want.shape, k
        assert np.abs(v - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (k, np.abs(v - want).max())


def _mod(gate="tok_mlp", heads=2, hidden=128, **kw):
    import outeffhop_amd as oa
    from tests.test_host_cpu import Cfg, gate_kwargs

    class C_(Cfg):
        hidden_size = hidden
        num_attention_heads = heads
        attention_probs_dropout_prob = 0.0

    return oa.BertSelfAttentionWithExtras(C_(), **{**gate_kwargs(gate), **kw})


def test_route_predicate_and_counters():
    from outeffhop_amd import attention as A

    x = torch.randn(2, 5, 128)
    assert A.FUSED_GATE_TRAIN is False and set(A.GATE_TRAIN_CALLS) == {"forward", "backward", "torch"}
    assert A.gate_train_scope(_mod("tok_mlp"), x, 2) == 16       # 64 -> 16 -> 1
    assert A.gate_train_scope(_mod("tok_mlp2"), x, 2) == 64      # 64 -> 64 -> 1
    assert A.gate_train_scope(_mod("tok_linear"), x, 2) == 0
    assert A.gate_train_scope(_mod("tok_mlp", heads=4), x, 4) == 8  # d = 32
    with torch.no_grad():
        assert A.gate_train_scope(_mod("tok_mlp"), x, 2) is None     # autograd is not recording
    frozen = _mod("tok_mlp").requires_grad_(False)
    assert A.gate_train_scope(frozen, x, 2) is None and A.gate_train_scope(frozen, x.clone().requires_grad_(), 2) == 16
    for refused in (_mod("uncond_head"), _mod("nogate"), _mod(attn_gate_type="conditional_per_head"),
                    _mod(attn_gate_type="conditional_per_token", attn_gate_linear_all_features=True)):
        assert A.gate_train_scope(refused, x, 2) is None
    assert A.gate_train_scope(_mod("tok_mlp", heads=1), x, 1) is None      # d = 128
    assert A.gate_train_scope(_mod("tok_mlp", heads=8), x, 8) is None      # d = 16
    wide = _mod("tok_mlp2")
    wide.alpha = torch.nn.ModuleList(torch.nn.Sequential(torch.nn.Linear(64, 65), torch.nn.ReLU(), torch.nn.Linear(65, 1)) for _ in range(2))
    assert A.gate_train_scope(wide, x, 2) is None                          # 65 hidden units
    assert A.gate_train_scope(_mod("tok_mlp").double(), x.double(), 2) is None
    assert A.gate_train_scope(_mod("tok_mlp"), torch.randn(2, 5, 256)[..., ::2], 2) is None  # last dimension not contiguous
    hooked = _mod("tok_mlp")
    hooked.alpha[0].register_forward_hook(lambda *a: None)
    assert A.gate_train_scope(hooked, x, 2) is None

    # tensors that are not on a GPU keep the torch loop whatever the switch says (the kernels are the only implementation)
    assert A.gate_train_scope(_mod("tok_mlp"), x, 2) == 16 and A.gate_train_units(_mod("tok_mlp"), x, 2) is None

    # the switch: off - the torch loop, counted; on - a deferred record for gated_merge
    m = _mod("tok_mlp")
    n0 = dict(A.GATE_TRAIN_CALLS)
    g = A.gate_autograd(m, x, 2)
    assert g.shape == (2, 2, 5, 1) and g.requires_grad
    assert {k: A.GATE_TRAIN_CALLS[k] - n0[k] for k in n0} == {"forward": 0, "backward": 0, "torch": 1}
    prev = A.set_fused_gate_train(True)
    try:
        assert prev is False and A.FUSED_GATE_TRAIN is True
        n0 = dict(A.GATE_TRAIN_CALLS)
        with pytest.raises(Exception, match="GPU"):  # a CPU module with the switch on: module_gate keeps gate_autograd's route, which asks for a GPU
            A.module_gate(m, x, 2, in_kernel=False)
        assert A.GATE_TRAIN_CALLS["forward"] == n0["forward"]
        rec = A.DeferredGate(m, x, 2, 1.0, A.gate_train_scope(m, x, 2))  # (what module_gate returns for GPU tensors)
        assert rec.units == 16 and len(rec.params()) == 8
        assert rec.takes(torch.empty(2, 2, 5, 64)) and not rec.takes(torch.empty(2, 2, 5, 64, dtype=torch.float16)) and not rec.takes(torch.empty(2, 2, 6, 64))
        assert not rec.takes(torch.empty(2 * 2 * 5 * 64 + 1)[1:].view(2, 2, 5, 64))         # rows 4 bytes off a 16-byte boundary
        assert not rec.takes(torch.empty(2, 2, 5, 66)[..., :64])                             # a token stride of 264 bytes
        # a context the kernels do not take after all: the torch loop, now
        n0 = dict(A.GATE_TRAIN_CALLS)
        merged = A.gated_merge(torch.randn(2, 2, 5, 64).double(), rec)
        assert merged.shape == (2, 5, 128) and A.GATE_TRAIN_CALLS["torch"] == n0["torch"] + 1 and A.GATE_TRAIN_CALLS["forward"] == n0["forward"]
    finally:
        assert A.set_fused_gate_train(prev) is True
    assert A.FUSED_GATE_TRAIN is False


def _desc(B=2, T=8, H=3, d=64, units=16, dtype=0, scaling=1.0):
    from outeffhop_amd import _lib

    g = _lib.oeh_gate_train_desc()
    g.B, g.T, g.H, g.d, g.units, g.dtype, g.scaling = B, T, H, d, units, dtype, scaling
    E = H * d
    g.hidden_stride, g.out_stride, g.dhidden_stride = (T * E, E), (T * E, E), (T * E, E)
    g.ctx_stride, g.dctx_stride = (H * T * d, T * d, d), (H * T * d, T * d, d)
    return g


def test_argument_validation_without_gpu():
    """Every refusal code, in the stated order: OEH_EINVAL (-22) before OEH_ENOTSUP (-95) before OEH_EALIGN (-14); nothing is launched."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    one, off = C.c_void_p(64), C.c_void_p(68)
    fwd = lambda g, hidden=one, w1=one, b1=one, w2=one, b2=one, ctx=one, gate=one, out=one: lib.oeh_gate_apply_fwd(  # noqa: E731
        None if g is None else C.byref(g), hidden, w1, b1, w2, b2, ctx, gate, out, None)

    def bwd(g, **kw):
        a = dict(dout=one, ctx=one, hidden=one, gate=one, w1=one, b1=one, w2=one, b2=one, dctx=one, dhidden=one, dw1=one, db1=one, dw2=one, db2=one, work=one)
        a.update(kw)
        return lib.oeh_gate_apply_bwd(None if g is None else C.byref(g), *[a[k] for k in ("dout", "ctx", "hidden", "gate", "w1", "b1", "w2", "b2", "dctx", "dhidden",
                                                                                     "dw1", "db1", "dw2", "db2", "work")], None)

    # OEH_EINVAL
    assert fwd(None) == -22 and bwd(None) == -22
    for name in ("hidden", "w1", "b1", "ctx", "gate", "out"):
        assert fwd(_desc(), **{name: None}) == -22, name
    for name in ("dout", "ctx", "hidden", "gate", "w1", "b1", "dctx", "dw1", "db1", "work"):
        assert bwd(_desc(), **{name: None}) == -22, name
    assert fwd(_desc(), w2=None) == -22 and fwd(_desc(), b2=None) == -22           # units > 0 without the second layer
    assert bwd(_desc(), dw2=None) == -22 and bwd(_desc(), db2=None) == -22
    for bad in (dict(B=0), dict(T=0), dict(H=0), dict(d=0), dict(units=-1), dict(dtype=7), dict(scaling=float("inf")), dict(scaling=float("nan"))):
        assert fwd(_desc(**bad)) == -22 and bwd(_desc(**bad)) == -22, bad
    g = _desc()
    g.reserved = 1
    assert fwd(g) == -22
    g = _desc()
    g.ctx_stride = (-1, 8, 64)
    assert fwd(g) == -22
    # ... before OEH_ENOTSUP and OEH_EALIGN
    assert fwd(_desc(d=48), hidden=None) == -22 and fwd(_desc(d=48, scaling=float("nan")), hidden=off) == -22
    assert bwd(_desc(units=65), work=None) == -22
    # OEH_ENOTSUP
    for bad in (dict(d=48), dict(d=128), dict(d=16), dict(units=65), dict(H=65536), dict(B=1 << 15, T=1 << 15, H=2)):
        assert fwd(_desc(**bad)) == -95 and bwd(_desc(**bad)) == -95, bad
    # ... before OEH_EALIGN
    assert fwd(_desc(d=48), hidden=off) == -95 and bwd(_desc(units=65), work=C.c_void_p(4)) == -95
    # OEH_EALIGN: a row of every strided tensor (pointer or stride) off 16 bytes, work off 8
    for name in ("hidden", "ctx", "out"):
        assert fwd(_desc(), **{name: off}) == -14, name
    for name in ("hidden", "ctx", "dout", "dctx", "dhidden"):
        assert bwd(_desc(), **{name: off}) == -14, name
    assert bwd(_desc(), work=C.c_void_p(68)) == -14 and bwd(_desc(), work=C.c_void_p(72), dout=off) == -14
    for field in ("hidden_stride", "ctx_stride", "out_stride", "dctx_stride", "dhidden_stride"):
        g = _desc()
        st = list(getattr(g, field))
        st[0] += 4  # 8 bytes of fp16
        setattr(g, field, tuple(st))
        assert bwd(g) == -14, field
        if field in ("hidden_stride", "ctx_stride", "out_stride"):
            assert fwd(g) == -14, field
    # the work size: bytes, or the code
    wb = lib.oeh_gate_apply_bwd_work_bytes
    assert wb(0, 8, 3, 64, 16) == -22 and wb(2, 8, 3, 64, -1) == -22 and wb(2, 8, 3, 48, 16) == -95 and wb(2, 8, 3, 64, 65) == -95
    assert wb(1 << 15, 1 << 15, 2, 64, 0) == -95
    assert wb(2, 8, 3, 64, 16) == 1 * 3 * (16 * 64 + 2 * 16 + 1) * 8 and wb(2, 8, 3, 32, 0) == 1 * 3 * 33 * 8


def test_variant_strings_for_the_plan_cases():
    from outeffhop_amd import _lib, ops

    v = ops.gate_apply_variant
    assert v(32, 128, 12, 64, 16) == "gate_train/fwd/D64/M16/f16"
    assert v(2, 5, 3, 32, 0, torch.float32) == "gate_train/fwd/D32/M0/f32"
    assert v(1, 1, 1, 32, 0, torch.bfloat16, backward=True) == "gate_train/bwd/D32/M0/bf16/G1x1"
    assert v(1, 64, 3, 64, 5, backward=True).endswith("/G1x1") and v(1, 65, 3, 64, 5, backward=True).endswith("/G2x1")
    # the bound: OEH_GATE_TRAIN_MAX_GROUPS workgroups over all heads; beyond it a workgroup walks several tiles
    assert _lib.GATE_TRAIN_MAX_GROUPS == 1024
    assert v(32, 128, 12, 64, 16, backward=True) == "gate_train/bwd/D64/M16/f16/G64x1"      # BERT-base B32 S128: 64 tiles <= 1024 // 12 = 85
    assert v(16, 512, 12, 64, 16, backward=True) == "gate_train/bwd/D64/M16/f16/G64x2"      # OPT B16 S512: 128 tiles
    assert v(1, 85 * 64, 12, 64, 0, backward=True).endswith("/G85x1") and v(1, 85 * 64 + 1, 12, 64, 0, backward=True).endswith("/G43x2")
    assert v(1, 1024 * 64, 1, 32, 0, backward=True).endswith("/G1024x1") and v(1, 1024 * 64 + 1, 1, 32, 0, backward=True).endswith("/G513x2")
    assert v(1, 8, 2048, 32, 0, backward=True).endswith("/G1x1")                             # more heads than the bound: one workgroup per head
    assert v(1, 1, 65535, 32, 0, backward=True).endswith("/G1x1") and v(1, 1, 65536, 32, 0, backward=True) is None  # the head is a grid dimension
    assert v(2, 5, 3, 48, 5) is None and v(2, 5, 3, 64, 65) is None and v(0, 5, 3, 64, 5) is None and v(1 << 15, 1 << 15, 2, 64, 0, backward=True) is None
