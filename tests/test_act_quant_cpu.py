"""Host side of the fused feed-forward (oeh_act_quant, QuantLinear.forward_index, quantization.feed_forward) without a GPU: the ABI, the
refusals of the entry point, the launch-form names, the states in which the fused route must not be taken, and - in numpy - the identity
that route (a) rests on."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import _act_quant_ref as R

torch = pytest.importorskip("torch")
nn = torch.nn

EINVAL, ENOTSUP, EALIGN = -22, -95, -14


@pytest.fixture()
def Qon():
    from outeffhop_amd import quantization as Q

    prev = Q.set_fused_ffn(True)
    yield Q
    Q.set_fused_ffn(prev)


def _qp(Q):
    qp = Q.val_qparams(Q.get_quant_config())
    qp["quant_dict"] = {}
    return qp


def _fc1(Q, act, E=32, F=64):
    m = Q.quantize_model(nn.Sequential(nn.Linear(E, F), act), **_qp(Q))[0]
    m.quantized()
    m.weight_quantizer.set_quant_range(m.weight.min().detach(), m.weight.max().detach())
    m.activation_quantizer.set_quant_range(0.0, 4.0)
    m.fix_ranges()
    return m.eval()


def test_symbols_constants_and_abi():
    from outeffhop_amd import _lib, ops, quantization as Q

    lib = _lib.load()
    assert hasattr(lib, "oeh_act_quant") and hasattr(lib, "oeh_act_quant_variant") and lib.oeh_abi_version() == 6
    assert {"oeh_act_quant", "oeh_act_quant_variant"} <= set(_lib.EXPORTS)
    assert (_lib.OEH_ACT_NONE, _lib.OEH_ACT_RELU, _lib.OEH_ACT_GELU) == (0, 1, 2)
    assert callable(ops.act_quant) and callable(ops.act_quant_variant)
    assert Q.FUSED_FFN is False  # the default of this switch
    assert Q.set_fused_ffn(True) is False and Q.FUSED_FFN is True and Q.set_fused_ffn(False) is True and Q.FUSED_FFN is False


def test_argument_validation_without_gpu():
    from outeffhop_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(4096)

    def call(x=one, out=one, y=one, rows=4, cols=64, xs=64, ys=64, dtype=2, act=1, scale=0.1, zp=0.0, bias=None):
        return lib.oeh_act_quant(x, out, y, rows, cols, xs, ys, dtype, act, scale, zp, 1.0, bias, None)

    assert call(x=None) == EINVAL and call(out=None, y=None) == EINVAL
    assert call(rows=-1) == EINVAL and call(cols=0) == EINVAL and call(dtype=3) == EINVAL and call(dtype=7) == EINVAL
    assert call(act=3) == EINVAL and call(act=-1) == EINVAL
    assert call(scale=0.0) == EINVAL and call(zp=256.0) == EINVAL and call(zp=-1.0) == EINVAL and call(zp=0.5) == EINVAL
    assert call(xs=-64) == EINVAL and call(ys=32) == EINVAL  # rows of y would overlap
    assert call(cols=72, xs=72, ys=72) == ENOTSUP and call(cols=8, xs=8, ys=8) == ENOTSUP
    assert call(x=C.c_void_p(4100)) == EALIGN and call(out=C.c_void_p(4104)) == EALIGN and call(y=C.c_void_p(4098)) == EALIGN
    assert call(bias=C.c_void_p(4100)) == EALIGN
    assert call(xs=66) == EALIGN and call(ys=68, dtype=0) == EALIGN  # 264 / 136 bytes between rows
    assert call(rows=0) == 0 and call(rows=0, out=None) == 0 and call(rows=0, y=None, ys=0) == 0  # nothing to do: no launch, no device needed
    # the order: a bad argument before the shape, the shape before the alignment
    assert call(cols=72, act=9) == EINVAL and call(cols=72, xs=72, ys=72, x=C.c_void_p(4100)) == ENOTSUP


def test_launch_form_names_host_only():
    from outeffhop_amd import ops

    assert ops.act_quant_variant(8192, 3072, act="relu", want_index=True) == "actq/relu/f32/y+i8/loop"
    assert ops.act_quant_variant(4096, 3072, torch.float16, act="gelu", want_values=False, want_index=True) == "actq/gelu/f16/i8/loop"
    assert ops.act_quant_variant(4099, 64, torch.bfloat16) == "actq/none/bf16/y/once"
    assert ops.act_quant_variant(2048, 4096, act="relu") == "actq/relu/f32/y/once"   # 2048 * 256 chunks: every thread of 2048 workgroups takes one
    assert ops.act_quant_variant(2052, 4096, act="relu") == "actq/relu/f32/y/loop"
    assert ops.act_quant_variant(64, 768, row_stride=800) == "actq/none/f32/y/once"
    assert ops.act_quant_variant(64, 72) is None and ops.act_quant_variant(64, 768, row_stride=770) is None
    assert ops.act_quant_variant(64, 768, want_values=False, want_index=False) is None
    with pytest.raises(ValueError):
        ops.act_quant_variant(64, 768, act="tanh")


def test_no_cpu_fallback():
    from outeffhop_amd import _lib, ops

    with pytest.raises(_lib.OehError):
        ops.act_quant(torch.zeros(4, 64), ops.FakeQuantSpec(0.1, 0.0), act="relu")


def test_forward_index_is_refused_outside_frozen_inference(Qon):
    Q = Qon
    x = torch.randn(16, 32)
    m = _fc1(Q, nn.ReLU())
    assert m.fused_act() == "relu" and _fc1(Q, nn.GELU()).fused_act() == "gelu"  # the host-side conditions hold ...
    assert m.forward_index(x) is None  # ... and a CPU tensor is refused: there is no CPU path
    # training
    m.train()
    assert m.fused_act() is None and m.forward_index(x) is None
    m.eval()
    assert m.fused_act() == "relu"
    # a forward hook on the module, or on a member
    h = m.register_forward_hook(lambda mod, i, o: None)
    assert m.fused_act() is None and m.forward_index(x) is None
    h.remove()
    h = m.activation_quantizer.register_forward_hook(lambda mod, i, o: None)
    assert m.fused_act() is None
    h.remove()
    assert m.fused_act() == "relu"
    # ranges that still move
    m.estimate_ranges()
    assert m.fused_act() is None and m.forward_index(x) is None
    m.fix_ranges()
    assert m.fused_act() == "relu"
    # activations not quantised
    m.full_precision_acts()
    assert m.fused_act() is None
    m.quantized_acts()
    # the tanh form of GELU is not in the kernel
    t = _fc1(Q, nn.GELU(approximate="tanh"))
    assert t.fused_act() is None and t.forward_index(x) is None
    # the switch
    Q.set_fused_ffn(False)
    assert m.fused_act() is None and m.forward_index(x) is None
    Q.set_fused_ffn(True)
    assert m.fused_act() == "relu"
    # out_features % 16
    assert _fc1(Q, nn.ReLU(), F=72).fused_act() is None


def test_unfused_cpu_forward_is_what_it_was(Qon):
    """With the switch on, a CPU tensor still takes the torch ops (the fused pass asks for a GPU tensor)."""
    Q = Qon
    m = _fc1(Q, nn.ReLU())
    x = torch.randn(16, 32)
    w, b = m.get_params()
    with torch.no_grad():
        lin = nn.functional.linear(x, w, b)
    from outeffhop_amd import _lib

    with pytest.raises(_lib.OehError):  # the quantiser itself is a HIP kernel: no CPU path
        m(x)
    m.full_precision_acts()
    with torch.no_grad():
        assert torch.equal(m(x), torch.relu(lin))


def test_quantize_intermediate_and_feed_forward_classes():
    from outeffhop_amd import quantization as Q

    F = nn.functional
    for act in (F.gelu, nn.GELU(), nn.ReLU()):
        seq = Q.quantize_intermediate(types.SimpleNamespace(dense=nn.Linear(16, 32), intermediate_act_fn=act), **_qp(Q))
        assert type(seq) is nn.Sequential and len(seq) == 1 and type(seq[0]) is Q.QuantLinear
        assert isinstance(seq[0].activation_function, nn.ReLU if isinstance(act, nn.ReLU) else nn.GELU)
    for act in (torch.tanh, F.relu, F.silu):
        with pytest.raises(NotImplementedError):
            Q.quantize_intermediate(types.SimpleNamespace(dense=nn.Linear(16, 32), intermediate_act_fn=act), **_qp(Q))
    org = types.SimpleNamespace(intermediate=types.SimpleNamespace(dense=nn.Linear(16, 32), intermediate_act_fn=F.gelu),
                                output=types.SimpleNamespace(dense=nn.Linear(32, 16), LayerNorm=nn.LayerNorm(16, eps=1e-12), dropout=nn.Dropout(0.1)))
    ff = Q.QuantizedBertFeedForward(org, **_qp(Q))
    assert type(ff.intermediate[0]) is Q.QuantLinear and type(ff.output) is Q.QuantizedBertOutput and isinstance(ff, Q.QuantizedModel)
    keys = set(ff.state_dict())
    assert {"intermediate.0.weight", "intermediate.0.bias", "output.dense.weight", "output.LayerNorm.weight"} <= keys
    # full precision on the CPU: the plain chain
    ff.eval()
    x = torch.randn(2, 3, 16)
    with torch.no_grad():
        want = org.output.LayerNorm(org.output.dense(F.gelu(org.intermediate.dense(x))) + x)
        assert torch.equal(ff(x), want)


@pytest.mark.parametrize("scale", [0.03125, 0.1, 0.0437])
def test_relu_is_the_clamp_at_index_zero_only_for_zero_point_zero(scale):
    """fq(relu(v)) == fq(v) index for index at zero point 0 - over every index's value, both of its rounding boundaries and their fp32
    neighbours, negative values, -0, +-inf and the fp32 extremes.  At zero point 3 it is false: the condition of route (a)."""
    s = np.float32(scale)
    k = np.arange(0, 256, dtype=np.float32)
    pts = [s * k, s * (k + np.float32(0.5)), s * (k - np.float32(0.5))]
    pts += [np.nextafter(p, np.float32(np.inf)) for p in pts[:3]] + [np.nextafter(p, np.float32(-np.inf)) for p in pts[:3]]
    v = np.concatenate(pts + [np.array([-0.0, 0.0, np.inf, -np.inf, 3.0e38, -3.0e38, 1e-45, -1e-45, 300.0 * s, -300.0 * s], dtype=np.float32)])
    v = np.concatenate([v, -v]).astype(np.float32)
    a = R.fq_index32(R.relu(v), s, 0.0)
    b = R.fq_index32(v, s, 0.0)
    assert np.array_equal(a, b) and set(np.unique(a)) == set(range(256))
    a3, b3 = R.fq_index32(R.relu(v), s, 3.0), R.fq_index32(v, s, 3.0)
    assert not np.array_equal(a3, b3) and (a3 >= 3).all() and b3.min() == 0.0
    assert (a3[v >= 0] == b3[v >= 0]).all()


def test_gelu_oracle_conditions_on_the_cpu():
    """The interval oracle of the GPU test on its own input law: few ambiguous elements, never wider than one step, and torch's own fp32
    GELU on the CPU inside the interval (a plausibility check of delta, not the device's)."""
    rng = np.random.default_rng(7)
    for dtype, tdt in (("f32", torch.float32), ("f16", torch.float16)):
        v = R.round_to(rng.standard_normal((48, 3072)) * 2.0, dtype)
        a = R.gelu64(v)
        delta, zf = R.percentile_grid(a)
        zp = float(min(max(np.rint(zf), 0.0), 255.0))
        lo, hi, _ = R.gelu_index_interval(v, delta, zp, dtype)
        share = float((lo != hi).mean())
        print(f"\n{dtype}: ambiguous {share:.1e}, widest {int((hi - lo).max())}, index 0: {float((hi == 0).mean()):.2f}")
        assert share <= 1e-3 and (hi - lo).max() <= 1
        t = nn.functional.gelu(torch.from_numpy(v.astype(np.float32))).to(tdt).float().numpy()
        idx = R.fq_index32(t, delta, zp)
        assert ((idx >= lo) & (idx <= hi)).all()
