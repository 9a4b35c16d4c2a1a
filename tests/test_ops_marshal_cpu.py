"""What every attention entry point of outeffhop_amd/ops.py hands to the C ABI, checked without a GPU: the real entry points run on
CPU tensors, everything that touches a device is replaced, and a stand-in for the library records each call with a copy of the
descriptors behind its `byref` arguments.  Every field of the recorded `oeh_attn_desc` / `oeh_fq_desc` is compared with values written
out here from include/oeh.h - which field each entry point sets, and where the entry points differ on purpose (the default `mask_min`,
`o_dtype`, how the key-padding vector is viewed, `key_pad_boolean`, which masks / gate forms / quantiser descriptors a path takes)."""
import contextlib
import ctypes as C
import types

import pytest
import torch

from outeffhop_amd import _lib, ops
from outeffhop_amd._lib import oeh_attn_desc, oeh_attn_opts, oeh_dropout, oeh_fq_desc

F16, BF16, F32, I8 = 0, 1, 2, 3  # include/oeh.h: OEH_F16, OEH_BF16, OEH_F32, OEH_I8
F16_MIN, BF16_MIN, F32_MIN = -65504.0, -3.3895313892515355e38, -3.4028234663852886e38  # finfo(...).min
B, H, Sq, Sk, D = 2, 3, 5, 7, 64
STREAM = 0x5EED
WORK_BYTES = 4096
f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32
SM_CLIP = ops.SoftmaxSpec(1, True, -0.025, 1.1)


def c32(x):
    return C.c_float(x).value


def _snapshot(a):
    if hasattr(a, "_obj"):  # byref(structure): the structure as it is at the call
        return type(a._obj).from_buffer_copy(a._obj)
    if isinstance(a, C.c_void_p):
        return a.value or 0
    if isinstance(a, C.Array):
        return list(a)
    return a


class _Lib:
    """Stand-in for liboeh_hip.so: every symbol records (name, arguments) and returns 0, a work size or a variant name."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, [_snapshot(a) for a in args]))
            if name.endswith("work_bytes"):
                return WORK_BYTES
            if "variant" in name:
                return b"stub/" + name.encode()
            return 0

        return fn


@pytest.fixture
def lib(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts, allow_grad=False: torch.device("cpu"))
    monkeypatch.setattr(ops, "_on_device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(ops, "_stream", lambda: C.c_void_p(STREAM))
    monkeypatch.setattr(ops, "FAST_CALLS", False)
    monkeypatch.setattr(_lib, "load", lambda: fake)
    # the per-stream scratch: not capturing, one stream, fresh tables (its buffers are then CPU tensors)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=STREAM))
    for name in ("_decode_work", "_calib_work", "_stats_work", "_qmse_work"):
        monkeypatch.setattr(ops, name, {})
    return fake


def fields(s):
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            v = fields(v)
        elif isinstance(v, C.Array):
            v = list(v)
        elif v is None:
            v = 0
        out[name] = v
    return out


def check(s, **want):
    """Every field of the structure: the value given here, a predicate given here, or zero / null."""
    got = fields(s)
    exp = fields(type(s)())
    assert set(want) <= set(exp), set(want) - set(exp)
    exp.update(want)
    for name, e in exp.items():
        if callable(e):
            assert e(got[name]), (name, got[name])
        else:
            assert got[name] == e, (name, got[name], e)


def own_copy(*of):
    """A pointer to a view the call made itself: neither null nor one of the caller's tensors."""
    return lambda p: p not in (0,) + tuple(t.data_ptr() for t in of)


def fq_of(spec):
    return dict(enable=1, scale=c32(spec.scale), zero_point=c32(spec.zero_point), qmax=c32(spec.qmax), dump_idx=0)


def bhsd(S, dt, d=D):  # contiguous: strides (H*S*d, S*d, d)
    return torch.zeros(B, H, S, d, dtype=dt)


def bshd(S, dt, d=D):  # a projection's output viewed per head: strides (S*H*d, d, H*d)
    return torch.zeros(B, S, H, d, dtype=dt).permute(0, 2, 1, 3)


ST_BHSD = lambda S, d=D: [H * S * d, S * d, d]  # noqa: E731
ST_BSHD = lambda S, d=D: [S * H * d, d, H * d]  # noqa: E731
SCORES, PROBS, CTX = ops.FakeQuantSpec(0.25, 3.0), ops.FakeQuantSpec(1 / 255, 0.0), ops.FakeQuantSpec(0.5, 128.0, 15.0)


# ---- attn_fwd (the path below the repeated-call table)
def test_attn_fwd_masks_and_gate_values(lib):
    q = torch.zeros(B, H, D, Sq, dtype=f16).transpose(2, 3)  # head-dim stride Sq: the call reads a contiguous copy
    k, v = bshd(Sk, f16), bhsd(Sk, f16)
    kpm = torch.zeros(B, 1, 1, Sk, dtype=torch.int64)
    fm = torch.zeros(B, 1, Sk, Sq).transpose(2, 3)  # key stride Sq: copied
    gate = torch.ones(H, 1, 1)
    out = ops.attn_fwd(q, k, v, softmax=SM_CLIP, scale=0.5, scale_div=8.0, key_pad_mask=kpm, full_mask=fm, key_pad_boolean=True, causal=True,
                       clamp_min=True, gate=gate)
    assert out.shape == (B, H, Sq, D) and out.dtype == f16 and list(out.stride()[:3]) == ST_BSHD(Sq)
    (name, a), (vname, va) = lib.calls  # the launch, then the host-only probe behind the any-shape warning
    assert (name, vname) == ("oeh_attn_fwd", "oeh_attn_variant")
    check(a[0], B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=F16, o_dtype=F16, q_stride=ST_BHSD(Sq), k_stride=ST_BSHD(Sk), v_stride=ST_BHSD(Sk), o_stride=ST_BSHD(Sq),
          scale=0.5, scale_div=8.0, softmax_base=1, clip=1, gamma=c32(-0.025), eta=c32(1.1),
          key_pad_mask=own_copy(kpm), key_pad_dtype=F32, key_pad_stride=Sk, key_pad_boolean=1,
          full_mask=own_copy(fm), full_mask_dtype=F32, full_mask_stride=[Sq * Sk, Sk],
          causal=1, clamp_min=1, mask_min=F16_MIN, gate=gate.data_ptr(), gate_stride=[0, 1, 0])
    assert own_copy(q)(a[1]) and a[2:] == [k.data_ptr(), v.data_ptr(), out.data_ptr(), None, STREAM]
    assert bytes(va[0]) == bytes(a[0]) and va[1] is None


def test_attn_fwd_views_read_in_place_fq_and_out(lib):
    q, k, v = bshd(Sq, bf16), bshd(Sk, bf16), bshd(Sk, bf16)
    kpm = torch.zeros(B, Sk, dtype=f16)
    fm = torch.zeros(B, 1, Sq, Sk + 1, dtype=f16)[..., :Sk]
    out = torch.zeros(B, H, Sq, D, dtype=f32)
    fq = ops.AttnFakeQuant(scores=SCORES, ctx=CTX, ctx_before_gate=False, ctx_emit_index=True)
    res = ops.attn_fwd(q, k, v, softmax=ops.SoftmaxSpec(0), key_pad_mask=kpm, full_mask=fm, mask_min=-1e4, fq=fq, out=out, out_dtype=f32)
    assert res is out
    name, a = lib.calls[0]
    assert name == "oeh_attn_fwd"
    check(a[0], B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=BF16, o_dtype=F32, q_stride=ST_BSHD(Sq), k_stride=ST_BSHD(Sk), v_stride=ST_BSHD(Sk), o_stride=ST_BHSD(Sq),
          scale=1.0, softmax_base=0, eta=1.0, key_pad_mask=kpm.data_ptr(), key_pad_dtype=F16, key_pad_stride=Sk,
          full_mask=fm.data_ptr(), full_mask_dtype=F16, full_mask_stride=[Sq * (Sk + 1), Sk + 1], mask_min=-1e4)
    check(a[5], scores=fq_of(SCORES), ctx=fq_of(CTX), ctx_emit_index=1)
    assert a[1:5] + a[6:] == [q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), STREAM]
    assert bytes(lib.calls[1][1][1]) == bytes(a[5])  # the probe sees the quantisers too


@pytest.mark.parametrize("dt,code,fmin", [(f16, F16, F16_MIN), (bf16, BF16, BF16_MIN), (f32, F32, F32_MIN)])
def test_attn_fwd_plain_default_mask_min(lib, dt, code, fmin):
    q, k, v = bhsd(Sq, dt), bhsd(Sk, dt), bhsd(Sk, dt)
    out = ops.attn_fwd(q, k, v, fq=ops.AttnFakeQuant())  # no quantiser enabled: no oeh_fq_desc
    name, a = lib.calls[0]
    check(a[0], B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=code, o_dtype=code, q_stride=ST_BHSD(Sq), k_stride=ST_BHSD(Sk), v_stride=ST_BHSD(Sk), o_stride=ST_BSHD(Sq),
          scale=1.0, softmax_base=1, eta=1.0, mask_min=c32(fmin))
    assert a[1:] == [q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), None, STREAM]


def test_attn_fwd_gate_predictor(lib):
    m = 4
    q, k, v = bshd(Sq, f16), bshd(Sk, f16), bshd(Sk, f16)
    hid = torch.zeros(B, Sq, H * D, dtype=f16)
    w1, b1, w2, b2 = torch.zeros(H, m, D), torch.zeros(H, m), torch.zeros(H, m), torch.zeros(H)
    gout = torch.zeros(B, H, Sq)
    ops.attn_fwd(q, k, v, scale_div=8.0, gate_mlp=ops.GatePredictor(hid, w1, b1, w2, b2, scaling=0.5, out=gout))
    check(lib.calls[0][1][0], B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=F16, o_dtype=F16, q_stride=ST_BSHD(Sq), k_stride=ST_BSHD(Sk), v_stride=ST_BSHD(Sk),
          o_stride=ST_BSHD(Sq), scale=1.0, scale_div=8.0, softmax_base=1, eta=1.0, mask_min=F16_MIN,
          gate_hidden=hid.data_ptr(), gate_hidden_stride=[Sq * H * D, H * D], gate_w1=w1.data_ptr(), gate_b1=b1.data_ptr(), gate_w2=w2.data_ptr(),
          gate_b2=b2.data_ptr(), gate_units=m, gate_scaling=0.5, gate_out=gout.data_ptr())
    lib.calls.clear()
    ops.attn_fwd(q, k, v, gate_mlp=ops.GatePredictor(hid, w1[:, 0].contiguous(), b1[:, 0].contiguous()))  # Linear(D, 1): no second layer
    got = fields(lib.calls[0][1][0])
    assert (got["gate_units"], got["gate_w2"], got["gate_b2"], got["gate_out"], got["gate_scaling"]) == (0, 0, 0, 0, 1.0)
    with pytest.raises(ValueError, match="pass either `gate`"):
        ops.attn_fwd(q, k, v, gate=torch.ones(H, 1, 1), gate_mlp=ops.GatePredictor(hid, w1, b1, w2, b2))


def test_attn_fwd_prepared_box_and_pv_pairs(lib):
    q, k, v = bhsd(Sq, f32), bhsd(Sk, f32), bhsd(Sk, f32)
    kpm = torch.zeros(B, 1, 1, Sk, dtype=torch.int64)
    box = []
    out = ops.attn_fwd(q, k, v, key_pad_mask=kpm, fq=ops.AttnFakeQuant(probs=PROBS), pv_pairs=True, _prepared=box)
    assert [n for n, _ in lib.calls] == ["oeh_attn_variant"]  # nothing launched
    fn, args, (d, fqd, keep, q_, k_, v_, out_) = box
    assert (q_, k_, v_, out_) == (q, k, v, out) and isinstance(d, oeh_attn_desc) and isinstance(fqd, oeh_fq_desc)
    assert d.key_pad_mask in [t.data_ptr() for t in keep if isinstance(t, torch.Tensor)]  # the box keeps the view alive
    check(fqd, probs=fq_of(PROBS), ctx_quant_before_gate=1)
    assert args[0]._obj is d and args[5]._obj is fqd and [x.value for x in args[1:5]] == [q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()]
    assert fn(*args, C.c_void_p(STREAM)) == 0
    name, a = lib.calls[-1]
    assert name == "oeh_attn_fwd_ex" and isinstance(a[1], oeh_attn_opts) and a[1].pv_pairs == 1
    assert bytes(a[0]) == bytes(d) and a[2:6] == [q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()] and a[7] == STREAM


@pytest.mark.parametrize("mask_min,want", [(None, F16_MIN), (-100.0, -100.0)])
def test_attn_fwd_pads_head_dim(lib, mask_min, want):
    q, k, v = bhsd(Sq, f16, 80), bhsd(Sk, f16, 80), bhsd(Sk, f16, 80)
    out = ops.attn_fwd(q, k, v, causal=True, mask_min=mask_min)
    assert out.shape == (B, H, Sq, 80)
    check(lib.calls[0][1][0], B=B, H=H, Sq=Sq, Sk=Sk, D=128, dtype=F16, o_dtype=F16, q_stride=ST_BHSD(Sq, 128), k_stride=ST_BHSD(Sk, 128),
          v_stride=ST_BHSD(Sk, 128), o_stride=ST_BSHD(Sq, 128), scale=1.0, softmax_base=1, eta=1.0, causal=1, mask_min=want)


def test_attn_fwd_raises_in_order(lib):
    q, k, v = bhsd(Sq, f16), bhsd(Sk, f16), bhsd(Sk, f16)
    with pytest.raises(ValueError, match=r"q, k, v must be 4-D \(B,H,S,D\) views"):
        ops.attn_fwd(q[0], k.float(), v, out_dtype=torch.int8)
    with pytest.raises(ValueError, match=r"shape mismatch: q \(2, 3, 5, 64\) k \(2, 3, 5, 64\) v \(2, 3, 7, 64\)"):
        ops.attn_fwd(q, q.float(), v, out_dtype=torch.int8)
    with pytest.raises(ValueError, match="q/k/v dtypes must match and be fp16/bf16/fp32, got torch.float16, torch.float32, torch.float16"):
        ops.attn_fwd(q, k.float(), v, out_dtype=torch.int8)
    with pytest.raises(ValueError, match="q/k/v dtypes must match and be fp16/bf16/fp32, got torch.int8"):
        ops.attn_fwd(q.to(torch.int8), k.to(torch.int8), v.to(torch.int8))
    with pytest.raises(ValueError, match="out_dtype must be the input dtype, or float32 for fp16 / bf16 inputs"):
        ops.attn_fwd(q, k, v, out_dtype=bf16, out=torch.zeros(1))
    with pytest.raises(ValueError, match=r"out must be a \(B,H,Sq,D\) view with unit head-dim stride and the input dtype"):
        ops.attn_fwd(q, k, v, out=torch.zeros(B, H, Sq, D))
    with pytest.raises(ValueError, match=r"Attention mask should be of size \(2, 1, 5, 7\), but is \(2, 1, 7, 7\)"):
        ops.attn_fwd(q, k, v, full_mask=torch.zeros(B, 1, Sk, Sk))
    assert lib.calls == []


# ---- attn_fwd_i8
GRIDS = (ops.QuantGrid(0.125, 7.0), ops.QuantGrid(0.25, 128.0), ops.QuantGrid(0.5, 0.0))
GRID_FIELDS = dict(q_grid=dict(scale=0.125, zero_point=7.0), k_grid=dict(scale=0.25, zero_point=128.0), v_grid=dict(scale=0.5, zero_point=0.0))


def _i8_qkv():
    return bshd(Sq, torch.int8), bshd(Sk, torch.int8), torch.zeros(B, H, D, Sk, dtype=torch.int8)


def test_attn_fwd_i8_broadcast_key_padding(lib):
    q, k, vt = _i8_qkv()
    kpm = torch.zeros(1, Sk)  # one row for every batch: read in place with a zero batch stride
    gate = torch.ones(H, 1, 1)
    fq = ops.AttnFakeQuant(scores=SCORES, probs=PROBS, ctx=CTX)
    out = ops.attn_fwd_i8(q, k, vt, GRIDS, fq=fq, softmax=SM_CLIP, scale=0.5, scale_div=8.0, causal=True, clamp_min=True, gate=gate, key_pad_mask=kpm)
    assert out.dtype == f16 and list(out.stride()[:3]) == ST_BSHD(Sq)
    (name, a), = lib.calls
    assert name == "oeh_attn_fwd"
    check(a[0], B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=I8, o_dtype=F16, q_stride=ST_BSHD(Sq), k_stride=ST_BSHD(Sk), v_stride=[H * D * Sk, D * Sk, Sk],
          o_stride=ST_BSHD(Sq), scale=0.5, scale_div=8.0, softmax_base=1, clip=1, gamma=c32(-0.025), eta=c32(1.1), causal=1, clamp_min=1, mask_min=c32(F32_MIN),
          key_pad_mask=kpm.data_ptr(), key_pad_dtype=F32, key_pad_stride=0, key_pad_boolean=1, gate=gate.data_ptr(), gate_stride=[0, 1, 0], **GRID_FIELDS)
    check(a[5], scores=fq_of(SCORES), probs=fq_of(PROBS), ctx=fq_of(CTX), ctx_quant_before_gate=1)
    assert a[1:5] + a[6:] == [q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), STREAM]


def test_attn_fwd_i8_index_output_and_prepared_box(lib):
    q, k, vt = _i8_qkv()
    kpm = torch.zeros(B, 1, 1, Sk, dtype=torch.int64)  # made float, then (B,Sk)
    box = []
    out = ops.attn_fwd_i8(q, k, vt, GRIDS, fq=ops.AttnFakeQuant(), out_dtype=torch.int8, mask_min=-1e4, key_pad_mask=kpm, _prepared=box)
    assert lib.calls == [] and out.dtype == torch.int8
    fn, args, (d, fqd, keep, q_, k_, v_, out_) = box
    assert (q_, k_, v_, out_) == (q, k, vt, out) and args[0]._obj is d and args[5]._obj is fqd
    assert [x.value for x in args[1:5]] == [q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr()]
    check(d, B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=I8, o_dtype=I8, q_stride=ST_BSHD(Sq), k_stride=ST_BSHD(Sk), v_stride=[H * D * Sk, D * Sk, Sk], o_stride=ST_BSHD(Sq),
          scale=1.0, softmax_base=1, eta=1.0, mask_min=-1e4, key_pad_mask=own_copy(kpm), key_pad_dtype=F32, key_pad_stride=Sk, key_pad_boolean=1, **GRID_FIELDS)
    assert d.key_pad_mask == keep[0].data_ptr() and keep[0].shape == (B, Sk)
    check(fqd, ctx_quant_before_gate=1)  # built even with nothing enabled
    ops.attn_fwd_i8(q, k, vt, GRIDS, fq=ops.AttnFakeQuant(), out_dtype=f32, key_pad_mask=torch.zeros(B, Sk, dtype=f16))
    got = fields(lib.calls[0][1][0])
    assert (got["o_dtype"], got["key_pad_dtype"], got["key_pad_stride"], got["key_pad_boolean"]) == (F32, F16, Sk, 1)


# ---- attn_decode
def test_attn_decode(lib, monkeypatch):
    monkeypatch.setattr(ops, "DECODE_CALLS", 0)
    q, k, v = bhsd(Sq, f16), bshd(Sk, f16), bshd(Sk, f16)
    kpm = torch.zeros(B, 1, 1, Sk, dtype=torch.int64)
    gate = torch.ones(H, 1, 1)
    out = ops.attn_decode(q, k, v, softmax=SM_CLIP, scale=0.5, key_pad_mask=kpm, causal=True, clamp_min=True, gate=gate, out_dtype=f32, splits=3)
    assert out.dtype == f32 and list(out.stride()[:3]) == ST_BSHD(Sq) and ops.DECODE_CALLS == 1
    (wname, wa), (name, a) = lib.calls
    assert (wname, name) == ("oeh_attn_decode_work_bytes", "oeh_attn_decode")
    check(a[0], B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=F16, o_dtype=F32, q_stride=ST_BHSD(Sq), k_stride=ST_BSHD(Sk), v_stride=ST_BSHD(Sk), o_stride=ST_BSHD(Sq),
          scale=0.5, softmax_base=1, clip=1, gamma=c32(-0.025), eta=c32(1.1), key_pad_mask=own_copy(kpm), key_pad_dtype=F32, key_pad_stride=Sk,
          causal=1, clamp_min=1, mask_min=F16_MIN, gate=gate.data_ptr(), gate_stride=[0, 1, 0])  # key_pad_boolean: not set on this path
    assert bytes(wa[0]) == bytes(a[0]) and wa[1] == 3
    (key, work), = ops._decode_work.items()
    assert key == (None, STREAM) and work.numel() * work.element_size() >= WORK_BYTES
    assert a[1:] == [3, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), work.data_ptr(), STREAM]


def test_attn_decode_fq(lib):
    q, k, v = bhsd(1, bf16), bshd(Sk, bf16), bshd(Sk, bf16)
    kpm = torch.zeros(B, Sk, dtype=f16)
    fq = ops.AttnFakeQuant(probs=PROBS, ctx_before_gate=False)
    out = ops.attn_decode(q, k, v, key_pad_mask=kpm, fq=fq)
    name, a = lib.calls[1]
    assert name == "oeh_attn_decode_fq"
    check(a[0], B=B, H=H, Sq=1, Sk=Sk, D=D, dtype=BF16, o_dtype=BF16, q_stride=ST_BHSD(1), k_stride=ST_BSHD(Sk), v_stride=ST_BSHD(Sk), o_stride=ST_BSHD(1),
          scale=1.0, softmax_base=1, eta=1.0, key_pad_mask=kpm.data_ptr(), key_pad_dtype=F16, key_pad_stride=Sk, mask_min=c32(BF16_MIN))
    check(a[1], probs=fq_of(PROBS))
    work = ops._decode_work[(None, STREAM)]
    assert a[2:] == [0, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), work.data_ptr(), STREAM]
    lib.calls.clear()
    ops.attn_decode(q, k, v, fq=ops.AttnFakeQuant(), mask_min=-1e4)  # nothing enabled: the entry point without quantisers, the same scratch
    assert [n for n, _ in lib.calls] == ["oeh_attn_decode_work_bytes", "oeh_attn_decode"]
    assert lib.calls[1][1][0].mask_min == -1e4 and lib.calls[1][1][6] == work.data_ptr()
    with pytest.raises(ValueError, match="out_dtype must be the input dtype or float32"):
        ops.attn_decode(q, k, v, out_dtype=f16)


# ---- attn_calibrate
def test_attn_calibrate_scores_without_v(lib):
    q = torch.zeros(B, H, D, Sq, dtype=f16).transpose(2, 3)
    k = bshd(Sk, f16)
    kpm = torch.zeros(B, 1, 1, Sk, dtype=torch.int64)
    fm = torch.zeros(B, 1, Sk, Sq).transpose(2, 3)
    state = torch.zeros(2, dtype=torch.float64)
    res = ops.attn_calibrate(q, k, None, ops.CALIB_SCORES, softmax=SM_CLIP, scale=0.5, scale_div=8.0, key_pad_mask=kpm, full_mask=fm, causal=True, clamp_min=True,
                             n_bits=4, eps=1e-6, q_lo=0.5, q_hi=99.5, momentum=0.75, first=True, state=state)
    assert res is state
    (name, a), = lib.calls
    assert name == "oeh_attn_calibrate"
    # o_dtype stays 0; without v / without an output their stride triples are k's / q's
    check(a[0], B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=F16, q_stride=ST_BHSD(Sq), k_stride=ST_BSHD(Sk), v_stride=ST_BSHD(Sk), o_stride=ST_BHSD(Sq),
          scale=0.5, scale_div=8.0, softmax_base=1, clip=1, gamma=c32(-0.025), eta=c32(1.1), key_pad_mask=own_copy(kpm), key_pad_dtype=F32, key_pad_stride=Sk,
          full_mask=own_copy(fm), full_mask_dtype=F32, full_mask_stride=[Sq * Sk, Sk], causal=1, clamp_min=1, mask_min=F16_MIN)
    (key, work), = ops._calib_work.items()
    assert key == (None, STREAM) and work.numel() * work.element_size() >= 36864  # include/oeh.h: OEH_CALIB_WORK_BYTES
    assert own_copy(q)(a[1]) and a[2:] == [k.data_ptr(), 0, 0, 0, 0, 0, 4, 1e-6, 0.5, 99.5, 0.75, 1, state.data_ptr(), work.data_ptr(), STREAM]


def test_attn_calibrate_probs_and_context(lib):
    q, k, v = bshd(Sq, bf16), bshd(Sk, bf16), bhsd(Sk, bf16)
    kpm = torch.zeros(B, Sk, dtype=f16)
    fm = torch.zeros(B, 1, Sq, Sk + 1, dtype=f16)[..., :Sk]
    sr, pr, state = (torch.zeros(2, dtype=torch.float64) for _ in range(3))
    ops.attn_calibrate(q, k, v, ops.CALIB_PROBS, key_pad_mask=kpm, full_mask=fm, mask_min=-1e4, scores_range=sr, state=state)
    want = dict(B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=BF16, q_stride=ST_BSHD(Sq), k_stride=ST_BSHD(Sk), v_stride=ST_BHSD(Sk), scale=1.0, softmax_base=1, eta=1.0)
    a = lib.calls[0][1]
    check(a[0], o_stride=ST_BSHD(Sq), key_pad_mask=kpm.data_ptr(), key_pad_dtype=F16, key_pad_stride=Sk, full_mask=fm.data_ptr(), full_mask_dtype=F16,
          full_mask_stride=[Sq * (Sk + 1), Sk + 1], mask_min=-1e4, **want)
    work = ops._calib_work[(None, STREAM)]
    assert a[1:] == [q.data_ptr(), k.data_ptr(), v.data_ptr(), 0, 1, sr.data_ptr(), 0, 8, 1e-8, 0.001, 99.999, 0.9, 0, state.data_ptr(), work.data_ptr(), STREAM]
    lib.calls.clear()
    out = ops.attn_calibrate(q, k, v, ops.CALIB_CONTEXT, scores_range=sr, probs_range=pr)
    assert out.dtype == f32 and out.shape == (B, H, Sq, D) and list(out.stride()[:3]) == ST_BSHD(Sq)
    a = lib.calls[0][1]
    check(a[0], o_stride=ST_BSHD(Sq), mask_min=c32(BF16_MIN), **want)
    assert a[1:] == [q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), 2, sr.data_ptr(), pr.data_ptr(), 8, 1e-8, 0.001, 99.999, 0.9, 0, 0, 0, STREAM]
    with pytest.raises(ValueError, match="ranges / state must be contiguous float64 tensors of 2 elements"):
        ops.attn_calibrate(q, k, v, ops.CALIB_CONTEXT, scores_range=sr.float())
    with pytest.raises(ValueError, match="state .* is required for the statistics passes"):
        ops.attn_calibrate(q, k, v, ops.CALIB_PROBS)
    with pytest.raises(ValueError, match="q / k / v dtypes must match and be fp16 / bf16 / fp32"):
        ops.attn_calibrate(q, k.half(), v, ops.CALIB_CONTEXT)


# ---- training
def test_attn_fwd_train_and_bwd(lib):
    q, k, v = (bshd(S, f16).requires_grad_() for S in (Sq, Sk, Sk))
    kpm = torch.zeros(B, 1, 1, Sk, dtype=torch.int64)
    fm = torch.zeros(B, 1, Sk, Sq).transpose(2, 3)
    o, lse = ops.attn_fwd_train(q, k, v, softmax=SM_CLIP, scale_div=8.0, key_pad_mask=kpm, full_mask=fm, causal=True, clamp_min=True)
    assert o.dtype == f16 and list(o.stride()[:3]) == ST_BSHD(Sq) and lse.shape == (B, H, Sq) and lse.dtype == f32
    (name, a), = lib.calls
    assert name == "oeh_attn_fwd_train"
    want = dict(B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=F16, o_dtype=F16, q_stride=ST_BSHD(Sq), k_stride=ST_BSHD(Sk), v_stride=ST_BSHD(Sk), o_stride=ST_BSHD(Sq),
                scale=1.0, scale_div=8.0, softmax_base=1, clip=1, gamma=c32(-0.025), eta=c32(1.1), key_pad_mask=own_copy(kpm), key_pad_dtype=F32, key_pad_stride=Sk,
                full_mask=own_copy(fm), full_mask_dtype=F32, full_mask_stride=[Sq * Sk, Sk], causal=1, clamp_min=1, mask_min=F16_MIN)
    check(a[0], **want)
    assert a[1:] == [q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), STREAM]
    lib.calls.clear()
    do = bhsd(Sq, f16)
    dq, dk, dv = ops.attn_bwd(q, k, v, o, do, lse, softmax=SM_CLIP, scale_div=8.0, key_pad_mask=kpm, full_mask=fm, causal=True, clamp_min=True)
    (wname, wa), (name, a) = lib.calls
    assert (wname, name) == ("oeh_attn_bwd_work_bytes", "oeh_attn_bwd")
    check(a[0], **want)
    assert bytes(wa[0]) == bytes(a[0])
    assert a[1:14] == [q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), ST_BHSD(Sq), lse.data_ptr(), dq.data_ptr(), ST_BSHD(Sq),
                       dk.data_ptr(), ST_BSHD(Sk), dv.data_ptr(), ST_BSHD(Sk)] and a[14] != 0 and a[15] == STREAM


def test_train_dropout_and_masks_read_in_place(lib):
    q, k, v = bshd(Sq, bf16), bshd(Sk, bf16), bshd(Sk, bf16)
    kpm = torch.zeros(B, Sk, dtype=f16)
    fm = torch.zeros(B, 1, Sq, Sk, dtype=f16)
    o, lse = ops.attn_fwd_train(q, k, v, key_pad_mask=kpm, full_mask=fm, mask_min=-1e4, dropout_p=0.25, dropout_seed=2 ** 63 + 5)
    (name, a), = lib.calls
    assert name == "oeh_attn_fwd_train_dropout"
    check(a[0], B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=BF16, o_dtype=BF16, q_stride=ST_BSHD(Sq), k_stride=ST_BSHD(Sk), v_stride=ST_BSHD(Sk), o_stride=ST_BSHD(Sq),
          scale=1.0, softmax_base=1, eta=1.0, key_pad_mask=kpm.data_ptr(), key_pad_dtype=F16, key_pad_stride=Sk, full_mask=fm.data_ptr(), full_mask_dtype=F16,
          full_mask_stride=[Sq * Sk, Sk], mask_min=-1e4)
    assert isinstance(a[1], oeh_dropout) and (a[1].p, a[1].reserved, a[1].seed) == (0.25, 0, 2 ** 63 + 5)
    d, keep = ops._train_desc(q, k, v, o, ops.SoftmaxSpec(), 1.0, 0.0, None, None, False, False, None)  # (the call the training sweep makes)
    check(d, B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=BF16, o_dtype=BF16, q_stride=ST_BSHD(Sq), k_stride=ST_BSHD(Sk), v_stride=ST_BSHD(Sk), o_stride=ST_BSHD(Sq),
          scale=1.0, softmax_base=1, eta=1.0, mask_min=c32(BF16_MIN))
    assert keep == []
    with pytest.raises(ValueError, match=r"shape mismatch: q \(2, 3, 5, 64\) k \(2, 3, 7, 64\) v \(2, 3, 5, 64\)"):
        ops._train_desc(q, k, q, o, ops.SoftmaxSpec(), 1.0, 0.0, None, None, False, False, None)
    with pytest.raises(ValueError, match="q/k/v dtypes must match and be fp16/bf16/fp32, got torch.bfloat16, torch.float16, torch.bfloat16"):
        ops._train_desc(q, k.half(), v, o, ops.SoftmaxSpec(), 1.0, 0.0, None, None, False, False, None)


# ---- the host-only probes: only the nullness of pointers matters to them
def test_attn_variant(lib):
    r = ops.attn_variant(B, H, Sq, Sk, D, bf16, fq=True, clip=True, base=0, gamma=-0.5, key_pad=True, full_mask=True, causal=True, scale=0.5, scale_div=8.0,
                         key_pad_boolean=True, gate_hidden=True)
    assert r == "stub/oeh_attn_variant"
    (name, a), = lib.calls
    check(a[0], B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=BF16, scale=0.5, scale_div=8.0, softmax_base=0, clip=1, gamma=-0.5, eta=1.0, causal=1, mask_min=c32(F32_MIN),
          key_pad_mask=1, key_pad_dtype=F32, key_pad_boolean=1, full_mask=1, full_mask_dtype=F32, gate_hidden=1, gate_w1=1, gate_b1=1)
    probe_fq = dict(enable=1, scale=1.0, zero_point=0.0, qmax=255.0, dump_idx=0)
    check(a[1], scores=probe_fq, probs=probe_fq)
    lib.calls.clear()
    assert ops.attn_variant(B, H, Sq, Sk, D, mask_min=-1e4, pv_pairs=True) == "stub/oeh_attn_variant_ex"
    (name, a), = lib.calls
    check(a[0], B=B, H=H, Sq=Sq, Sk=Sk, D=D, dtype=F16, scale=1.0, softmax_base=1, mask_min=-1e4, key_pad_dtype=F32, full_mask_dtype=F32)
    assert isinstance(a[1], oeh_attn_opts) and a[1].pv_pairs == 1 and a[2] is None


def test_attn_decode_variant(lib):
    assert ops.attn_decode_variant(B, H, 1, Sk, clip=True, gamma=-0.5, causal=True, splits=5, fq=True) == "stub/oeh_attn_decode_fq_variant"
    (name, a), = lib.calls
    check(a[0], B=B, H=H, Sq=1, Sk=Sk, D=D, dtype=F16, scale=1.0, softmax_base=1, clip=1, gamma=-0.5, eta=1.0, causal=1, mask_min=c32(F32_MIN))
    probe_fq = dict(enable=1, scale=1.0, zero_point=0.0, qmax=255.0, dump_idx=0)
    check(a[1], scores=probe_fq, probs=probe_fq)
    assert a[2] == 5
    lib.calls.clear()
    assert ops.attn_decode_variant(B, H, 1, Sk, 128, bf16) == "stub/oeh_attn_decode_variant"
    (name, a), = lib.calls
    check(a[0], B=B, H=H, Sq=1, Sk=Sk, D=128, dtype=BF16, scale=1.0, softmax_base=1, mask_min=c32(F32_MIN))
    assert a[1] == 0


# ---- the small argument checks of the row / quantiser / statistics entry points: they raise before anything is launched
def test_dtype_and_float64_vector_checks(lib):
    xi = torch.zeros(4, 8, dtype=torch.int32)
    x = torch.zeros(4, 8)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64)  # noqa: E731
    for call in (lambda: ops.softmax_rows(xi), lambda: ops.fake_quant(xi, SCORES), lambda: ops.percentile_ema(xi, 0.1, 99.9, f64(2)),
                 lambda: ops.fake_quant_range(xi, f64(2)), lambda: ops.outlier_stats(xi), lambda: ops.quant_mse(xi, torch.zeros(3, 4))):
        with pytest.raises(ValueError, match="^unsupported dtype torch.int32$"):
            call()
    for bad in (f64(3), torch.zeros(2), f64(4)[::2]):
        with pytest.raises(ValueError, match="^state must be a contiguous float64 tensor of 2 elements$"):
            ops.percentile_ema(x, 0.1, 99.9, bad)
        with pytest.raises(ValueError, match="^xmin_xmax must be a contiguous float64 tensor of 2 elements$"):
            ops.fake_quant_range(x, bad)
    with pytest.raises(ValueError, match="^meter must be a contiguous float64 tensor of 4 elements$"):
        ops.outlier_stats(x, meter=f64(2))
    with pytest.raises(ValueError, match="^loss must be a contiguous float64 tensor of K elements$"):
        ops.quant_mse(x, torch.zeros(3, 4), loss=f64(2))
    assert lib.calls == []
    state = f64(2)
    assert ops.percentile_ema(x, 0.1, 99.9, state) is state and lib.calls[0][0] == "oeh_percentile_ema"
    assert lib.calls[0][1][-2] == ops._calib_work[(None, STREAM)].data_ptr()
