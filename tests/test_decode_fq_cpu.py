"""Host-side checks of the split-key decode entry points with the fused INT8 chain (include/oeh.h: oeh_attn_decode_fq,
oeh_attn_decode_fq_variant) and of the modules' routing to them - no GPU needed: every refusal is made before anything touches a device."""
import ctypes as C
import re

import pytest
import torch

from tests.test_decode_cpu import EINVAL, ENOTSUP, HDR, _desc

NEW = ("oeh_attn_decode_fq", "oeh_attn_decode_fq_variant")


def _lib():
    from outeffhop_amd import _lib as L

    return L


def _fq(scores=True, probs=True, ctx=True, **kw):
    f = _lib().oeh_fq_desc()
    for name, on in (("scores", scores), ("probs", probs), ("ctx", ctx)):
        q = getattr(f, name)
        q.enable, q.scale, q.zero_point, q.qmax = int(on), 0.05, 128.0, 255.0
    f.ctx_quant_before_gate = 1
    for name, val in kw.items():
        setattr(f, name, val)
    return f


def _call(d, fq, splits=0, q=256, k=256, v=256, o=256, work=256):
    p = lambda a: None if a is None else C.c_void_p(a)  # noqa: E731
    return _lib().load().oeh_attn_decode_fq(None if d is None else C.byref(d), None if fq is None else C.byref(fq), splits, p(q), p(k), p(v), p(o), p(work), None)


def _variant(d, fq, splits=0):
    r = _lib().load().oeh_attn_decode_fq_variant(C.byref(d), None if fq is None else C.byref(fq), splits)
    return None if r is None else r.decode()


def _plain_variant(d, splits=0):
    r = _lib().load().oeh_attn_decode_variant(C.byref(d), splits)
    return None if r is None else r.decode()


def test_symbols_declared_bound_and_exported():
    L = _lib()
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in L.EXPORTS
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.oeh_abi_version() == 6


def test_refusal_order_without_a_device():
    """oeh_attn_decode's refusals first and in its order (a NULL fq: exactly its validation), then OEH_EINVAL for a grid that is none, then
    OEH_ENOTSUP for ctx_emit_index and for a uint8 dump of a wider grid."""
    for fq in (None, _fq(), _fq(False, False, False)):
        assert _call(None, fq) == EINVAL
        for null in ("q", "k", "v", "o", "work"):
            assert _call(_desc(), fq, **{null: None}) == EINVAL, null
        assert _call(_desc(), fq, splits=-1) == EINVAL and _call(_desc(), fq, splits=65) == EINVAL
        for bad in (dict(D=32), dict(Sq=17), dict(dtype=2), dict(dtype=3), dict(full_mask=256), dict(gate_hidden=256)):
            assert _call(_desc(**bad), fq) == ENOTSUP, bad
        assert _call(_desc(), fq, q=258) == -14 and _call(_desc(), fq, work=264) == -14
    # the quantisers' own refusals come after every one of those
    emit = _fq(ctx_emit_index=1, ctx_quant_before_gate=0)
    assert _call(_desc(), emit) == ENOTSUP
    assert _call(_desc(D=32), emit) == ENOTSUP and _call(_desc(), emit, q=None) == EINVAL and _call(_desc(), emit, q=258) == -14
    for name in ("scores", "probs", "ctx"):
        for scale in (0.0, -1.0, float("inf"), float("nan")):
            f = _fq()
            getattr(f, name).scale = scale
            assert _call(_desc(), f) == EINVAL, (name, scale)
            assert _call(_desc(), f, q=258) == -14  # (alignment is oeh_attn_decode's refusal: it wins)
        f = _fq()
        getattr(f, name).qmax = float("inf")
        assert _call(_desc(), f) == EINVAL, name
        f = _fq()
        getattr(f, name).qmax, getattr(f, name).dump_idx = 1023.0, 256
        assert _call(_desc(), f) == ENOTSUP, name
    # a disabled quantiser's fields are not judged; scale 0 wins over ctx_emit_index (OEH_EINVAL before OEH_ENOTSUP)
    f = _fq(ctx_emit_index=1)
    f.scores.scale = 0.0
    assert _call(_desc(), f) == EINVAL
    assert _variant(_desc(), f) is None and _variant(_desc(), emit) is None


def test_variant_names():
    for Sk, splits in ((1000, 16), (77, 4), (2049, 32), (2049, 0), (130, 64), (1, 0)):
        for kw in (dict(), dict(dtype=1), dict(clip=1, gamma=-0.025, eta=1.0)):
            plain = _plain_variant(_desc(Sk=Sk, **kw), splits)
            assert plain is not None
            assert _variant(_desc(Sk=Sk, **kw), None, splits) == plain
            assert _variant(_desc(Sk=Sk, **kw), _fq(False, False, False), splits) == plain
            for sub in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
                assert _variant(_desc(Sk=Sk, **kw), _fq(*sub), splits) == plain + "/fq"
    assert _variant(_desc(Sk=2048, B=1), _fq(), 0) == "decode16/SP8/D64/f16/fq"
    assert _variant(_desc(Sk=2048, B=1, clip=1, gamma=-0.025, eta=1.0), _fq(), 0) == "decode16/SP8/D64/f16/clip/fq"
    assert _variant(_desc(D=32), _fq()) is None and _variant(_desc(Sq=17), _fq()) is None and _variant(_desc(dtype=2), _fq()) is None


def test_ops_variant_helper():
    from outeffhop_amd import ops

    assert ops.attn_decode_variant(2, 12, 1, 1000, splits=16, fq=True) == "decode16/SP16/D64/f16/fq"
    assert ops.attn_decode_variant(2, 12, 1, 1000, dtype=torch.bfloat16, clip=True, splits=16, fq=True) == "decode16/SP16/D64/bf16/clip/fq"
    assert ops.attn_decode_variant(2, 12, 1, 1000, splits=16) == "decode16/SP16/D64/f16"
    assert ops.attn_decode_variant(2, 12, 1, 1000, D=32, fq=True) is None


@pytest.mark.parametrize("on", [True, False])
def test_attention_core_routes_a_quantised_generation_step(monkeypatch, on):
    """With SPLIT_DECODE on, attention_core(..., fq=<spec>, decode=True) reaches ops.attn_decode with that fq; with it off, ops.attn_fwd."""
    import outeffhop_amd as oa
    from outeffhop_amd import attention, ops

    seen = []

    def recorder(name):
        def f(q, k, v, **kw):
            seen.append((name, kw.get("fq")))
            return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3], dtype=q.dtype).permute(0, 2, 1, 3)
        return f

    monkeypatch.setattr(ops, "attn_decode", recorder("attn_decode"))
    monkeypatch.setattr(ops, "attn_fwd", recorder("attn_fwd"))
    spec = ops.AttnFakeQuant(ops.FakeQuantSpec(0.1, 128.0, 255.0), ops.FakeQuantSpec(1 / 255, 0.0, 255.0), ops.FakeQuantSpec(0.02, 128.0, 255.0))
    q, k, v = torch.zeros(1, 2, 1, 64).half(), torch.zeros(1, 2, 40, 64).half(), torch.zeros(1, 2, 40, 64).half()
    before = attention.SPLIT_DECODE
    try:
        attention.set_split_decode(on)
        out = attention.attention_core(q, k, v, softmax_fn=oa.SOFTMAX_MAPPING["softmax1"], fq=spec, decode=True)
    finally:
        attention.set_split_decode(before)
    assert out.shape == (1, 1, 128)
    assert seen == [("attn_decode" if on else "attn_fwd", spec)]
    assert seen[0][1] is spec
