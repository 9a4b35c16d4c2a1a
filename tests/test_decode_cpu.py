"""Host-side checks of the split-key decode entry points (include/oeh.h: oeh_attn_decode_work_bytes, oeh_attn_decode,
oeh_attn_decode_variant) and of ops.attn_decode's refusal of CPU tensors - no GPU needed: the plan (validation, split count, scratch size)
is made before anything touches a device."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "oeh.h")
NEW = ("oeh_attn_decode_work_bytes", "oeh_attn_decode", "oeh_attn_decode_variant")
EINVAL, ENOTSUP, EALIGN = -22, -95, -14


def _lib():
    from outeffhop_amd import _lib as L

    return L


def _desc(B=2, H=12, Sq=1, Sk=1000, D=64, dtype=0, **kw):
    d = _lib().oeh_attn_desc()
    d.B, d.H, d.Sq, d.Sk, d.D, d.dtype = B, H, Sq, Sk, D, dtype
    d.o_dtype = dtype
    d.q_stride[:] = [H * Sq * D, Sq * D, D]
    d.o_stride[:] = [H * Sq * D, Sq * D, D]
    d.k_stride[:] = [H * Sk * D, Sk * D, D]
    d.v_stride[:] = [H * Sk * D, Sk * D, D]
    d.scale, d.softmax_base = 1.0, 1
    d.mask_min = float(torch.finfo(torch.float32).min)
    for name, val in kw.items():
        setattr(d, name, val)
    return d


def _variant(d, splits):
    r = _lib().load().oeh_attn_decode_variant(C.byref(d), splits)
    return None if r is None else r.decode()


def _splits_of(d, splits=0):
    name = _variant(d, splits)
    assert name is not None
    return int(re.match(r"decode16/SP(\d+)/D64/", name).group(1))


def test_symbols_declared_bound_and_exported():
    L = _lib()
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = L.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in L.EXPORTS
        assert hasattr(lib, name)
    assert re.search(r"#define\s+OEH_DECODE_MAX_SPLITS\s+64\b", txt) and L.DECODE_MAX_SPLITS == 64
    assert lib.oeh_abi_version() == 6


@pytest.mark.parametrize("Sk,splits,n", [(1000, 16, 16), (77, 4, 2), (16, 4, 1), (130, 64, 3), (2049, 32, 17), (1, 0, 1)])
def test_variant_names_print_the_effective_split_count(Sk, splits, n):
    """C = roundup64(ceil(Sk / splits)), n = ceil(Sk / C)."""
    assert _variant(_desc(Sk=Sk), splits) == f"decode16/SP{n}/D64/f16"
    assert _variant(_desc(Sk=Sk, dtype=1), splits) == f"decode16/SP{n}/D64/bf16"
    assert _variant(_desc(Sk=Sk, clip=1, gamma=-0.025, eta=1.0), splits) == f"decode16/SP{n}/D64/f16/clip"
    assert _variant(_desc(Sk=Sk, dtype=1, clip=1, gamma=0.0, eta=1.003), splits) == f"decode16/SP{n}/D64/bf16/clip"


def test_ops_variant_helper():
    from outeffhop_amd import ops

    assert ops.attn_decode_variant(2, 12, 1, 1000, splits=16) == "decode16/SP16/D64/f16"
    assert ops.attn_decode_variant(2, 12, 1, 1000, dtype=torch.bfloat16, clip=True, splits=16) == "decode16/SP16/D64/bf16/clip"
    assert ops.attn_decode_variant(2, 12, 1, 1000, D=32) is None
    assert ops.attn_decode_variant(2, 12, 17, 1000) is None


def _call(d, splits=0, q=256, k=256, v=256, o=256, work=256):
    p = lambda a: None if a is None else C.c_void_p(a)  # noqa: E731
    return _lib().load().oeh_attn_decode(None if d is None else C.byref(d), splits, p(q), p(k), p(v), p(o), p(work), None)


def test_refusals_without_a_device():
    """Every refusal returns its code before anything touches a device: OEH_EINVAL, then OEH_ENOTSUP, then OEH_EALIGN."""
    lib = _lib().load()
    # OEH_EINVAL
    assert _call(None) == EINVAL and lib.oeh_attn_decode_work_bytes(None, 0) == EINVAL and lib.oeh_attn_decode_variant(None, 0) is None
    for null in ("q", "k", "v", "o", "work"):
        assert _call(_desc(), **{null: None}) == EINVAL, null
    for bad in (dict(B=0), dict(H=0), dict(Sq=0), dict(Sk=0), dict(D=0), dict(Sk=-5)):
        d = _desc()
        for n_, v_ in bad.items():
            setattr(d, n_, v_)
        assert _call(d) == EINVAL, bad
        assert lib.oeh_attn_decode_work_bytes(C.byref(d), 0) == EINVAL, bad
        assert _variant(d, 0) is None, bad
    for splits in (-1, 65):
        assert _call(_desc(), splits) == EINVAL
        assert lib.oeh_attn_decode_work_bytes(C.byref(_desc()), splits) == EINVAL
        assert _variant(_desc(), splits) is None
    assert _variant(_desc(), 64) is not None and lib.oeh_attn_decode_work_bytes(C.byref(_desc()), 64) > 0
    # OEH_ENOTSUP
    unsupported = (dict(full_mask=256), dict(gate_hidden=256), dict(dtype=2), dict(dtype=3), dict(D=32), dict(D=128), dict(Sq=17),
                   dict(clip=1, gamma=0.01, eta=1.0), dict(causal=1, Sq=5, Sk=3))
    for bad in unsupported:
        d = _desc(**bad)
        assert _call(d) == ENOTSUP, bad
        assert lib.oeh_attn_decode_work_bytes(C.byref(d), 0) == ENOTSUP, bad
        assert _variant(d, 0) is None, bad
    # the order: an invalid argument wins over an unsupported option, an unsupported option over a misaligned pointer
    assert _call(_desc(D=32), -1) == EINVAL
    assert _call(_desc(D=32), q=None) == EINVAL
    assert _call(_desc(D=32), q=258) == ENOTSUP
    assert _call(_desc(Sq=17), work=8) == ENOTSUP
    # OEH_EALIGN
    for arg in ("q", "k", "v", "o"):
        assert _call(_desc(), **{arg: 258}) == EALIGN, arg
    assert _call(_desc(), work=264) == EALIGN
    for f in ("q_stride", "k_stride", "v_stride", "o_stride"):
        d = _desc()
        getattr(d, f)[2] = 68  # rows of 136 bytes
        assert _call(d) == EALIGN, f
    d = _desc(o_dtype=2)
    d.o_stride[:] = [12 * 66, 66, 66]  # fp32 output rows of 264 bytes
    assert _call(d) == EALIGN


def test_work_bytes_positive_and_monotone():
    lib = _lib().load()
    wb = lambda splits=16, **kw: lib.oeh_attn_decode_work_bytes(C.byref(_desc(**kw)), splits)  # noqa: E731
    assert wb() > 0 and wb(B=1, H=1, Sk=1, splits=0) > 0
    sizes = [wb(B=b) for b in (1, 2, 3, 16)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    sizes = [wb(H=h) for h in (1, 2, 12, 32)]
    assert sizes == sorted(sizes)
    # the effective split count: n = 1, 2, 4, 8, 16 (Sk = 1000: chunks of 1024, 512, 256, 128, 64)
    eff = [_splits_of(_desc(), s) for s in (1, 2, 4, 8, 16)]
    assert eff == [1, 2, 4, 8, 16]
    sizes = [wb(splits=s) for s in (1, 2, 4, 8, 16)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # asking for more splits than there are 64-key chunks changes nothing
    assert wb(Sk=130, splits=64) == wb(Sk=130, splits=3) and _splits_of(_desc(Sk=130), 64) == 3
    # the scratch holds at least the (m, l) pair and 64 accumulators per (batch, head, split, query row)
    assert wb(B=2, H=3, Sq=5, splits=4, Sk=1000) >= 2 * 3 * 4 * 5 * 66 * 4


def test_default_split_rule_properties():
    """Properties of the library's own choice (splits == 0), not its values: one split for short rows and once the heads fill the chip."""
    for Sk in (1, 16, 64, 100, 128):
        for B, H in ((1, 1), (1, 12), (16, 12), (64, 32)):
            assert _splits_of(_desc(B=B, H=H, Sk=Sk)) == 1, (B, H, Sk)
    for B, H in ((512, 1), (16, 32), (64, 12), (1, 512)):
        for Sk in (129, 2048, 100000):
            assert _splits_of(_desc(B=B, H=H, Sk=Sk)) == 1, (B, H, Sk)
    for B, H in ((1, 1), (1, 12), (2, 12), (16, 12), (3, 7), (40, 12)):
        for Sq in (1, 16):
            for Sk in (129, 512, 2048, 2049, 65536, 1000000):
                n = _splits_of(_desc(B=B, H=H, Sq=Sq, Sk=Sk))
                assert 1 <= n <= 64, (B, H, Sq, Sk, n)


def test_attn_decode_needs_gpu_tensors():
    from outeffhop_amd import ops
    from outeffhop_amd._lib import OehError

    q, k, v = torch.zeros(1, 2, 1, 64).half(), torch.zeros(1, 2, 40, 64).half(), torch.zeros(1, 2, 40, 64).half()
    calls = ops.DECODE_CALLS
    with pytest.raises(OehError):
        ops.attn_decode(q, k, v)
    assert ops.DECODE_CALLS == calls


def test_module_switch():
    from outeffhop_amd import attention

    assert attention.SPLIT_DECODE is False  # opt-in until the path has been timed against ops.attn_fwd
    try:
        attention.set_split_decode(True)
        assert attention.SPLIT_DECODE is True
        attention.set_split_decode(False)
        assert attention.SPLIT_DECODE is False
    finally:
        attention.set_split_decode(False)
