"""Host-side checks of the probability pairs (include/oeh.h: oeh_attn_opts, oeh_attn_fwd_ex, oeh_attn_variant_ex) and of the
`attention.set_compensated_pv` switch - no GPU needed: every call below returns before any device work."""
import ctypes as C
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "oeh.h")
NEW = ("oeh_attn_fwd_ex", "oeh_attn_variant_ex")


def _desc(dtype, B=1, H=1, S=64, D=64):
    from outeffhop_amd import _lib

    d = _lib.oeh_attn_desc()
    d.B, d.H, d.Sq, d.Sk, d.D, d.dtype = B, H, S, S, D, dtype
    d.scale, d.softmax_base, d.mask_min = 0.125, 1, -3.0e38
    for name in ("q_stride", "k_stride", "v_stride", "o_stride"):
        getattr(d, name)[:] = [H * S * D, S * D, D]
    return d


def test_new_symbols_are_declared_bound_and_exported():
    from outeffhop_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert "typedef struct oeh_attn_opts" in txt
    assert C.sizeof(_lib.oeh_attn_opts) == 16 and _lib.oeh_attn_opts.reserved.offset == 4
    assert lib.oeh_abi_version() == 6


def test_return_codes_without_a_device():
    from outeffhop_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(16)
    # opts == NULL: exactly oeh_attn_fwd's codes
    bad = _desc(_lib.OEH_F32)
    bad.softmax_base = 3
    assert lib.oeh_attn_fwd_ex(C.byref(bad), None, one, one, one, one, None, None) == lib.oeh_attn_fwd(C.byref(bad), one, one, one, one, None, None) == -22
    assert lib.oeh_attn_fwd_ex(None, None, None, None, None, None, None, None) == lib.oeh_attn_fwd(None, None, None, None, None, None, None) == -22
    # a reserved word: -22 before anything else (even a valid problem, even pv_pairs == 0)
    d = _desc(_lib.OEH_F32)
    for i in range(3):
        o = _lib.oeh_attn_opts(pv_pairs=1)
        o.reserved[i] = 1
        assert lib.oeh_attn_fwd_ex(C.byref(d), C.byref(o), one, one, one, one, None, None) == -22
        assert lib.oeh_attn_variant_ex(C.byref(d), C.byref(o), None) is None
    o = _lib.oeh_attn_opts(pv_pairs=0)
    o.reserved[2] = 7
    assert lib.oeh_attn_fwd_ex(C.byref(d), C.byref(o), one, one, one, one, None, None) == -22
    # what the pairs do not cover: -95
    pv = _lib.oeh_attn_opts(pv_pairs=1)
    for dt in (_lib.OEH_F16, _lib.OEH_BF16):
        assert lib.oeh_attn_fwd_ex(C.byref(_desc(dt)), C.byref(pv), one, one, one, one, None, None) == -95
        d16 = _desc(dt)
        d16.o_dtype = _lib.OEH_F32
        assert lib.oeh_attn_fwd_ex(C.byref(d16), C.byref(pv), one, one, one, one, None, None) == -95
        assert lib.oeh_attn_variant_ex(C.byref(d16), C.byref(pv), None) is None
    fq = _lib.oeh_fq_desc()
    fq.scores.enable, fq.scores.scale, fq.scores.qmax = 1, 0.1, 255.0
    fq.probs.enable, fq.probs.scale, fq.probs.qmax = 1, 1.0 / 255, 255.0
    assert lib.oeh_attn_fwd_ex(C.byref(d), C.byref(pv), one, one, one, one, C.byref(fq), None) == -95
    assert lib.oeh_attn_variant_ex(C.byref(d), C.byref(pv), C.byref(fq)) is None
    dg = _desc(_lib.OEH_F32)
    dg.gate_hidden, dg.gate_w1, dg.gate_b1 = 16, 16, 16
    dg.gate_hidden_stride[:] = [64 * 64, 64]
    assert lib.oeh_attn_fwd_ex(C.byref(dg), C.byref(pv), one, one, one, one, None, None) == -95


def test_variant_names_carry_the_suffix_on_the_matrix_core_kernels_only():
    from outeffhop_amd import ops

    f32 = torch.float32
    # one-pass kernel: plain, two-pass clip, key padding (head dim 64 with padding: one block per wave)
    assert ops.attn_variant(16, 12, 512, 512, 64, f32, causal=True, pv_pairs=True) == "flash16/MQ2/D64/f32+pv2"
    assert ops.attn_variant(1, 1, 8, 100000, 64, f32, clip=True, pv_pairs=True) == "flash16/MQ1/D64/f32/clip2p+pv2"
    assert ops.attn_variant(2, 12, 704, 704, 64, f32, key_pad=True, pv_pairs=True) == "flash16/MQ1/D64/f32+pv2"
    assert ops.attn_variant(16, 12, 512, 512, 128, f32, causal=True, pv_pairs=True) == "flash16/MQ1/D128/f32+pv2"
    # full-row kernel: clipped rows of <= 512 keys, short rows
    assert ops.attn_variant(16, 12, 512, 512, 64, f32, clip=True, causal=True, pv_pairs=True) == "fast16/NT32/D64/f32/clip+pv2"
    assert ops.attn_variant(32, 12, 128, 128, 64, f32, key_pad=True, pv_pairs=True) == "fast16/NT8/D64/f32+pv2"
    assert ops.attn_variant(4, 2, 64, 64, 32, f32, pv_pairs=True) == "fast16/NT8/D32/f32+pv2"
    # fp32-exact already: the small-shape and any-shape kernels, unchanged and without the suffix
    assert ops.attn_variant(224, 4, 28, 28, 64, f32, pv_pairs=True) == ops.attn_variant(224, 4, 28, 28, 64, f32) == "small/ST2/D64/f32"
    assert ops.attn_variant(2, 2, 40, 40, 48, f32, pv_pairs=True) == "generic"
    # the general kernel's fp32 form rounds P to one fp16 operand: with the pairs such a problem goes to the any-shape kernel
    assert ops.attn_variant(2, 2, 64, 64, 64, f32, full_mask=True).startswith("mfma16/")
    assert ops.attn_variant(2, 2, 64, 64, 64, f32, full_mask=True, pv_pairs=True) == "generic"
    # refused: 16-bit storage, fake-quant, the in-kernel gate predictor
    assert ops.attn_variant(16, 12, 512, 512, 64, torch.float16, pv_pairs=True) is None
    assert ops.attn_variant(16, 12, 512, 512, 64, f32, fq=True, pv_pairs=True) is None
    assert ops.attn_variant(16, 12, 512, 512, 64, f32, gate_hidden=True, pv_pairs=True) is None
    # without the pairs: the names of today
    assert ops.attn_variant(16, 12, 512, 512, 64, f32, causal=True, pv_pairs=False) == ops.attn_variant(16, 12, 512, 512, 64, f32, causal=True) == "flash16/MQ2/D64/f32"


def test_the_switch_is_off_by_default_and_narrows_the_gate_predictor():
    from outeffhop_amd import attention, ops

    assert attention.COMPENSATED_PV is False
    q32, q16 = torch.zeros(1, 1, 4, 64), torch.zeros(1, 1, 4, 64, dtype=torch.float16)
    assert not attention.pv_pairs_for(q32)
    try:
        attention.set_compensated_pv(True)
        assert attention.COMPENSATED_PV is True
        assert attention.pv_pairs_for(q32) and not attention.pv_pairs_for(q16) and not attention.pv_pairs_for(q32, fq=object())
    finally:
        attention.set_compensated_pv(False)
    assert attention.COMPENSATED_PV is False
    # the in-kernel gate predictor is declined with the pairs (the gate then runs as oeh_gate_fwd + gate values)
    kw = dict(base=1, gamma=0.0, key_pad=False, causal=False, scale=0.125, scale_div=0.0, mask_min=-3.0e38)
    assert ops.fused_gate_ok(32, 12, 128, 128, 64, torch.float32, **kw)
    assert not ops.fused_gate_ok(32, 12, 128, 128, 64, torch.float32, pv_pairs=True, **kw)
