"""Host-side checks of the fused attention dropout (include/oeh.h: oeh_dropout, oeh_attn_fwd_train_dropout, oeh_attn_bwd_dropout,
oeh_attn_dropout_mask; csrc/oeh_philox.h) - no GPU needed.  `philox4x32_10` / `keep_mask` are the numpy restatement of the generator
and of the keep rule that tests/test_attn_dropout_gpu.py compares the device's masks with bit for bit."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "oeh.h")
PHILOX_H = os.path.join(ROOT, "outeffhop_amd", "csrc", "oeh_philox.h")
NEW = ("oeh_attn_fwd_train_dropout", "oeh_attn_bwd_dropout", "oeh_attn_dropout_mask")

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)

# Philox4x32-10 known answers (counter words 0..3, key words 0..1 -> output words 0..3), Random123's kat_vectors
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10: counter words and key words (broadcastable integer arrays) -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) & _U32 for x in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    m0, m1, w0, w1, s32 = np.uint64(M0), np.uint64(M1), np.uint64(W0), np.uint64(W1), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # (exact: both factors < 2^32)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _U32, (p0 >> s32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + w0) & _U32, (k1 + w1) & _U32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def dropout_threshold(p):
    """thr = floor(p_f32 * 2^32): a word keeps its element iff word >= thr."""
    return int(np.floor(float(np.float32(p)) * 2.0 ** 32))


def keep_mask(B, H, Sq, Sk, p, seed):
    """The (B,H,Sq,Sk) bool keep mask of the training kernels: key (seed & 0xffffffff, seed >> 32), counter (j >> 2, i, b*H + h, 0),
    word j & 3 of element (b, h, i, j), kept iff word >= floor(p * 2^32)."""
    nc = (Sk + 3) // 4
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    i = np.arange(Sq, dtype=np.uint64)[None, :, None]
    c = np.arange(nc, dtype=np.uint64)[None, None, :]
    w = philox4x32_10(c, i, bh, 0, seed & 0xFFFFFFFF, seed >> 32)
    words = np.stack(w, axis=-1).reshape(B * H, Sq, 4 * nc)[..., :Sk]
    return (words >= np.uint32(dropout_threshold(p)) if p > 0 else np.ones_like(words, dtype=bool)).reshape(B, H, Sq, Sk)


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_numpy_philox_known_answers(ctr, key, out):
    got = philox4x32_10(*ctr, *key)
    assert tuple(int(x) for x in got) == out


def test_keep_mask_restatement():
    """The restatement's layout: counter word 0 counts groups of 4 keys, so a wider row only appends; rate near 1 - p."""
    a = keep_mask(2, 3, 17, 256, 0.25, 0x0123456789ABCDEF)
    b = keep_mask(2, 3, 17, 203, 0.25, 0x0123456789ABCDEF)
    assert np.array_equal(a[..., :203], b)
    w = philox4x32_10(5, 7, 1 * 3 + 2, 0, 0x89ABCDEF, 0x01234567)  # element (b=1, h=2, i=7, j=20..23)
    assert [bool(x >= dropout_threshold(0.25)) for x in w] == list(a[1, 2, 7, 20:24])
    assert abs(float(a.mean()) - 0.75) < 0.02
    assert keep_mask(1, 1, 4, 9, 0.0, 1).all()
    assert dropout_threshold(0.5) == 2 ** 31 and dropout_threshold(0.1) == int(float(np.float32(0.1)) * 2 ** 32)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_header_generator_matches_known_answers(tmp_path):
    """csrc/oeh_philox.h compiled for the host gives the same known answers (the device uses the same definition)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "kat.cpp"
    lines = [f"  {{ auto r = oeh::philox4x32_10({', '.join(hex(x) + 'u' for x in ctr)}, {', '.join(hex(x) + 'u' for x in key)}); "
             f'printf("%08x %08x %08x %08x\\n", r.x[0], r.x[1], r.x[2], r.x[3]); }}' for ctr, key, _ in KAT]
    src.write_text(f'#include "{PHILOX_H}"\n#include <cstdio>\nint main() {{\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "kat"
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", str(src), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    for line, (_, _, want) in zip(out, KAT):
        assert line == " ".join(f"{x:08x}" for x in want)


def test_new_symbols_declared_bound_and_exported():
    from outeffhop_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert re.search(r"typedef struct oeh_dropout\s*\{\s*float p;\s*uint32_t reserved;\s*uint64_t seed;\s*\}\s*oeh_dropout;", txt)
    assert C.sizeof(_lib.oeh_dropout) == 16
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None
    assert lib.oeh_abi_version() == 6


def _desc(dtype=0, D=64):
    from outeffhop_amd import _lib

    d = _lib.oeh_attn_desc()
    d.B, d.H, d.Sq, d.Sk, d.D, d.dtype = 2, 12, 512, 512, D, dtype
    d.o_dtype = dtype
    for f in ("q_stride", "k_stride", "v_stride", "o_stride"):
        getattr(d, f)[:] = [12 * 512 * D, 512 * D, D]
    d.scale = 1.0
    return d


def _calls(lib, d, drop, ptr):
    st = (C.c_int64 * 3)(12 * 512 * 64, 512 * 64, 64)
    dp = None if drop is None else C.byref(drop)
    return (lib.oeh_attn_fwd_train_dropout(C.byref(d), dp, ptr, ptr, ptr, ptr, ptr, None),
            lib.oeh_attn_bwd_dropout(C.byref(d), dp, ptr, ptr, ptr, ptr, ptr, st, ptr, ptr, st, ptr, st, ptr, st, ptr, None))


def test_validation_codes_without_gpu():
    """p outside [0, 1) or NaN: -22 from every new entry point, before anything else; fp32 / INT8 storage or another head dim with
    dropout: -95 as without it.  (Fake device pointers: none of these calls may reach the device.)"""
    from outeffhop_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(256)
    for p in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        drop = _lib.oeh_dropout(p, 0, 1234)
        assert _calls(lib, _desc(), drop, one) == (-22, -22), p
        assert _calls(lib, _desc(dtype=2), drop, one) == (-22, -22), p
        assert lib.oeh_attn_dropout_mask(C.byref(_desc()), C.byref(drop), one, None) == -22, p
    assert _calls(lib, _desc(), None, one) == (-22, -22)                       # no dropout descriptor
    assert lib.oeh_attn_dropout_mask(C.byref(_desc()), None, one, None) == -22
    ok = _lib.oeh_dropout(0.1, 0, 1234)
    assert lib.oeh_attn_dropout_mask(None, C.byref(ok), one, None) == -22
    assert lib.oeh_attn_dropout_mask(C.byref(_desc()), C.byref(ok), None, None) == -22  # null mask
    bad_shape = _desc()
    bad_shape.Sk = 0
    assert lib.oeh_attn_dropout_mask(C.byref(bad_shape), C.byref(ok), one, None) == -22
    for bad in (dict(dtype=2), dict(dtype=3), dict(D=32), dict(D=128)):
        assert _calls(lib, _desc(**bad), ok, one) == (-95, -95), bad
    assert _calls(lib, _desc(), ok, None) == (-22, -22)                         # null pointers after a valid p


def test_fused_attention_takes_dropout_arguments():
    """fused_attention / the ops accept the dropout keywords (no TypeError); without a GPU the op refuses as before."""
    from outeffhop_amd import _lib, fused_attention, ops

    q = torch.zeros(1, 2, 64, 64, dtype=torch.float16)
    with pytest.raises(_lib.OehError):
        fused_attention(q, q, q, dropout_p=0.1)
    with pytest.raises(_lib.OehError):
        fused_attention(q, q, q, dropout_p=0.1, dropout_seed=7)
    with pytest.raises(_lib.OehError):
        ops.attn_fwd_train(q, q, q, dropout_p=0.1, dropout_seed=7)
    with pytest.raises(_lib.OehError):
        ops.attn_dropout_mask(1, 2, 64, 64, 0.1, 7, "cpu")
    with pytest.raises(ValueError):
        ops._dropout(0.1, None)
    with pytest.raises(ValueError):
        ops._dropout(0.1, 2 ** 64)
    assert ops._dropout(0.0, None) is None


def test_seed_comes_from_the_default_cpu_generator():
    from outeffhop_amd.autograd_attention import draw_seed

    torch.manual_seed(3)
    a = [draw_seed() for _ in range(4)]
    torch.manual_seed(3)
    b = [draw_seed() for _ in range(4)]
    assert a == b and len(set(a)) == 4 and all(0 <= s < 2 ** 64 for s in a)
    assert any(s >= 2 ** 32 for s in a)


def test_fused_dropout_switch_is_off_by_default():
    import outeffhop_amd
    from outeffhop_amd import attention as A

    assert A.FUSED_DROPOUT is False
    assert outeffhop_amd.set_fused_dropout is A.set_fused_dropout
    try:
        A.set_fused_dropout(True)
        assert A.FUSED_DROPOUT is True
    finally:
        A.set_fused_dropout(False)
    assert A.FUSED_DROPOUT is False
