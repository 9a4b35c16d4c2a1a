"""Host-side checks of the training entry points (include/oeh.h: oeh_attn_fwd_train, oeh_attn_bwd_work_bytes, oeh_attn_bwd) and of
outeffhop_amd.fused_attention's refusals - no GPU needed: argument validation happens before anything touches a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "oeh.h")
NEW = ("oeh_attn_fwd_train", "oeh_attn_bwd_work_bytes", "oeh_attn_bwd")


def test_new_symbols_declared_bound_and_exported():
    from outeffhop_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", txt), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
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


def _bwd(lib, d, ptr):
    st = (C.c_int64 * 3)(12 * 512 * 64, 512 * 64, 64)
    return lib.oeh_attn_bwd(C.byref(d), ptr, ptr, ptr, ptr, ptr, st, ptr, ptr, st, ptr, st, ptr, st, ptr, None)


def test_validation_codes_and_work_size_without_gpu():
    """The entry points' error codes, and the size of `work`: two fp32 terms per query row - delta, and log(den) of a saturated row
    (include/oeh.h: oeh_attn_bwd)."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(256)
    assert lib.oeh_attn_fwd_train(None, one, one, one, one, one, None) == -22
    assert lib.oeh_attn_bwd_work_bytes(None) == -22
    d = _desc()
    assert lib.oeh_attn_bwd_work_bytes(C.byref(d)) == 2 * (2 * 12 * 512) * 4  # B * H * Sq rows, 2 fp32 terms each
    assert lib.oeh_attn_fwd_train(C.byref(d), None, one, one, one, one, None) == -22  # null q
    assert _bwd(lib, d, None) == -22                                                  # null pointers
    for bad, code in ((dict(dtype=2), -95), (dict(dtype=3), -95), (dict(D=128), -95), (dict(D=32), -95), (dict(dtype=7), -22)):
        d = _desc(**bad)
        assert lib.oeh_attn_fwd_train(C.byref(d), one, one, one, one, one, None) == code, bad
        assert lib.oeh_attn_bwd_work_bytes(C.byref(d)) == code, bad
        assert _bwd(lib, d, one) == code, bad
    d = _desc()
    d.softmax_base = 2
    assert lib.oeh_attn_fwd_train(C.byref(d), one, one, one, one, one, None) == -22
    d = _desc()
    d.gate = 256  # the gate stays outside the differentiable core
    assert lib.oeh_attn_fwd_train(C.byref(d), one, one, one, one, one, None) == -95
    d = _desc()
    d.gate_hidden, d.gate_w1, d.gate_b1 = 256, 256, 256  # the in-kernel gate predictor
    assert _bwd(lib, d, one) == -95
    d = _desc()
    d.o_dtype = 2  # the inference kernels' fp32-accumulator output
    assert lib.oeh_attn_fwd_train(C.byref(d), one, one, one, one, one, None) == -95
    d = _desc()
    assert lib.oeh_attn_fwd_train(C.byref(d), C.c_void_p(258), one, one, one, one, None) == -14  # rows not 16-byte aligned


def test_plain_c_host_links_the_training_entry_points(tmp_path):
    from outeffhop_amd import _lib

    gcc = shutil.which("gcc")
    if gcc is None or not os.path.exists(_lib.LIB_PATH):
        pytest.skip("no C compiler or library not built")
    src = tmp_path / "host.c"
    src.write_text(f'''#include <stdio.h>
#include <string.h>
#include "{HDR}"
int main(void) {{
  oeh_attn_desc d;
  memset(&d, 0, sizeof d);
  d.B = 1; d.H = 1; d.Sq = 8; d.Sk = 8; d.D = 64; d.dtype = OEH_F32;
  printf("%d %lld %d\\n", oeh_attn_fwd_train(NULL, NULL, NULL, NULL, NULL, NULL, NULL), (long long)oeh_attn_bwd_work_bytes(&d),
         oeh_attn_bwd(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));
  return 0;
}}
''')
    exe = tmp_path / "host"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src), "-L" + libdir, "-loeh_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                    "-Wl,--allow-shlib-undefined"], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out == ["-22", "-95", "-22"], out


def test_fused_attention_refuses_what_the_kernels_do_not_take():
    from outeffhop_amd import _lib, fused_attention
    from outeffhop_amd.ops import SoftmaxSpec

    q16 = torch.zeros(1, 2, 8, 64, dtype=torch.float16)
    for q, sm in ((torch.zeros(1, 2, 8, 64), SoftmaxSpec()),                       # fp32 storage
                  (torch.zeros(1, 2, 8, 32, dtype=torch.float16), SoftmaxSpec()),  # head dim 32
                  (q16, lambda x, dim=-1: torch.softmax(x, dim))):                 # a user callable
        with pytest.raises(_lib.OehError) as e:
            fused_attention(q, q, q, softmax=sm)
        assert e.value.code == -95
    with pytest.raises(_lib.OehError):  # CPU tensors: no CPU path
        fused_attention(q16, q16, q16)


def test_switch_is_off_by_default_and_settable():
    from outeffhop_amd import attention as A, set_fused_backward

    assert A.FUSED_BACKWARD is False
    try:
        set_fused_backward(True)
        assert A.FUSED_BACKWARD is True
    finally:
        set_fused_backward(False)
    assert A.FUSED_BACKWARD is False


def test_forward_only_ops_still_refuse_autograd():
    """ops.attn_fwd keeps raising "forward-only" for grad-requiring inputs (the training op is separate)."""
    from outeffhop_amd import _lib, ops

    q = torch.zeros(1, 2, 8, 64, dtype=torch.float16, requires_grad=True)
    with pytest.raises(_lib.OehError):
        ops.attn_fwd(q, q, q)
