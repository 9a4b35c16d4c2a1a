"""Host side of the cross-entropy entry points (oeh_xent_fwd / oeh_xent_bwd / oeh_xent_variant, outeffhop_amd.losses) without a GPU: the
header against the binding, the descriptor's layout, every refusal code in its order, the launch-form names, the torch path against the
reference's literal lines, the perplexity meter's arithmetic, and the float64 restatement against torch and against an fp32 emulation of
the kernel's order of operations."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _xent_ref as X

torch = pytest.importorskip("torch")
nn = torch.nn
F = torch.nn.functional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "oeh.h")
EINVAL, ENOTSUP, EALIGN = -22, -95, -14
NAMES = ("oeh_xent_fwd", "oeh_xent_bwd", "oeh_xent_variant")


def test_header_binding_and_struct_layout_agree(tmp_path):
    from outeffhop_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(oeh_[a-z0-9_]+)\s*\(", txt))
    assert set(NAMES) <= declared and set(NAMES) <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NAMES) and lib.oeh_abi_version() == 6
    assert re.search(r"#define OEH_XENT_SLOTS 4\b", txt) and _lib.XENT_SLOTS == 4
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    st = _lib.oeh_xent_desc
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HDR}"', "int main(void) {", '  printf("size %zu\\n", sizeof(oeh_xent_desc));']
    lines += [f'  printf("{f} %zu\\n", offsetof(oeh_xent_desc, {f}));' for f, _ in st._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], check=True, capture_output=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(out[f]) == getattr(st, f).offset, f


def _desc(B=2, S=3, V=1000, dtype=0, **kw):
    from outeffhop_amd import _lib

    d = _lib.oeh_xent_desc()
    d.B, d.S, d.V, d.dtype, d.label_dtype, d.ignore_index = B, S, V, dtype, _lib.OEH_ID_I64, -100
    d.x_stride[0], d.x_stride[1], d.label_stride[0], d.label_stride[1], d.dx_stride[0], d.dx_stride[1] = S * V, V, S, 1, S * V, V
    for k, v in kw.items():
        if "__" in k:
            name, i = k.split("__")
            getattr(d, name)[int(i)] = v
        else:
            setattr(d, k, v)
    return d


def test_argument_validation_without_gpu():
    """Every refusal with fake pointers, in the order EINVAL -> ENOTSUP -> EALIGN: none of these reaches a launch."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(4096)

    def fwd(d, logits=one, labels=one, lse=one, rl=one, out2=one, mean=one, meter=one, bad=one):
        return lib.oeh_xent_fwd(None if d is None else C.byref(d), logits, labels, lse, rl, out2, mean, meter, bad, None)

    def bwd(d, logits=one, labels=one, lse=one, out2=one, grad=one, gs=0, dx=one):
        return lib.oeh_xent_bwd(None if d is None else C.byref(d), logits, labels, lse, out2, grad, gs, dx, None)

    big = dict(B=1 << 16, S=1 << 15)  # B * S = 2^31
    for call in (fwd, bwd):
        assert call(None) == EINVAL and call(_desc(), logits=None) == EINVAL and call(_desc(), labels=None) == EINVAL
        assert call(_desc(), lse=None) == EINVAL and call(_desc(), out2=None) == EINVAL
        assert call(_desc(V=0)) == EINVAL and call(_desc(B=-1)) == EINVAL and call(_desc(S=-1)) == EINVAL
        assert call(_desc(dtype=3)) == EINVAL and call(_desc(dtype=-1)) == EINVAL and call(_desc(label_dtype=2)) == EINVAL
        assert call(_desc(x_stride__0=-1)) == EINVAL and call(_desc(x_stride__1=-1)) == EINVAL and call(_desc(label_stride__1=-1)) == EINVAL
        for ls in (-0.1, 1.0, 1.5, float("nan")):
            assert call(_desc(label_smoothing=ls)) == EINVAL
        assert call(_desc(reserved=1)) == EINVAL
        # OEH_ENOTSUP, behind every OEH_EINVAL and in front of every OEH_EALIGN
        assert call(_desc(**big)) == ENOTSUP and call(_desc(**big, reserved=1)) == EINVAL and call(_desc(**big, label_smoothing=1.0)) == EINVAL
        assert call(_desc(**big), logits=C.c_void_p(4097)) == ENOTSUP and call(_desc(**big), lse=C.c_void_p(4098)) == ENOTSUP
        # OEH_EALIGN, last
        assert call(_desc(), logits=C.c_void_p(4097)) == EALIGN and call(_desc(dtype=2), logits=C.c_void_p(4098)) == EALIGN
        assert call(_desc(), labels=C.c_void_p(4100)) == EALIGN and call(_desc(), lse=C.c_void_p(4098)) == EALIGN
        assert call(_desc(), out2=C.c_void_p(4100)) == EALIGN
        assert call(_desc(reserved=1), logits=C.c_void_p(4097)) == EINVAL
    assert fwd(_desc(label_smoothing=0.1), rl=None) == EINVAL  # the smoothed loss has to be stored
    assert fwd(_desc(), rl=C.c_void_p(4098)) == EALIGN and fwd(_desc(), mean=C.c_void_p(4097)) == EALIGN and fwd(_desc(), meter=C.c_void_p(4100)) == EALIGN
    assert fwd(_desc(), bad=C.c_void_p(4098)) == EALIGN
    assert bwd(_desc(), grad=None) == EINVAL and bwd(_desc(), dx=None) == EINVAL and bwd(_desc(), gs=-1) == EINVAL
    assert bwd(_desc(dx_stride__1=-1)) == EINVAL and bwd(_desc(dx_stride__1=999)) == EINVAL and bwd(_desc(dx_stride__0=999)) == EINVAL
    assert bwd(_desc(**big, dx_stride__1=999)) == EINVAL
    assert bwd(_desc(), grad=C.c_void_p(4098)) == EALIGN and bwd(_desc(), dx=C.c_void_p(4097)) == EALIGN
    # a forward descriptor need not fill dx_stride
    assert lib.oeh_xent_variant(C.byref(_desc(dx_stride__1=0)), one, None) == b"xent/block/CH4/f16"
    assert lib.oeh_xent_variant(C.byref(_desc(dx_stride__1=0)), one, one) is None


def test_launch_form_names_host_only():
    from outeffhop_amd import ops

    v = ops.xent_variant
    assert v(16, 511, 50272) == "xent/block/CH4/f16" and v(32, 128, 30522, torch.bfloat16) == "xent/block/CH4/bf16"
    assert v(1, 1024, 1000, torch.float32, label_smoothing=0.1) == "xent/block/CH4/f32/ls"
    assert v(1, 1, 1) == "xent/block/CH4/f16" and v(0, 5, 7) == "xent/block/CH4/f16"
    assert v(1, 1, 0) is None and v(1, 1, 8, torch.float64) is None and v(1 << 16, 1 << 15, 8) is None and v(1, 1, 8, label_smoothing=1.0) is None
    # the gradient's store form: 16 bytes wide when each of its rows sits as far from a 16-byte boundary as its logits row
    assert v(2, 5, 30522, dx_offset=0) == "xent/block/CH4/f16" and v(2, 5, 30522, offset=3, dx_offset=3) == "xent/block/CH4/f16"
    assert v(2, 5, 30522, offset=3, dx_offset=11) == "xent/block/CH4/f16" and v(2, 5, 30522, dx_offset=1) == "xent/block/CH4/f16/el"
    assert v(2, 5, 30528, dx_offset=0, dx_row_stride=30530) == "xent/block/CH4/f16/el" and v(2, 5, 30528, dx_offset=0, dx_row_stride=30536) == "xent/block/CH4/f16"
    assert v(1, 1, 30528, dx_offset=0, dx_row_stride=30530) == "xent/block/CH4/f16"  # one row: the strides do not matter
    assert v(2, 5, 1000, torch.float32, label_smoothing=0.1, dx_offset=2) == "xent/block/CH4/f32/ls/el"
    assert v(2, 5, 1000, torch.float32, dx_offset=4) == "xent/block/CH4/f32"
    assert v(2, 5, 1000, dx_offset=0, dx_row_stride=999) is None


def test_no_cpu_fallback_in_ops():
    from outeffhop_amd import _lib, ops

    x, y = torch.randn(2, 3, 7), torch.randint(0, 7, (2, 3))
    with pytest.raises(_lib.OehError):
        ops.xent_fwd(x, y)
    with pytest.raises(_lib.OehError):
        ops.xent_bwd(x, y, torch.zeros(6), torch.zeros(2, dtype=torch.float64), torch.ones(1))


def test_torch_path_on_cpu_equals_the_references_lines():
    import outeffhop_amd as P
    from outeffhop_amd import losses, ops

    for name in ("cross_entropy", "FusedCrossEntropyLoss", "causal_lm_loss", "masked_lm_loss", "PerplexityMeter"):
        assert getattr(P, name) is getattr(losses, name)
    assert losses.FUSED_XENT in (True, False)
    torch.manual_seed(0)
    V = 97
    logits = torch.randn(2, 6, V, requires_grad=True)
    labels = torch.randint(0, V, (2, 6))
    labels[0, 3] = -100
    before = ops.XENT_CALLS
    # quantized_opt.py:872-877
    shift_logits = logits[..., :-1, :].contiguous()
    shift_labels = labels[..., 1:].contiguous()
    want = nn.CrossEntropyLoss()(shift_logits.view(-1, V), shift_labels.view(-1))
    got = losses.causal_lm_loss(logits, labels)
    assert torch.equal(got, want)
    g1, = torch.autograd.grad(got, logits)
    g2, = torch.autograd.grad(want, logits)
    assert torch.equal(g1, g2)
    # quantized_bert.py:910-915
    assert torch.equal(losses.masked_lm_loss(logits, labels), nn.CrossEntropyLoss()(logits.view(-1, V), labels.view(-1)))
    # the module: nn.CrossEntropyLoss's constructor, forward and results
    w = torch.rand(V)
    for kw in (dict(weight=w), dict(weight=w, reduction="sum"), dict(label_smoothing=0.1, reduction="none"), dict(size_average=False), dict()):
        a, b = losses.FusedCrossEntropyLoss(**kw), nn.CrossEntropyLoss(**kw)
        assert a.reduction == b.reduction and torch.equal(a(logits.view(-1, V), labels.view(-1)), b(logits.view(-1, V), labels.view(-1)))
        assert a._fused_xent_calls == 0
    probs = torch.softmax(torch.randn(12, V), -1)
    assert torch.equal(losses.FusedCrossEntropyLoss()(logits.view(-1, V), probs), nn.CrossEntropyLoss()(logits.view(-1, V), probs))
    assert "weight" in losses.FusedCrossEntropyLoss(weight=w).state_dict()
    assert torch.equal(losses.cross_entropy(logits, labels, reduction="none"), F.cross_entropy(logits.view(-1, V), labels.view(-1), reduction="none").view(2, 6))
    with pytest.raises(ValueError):
        losses.cross_entropy(logits, labels, reduction="batchmean")
    assert ops.XENT_CALLS == before


def test_perplexity_meter_arithmetic_against_the_host_loop():
    from outeffhop_amd import losses

    means = [3.25, 2.875, 4.0625, 3.5]
    # validate_clm.py:556-594: the per-batch losses, repeated per sample, concatenated, their mean, exp
    per_batch = [torch.tensor(m).repeat(8) for m in means]
    want = math.exp(torch.mean(torch.cat(per_batch)))
    pm = losses.PerplexityMeter()
    for m in means:
        pm.add_mean(m)
    assert pm.state() == (sum(means), 4.0) and pm.perplexity() == want == math.exp(sum(means) / 4)
    pm.add_mean(4000.0)
    assert pm.perplexity() == float("inf")  # OverflowError -> inf, as the reference
    pm.reset()
    assert math.isnan(pm.perplexity())
    # update() on CPU tensors takes the torch path
    torch.manual_seed(1)
    logits, labels = torch.randn(2, 5, 11), torch.randint(0, 11, (2, 5))
    loss = pm.update(logits, labels)
    assert torch.equal(loss, F.cross_entropy(logits[:, :-1].reshape(-1, 11), labels[:, 1:].reshape(-1))) and pm.perplexity() == math.exp(float(loss))


def test_float64_restatement_and_the_bound_of_the_kernels_order():
    """tests/_xent_ref.py against torch's float64 cross-entropy, and where the forward bound comes from: the kernel's order of operations in
    fp32 on the host (256 lanes, sequential fp32 sums, fp32 exp2((x - m) * log2e)) measures at most 1.31 ulp32 of the float64 lse on these inputs and is held to HALF the bound, 2 ulp32 -
    the final M + log(L) and the logarithm round by up to half an ulp each, the rest is the sum's relative error - which leaves the other
    half to the hardware's exponential and logarithm."""
    rng = np.random.default_rng(0)
    x = X.inputs("n8", 6, 211, 1)
    y = rng.integers(0, 211, 6)
    y[2] = -100
    for eps in (0.0, 0.1):
        lse, loss, counted, _ = X.forward64(x, y, eps=eps)
        xt = torch.from_numpy(x).requires_grad_()
        want = F.cross_entropy(xt, torch.from_numpy(y), label_smoothing=eps, reduction="none")
        assert np.allclose(loss, want.detach().numpy(), rtol=1e-13, atol=1e-13) and list(counted) == [True, True, False, True, True, True]
        g = rng.standard_normal(6)
        (want * torch.from_numpy(g)).sum().backward()
        d, p = X.backward64(x, y, g, eps=eps)
        assert np.allclose(d, xt.grad.numpy(), rtol=1e-12, atol=1e-15) and np.allclose(p.sum(axis=1), 1.0)
    bad = X.forward64(x, np.array([0, 211, -1, 3, 4, 5]))
    assert np.isnan(bad[1][[1, 2]]).all() and bad[2].all()
    worst = 0.0
    for kind, V in (("n1", 1000), ("n8", 1000), ("t3", 1000), ("spike", 1000), ("n8", 30522)):
        x32 = X.inputs(kind, 1, V, 7)[0].astype(np.float32)
        lse64 = X.forward64(x32[None].astype(np.float64), [0])[0][0]
        worst = max(worst, abs(float(X.emulate_lse32(x32)) - lse64) / float(np.spacing(np.float32(lse64))))
    assert worst <= 2.0, worst


def test_the_smoothing_sum_check_sees_one_dropped_element():
    """tests/_xent_ref.py: smoothing_sum_error on the expression itself - an exact sum(x) / V passes at 0, a sum that lost ONE element of
    30522 (an error of about 40 times the 2^-20 mean|x| the kernel is held to) does not."""
    f = np.float32
    x = X.inputs("n1", 4, 30522, 11).astype(np.float16).astype(np.float64)
    y = np.array([5, 17, 30521, 0])
    counted = np.ones(4, bool)
    lse32 = X.forward64(x, y)[0].astype(f)
    xy = x[np.arange(4), y].astype(f)

    def loss32(sums):
        b = (lse32 - (sums / 30522).astype(f)).astype(f)
        return (((f(1.0) - f(0.1)) * (lse32 - xy).astype(f)).astype(f) + (f(0.1) * b).astype(f)).astype(f)

    assert X.smoothing_sum_error(lse32, loss32(x.sum(axis=1)), x, y, counted, 0.1) == 0.0
    big = np.abs(x).argmax(axis=1)
    assert X.smoothing_sum_error(lse32, loss32(x.sum(axis=1) - x[np.arange(4), big]), x, y, counted, 0.1) > 1.0
