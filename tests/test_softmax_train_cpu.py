"""The differentiable row softmax (include/oeh.h: oeh_softmax_train_fwd / oeh_softmax_train_bwd) without a GPU: header, binding and struct
layout, every refusal in its order, the launch-form names, the routing of softmax.masked_softmax, and the float64 yardstick of the GPU tests."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _softmax_train_ref as T

torch = pytest.importorskip("torch")
nn = torch.nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "oeh.h")
NEW = ("oeh_softmax_train_fwd", "oeh_softmax_train_bwd", "oeh_softmax_train_variant")
EINVAL, ENOTSUP = -22, -95


def test_header_binding_and_struct_layout_agree(tmp_path):
    from outeffhop_amd import _lib, ops

    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(oeh_[a-z0-9_]+)\s*\(", txt))
    assert set(NEW) <= declared and declared == set(_lib.EXPORTS)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW) and lib.oeh_abi_version() == 6
    assert int(re.search(r"#define OEH_SOFTMAX_TRAIN_MAX_COLS (\d+)", txt).group(1)) == _lib.SOFTMAX_TRAIN_MAX_COLS == ops.SOFTMAX_TRAIN_MAX_COLS == 15872
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    st = _lib.oeh_softmax_train_desc
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HDR}"', "int main(void) {", '  printf("size %zu\\n", sizeof(oeh_softmax_train_desc));']
    lines += [f'  printf("{f} %zu\\n", offsetof(oeh_softmax_train_desc, {f}));' for f, _ in st._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], check=True, capture_output=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(out[f]) == getattr(st, f).offset, f


def _desc(B=2, H=3, Sq=5, Sk=24, x_dtype=2, y_dtype=None, mask_dtype=-1, p=0.0, **kw):
    from outeffhop_amd import _lib

    d = _lib.oeh_softmax_train_desc()
    d.B, d.H, d.Sq, d.Sk = B, H, Sq, Sk
    d.x_dtype, d.y_dtype, d.mask_dtype = x_dtype, x_dtype if y_dtype is None else y_dtype, mask_dtype
    d.softmax_base, d.scale, d.eta = 1, 1.0, 1.0
    st = (H * Sq * Sk, Sq * Sk, Sk)
    for f in ("x", "y", "u", "mask", "dy", "du", "dx"):
        setattr(d, f + "_stride", st)
    d.drop.p = p
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _calls():
    from outeffhop_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(4096)
    ref = lambda d: None if d is None else C.byref(d)  # noqa: E731

    def fwd(d, x=one, mask=None, y=one, u=None, stats=one):
        return lib.oeh_softmax_train_fwd(ref(d), x, mask, y, u, stats, None)

    def bwd(d, x=one, mask=None, stats=one, dy=one, du=None, dx=one):
        return lib.oeh_softmax_train_bwd(ref(d), x, mask, stats, dy, du, dx, None)

    def var(d, backward=0):
        return lib.oeh_softmax_train_variant(ref(d), backward)

    return lib, fwd, bwd, var, one


def test_every_refusal_in_its_order_without_gpu():
    lib, fwd, bwd, var, one = _calls()
    nan = float("nan")
    for call in (fwd, bwd):
        assert call(None) == EINVAL
        # the dropout checks come first: before a NULL pointer, before ENOTSUP
        for p in (-0.1, 1.0, 1.5, nan):
            assert call(_desc(p=p)) == EINVAL and call(_desc(p=p, Sk=20000)) == EINVAL and var(_desc(p=p)) is None
        d = _desc()
        d.drop.reserved = 1
        assert call(d) == EINVAL and var(d) is None
        assert call(_desc(reserved=1)) == EINVAL and var(_desc(reserved=1)) is None
        # required pointers
        assert call(_desc(), x=None) == EINVAL and call(_desc(), stats=None) == EINVAL
        # dtypes
        for bad in (3, 7, -1):
            assert call(_desc(x_dtype=bad)) == EINVAL
        assert call(_desc(x_dtype=0, y_dtype=1)) == EINVAL and call(_desc(x_dtype=2, y_dtype=0)) == EINVAL
        assert call(_desc(mask_dtype=5), mask=one) == EINVAL
        assert var(_desc(x_dtype=0, y_dtype=1)) is None
        # extents and strides
        assert call(_desc(Sk=0)) == EINVAL and call(_desc(B=-1)) == EINVAL and call(_desc(Sq=-1)) == EINVAL and call(_desc(H=-2)) == EINVAL
        for f in ("x", "y", "u", "mask", "dy", "du", "dx"):
            assert call(_desc(**{f + "_stride": (360, 120, -24)})) == EINVAL, f
        # the softmax, the clip, the scale
        assert call(_desc(softmax_base=2)) == EINVAL and call(_desc(softmax_base=-1)) == EINVAL
        assert call(_desc(clip=1, gamma=0.0, eta=0.0)) == EINVAL and call(_desc(clip=1, gamma=0.5, eta=0.25)) == EINVAL
        assert call(_desc(scale_div=-1.0)) == EINVAL and call(_desc(scale_div=nan)) == EINVAL
        assert call(_desc(scale=nan)) == EINVAL and call(_desc(gamma=nan)) == EINVAL and call(_desc(eta=nan)) == EINVAL
        # EINVAL before ENOTSUP
        assert call(_desc(Sk=15873)) == ENOTSUP and call(_desc(Sk=15873, softmax_base=2)) == EINVAL
        assert call(_desc(B=2 ** 15, H=2 ** 8, Sq=2 ** 8)) == ENOTSUP and var(_desc(B=2 ** 15, H=2 ** 8, Sq=2 ** 8)) is None
        assert var(_desc(Sk=15873)) is None and var(_desc(Sk=15872)) is not None
        # nothing to do: no launch, no device needed
        assert call(_desc(B=0)) == 0 and call(_desc(B=0, Sk=15872)) == 0 and call(_desc(B=0, Sk=15873)) == ENOTSUP
    # forward: at least one output, u only with dropout; its outputs' strides
    assert fwd(_desc(), y=None) == EINVAL and fwd(_desc(), u=one) == EINVAL and fwd(_desc(p=0.5, B=0), y=None, u=one) == 0
    assert fwd(_desc(p=0.5), y=None, u=None) == EINVAL
    assert fwd(_desc(y_stride=(360, 120, 8))) == EINVAL and fwd(_desc(p=0.5, u_stride=(360, 8, 24)), u=one) == EINVAL
    assert fwd(_desc(B=0, u_stride=(360, 120, 8))) == 0  # (u is not given: its stride is nobody's)
    # backward: dx, at least one gradient, du only with dropout; dx's stride
    assert bwd(_desc(), dx=None) == EINVAL and bwd(_desc(), dy=None) == EINVAL and bwd(_desc(), du=one) == EINVAL
    assert bwd(_desc(p=0.5, B=0), dy=None, du=one) == 0 and bwd(_desc(dx_stride=(8, 120, 24))) == EINVAL
    assert bwd(_desc(B=0, y_stride=(360, 120, 8))) == 0
    # an input's stride below Sk is no refusal: rows may repeat (a broadcast mask has stride 0)
    assert fwd(_desc(B=0, x_stride=(0, 0, 0), mask_stride=(0, 0, 0), mask_dtype=2), mask=one) == 0


def _variant(Sk, dtype=None, **kw):
    from outeffhop_amd import ops

    return ops.softmax_train_variant(2, 3, 5, Sk, torch.float16 if dtype is None else dtype, **kw)


def test_launch_form_names_host_only():
    from outeffhop_amd.ops import SoftmaxSpec

    f16, bf16, f32 = torch.float16, torch.bfloat16, torch.float32
    # (a) short rows: lanes per row x elements per lane; 16-byte vectors where Sk is a multiple of one
    assert _variant(8) == "softmax_train/fwd/lanes/G1x8/f16/softmax1"
    assert _variant(24) == "softmax_train/fwd/lanes/G4x8/f16/softmax1"
    assert _variant(24, f32) == "softmax_train/fwd/lanes/G8x4/f32/softmax1"
    assert _variant(64, f32) == "softmax_train/fwd/lanes/G16x4/f32/softmax1" and _variant(64, bf16) == "softmax_train/fwd/lanes/G8x8/bf16/softmax1"
    assert _variant(1) == "softmax_train/fwd/lanes/G1x1/f16/softmax1" and _variant(3, f32) == "softmax_train/fwd/lanes/G4x1/f32/softmax1"
    assert _variant(7) == "softmax_train/fwd/lanes/G8x1/f16/softmax1" and _variant(63, f32) == "softmax_train/fwd/lanes/G64x1/f32/softmax1"
    assert _variant(24, row_stride=28) == "softmax_train/fwd/lanes/G32x1/f16/softmax1"  # rows off 16 bytes
    # ... and rows of up to 32 vectors, which would leave most of a wave idle
    assert _variant(72) == "softmax_train/fwd/lanes/G16x8/f16/softmax1" and _variant(128) == "softmax_train/fwd/lanes/G16x8/f16/softmax1"
    assert _variant(256) == "softmax_train/fwd/lanes/G32x8/f16/softmax1" and _variant(128, f32) == "softmax_train/fwd/lanes/G32x4/f32/softmax1"
    # (b) one wave per row: up to 512 vectors
    assert _variant(264) == "softmax_train/fwd/wave/CH1/f16/softmax1" and _variant(512) == "softmax_train/fwd/wave/CH1/f16/softmax1"
    assert _variant(520) == "softmax_train/fwd/wave/CH2/f16/softmax1" and _variant(1024) == "softmax_train/fwd/wave/CH2/f16/softmax1"
    assert _variant(1032) == "softmax_train/fwd/wave/CH4/f16/softmax1" and _variant(2048) == "softmax_train/fwd/wave/CH4/f16/softmax1"
    assert _variant(2056) == "softmax_train/fwd/wave/CH8/f16/softmax1" and _variant(4096) == "softmax_train/fwd/wave/CH8/f16/softmax1"
    assert _variant(132, f32) == "softmax_train/fwd/wave/CH1/f32/softmax1" and _variant(256, f32) == "softmax_train/fwd/wave/CH1/f32/softmax1"
    assert _variant(260, f32) == "softmax_train/fwd/wave/CH2/f32/softmax1" and _variant(2048, f32) == "softmax_train/fwd/wave/CH8/f32/softmax1"
    # (c) a workgroup per row
    assert _variant(65) == _variant(76) == _variant(4104) == _variant(15872) == "softmax_train/fwd/block/f16/softmax1"
    assert _variant(2052, f32) == "softmax_train/fwd/block/f32/softmax1" and _variant(72, row_stride=76) == "softmax_train/fwd/block/f16/softmax1"
    assert _variant(15873) is None
    # the rest of the name
    name = _variant(128, backward=True, spec=SoftmaxSpec(0, True, -0.025, 1.0), out_dtype=f32, mask_dtype=f32, clamp=True, p=0.1)
    assert name == "softmax_train/bwd/lanes/G16x8/f16>f32/softmax/clip/mask/clamp/drop"
    assert _variant(128, p=1.0) is None and _variant(128, spec=SoftmaxSpec(1, True, 0.5, 0.5)) is None


def test_keep_mask_restatement_is_the_attention_stream():
    from tests import test_attn_dropout_cpu as A

    for (B, H, Sq, Sk, p, seed) in ((2, 3, 5, 7, 0.1, 1234), (1, 2, 3, 24, 0.5, 2 ** 63 + 17), (1, 1, 2, 65, 0.9, 0)):
        assert np.array_equal(T.keep_mask(B, H, Sq, Sk, p, seed), A.keep_mask(B, H, Sq, Sk, p, seed))
    assert T.keep_mask(1, 2, 3, 9, 0.0, 5).all()
    assert tuple(int(x) for x in T.philox4x32_10(0, 0, 0, 0, 0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert T.inv_of(0.5) == 2.0 and T.inv_of(0.1) == float(np.float32(1) / np.float32(0.9))


def _chain64(x, mask, base, clip, gamma, eta, scale, scale_div, floor):
    s = x / scale_div if scale_div else x * scale
    if mask is not None:
        s = s + mask
    if floor is not None:
        s = torch.max(s, torch.tensor(floor, dtype=torch.float64))
    if base == 1:
        m = s.max(dim=-1, keepdim=True).values
        e = torch.exp(s - m)
        p = e / (e.sum(dim=-1, keepdim=True) + torch.exp(-m))
    else:
        p = torch.softmax(s, dim=-1)
    if clip:
        p = torch.clip(p * (eta - gamma) + gamma, 0, 1)
    return p


@pytest.mark.parametrize("base", (0, 1))
@pytest.mark.parametrize("clip", (False, True))
def test_float64_helper_is_the_gradient_of_the_op_chain(base, clip):
    """A self-check of the GPU tests' yardstick, not of the feature: forward() / backward() of tests/_softmax_train_ref.py against torch's
    float64 autograd of the op chain, with mask, clamp, dropout and both gradients."""
    rs = np.random.RandomState(7 + base + 2 * clip)
    B, H, Sq, Sk = 2, 3, 5, 24
    x = 3.0 * rs.standard_normal((B, H, Sq, Sk))
    mask = np.where(rs.rand(B, 1, Sq, Sk) < 0.3, -1e4, 0.0)
    dy, du = rs.standard_normal(x.shape), rs.standard_normal(x.shape)
    keep = T.keep_mask(B, H, Sq, Sk, 0.25, 99)
    c = T.Call(base=base, clip=clip, gamma=-0.5, eta=1.25, scale=0.5, clamp_min=-9000.0, p=0.25, seed=99)
    f = T.forward(c, x, mask)
    tx = torch.tensor(x, requires_grad=True)
    y = _chain64(tx, torch.tensor(mask), base, clip, c.gamma, c.gamma + c.w, c.scale, 0.0, c.clamp_min)
    assert np.abs(y.detach().numpy() - f["y"]).max() < 1e-15
    u = torch.where(torch.from_numpy(keep), y * c.inv, torch.zeros((), dtype=torch.float64))
    ((y * torch.tensor(dy)).sum() + (u * torch.tensor(du)).sum()).backward()
    dx, _ = T.backward(c, f, dy, du, keep)
    assert np.abs(dx - tx.grad.numpy()).max() < 3e-15
    c2 = T.Call(base=base, clip=clip, gamma=-0.5, eta=1.25, scale_div=8.0)
    f2 = T.forward(c2, x)
    tx = torch.tensor(x, requires_grad=True)
    y = _chain64(tx, None, base, clip, c2.gamma, c2.gamma + c2.w, 1.0, 8.0, None)
    (y * torch.tensor(dy)).sum().backward()
    assert np.abs(T.backward(c2, f2, dy)[0] - tx.grad.numpy()).max() < 3e-15


def test_half_gate_at_a_tie_and_the_closed_clip_interval():
    """The two conventions the kernels share with torch: max(z, floor) passes 1/2 of the gradient at a tie, and torch.clip's gradient is 1 on
    the CLOSED interval - checked on the yardstick against torch's float64 autograd."""
    floor = -8.0
    x = np.array([[[[-8.0, -9.0, 1.0, -8.0, 0.5, -7.5]]]])
    dy = np.array([[[[1.0, 2.0, -1.0, 0.5, 0.25, 3.0]]]])
    c = T.Call(base=0, clamp_min=floor)
    tx = torch.tensor(x, requires_grad=True)
    (_chain64(tx, None, 0, False, 0, 1, 1.0, 0.0, floor) * torch.tensor(dy)).sum().backward()
    dx, _ = T.backward(c, T.forward(c, x), dy)
    assert np.abs(dx - tx.grad.numpy()).max() < 1e-16
    z = np.maximum(x, floor)
    pz = np.exp(z - z.max()) / np.exp(z - z.max()).sum()
    full = pz * (dy - (pz * dy).sum())
    assert np.allclose(dx[..., 0], 0.5 * full[..., 0], rtol=1e-13) and dx[0, 0, 0, 1] == 0.0 and np.allclose(dx[..., 5], full[..., 5], rtol=1e-13)
    # the clip: a row whose probabilities are exactly 1/2, 1/4, 1/4 with w = 2, gamma = -1/2: t = 1/2, 0, 0 - the two zeros sit ON the boundary
    x = np.log(np.array([[[[2.0, 1.0, 1.0]]]]))
    dy = np.array([[[[1.0, 5.0, -3.0]]]])
    c = T.Call(base=0, clip=True, gamma=-0.5, eta=1.5)
    f = T.forward(c, x)
    assert np.array_equal(f["t"], np.array([[[[0.5, 0.0, 0.0]]]]))
    tx = torch.tensor(x, requires_grad=True)
    (_chain64(tx, None, 0, True, -0.5, 1.5, 1.0, 0.0, None) * torch.tensor(dy)).sum().backward()
    dx, _ = T.backward(c, f, dy)
    assert np.abs(dx - tx.grad.numpy()).max() < 1e-16 and np.abs(dx[..., 1:]).min() > 0.1  # the boundary elements carry gradient


class _Gpu(torch.Tensor):  # a CPU tensor that says it is on the GPU: _kernel_covers looks at metadata only
    is_cuda = True


def test_kernel_covers_routes():
    from outeffhop_amd import softmax as S

    mk = lambda *shape, dtype=torch.float16: torch.zeros(*shape, dtype=dtype).as_subclass(_Gpu)  # noqa: E731
    x = mk(2, 3, 5, 24)
    cov = lambda *a, **k: S._kernel_covers(*a, capturing=k.pop("capturing", False), **k)  # noqa: E731
    assert cov(x, None) and cov(x, mk(2, 1, 1, 24)) and cov(x, mk(2, 1, 5, 24, dtype=torch.float32)) and cov(x, mk(1, 1, 5, 24, dtype=torch.bfloat16))
    assert cov(x, mk(2, 1, 5, 24).expand(2, 3, 5, 24))                              # stride 0 over the heads
    assert cov(mk(6, 24, dtype=torch.float32), None) and cov(mk(24, 6), None, 0) and cov(mk(4, 2, 3, 5, 24), None, -1)
    assert not cov(torch.zeros(2, 3, 5, 24), None)                                  # a CPU tensor
    assert not cov(mk(2, 3, 5, 24, dtype=torch.float64), None)                      # float64
    assert not cov(x, mk(2, 1, 1, 24).requires_grad_())                             # a mask that wants a gradient
    assert not cov(x, mk(2, 1, 24, 5).transpose(2, 3))                              # a mask whose last stride is not 1
    assert not cov(x, mk(2, 1, 5, 1)) and not cov(x, mk(2, 2, 5, 24)) and not cov(x, mk(5, 24))
    assert not cov(x, torch.zeros(2, 1, 1, 24, dtype=torch.bool).as_subclass(_Gpu))
    assert not cov(mk(6, 24), mk(6, 24)) and not cov(x, mk(2, 1, 1, 5), 2)          # a mask only with 4-D scores and the last dimension
    assert cov(mk(2, 15872), None) and not cov(mk(2, 15873), None)                  # the staged limit
    assert not cov(mk(0, 24).reshape(0, 0), None) and not cov(x, None, 4)
    assert cov(x, None, -1, 0.5) and not cov(x, None, -1, 0.5, capturing=True) and cov(x, None, -1, 0.0, capturing=True)
    assert not cov(x, None, -1, 1.0) and not cov(x, None, -1, -0.1)
    prev = S.set_fused_softmax_train(True)
    assert prev is False and S.FUSED_SOFTMAX_TRAIN is True and S.set_fused_softmax_train(prev) is True and S.FUSED_SOFTMAX_TRAIN is False


def _callers(S):
    return (S.softmax_1, S.SOFTMAX_MAPPING["vanilla"], S.SOFTMAX_MAPPING["clippedsoftmax1(-.025:1)"], S.SOFTMAX_MAPPING["clipped(-.1:1)"],
            lambda x, dim=-1: S.clipped_softmax(x, dim), lambda x, dim=-1: S.clipped_softmax1(x, dim, 1.03, -0.03),
            S.Softmax_1(-1), S.ClipSoftmax(-1), S.ClipSoftmax_1(-1, 1.1, -0.025))


def test_switch_off_nobody_reaches_the_new_ops(monkeypatch):
    from outeffhop_amd import attention as A, ops, softmax as S

    def boom(*a, **k):
        raise AssertionError("the new ops were reached with the switch off")

    monkeypatch.setattr(ops, "softmax_train_fwd", boom)
    monkeypatch.setattr(ops, "softmax_train_bwd", boom)
    monkeypatch.setattr(S, "masked_softmax", boom)
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts, allow_grad=False: None)  # (CPU tensors through the torch-op forms)
    assert S.FUSED_SOFTMAX_TRAIN is False
    before = dict(S.CALLS)
    x = torch.randn(2, 3, 5, 24, requires_grad=True)
    for fn in _callers(S):
        fn(x, dim=-1).sum().backward() if not isinstance(fn, nn.Module) else fn(x).sum().backward()
    q, k, v = (torch.randn(2, 2, 6, 8, requires_grad=True) for _ in range(3))
    mask = torch.zeros(2, 1, 1, 6)
    ctx, probs, used = A.unfused_core(q, k, v, softmax_fn=S.softmax_1, scale_div=2.0, attention_mask=mask, clamp_min=True, dropout=nn.Dropout(0.1))
    ctx.sum().backward()
    assert q.grad is not None and S.CALLS == before


def _stub_ops(monkeypatch, ops):
    """ops.softmax_train_fwd / _bwd as CPU functions with the library's interface, from the float64 yardstick."""
    dt = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}
    seen = []

    def call(spec, kw):
        return T.Call(base=spec.base, clip=spec.clip, gamma=spec.gamma, eta=spec.eta, scale=kw.get("scale", 1.0), scale_div=kw.get("scale_div", 0.0),
                      clamp_min=kw.get("clamp_min"), p=kw.get("p", 0.0), seed=kw.get("seed") or 0)

    def fwd(x, spec, *, mask=None, out_dtype=None, want_y=True, **kw):
        assert x.dim() == 4 and not x.requires_grad
        c = call(spec, kw)
        f = T.forward(c, x.double().numpy(), None if mask is None else mask.double().numpy())
        od = x.dtype if out_dtype is None else out_dtype
        y = torch.from_numpy(f["y"]).to(od)
        u = None
        if c.p > 0:
            keep = T.keep_mask(*x.shape, c.p, c.seed)
            u = torch.from_numpy(T.dropped(c, y.double().numpy(), keep)).to(od)
        stats = torch.from_numpy(np.concatenate([f["m"], f["den"]], axis=-1)).float()
        seen.append(("fwd", dict(kw, mask=mask, out_dtype=od, want_y=want_y)))
        return (y if want_y else None), u, stats

    def bwd(x, stats, dy, du, spec, *, mask=None, **kw):
        c = call(spec, kw)
        f = T.forward(c, x.double().numpy(), None if mask is None else mask.double().numpy())
        keep = T.keep_mask(*x.shape, c.p, c.seed) if c.p > 0 else None
        dx, _ = T.backward(c, f, None if dy is None else dy.double().numpy(), None if du is None else du.double().numpy(), keep)
        seen.append(("bwd", dict(kw, dy=dy is not None, du=du is not None)))
        return torch.from_numpy(dx).to(x.dtype)

    monkeypatch.setattr(ops, "softmax_train_fwd", fwd)
    monkeypatch.setattr(ops, "softmax_train_bwd", bwd)
    return seen


def test_switch_on_routes_through_one_function(monkeypatch):
    """The Python layers with the device calls stubbed (CPU tensors, the float64 yardstick behind the ops' interface): every registry
    caller and unfused_core reach masked_softmax, gradients flow, and what is not covered runs the op chain."""
    from outeffhop_amd import attention as A, ops, softmax as S

    seen = _stub_ops(monkeypatch, ops)
    monkeypatch.setattr(ops, "_need_gpu", lambda *ts, allow_grad=False: None)
    real_covers = S._kernel_covers
    monkeypatch.setattr(S, "_kernel_covers", lambda s, m, dim=-1, p=0.0, capturing=None: real_covers(s.as_subclass(_Gpu), None if m is None else m.as_subclass(_Gpu), dim, p, capturing=False))
    monkeypatch.setattr(S, "FUSED_SOFTMAX_TRAIN", True)
    before = dict(S.CALLS)
    x = torch.randn(2, 3, 5, 24, requires_grad=True)
    n = 0
    for fn in _callers(S):
        S.FUSED_SOFTMAX_TRAIN = False
        want = fn(x) if isinstance(fn, nn.Module) else fn(x, dim=-1)
        gw, = torch.autograd.grad(want.square().sum(), x)
        S.FUSED_SOFTMAX_TRAIN = True
        got = fn(x) if isinstance(fn, nn.Module) else fn(x, dim=-1)
        gg, = torch.autograd.grad(got.square().sum(), x)
        n += 1
        assert torch.allclose(got, want, atol=2e-7) and torch.allclose(gg, gw, atol=1e-6)
        assert S.CALLS["forward"] == before["forward"] + n and S.CALLS["backward"] == before["backward"] + n
    # another dim, another rank: moved last and viewed as rows
    xt = torch.randn(6, 24, 3, requires_grad=True)
    got = S.softmax_1(xt, dim=1)
    want = S.softmax_autograd(xt, S.softmax_1.spec, 1)
    assert got.shape == want.shape and torch.allclose(got, want, atol=2e-7)
    assert torch.allclose(torch.autograd.grad(got[..., 0].sum() + 2 * got[:, 3].sum(), xt)[0], torch.autograd.grad(want[..., 0].sum() + 2 * want[:, 3].sum(), xt)[0], atol=1e-6)
    # without autograd the registry callable still runs the forward-only row kernel: not this function
    # unfused_core: one call for the span, the module's nn.Dropout behind it unless FUSED_DROPOUT is on as well
    q, k, v = (torch.randn(2, 2, 6, 8, requires_grad=True) for _ in range(3))
    mask = torch.where(torch.rand(2, 1, 6, 6) < 0.3, torch.finfo(torch.float32).min, 0.0)
    kw = dict(softmax_fn=S.SOFTMAX_MAPPING["clippedsoftmax1(-.025:1)"], scale_div=2.0, attention_mask=mask, clamp_min=True)
    S.FUSED_SOFTMAX_TRAIN = False
    c0, p0, u0 = A.unfused_core(q, k, v, **kw)
    g0 = torch.autograd.grad(c0.square().sum(), (q, k, v))
    S.FUSED_SOFTMAX_TRAIN = True
    del seen[:]
    c1, p1, u1 = A.unfused_core(q, k, v, **kw)
    g1 = torch.autograd.grad(c1.square().sum(), (q, k, v))
    assert [s[0] for s in seen] == ["fwd", "bwd"] and seen[0][1]["scale_div"] == 2.0 and seen[0][1]["clamp_min"] == torch.finfo(torch.float32).min
    assert torch.allclose(c1, c0, atol=1e-6) and torch.allclose(p1, p0, atol=1e-6) and u1 is p1
    assert all(torch.allclose(a, b, atol=1e-5) for a, b in zip(g1, g0))
    # hooks on scores_tap, a quantiser, a callable without a spec: today's chain
    tap = nn.Identity()
    tap.register_forward_hook(lambda m, i, o: None)
    del seen[:]
    A.unfused_core(q, k, v, scores_tap=tap, **kw)
    A.unfused_core(q, k, v, fq_probs=lambda t: t, **kw)
    A.unfused_core(q, k, v, **dict(kw, softmax_fn=lambda t, dim=-1: torch.softmax(t, dim)))
    # (the registry callable inside the chain still takes the kernels for the softmax alone: no scale, no mask, no clamp in those calls)
    assert [s[0] for s in seen] == ["fwd", "fwd"] and all(s[1]["mask"] is None and s[1]["clamp_min"] is None and s[1]["scale_div"] == 0.0 for s in seen)
    # dropout: nn.Dropout's stream unless FUSED_DROPOUT; then the kernel's, and need_probs=False skips probs
    drop = nn.Dropout(0.5)
    A.unfused_core(q, k, v, dropout=drop, **kw)
    assert seen[-1][1]["p"] == 0.0
    monkeypatch.setattr(A, "FUSED_DROPOUT", True)
    c2, p2, u2 = A.unfused_core(q, k, v, dropout=drop, need_probs=False, **kw)
    assert seen[-1][1]["p"] == 0.5 and seen[-1][1]["want_y"] is False and p2 is None and (u2 == 0).any()
    torch.autograd.grad(c2.sum(), q)
    assert seen[-1][0] == "bwd" and seen[-1][1] == dict(scale=1.0, scale_div=2.0, clamp_min=torch.finfo(torch.float32).min, p=0.5, seed=seen[-1][1]["seed"], dy=False, du=True)
    hooked = nn.Identity()
    hooked.register_forward_hook(lambda m, i, o: None)
    A.unfused_core(q, k, v, dropout=drop, probs_tap=hooked, **kw)
    assert seen[-1][1]["p"] == 0.0
    drop.eval()
    c3, p3, u3 = A.unfused_core(q, k, v, dropout=drop, **kw)
    assert seen[-1][1]["p"] == 0.0 and u3 is p3
    # not covered: the chain, counted
    t0 = S.CALLS["torch"]
    probs, used = S.masked_softmax(torch.randn(2, 24, dtype=torch.float64, requires_grad=True), S.softmax_1.spec)
    assert S.CALLS["torch"] == t0 + 1 and used is probs and probs.requires_grad
    # the OPT upcast wrapper keeps its spec
    up = S.UpcastSoftmax(S.softmax_1, torch.float16)
    assert S.spec_of(up) == S.softmax_1.spec
    S.FUSED_SOFTMAX_TRAIN = False
    h = torch.randn(2, 2, 6, 6).half().requires_grad_()  # (under autograd: the torch-op form, which a CPU tensor can take)
    want = up(h + mask)  # an fp32 mask promotes the fp16 scores; the callable form still returns fp16
    assert want.dtype == torch.float16 and torch.equal(want, S.softmax_autograd((h + mask).float(), S.softmax_1.spec).half())
    S.FUSED_SOFTMAX_TRAIN = True
    qh, kh, vh = (torch.randn(2, 2, 6, 8).half().requires_grad_() for _ in range(3))
    _, ph, uh = A.unfused_core(qh, kh, vh, softmax_fn=up, attention_mask=mask, clamp_min=True)
    assert ph.dtype == torch.float16 and uh.dtype == torch.float16 and seen[-1][1]["out_dtype"] == torch.float32
    assert A._dropout_p(drop) == 0.0 and A._dropout_p(nn.Dropout(0.25)) == 0.25 and A._dropout_p(lambda t: t) is None


def test_ops_raise_on_cpu_tensors():
    from outeffhop_amd import _lib, ops, softmax as S

    x = torch.zeros(1, 1, 2, 8)
    with pytest.raises(_lib.OehError):
        ops.softmax_train_fwd(x)
    with pytest.raises(_lib.OehError):
        ops.softmax_train_bwd(x, torch.zeros(1, 1, 2, 2), x, None)
    with pytest.raises(_lib.OehError):
        S.masked_softmax(x.requires_grad_(), S.softmax_1.spec)  # not covered -> the chain -> raises as the registry callables do
