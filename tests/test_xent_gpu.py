"""The cross-entropy kernels (oeh_xent.hip: oeh_xent_fwd / oeh_xent_bwd) on the GPU against float64 on the same stored inputs: every V at
which the row loop takes another path, rows that start at every residue of the 16-byte grid, padded strides, both label types, the three
storage types, label smoothing, the three reductions, the gradient through autograd, aliasing and the element-store form, ignored rows,
labels that are none (with guard regions round every buffer), infinities against torch, determinism, the device meter and the switch.

The bounds are tests/_xent_ref.py's: 4 ulp32 of the float64 lse, half an fp32 ulp more for the loss, and for the gradient
|g| (2^-15 p + 2^-24) plus half an ulp of the storage type.  Every accuracy test prints its measured worst case before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _xent_ref as X
from tests._ln_ref import ulp_of

torch = pytest.importorskip("torch")
F = torch.nn.functional
pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
NAMES = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}
KINDS = ("n1", "n8", "t3", "spike")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64 if t.dtype == torch.float64 else torch.int16).numpy()


def _step(ops, dtype):
    """T: the elements one loop step of the workgroup covers, from the variant's CH."""
    ch = int(ops.xent_variant(1, 1, 8, dtype).split("/")[2][2:])
    return 256 * ch * (4 if dtype == torch.float32 else 8)


def _place(x64, dtype, offset=0, pad=0):
    """The values as a (1, rows, V) GPU view of `dtype` that starts `offset` elements into its buffer, rows V + pad elements apart."""
    rows, V = x64.shape
    buf = torch.full((offset + rows * (V + pad) + 8,), 7.0, dtype=dtype, device="cuda")
    view = buf[offset:offset + rows * (V + pad)].view(rows, V + pad)[:, :V]
    view.copy_(torch.from_numpy(x64).to(dtype))
    return view[None], buf


def _labels(rows, V, seed, dtype=torch.int64, ignore=()):
    y = torch.from_numpy(np.random.default_rng(seed).integers(0, V, rows))
    for r in ignore:
        y[r] = -100
    return y.to(dtype)


def _check_forward(ops, x, y, eps, tag):
    """One forward call against float64 on the stored values; returns (worst lse error, worst loss error) in ulp32 of the reference."""
    mean, out2, lse, rl = ops.xent_fwd(x, y.cuda()[None], label_smoothing=eps, want_rows=True)
    xs = x[0].float().cpu().double().numpy()
    lse64, loss64, counted, sxv = X.forward64(xs, y.numpy(), eps=eps)
    lse, rl, out2, mean = lse.cpu().double().numpy(), rl.cpu().double().numpy(), out2.cpu().numpy(), float(mean)
    e_lse = np.abs(lse - lse64) / ulp_of(lse64, "float32")
    bound = X.loss_bound(lse64, loss64)  # (with smoothing too: the same bound, nothing added)
    if eps > 0:
        e_sum = X.smoothing_sum_error(lse.astype(np.float32), rl.astype(np.float32), xs, y.numpy(), counted, eps)
        print(f"{tag}: max |loss - fp32 expression on the float64 sum(x) / V| / what a 2^-20 mean|x| error of sum(x) / V can move it = {e_sum:.3f}")
        assert e_sum <= 1.0, tag
    e_loss = np.abs(rl - loss64) / bound
    print(f"{tag}: max |lse - lse64| = {e_lse.max():.3f} ulp32, max |loss - loss64| / bound = {e_loss.max():.3f}")
    assert (e_lse <= 4.0).all() and (e_loss <= 1.0).all(), tag
    assert (lse[~counted] == 0).all() and (rl[~counted] == 0).all()
    want = rl[counted].sum()  # the float64 sum of the returned fp32 row losses
    assert abs(out2[0] - want) <= 1e-12 * abs(want) and out2[1] == counted.sum()
    assert mean == np.float32(out2[0] / out2[1])
    return float(e_lse.max()), float(e_loss.max())


@pytest.mark.parametrize("eps", (0.0, 0.1))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_forward_every_row_length(ops, dt, eps):
    dtype, T = DTYPES[dt], _step(ops, DTYPES[dt])
    assert ops.xent_variant(2, 3, 77, dtype, label_smoothing=eps) == f"xent/block/CH{ops.XENT_SLOTS}/{dt.replace('fp', 'f')}{'/ls' if eps else ''}"
    for i, V in enumerate((1, 7, 8, 9, T - 1, T, T + 1, 2 * T + 3)):
        x, _ = _place(X.inputs(KINDS[i % 4], 3, V, 10 + i), dtype, offset=i % 8, pad=(0, 5)[i % 2])
        y = _labels(3, V, i, (torch.int64, torch.int32)[i % 2], ignore=(1,) if i % 3 == 0 else ())
        _check_forward(ops, x, y, eps, f"{dt} V={V} eps={eps}")


@pytest.mark.parametrize("dt", ("fp16", "bf16"))
def test_forward_vocabularies_at_every_residue(ops, dt):
    """V = 30522 (rows of 61044 bytes) with the base 0..7 elements off the 16-byte grid, and V = 50272: every input kind."""
    worst = {}
    for off in range(8):
        kind = KINDS[off % 4]
        x, _ = _place(X.inputs(kind, 3, 30522, 40 + off), DTYPES[dt], offset=off)
        e = _check_forward(ops, x, _labels(3, 30522, off), 0.0, f"{dt} V=30522 offset={off} {kind}")
        worst[kind] = max(worst.get(kind, 0.0), e[0])
    for i, kind in enumerate(KINDS):
        x, _ = _place(X.inputs(kind, 3, 50272, 60 + i), DTYPES[dt])
        e = _check_forward(ops, x, _labels(3, 50272, i, torch.int32), (0.0, 0.1)[i % 2], f"{dt} V=50272 {kind}")
        worst[kind] = max(worst.get(kind, 0.0), e[0])
    print("worst |lse - lse64| in ulp32 per input:", {k: round(v, 3) for k, v in worst.items()})


def test_forward_fp32_vocabulary_and_a_batch_of_views(ops):
    x, _ = _place(X.inputs("n8", 3, 50272, 3), torch.float32, offset=3)
    _check_forward(ops, x, _labels(3, 50272, 1), 0.1, "fp32 V=50272 n8")
    # (B, S) = (2, 5) through causal_lm_loss: the shifted views against explicit copies, bit for bit, forward and gradient
    from outeffhop_amd import losses

    torch.manual_seed(0)
    logits = torch.randn(2, 5, 1003, device="cuda").half().requires_grad_()
    labels = torch.randint(0, 1003, (2, 5), device="cuda")
    labels[1, 2] = -100
    a = losses.causal_lm_loss(logits, labels)
    a.backward()
    copy = logits.detach()[..., :-1, :].contiguous().requires_grad_()
    b = losses.cross_entropy(copy, labels[..., 1:].contiguous())
    b.backward()
    assert a.dtype == torch.float32 and np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(logits.grad[:, :-1]), _bits(copy.grad)) and not logits.grad[:, -1].any()
    want = F.cross_entropy(logits.detach()[..., :-1, :].float().reshape(-1, 1003), labels[..., 1:].reshape(-1))
    assert abs(float(a.detach()) - float(want)) <= 1e-5 * float(want)


@pytest.mark.parametrize("eps", (0.0, 0.1))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_backward_every_row_length(ops, dt, eps):
    dtype, T = DTYPES[dt], _step(ops, DTYPES[dt])
    worst = 0.0
    for i, V in enumerate((1, 7, 8, 9, T - 1, T, T + 1, 2 * T + 3, 30522)):
        rows = 3
        x, _ = _place(X.inputs(KINDS[i % 4], rows, V, 20 + i), dtype, offset=(i + 1) % 8, pad=(0, 3)[i % 2])
        y = _labels(rows, V, i, (torch.int64, torch.int32)[i % 2], ignore=(2,) if i % 3 == 0 else ())
        yc = y.cuda()[None]
        _, out2, lse, _ = ops.xent_fwd(x, yc, label_smoothing=eps)
        mean_red = i % 2 == 0
        g = torch.tensor([1.7], device="cuda") if mean_red else torch.from_numpy(np.random.default_rng(i).standard_normal(rows).astype(np.float32)).cuda()
        d = ops.xent_bwd(x, yc, lse, out2, g, label_smoothing=eps, mean_reduction=mean_red)
        assert d.shape == x.shape and d.dtype == dtype
        # the reference: float64 throughout on the stored logits, with the fp32 factor the kernel is defined to use
        g32 = np.full(rows, np.float32(np.float64(np.float32(1.7)) / float(out2[1])), np.float32) if mean_red else g.cpu().numpy()
        d64, p64 = X.backward64(x[0].float().cpu().double().numpy(), y.numpy(), g32, eps=eps)
        bound = X.grad_bound(d64, p64, g32, NAMES[dtype])
        err = np.abs(d[0].float().cpu().double().numpy() - d64)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"{dt} V={V}: max err / bound = {(err / bound).max():.3f}"
        assert (np.abs(d[0].float().cpu().double().numpy().sum(axis=1)) <= bound.sum(axis=1)).all()  # a row's gradients sum to zero
        assert not d[0, 2].any() if i % 3 == 0 else True  # the ignored row
        # the 16-byte form, the element-store form and an aliased call give the same bits
        if i % 2 == 0:
            forms = set()
            for same in (True, False):
                buf = torch.zeros(rows * V + 32, dtype=dtype, device="cuda")
                start = next(s for s in range(8, 17) if ((buf[s:].data_ptr() - x.data_ptr()) % 16 == 0) == same)
                out = buf[start:start + rows * V].view(1, rows, V)
                ops.xent_bwd(x, yc, lse, out2, g, label_smoothing=eps, mean_reduction=mean_red, out=out)
                assert np.array_equal(_bits(out), _bits(d))
                assert not buf[:start].any() and not buf[start + rows * V:].any()
                eb = x.element_size()  # the form of THIS call: the two tensors' own residues and row strides
                forms.add(ops.xent_variant(1, rows, V, dtype, label_smoothing=eps, row_stride=x.stride(1), offset=(x.data_ptr() % 16) // eb,
                                           dx_row_stride=out.stride(1), dx_offset=(out.data_ptr() % 16) // eb).endswith("/el"))
            assert forms == {True, False}
            keep = x.clone()
            ops.xent_bwd(x, yc, lse, out2, g, label_smoothing=eps, mean_reduction=mean_red, out=x)
            assert np.array_equal(_bits(x), _bits(d))
            x.copy_(keep)
    print(f"{dt} eps={eps}: worst gradient error / bound = {worst:.3f}")


def test_store_form_names(ops):
    assert ops.xent_variant(2, 5, 30522, dx_offset=0) == "xent/block/CH4/f16" and ops.xent_variant(2, 5, 30522, dx_offset=1) == "xent/block/CH4/f16/el"


@pytest.mark.parametrize("reduction", ("mean", "sum", "none"))
def test_reductions_and_autograd_equal_the_direct_call(ops, reduction):
    from outeffhop_amd import losses

    torch.manual_seed(1)
    x = (2.0 * torch.randn(3, 7, 1000, device="cuda")).to(torch.bfloat16)
    y = torch.randint(0, 1000, (3, 7), device="cuda")
    y[0, 0] = y[2, 6] = -100
    for eps in (0.0, 0.1):
        leaf = x.clone().requires_grad_()
        loss = losses.cross_entropy(leaf, y, label_smoothing=eps, reduction=reduction)
        want = F.cross_entropy(x.float().view(-1, 1000), y.view(-1), label_smoothing=eps, reduction=reduction)
        assert loss.dtype == torch.float32 and tuple(loss.shape) == ((3, 7) if reduction == "none" else ())
        assert torch.allclose(loss.reshape(-1), want.reshape(-1), rtol=2e-6, atol=2e-6)
        up = torch.randn(3, 7, device="cuda") if reduction == "none" else None
        ((loss * up).sum() if reduction == "none" else loss * 3).backward()
        _, out2, lse, _ = ops.xent_fwd(x, y, label_smoothing=eps)
        g = up.reshape(-1).contiguous() if reduction == "none" else torch.tensor([3.0], device="cuda")
        direct = ops.xent_bwd(x, y, lse, out2, g, label_smoothing=eps, mean_reduction=reduction == "mean")
        assert np.array_equal(_bits(leaf.grad), _bits(direct))
        ref = x.float().requires_grad_()
        lr = F.cross_entropy(ref.view(-1, 1000), y.view(-1), label_smoothing=eps, reduction=reduction)
        ((lr.view(3, 7) * up).sum() if reduction == "none" else lr * 3).backward()
        assert torch.allclose(leaf.grad.float(), ref.grad, rtol=2 ** -7, atol=1e-6)  # (bf16 storage)
    m = losses.FusedCrossEntropyLoss(reduction=reduction, label_smoothing=0.1)
    assert torch.allclose(m(x.float().view(-1, 1000), y.view(-1)).reshape(-1), F.cross_entropy(x.float().view(-1, 1000), y.view(-1), label_smoothing=0.1, reduction=reduction).reshape(-1), rtol=2e-6, atol=2e-6)
    assert m._fused_xent_calls == 1
    # class-second (N, C, d1), and what the kernel does not cover
    cs = x.float().permute(0, 2, 1).contiguous()
    assert torch.allclose(m(cs, y), F.cross_entropy(cs, y, label_smoothing=0.1, reduction=reduction), rtol=2e-6, atol=2e-6) and m._fused_xent_calls == 2
    w = torch.rand(1000, device="cuda")
    mw = losses.FusedCrossEntropyLoss(weight=w, reduction=reduction)
    assert torch.equal(mw(x.float().view(-1, 1000), y.view(-1)), F.cross_entropy(x.float().view(-1, 1000), y.view(-1), weight=w, reduction=reduction)) and mw._fused_xent_calls == 0
    assert torch.equal(m(x.double().view(-1, 1000), y.view(-1)), F.cross_entropy(x.double().view(-1, 1000), y.view(-1), label_smoothing=0.1, reduction=reduction)) and m._fused_xent_calls == 2


def test_ignored_rows_and_a_batch_without_labels(ops):
    x, _ = _place(X.inputs("n1", 4, 777, 5), torch.float16, offset=3)
    y = torch.tensor([5, -100, -100, 776])
    mean, out2, lse, rl = ops.xent_fwd(x, y.cuda()[None], want_rows=True)
    assert lse[1] == 0 and lse[2] == 0 and rl[1] == 0 and rl[2] == 0 and out2[1] == 2 and float(mean) == np.float32(float(out2[0]) / 2)
    d = ops.xent_bwd(x, y.cuda()[None], lse, out2, torch.ones(1, device="cuda"), mean_reduction=True)
    assert not d[0, 1:3].any() and d[0, 0].any() and d[0, 3].any()
    # an ignored row's logits are not read: NaN there changes nothing
    x2 = x.clone()
    x2[0, 1:3] = float("nan")
    r2 = ops.xent_fwd(x2, y.cuda()[None], want_rows=True)
    assert np.array_equal(_bits(r2[0]), _bits(mean)) and np.array_equal(_bits(r2[3]), _bits(rl))
    # every row ignored: NaN, as torch
    none = torch.full((1, 4), -100, device="cuda")
    mean, out2, lse, rl = ops.xent_fwd(x, none, want_rows=True)
    assert math.isnan(float(mean)) and out2[0] == 0 and out2[1] == 0 and not lse.any() and not rl.any()
    assert math.isnan(float(F.cross_entropy(x[0].float(), none[0])))
    assert not ops.xent_bwd(x, none, lse, out2, torch.ones(1, device="cuda")).any()
    # a custom ignore_index, and no row at all
    mean = ops.xent_fwd(x, torch.tensor([[5, 3, 3, 776]], device="cuda"), ignore_index=3)[0]
    assert torch.allclose(mean, F.cross_entropy(x[0].float(), torch.tensor([5, 3, 3, 776], device="cuda"), ignore_index=3), rtol=1e-6)
    mean, out2, _, _ = ops.xent_fwd(torch.empty(2, 0, 9, device="cuda"), torch.empty(2, 0, dtype=torch.int64, device="cuda"))
    assert math.isnan(float(mean)) and out2[1] == 0


def _guarded(n, dtype, fill):
    """n elements of `dtype` with 64 guard elements on either side: (whole buffer, the middle)."""
    buf = torch.full((n + 128,), fill, dtype=dtype, device="cuda")
    return buf, buf[64:64 + n]


@pytest.mark.parametrize("ldt", (torch.int32, torch.int64))
def test_labels_that_are_none_with_guards_round_every_buffer(ops, ldt):
    from outeffhop_amd import _lib

    lib = _lib.load()
    rows, V = 5, 30522
    xbuf, xm = _guarded(rows * V, torch.float16, 3.0)
    xm.copy_(torch.from_numpy(X.inputs("n1", rows, V, 9)).reshape(-1))
    labels = [7, V, 11, -1, 2 ** 40 if ldt == torch.int64 else 2 ** 31 - 1]
    ybuf, ym = _guarded(rows, ldt, -100)
    ym.copy_(torch.tensor(labels, dtype=ldt))
    bufs = {"lse": _guarded(rows, torch.float32, 5.0), "rl": _guarded(rows, torch.float32, 5.0), "out2": _guarded(2, torch.float64, 5.0),
            "mean": _guarded(1, torch.float32, 5.0), "meter": _guarded(2, torch.float64, 0.0), "bad": _guarded(1, torch.int32, 0),
            "dx": _guarded(rows * V, torch.float16, 5.0), "g": _guarded(1, torch.float32, 1.0)}
    d = _lib.oeh_xent_desc()
    d.B, d.S, d.V, d.dtype, d.label_dtype, d.ignore_index = 1, rows, V, _lib.OEH_F16, ops._ID_DT[ldt], -100
    d.x_stride[0], d.x_stride[1], d.label_stride[0], d.label_stride[1], d.dx_stride[0], d.dx_stride[1] = rows * V, V, rows, 1, rows * V, V
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    m = {k: v[1] for k, v in bufs.items()}
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.oeh_xent_fwd(C.byref(d), p(xm), p(ym), p(m["lse"]), p(m["rl"]), p(m["out2"]), p(m["mean"]), p(m["meter"]), p(m["bad"]), st) == 0
    assert lib.oeh_xent_bwd(C.byref(d), p(xm), p(ym), p(m["lse"]), p(m["out2"]), p(m["g"]), 0, p(m["dx"]), st) == 0
    torch.cuda.synchronize()
    lse, rl = m["lse"].cpu().numpy(), m["rl"].cpu().numpy()
    badr = np.array([False, True, False, True, True])
    assert np.isnan(lse[badr]).all() and np.isnan(rl[badr]).all() and int(m["bad"]) == 3
    assert m["out2"][1] == 5 and math.isnan(float(m["out2"][0])) and math.isnan(float(m["mean"]))  # counted
    lse64, loss64, _, _ = X.forward64(xm.view(rows, V).float().cpu().double().numpy(), np.where(badr, 0, np.array(labels)))
    assert (np.abs(lse[~badr] - lse64[~badr]) <= X.lse_bound(lse64[~badr])).all()  # the neighbours are untouched
    assert (np.abs(rl[~badr] - loss64[~badr]) <= X.loss_bound(lse64[~badr], loss64[~badr])).all()
    dx = m["dx"].view(rows, V)
    bt = torch.from_numpy(badr).cuda()
    assert torch.isnan(dx[bt]).all() and torch.isfinite(dx[~bt]).all()
    assert torch.allclose(dx[0].float().sum(), torch.zeros((), device="cuda"), atol=1e-2)
    assert float(m["meter"][1]) == 1 and math.isnan(float(m["meter"][0]))
    for k, (buf, _) in bufs.items():
        fill = {"meter": 0.0, "bad": 0, "g": 1.0}.get(k, 5.0)
        assert (buf[:64] == fill).all() and (buf[-64:] == fill).all(), k
    assert (xbuf[:64] == 3.0).all() and (xbuf[-64:] == 3.0).all() and (ybuf[:64] == -100).all() and (ybuf[-64:] == -100).all()
    assert (m["g"] == 1.0).all()


def test_infinities_as_torch(ops):
    V = 300
    x = torch.from_numpy(X.inputs("n1", 5, V, 2)).float()
    x[0, 17] = float("inf")            # a row holding +inf
    x[1, 5:90] = float("-inf")         # -inf entries, the label on a finite one
    x[2, 5:90] = float("-inf")         # ... and the label on one of them
    x[3, :] = float("-inf")            # a row of nothing else
    y = torch.tensor([3, 100, 50, 7, 9])
    xc = x.cuda()
    want = F.cross_entropy(xc, y.cuda(), reduction="none").cpu().numpy()
    _, _, lse, rl = ops.xent_fwd(xc[None], y.cuda()[None], want_rows=True)
    got = rl.cpu().numpy()
    print("torch:", want, "kernel:", got)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    assert fin[1] and fin[4] and np.array_equal(np.sign(got[~fin & ~np.isnan(want)]), np.sign(want[~fin & ~np.isnan(want)]))
    # equal where finite: both within the forward bound of float64 (torch's own fp32 chain is no exact reference)
    lse64, loss64, _, _ = X.forward64(x.double().numpy()[fin], y.numpy()[fin])
    assert (np.abs(got[fin] - loss64) <= X.loss_bound(lse64, loss64)).all() and np.allclose(got[fin], want[fin], rtol=2e-6)
    out2 = torch.tensor([0.0, 5.0], dtype=torch.float64, device="cuda")
    d = ops.xent_bwd(xc[None], y.cuda()[None], lse, out2, torch.ones(1, device="cuda"))[0]
    assert not d[1, 5:90].any() and torch.isfinite(d[1]).all()  # p = 0 at the -inf entries


def test_two_calls_give_the_same_bits_and_the_reduce_without_stored_rows(ops):
    x, _ = _place(X.inputs("t3", 300, 1500, 8), torch.bfloat16, offset=5)
    y = _labels(300, 1500, 3, ignore=range(0, 300, 7)).cuda()[None]
    g = torch.randn(300, device="cuda")
    runs = []
    for _ in range(2):
        mean, out2, lse, rl = ops.xent_fwd(x, y, label_smoothing=0.1, want_rows=True)
        runs.append((mean, out2, lse, rl, ops.xent_bwd(x, y, lse, out2, g, label_smoothing=0.1)))
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b))
    with_rows, without = ops.xent_fwd(x, y, want_rows=True), ops.xent_fwd(x, y)
    assert without[3] is None and np.array_equal(_bits(with_rows[1]), _bits(without[1])) and np.array_equal(_bits(with_rows[0]), _bits(without[0]))


def test_meter_and_perplexity(ops):
    from outeffhop_amd import losses

    torch.manual_seed(4)
    meter = torch.zeros(2, dtype=torch.float64, device="cuda")
    pm = losses.PerplexityMeter()
    means = []
    for i in range(3):
        logits = (3.0 * torch.randn(2, 6, 2000 + i, device="cuda")).half()
        labels = torch.randint(0, 2000, (2, 6), device="cuda")
        out2 = ops.xent_fwd(logits[:, :-1], labels[:, 1:], meter=meter)[1].cpu().numpy()
        means.append(out2[0] / out2[1])
        got = pm.update(logits, labels)
        assert float(got) == np.float32(means[-1])
    m = meter.cpu().numpy()
    assert m[1] == 3 and m[0] == (means[0] + means[1]) + means[2]
    assert pm.state() == (m[0], 3.0) and pm.perplexity() == math.exp(m[0] / 3)
    pm.add_mean(800.0 * 4 - m[0])
    assert pm.perplexity() == float("inf")  # validate_clm.py:589-593
    pm.reset()
    assert pm.state() == (0.0, 0.0)


def test_the_switch_runs_the_torch_ops(ops, monkeypatch):
    from outeffhop_amd import losses

    torch.manual_seed(6)
    logits = torch.randn(2, 5, 333, device="cuda", requires_grad=True)
    labels = torch.randint(0, 333, (2, 5), device="cuda")
    monkeypatch.setattr(losses, "FUSED_XENT", False)
    before = ops.XENT_CALLS
    m = losses.FusedCrossEntropyLoss()
    got = (losses.causal_lm_loss(logits, labels), losses.masked_lm_loss(logits, labels), m(logits.view(-1, 333), labels.view(-1)))
    pm = losses.PerplexityMeter()
    pm.update(logits, labels)
    assert ops.XENT_CALLS == before and m._fused_xent_calls == 0
    want = F.cross_entropy(logits[..., :-1, :].contiguous().view(-1, 333), labels[..., 1:].contiguous().view(-1))
    assert torch.equal(got[0], want) and torch.equal(got[1], F.cross_entropy(logits.view(-1, 333), labels.view(-1))) and torch.equal(got[2], got[1])
    assert pm.perplexity() == math.exp(float(want.detach()))
    monkeypatch.setattr(losses, "FUSED_XENT", True)
    losses.causal_lm_loss(logits, labels).backward()
    assert ops.XENT_CALLS == before + 1 and logits.grad is not None
