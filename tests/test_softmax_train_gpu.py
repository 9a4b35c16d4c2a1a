"""The differentiable row softmax on the device (include/oeh.h: oeh_softmax_train_fwd / oeh_softmax_train_bwd) against the float64
restatement and the derived bounds of tests/_softmax_train_ref.py, at B = 2, H = 3, Sq = 5 and every Sk at which a launch form changes."""
import functools
import re

import numpy as np
import pytest

from tests import _softmax_train_ref as T

torch = pytest.importorskip("torch")
nn = torch.nn

pytestmark = pytest.mark.gpu

B, H, SQ = 2, 3, 5
DTS = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
NAME = {v: k for k, v in DTS.items()}
SEED = 0x1234_5678_9ABC_DEF0


def _ops():
    from outeffhop_amd import ops

    return ops


@functools.lru_cache(maxsize=None)
def sks(dt: str):
    """Every Sk of the issue's list, with the last Sk of each register-form chunk count and the first of the next read from the variant
    function."""
    ops = _ops()
    n = 4 if dt == "f32" else 8
    out = [1, 3, 7, 8, 24, 63, 64, 65, 72, 76]
    prev = None
    for sk in range(72 - 72 % n, 4096 + 2 * n, n):
        name = re.search(r"lanes/G\d+x\d+|wave/CH\d+|block", ops.softmax_train_variant(B, H, SQ, sk, DTS[dt])).group(0)
        if prev is not None and name != prev:
            out += [sk - n, sk]
        prev = name
    assert len(out) >= 10 + 8  # (lanes G16|G32|) CH1|CH2|CH4|CH8|block: at least four boundaries
    return tuple(sorted(set(out + [4104, 15872])))


@functools.lru_cache(maxsize=None)
def scores(dt: str, sk: int):
    """3 N(0,1) scores in storage precision: the device tensor and its exact float64 values (computed once, shared, never written)."""
    g = torch.Generator().manual_seed(1000 * sk + len(dt))
    x = (3.0 * torch.randn(B, H, SQ, sk, generator=g)).to(DTS[dt]).cuda()
    return x, x.double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def grads(dt: str, sk: int, which: int):
    g = torch.Generator().manual_seed(7000 * sk + 10 * which + len(dt))
    t = torch.randn(B, H, SQ, sk, generator=g).to(DTS[dt]).cuda()
    return t, t.double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def mask_of(form: str, mdt: str, sk: int):
    """An additive mask in one of the three broadcast forms: 0 or finfo.min of its dtype, a quarter masked, column 0 open."""
    shape = {"pad": (B, 1, 1, sk), "full": (B, 1, SQ, sk), "shared": (1, 1, SQ, sk)}[form]
    g = torch.Generator().manual_seed(31 * sk + len(form))
    hit = torch.rand(shape, generator=g) < 0.25
    hit[..., 0] = False
    m = torch.where(hit, torch.finfo(DTS[mdt]).min, 0.0).to(DTS[mdt]).cuda()
    return m, m.double().cpu().numpy()


# the cases of tests 2, 4 and 6: every option, every mask form, every mask dtype, y_dtype = f32 on 16-bit scores (through torch.result_type)
CASES = {
    "softmax1": dict(base=1),
    "scale": dict(base=0, scale=0.3),
    "div_pad_drop": dict(base=1, scale_div=8.0, mask=("pad", "f32"), p=0.1),
    "causal_clamp_clip_drop": dict(base=1, clip=True, gamma=-0.025, eta=1.0, mask=("full", "same"), clamp=True, p=0.5),
    "shared_bf16_clip": dict(base=0, clip=True, gamma=-0.1, eta=1.1, scale=0.5, mask=("shared", "bf16"), clamp=True),
    "pad_f16_clamp": dict(base=1, scale=0.25, mask=("pad", "f16"), clamp=True),
}


def setup(case: str, dt: str, sk: int):
    """(kwargs of the ops, T.Call, mask float64 | None, out dtype name) of one case."""
    ops = _ops()
    c = dict(CASES[case])
    x, _ = scores(dt, sk)
    mask = m64 = None
    if "mask" in c:
        form, mdt = c["mask"]
        mask, m64 = mask_of(form, dt if mdt == "same" else mdt, sk)
    odt = x.dtype if mask is None else torch.result_type(x, mask)
    floor = float(torch.finfo(odt).min) if c.get("clamp") else None
    spec = ops.SoftmaxSpec(c["base"], c.get("clip", False), c.get("gamma", 0.0), c.get("eta", 1.0))
    p = c.get("p", 0.0)
    kw = dict(scale=c.get("scale", 1.0), scale_div=c.get("scale_div", 0.0), mask=mask, clamp_min=floor, p=p, seed=SEED if p else None)
    call = T.Call(base=spec.base, clip=spec.clip, gamma=spec.gamma, eta=spec.eta, scale=kw["scale"], scale_div=kw["scale_div"], clamp_min=floor, p=p, seed=SEED)
    return spec, kw, call, m64, odt


def canaried(shape, dtype):
    """A tensor of `shape` inside a buffer with 64 canary elements on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 128,), 7.0, dtype=dtype, device="cuda")
    return buf, buf[64:64 + n].view(shape)


def canaries_intact(buf):
    return bool((buf[:64] == 7.0).all() and (buf[-64:] == 7.0).all())


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_plain_case_has_the_forward_only_kernels_bits(dt):
    ops = _ops()
    for sk in sks(dt):
        x, _ = scores(dt, sk)
        for base in (0, 1):
            for clip in (False, True):
                spec = ops.SoftmaxSpec(base, clip, -0.025, 1.1)
                y, u, stats = ops.softmax_train_fwd(x, spec)
                want = ops.softmax_rows(x, spec)
                assert u is None and torch.equal(y.view(torch.uint8), want.view(torch.uint8)), (sk, base, clip, ops.softmax_train_variant(B, H, SQ, sk, DTS[dt]))


# ---- 2, 3, 4, 6 ---------------------------------------------------------------------------------------------------------------------------
def chain(x, spec, kw, keep, inv, dy, du):
    """The parent's path on the same inputs and keep mask: unfused_core's ops in storage precision, softmax_autograd, dropout by the mask."""
    from outeffhop_amd.softmax import softmax_autograd

    xs = x.detach().clone().requires_grad_(True)
    s = xs
    if kw["scale_div"]:
        s = s / kw["scale_div"]
    elif kw["scale"] != 1.0:
        s = s * kw["scale"]
    if kw["mask"] is not None:
        s = s + kw["mask"]
    if kw["clamp_min"] is not None:
        s = torch.max(s, torch.tensor(torch.finfo(s.dtype).min, device=s.device))
    y = softmax_autograd(s, spec, -1)
    loss = (y * dy).sum(dtype=torch.float32) if dy is not None else 0.0
    u = None
    if keep is not None:
        u = torch.where(keep, y * inv, torch.zeros((), dtype=y.dtype, device=y.device))
        if du is not None:
            loss = loss + (u * du).sum(dtype=torch.float32)
    loss.backward()
    return y.detach(), u, xs.grad


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", CASES)
def test_forward_and_backward_against_float64(case, dt):
    """Tests 2, 3, 4 and 6 of one case over every Sk: y, u, dx inside the derived bounds with no exclusions; u from the stored y and the
    attention keep mask; stats and y unchanged by dropout; and, for 16-bit storage, no farther from float64 than the torch chain."""
    ops = _ops()
    worst = dict(y=0.0, dx=0.0)
    far = dict(y=[0.0, 0.0], dx=[0.0, 0.0])  # max |fused - f64|, max |chain - f64| over the case
    for sk in sks(dt):
        x, x64 = scores(dt, sk)
        spec, kw, call, m64, odt = setup(case, dt, sk)
        f = T.forward(call, x64, m64)
        y, u, stats = ops.softmax_train_fwd(x, spec, out_dtype=odt, **kw)
        assert y.dtype == odt and stats.shape == (B, H, SQ, 2)
        err = np.abs(y.double().cpu().numpy() - f["y"])
        bound = T.y_bound(f, NAME[odt])
        assert (err <= bound).all(), (case, dt, sk, float((err / bound).max()))
        worst["y"] = max(worst["y"], float((err / bound).max()))
        st = stats.double().cpu().numpy()
        assert np.allclose(st[..., :1], f["m"], rtol=1e-5, atol=1e-5) and np.allclose(st[..., 1:], f["den"], rtol=1e-4)
        keep = keep_t = None
        if call.p > 0:
            keep_t = ops.attn_dropout_mask(B, H, SQ, sk, call.p, SEED, x.device)
            keep = keep_t.cpu().numpy()
            assert np.array_equal(keep, T.keep_mask(B, H, SQ, sk, call.p, SEED))
            inv = torch.tensor(call.inv, dtype=torch.float32, device=x.device)
            want_u = torch.where(keep_t, (y.float() * inv).to(odt), torch.zeros((), dtype=odt, device=x.device))
            assert torch.equal(u.view(torch.uint8), want_u.view(torch.uint8)), (case, dt, sk)
            y0, u0, stats0 = ops.softmax_train_fwd(x, spec, out_dtype=odt, **dict(kw, p=0.0, seed=None))
            assert u0 is None and torch.equal(y0.view(torch.uint8), y.view(torch.uint8)) and torch.equal(stats0, stats)
            yn, un, _ = ops.softmax_train_fwd(x, spec, out_dtype=odt, want_y=False, **kw)
            assert yn is None and torch.equal(un.view(torch.uint8), u.view(torch.uint8))
        else:
            assert u is None
        chain_is_16bit = dt != "f32" and odt == x.dtype  # (an fp32 mask promotes the parent's whole chain to fp32: nothing to compare)
        modes = (("dy", True, False), ("du", False, True), ("both", True, True)) if call.p > 0 else (("dy", True, False),)
        gdt = NAME[odt]
        for mode, with_dy, with_du in modes:
            dy, dy64 = grads(gdt, sk, 1) if with_dy else (None, None)
            du, du64 = grads(gdt, sk, 2) if with_du else (None, None)
            dx = ops.softmax_train_bwd(x, stats, dy, du, spec, **kw)
            want, werr = T.backward(call, f, dy64, du64, keep)
            err = np.abs(dx.double().cpu().numpy() - want)
            bound = T.dx_bound(want, werr, dt)
            assert (err <= bound).all(), (case, dt, sk, mode, float((err / bound).max()))
            worst["dx"] = max(worst["dx"], float((err / bound).max()))
            if chain_is_16bit and mode in ("dy", "both"):
                yc, uc, dxc = chain(x, spec, kw, keep_t, call.inv, dy, du)
                far["dx"][0] = max(far["dx"][0], float(err.max()))
                far["dx"][1] = max(far["dx"][1], float(np.abs(dxc.double().cpu().numpy() - want).max()))
                if mode == "dy" or not with_dy:
                    far["y"][0] = max(far["y"][0], float(np.abs(y.double().cpu().numpy() - f["y"]).max()))
                    far["y"][1] = max(far["y"][1], float(np.abs(yc.double().cpu().numpy() - f["y"]).max()))
    print(f"softmax_train {case} {dt}: max error / bound  y {worst['y']:.3f}  dx {worst['dx']:.3f};  max |.-f64| fused vs chain  y {far['y']}  dx {far['dx']}")
    if far["y"][1] > 0.0:
        assert far["y"][0] <= far["y"][1] and far["dx"][0] <= far["dx"][1], far


@pytest.mark.parametrize("dt", DTS)
def test_same_seed_same_bits_across_forms_and_strides(dt):
    """A row stride that is no multiple of 16 bytes sends the call to another launch form: the keep mask and u = RN(y * inv) stay."""
    ops = _ops()
    spec = ops.SoftmaxSpec(1, False, 0.0, 1.0)
    for sk in (24, 72, 264, 520):
        x, _ = scores(dt, sk)
        wide = torch.zeros(B, H, SQ, sk + 1, dtype=x.dtype, device="cuda")
        xs = wide[..., 1:] if dt == "f32" else wide[..., :sk]
        xs.copy_(x)
        assert not xs.is_contiguous()
        for p in (0.1, 0.5):
            y, u, _ = ops.softmax_train_fwd(x, spec, p=p, seed=SEED)
            y2, u2, _ = ops.softmax_train_fwd(xs, spec, p=p, seed=SEED)
            keep = ops.attn_dropout_mask(B, H, SQ, sk, p, SEED, x.device)
            inv = torch.tensor(T.inv_of(p), dtype=torch.float32, device="cuda")
            for yy, uu in ((y, u), (y2, u2)):
                want = torch.where(keep, (yy.float() * inv).to(yy.dtype), torch.zeros((), dtype=yy.dtype, device="cuda"))
                assert torch.equal(uu.view(torch.uint8), want.view(torch.uint8))
            assert torch.equal((u != 0), (u2 != 0)) and (y.float() - y2.float()).abs().max() <= 2.0 * float(T.half_ulp(1.0, dt)) * 2


def test_backward_recomputes_the_forwards_probabilities_exactly():
    """fp32 storage, g = 1 at one column c: dx_j = RN(p_j * RN(g_j - p_c)) from the forward's own fp32 p - bit for bit."""
    ops = _ops()
    for sk in sks("f32"):
        x, _ = scores("f32", sk)
        for base in (0, 1):
            spec = ops.SoftmaxSpec(base, False, 0.0, 1.0)
            y, _, stats = ops.softmax_train_fwd(x, spec)
            c = sk // 2
            dy = torch.zeros_like(x)
            dy[..., c] = 1.0
            dx = ops.softmax_train_bwd(x, stats, dy, None, spec)
            want = y * (dy - y[..., c:c + 1])
            assert torch.equal(dx, want), (sk, base)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_edge_rows():
    ops = _ops()
    sm, sm1 = ops.SoftmaxSpec(0, False, 0.0, 1.0), ops.SoftmaxSpec(1, False, 0.0, 1.0)
    for dt, tdt in DTS.items():
        # (fp16 scores with the fp32 mask of an autocast model: finfo(fp32).min absorbs the score, as finfo(bf16).min does; an fp16 mask
        # of -65504 does not in the kernel's fp32 arithmetic - it keeps the differences the fp16 chain rounds away)
        mdt = torch.float32 if dt == "f16" else tdt
        odt = torch.result_type(torch.zeros((), dtype=tdt), torch.zeros((), dtype=mdt))
        fmin = float(torch.finfo(mdt).min)
        for sk in (7, 24, 72, 76, 4104):
            x, x64 = scores(dt, sk)
            dy, dy64 = grads(NAME[odt], sk, 1)
            mask = torch.zeros(B, 1, SQ, sk, dtype=mdt, device="cuda")
            mask[1, 0, 2] = fmin  # one fully masked row per head of batch 1
            m64 = mask.double().cpu().numpy()
            for spec in (sm, sm1):
                y, _, stats = ops.softmax_train_fwd(x, spec, mask=mask, clamp_min=fmin, out_dtype=odt)
                dx = ops.softmax_train_bwd(x, stats, dy, None, spec, mask=mask, clamp_min=fmin)
                call = T.Call(base=spec.base, clamp_min=fmin)
                f = T.forward(call, x64, m64)
                want, werr = T.backward(call, f, dy64)
                assert (np.abs(y.double().cpu().numpy() - f["y"]) <= T.y_bound(f, NAME[odt])).all()
                assert (np.abs(dx.double().cpu().numpy() - want) <= T.dx_bound(want, werr, dt)).all()
                row_y, row_dx = y[1, :, 2].float(), dx[1, :, 2].float()
                if spec.base == 0:  # uniform; every element sits AT the floor, so dx is half of the uniform row's gradient (the yardstick's)
                    assert torch.equal(row_y, torch.full_like(row_y, 1.0 / sk).to(odt).float())
                else:
                    assert (row_y == 0).all() and (row_dx == 0).all() and (want[1, :, 2] == 0).all()
                assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all()
        # softmax_1 below the exp range: every score -100 (fp32 directly; fp16 through the scale)
        for sk in (8, 65, 520):
            x = torch.full((B, H, SQ, sk), -100.0 if dt == "f32" else -1.0, dtype=tdt, device="cuda")
            y, _, stats = ops.softmax_train_fwd(x, sm1, scale=1.0 if dt == "f32" else 100.0)
            dx = ops.softmax_train_bwd(x, stats, torch.ones_like(x), None, sm1, scale=1.0 if dt == "f32" else 100.0)
            assert (y == 0).all() and (dx == 0).all() and torch.isinf(stats[..., 1]).all()
    # clamp ties: a mask of finfo.min absorbs the score, so z sits AT the floor - half the gradient (bf16 and fp32 floors)
    for dt in ("bf16", "f32"):
        tdt = DTS[dt]
        fmin = float(torch.finfo(tdt).min)
        for sk in (8, 65, 520):
            x, x64 = scores(dt, sk)
            dy, dy64 = grads(dt, sk, 1)
            mask = torch.zeros(B, 1, 1, sk, dtype=tdt, device="cuda")
            mask[..., : sk // 2] = fmin  # batch 1: ties that carry no probability
            mask[0] = fmin               # batch 0: every row fully masked - all ties, uniform p
            m64 = mask.double().cpu().numpy()
            call = T.Call(base=0, clamp_min=fmin)
            f = T.forward(call, x64, m64)
            assert (f["z_pre"][0] == fmin).all()  # the ties are ties in float64 as well
            y, _, stats = ops.softmax_train_fwd(x, sm, mask=mask, clamp_min=fmin)
            dx = ops.softmax_train_bwd(x, stats, dy, None, sm, mask=mask, clamp_min=fmin)
            want, werr = T.backward(call, f, dy64)
            assert (np.abs(dx.double().cpu().numpy() - want) <= T.dx_bound(want, werr, dt)).all()
            if sk > 1:
                assert (dx[0].float().abs() > 0).any()  # half of a non-zero gradient, not zero
            call0 = T.Call(base=0)  # the same rows without the clamp: twice the gradient
            want0, _ = T.backward(call0, T.forward(call0, x64, m64), dy64)
            assert np.allclose(want[0], 0.5 * want0[0], rtol=1e-12, atol=0)
    # a NaN score: its row is NaN - y, stats, dx - and its neighbours are untouched
    for dt, tdt in DTS.items():
        for sk in (7, 24, 72, 76, 520, 4104):
            x, _ = scores(dt, sk)
            dy, _ = grads(dt, sk, 1)
            for spec in (sm1, ops.SoftmaxSpec(0, True, -0.025, 1.1)):
                y0, _, st0 = ops.softmax_train_fwd(x, spec, scale=0.5, clamp_min=float(torch.finfo(tdt).min))
                dx0 = ops.softmax_train_bwd(x, st0, dy, None, spec, scale=0.5, clamp_min=float(torch.finfo(tdt).min))
                xn = x.clone()
                xn[1, 2, 3, sk // 3] = float("nan")
                y, _, st = ops.softmax_train_fwd(xn, spec, scale=0.5, clamp_min=float(torch.finfo(tdt).min))
                dx = ops.softmax_train_bwd(xn, st, dy, None, spec, scale=0.5, clamp_min=float(torch.finfo(tdt).min))
                assert torch.isnan(y[1, 2, 3]).all() and torch.isnan(dx[1, 2, 3]).all() and torch.isnan(st[1, 2, 3]).all()
                y[1, 2, 3], dx[1, 2, 3], st[1, 2, 3] = y0[1, 2, 3], dx0[1, 2, 3], st0[1, 2, 3]
                assert torch.equal(y, y0) and torch.equal(dx, dx0) and torch.equal(st, st0)


@pytest.mark.parametrize("dt", DTS)
def test_strided_scores_stride0_masks_and_canaries(dt):
    """x as a (B,Sq,H,Sk)-contiguous buffer viewed (B,H,Sq,Sk), an expanded mask, gradients in the same layout; outputs written between
    canaries through the C entry points."""
    import ctypes as C

    from outeffhop_amd import _lib

    ops = _ops()
    lib = _lib.load()
    tdt = DTS[dt]
    spec = ops.SoftmaxSpec(1, True, -0.025, 1.0)
    for sk in (7, 24, 72, 76, 520, 4104):
        x, x64 = scores(dt, sk)
        xt = x.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)  # the same values, other strides
        mask, m64 = mask_of("pad", "f32" if dt == "f32" else dt, sk)
        mexp = mask.expand(B, H, SQ, sk)
        kw = dict(scale=0.5, mask=mask, clamp_min=float(torch.finfo(tdt).min), p=0.5, seed=SEED)
        y, u, stats = ops.softmax_train_fwd(x, spec, **kw)
        y2, u2, stats2 = ops.softmax_train_fwd(xt, spec, **dict(kw, mask=mexp))
        assert torch.equal(y, y2) and torch.equal(u, u2) and torch.equal(stats, stats2)
        dy, _ = grads(dt, sk, 1)
        du, _ = grads(dt, sk, 2)
        dyt = dy.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        dx = ops.softmax_train_bwd(x, stats, dy, du, spec, **kw)
        dx2 = ops.softmax_train_bwd(xt, stats, dyt, du, spec, **dict(kw, mask=mexp))
        assert torch.equal(dx, dx2)
        # canaries: the same calls through the C ABI into buffers with guard elements
        d = ops._softmax_train_desc(x, tdt, mask, spec, 0.5, 0.0, float(torch.finfo(tdt).min), 0.5, SEED)
        ybuf, yv = canaried(x.shape, tdt)
        ubuf, uv = canaried(x.shape, tdt)
        sbuf, sv = canaried((B, H, SQ, 2), torch.float32)
        d.y_stride, d.u_stride = ops._st3(yv), ops._st3(uv)
        rc = lib.oeh_softmax_train_fwd(C.byref(d), ops._ptr(x), ops._ptr(mask), ops._ptr(yv), ops._ptr(uv), ops._ptr(sv), ops._stream())
        assert rc == 0 and torch.equal(yv, y) and torch.equal(uv, u) and torch.equal(sv, stats)
        xbuf, dxv = canaried(x.shape, tdt)
        d.dy_stride, d.du_stride, d.dx_stride = ops._st3(dy), ops._st3(du), ops._st3(dxv)
        rc = lib.oeh_softmax_train_bwd(C.byref(d), ops._ptr(x), ops._ptr(mask), ops._ptr(sv), ops._ptr(dy), ops._ptr(du), ops._ptr(dxv), ops._stream())
        assert rc == 0 and torch.equal(dxv, dx)
        torch.cuda.synchronize()
        assert all(canaries_intact(b) for b in (ybuf, ubuf, sbuf, xbuf)), sk


# ---- 7, 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal():
    ops = _ops()
    spec = ops.SoftmaxSpec(1, True, -0.025, 1.0)
    for dt in DTS:
        for sk in (24, 65, 520, 4104, 15872):
            x, _ = scores(dt, sk)
            dy, _ = grads(dt, sk, 1)
            du, _ = grads(dt, sk, 2)
            a = ops.softmax_train_fwd(x, spec, scale=0.5, p=0.1, seed=SEED)
            b = ops.softmax_train_fwd(x, spec, scale=0.5, p=0.1, seed=SEED)
            assert all(torch.equal(s, t) for s, t in zip(a, b))
            da = ops.softmax_train_bwd(x, a[2], dy, du, spec, scale=0.5, p=0.1, seed=SEED)
            db = ops.softmax_train_bwd(x, a[2], dy, du, spec, scale=0.5, p=0.1, seed=SEED)
            assert torch.equal(da, db)


def test_refused_length_runs_the_torch_chain():
    from outeffhop_amd import softmax as S

    x = torch.randn(1, 1, 2, 15873, device="cuda", requires_grad=True)
    n = dict(S.CALLS)
    probs, used = S.masked_softmax(x, S.softmax_1.spec)
    assert S.CALLS["torch"] == n["torch"] + 1 and S.CALLS["forward"] == n["forward"] and used is probs
    want = S.softmax_autograd(x, S.softmax_1.spec)
    assert torch.equal(probs, want)
    probs[..., 0].sum().backward()
    assert x.grad is not None


def test_what_the_function_saves():
    from outeffhop_amd import softmax as S

    for dt, sk, p in (("f16", 72, 0.0), ("f32", 24, 0.5), ("bf16", 520, 0.1)):
        x = scores(dt, sk)[0].clone().requires_grad_(True)
        mask, _ = mask_of("pad", "f32", sk)
        saved = []
        with torch.autograd.graph.saved_tensors_hooks(lambda t: (saved.append(t), t)[1], lambda t: t):
            probs, used = S.masked_softmax(x, S.softmax_1.spec, scale=0.5, mask=mask, clamp_min=True, dropout_p=p, seed=SEED)
        assert sum(t.numel() * t.element_size() for t in saved) == x.numel() * x.element_size() + 8 * B * H * SQ
        assert probs.dtype == torch.float32 and (used is probs) == (p == 0.0)
        used.sum().backward()
        assert x.grad is not None and x.grad.dtype == x.dtype and torch.isfinite(x.grad.float()).all()


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------
class _FixedDropout(nn.Module):
    """nn.Dropout with a given keep mask: the float64 run of a module repeats the mask its low-precision runs drew."""

    def __init__(self, keep, p):
        super().__init__()
        self.keep, self.p = keep, p

    def forward(self, x):
        return torch.where(self.keep, x / (1.0 - self.p), torch.zeros((), dtype=x.dtype, device=x.device))


def _bert(dtype):
    from types import SimpleNamespace

    from outeffhop_amd import SOFTMAX_MAPPING, BertSelfAttentionWithExtras

    cfg = SimpleNamespace(hidden_size=128, num_attention_heads=2, attention_probs_dropout_prob=0.1, position_embedding_type="absolute",
                          max_position_embeddings=512, is_decoder=False)
    m = BertSelfAttentionWithExtras(cfg, softmax_fn=SOFTMAX_MAPPING["clippedsoftmax1(-.025:1)"])
    mask = torch.zeros(2, 1, 1, 40, device="cuda", dtype=dtype)
    mask[0, ..., 33:] = torch.finfo(dtype).min
    return m, (lambda mod, x: mod(x, attention_mask=mask.to(x.dtype) if x.dtype == torch.float64 else mask)[0]), "dropout"


def _opt(dtype):
    from outeffhop_amd import SOFTMAX_MAPPING, OPTAttentionWithExtras

    m = OPTAttentionWithExtras(128, 2, dropout=0.0, is_decoder=True, softmax_fn=SOFTMAX_MAPPING["softmax1"])
    fmin = torch.finfo(dtype).min
    mask = torch.triu(torch.full((40, 40), fmin, device="cuda", dtype=dtype), 1)[None, None].expand(2, 1, 40, 40).contiguous()
    mask[1, :, :, 30:] = fmin
    return m, (lambda mod, x: mod(x, attention_mask=mask.to(x.dtype) if x.dtype == torch.float64 else mask)[0]), None


class _Assoc(nn.Module):
    def __init__(self):
        super().__init__()
        from outeffhop_amd.hopfield import Association

        self.q, self.k, self.v = nn.Linear(128, 128), nn.Linear(128, 128), nn.Linear(128, 128)
        self.assoc = Association(attention_dropout=0.0, mode="softmax1")

    def forward(self, x):
        sh = (x.shape[0], x.shape[1], 2, 64)
        return self.assoc(self.q(x).view(sh), self.k(x).view(sh), self.v(x).view(sh)).reshape(x.shape)


class _Sm1(nn.Module):
    def __init__(self):
        super().__init__()
        from outeffhop_amd.softmax import Softmax_1

        self.lin, self.sm = nn.Linear(128, 128), Softmax_1(-1)

    def forward(self, x):
        return self.sm(self.lin(x))


MODULES = {
    "bert": (_bert, torch.float32),
    "opt": (_opt, torch.float16),
    "association": (lambda dtype: (_Assoc(), (lambda mod, x: mod(x)), None), torch.float32),
    "softmax_1": (lambda dtype: (_Sm1(), (lambda mod, x: mod(x)), None), torch.float32),
}


@pytest.mark.parametrize("name", MODULES)
def test_modules_with_the_switch_on_and_off(name):
    """hidden 128, 2 heads, S = 40, training mode: outputs and parameter gradients of the two settings agree within the sum of both paths'
    distances from a float64 run of the same op chain; softmax.CALLS shows which path ran."""
    import copy

    from outeffhop_amd import softmax as S

    make, dtype = MODULES[name]
    torch.manual_seed(11)
    mod, run, drop_attr = make(dtype)
    mod = mod.cuda().to(dtype).train()
    x0 = torch.randn(2, 40, 128, device="cuda").to(dtype)
    w = torch.randn(2, 40, 128, device="cuda")

    def once(m, xin, switch, seed=5):
        prev = S.set_fused_softmax_train(switch)
        n = dict(S.CALLS)
        try:
            torch.manual_seed(seed)
            m.zero_grad(set_to_none=True)
            xin = xin.clone().requires_grad_(True)
            out = run(m, xin)
            (out.double() * w.double()).sum().backward()
        finally:
            S.set_fused_softmax_train(prev)
        delta = {k: S.CALLS[k] - n[k] for k in n}
        return [out.detach().double(), xin.grad.double()] + [p.grad.double() for p in m.parameters() if p.grad is not None], delta

    keep = []
    if drop_attr:  # the mask nn.Dropout draws (the same for both settings: one seed, one shape, one dtype)
        h = getattr(mod, drop_attr).register_forward_hook(lambda m_, i, o: keep.append((o != 0) | (i[0] == 0)))
    off, d_off = once(mod, x0, False)
    if drop_attr:
        h.remove()
    on, d_on = once(mod, x0, True)
    assert d_off["forward"] == d_off["backward"] == 0, d_off           # with the switch off the counter stays
    assert d_on["forward"] == 1 and d_on["backward"] == 1 and d_on["torch"] == 0, d_on
    ref = copy.deepcopy(mod).double()
    if drop_attr:
        setattr(ref, drop_attr, _FixedDropout(keep[0], getattr(mod, drop_attr).p))
    gold, _ = once(ref, x0.double(), False)
    assert len(on) == len(off) == len(gold) >= 3
    for a, b, g in zip(on, off, gold):
        da, db = float((a - g).abs().max()), float((b - g).abs().max())
        assert torch.isfinite(a).all() and float((a - b).abs().max()) <= da + db + 1e-300
        print(f"softmax_train module {name}: |on - f64| {da:.3e}  |off - f64| {db:.3e}")
    if name in ("bert", "opt"):  # hooks on scores_tap: the fused span is skipped (the registry callable alone still takes the kernels)
        seen = []
        orig = S.masked_softmax
        h = mod.attn_scores.register_forward_hook(lambda m_, i, o: None)
        try:
            S.masked_softmax = lambda *a, **k: (seen.append(k), orig(*a, **k))[1]
            once(mod, x0, True)
        finally:
            S.masked_softmax = orig
            h.remove()
        assert all(k.get("mask") is None and not k.get("clamp_min") for k in seen)
