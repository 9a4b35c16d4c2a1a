"""The fused training kernels (include/oeh.h: oeh_attn_fwd_train / oeh_attn_bwd[_dropout]) over what tests/test_attn_bwd_gpu.py and
tests/test_attn_dropout_gpu.py do not reach: Sq != Sk (cross attention, causal with a KV offset, causal with more queries than keys),
single partial tiles and S = 1, fp16 / bf16 / stride-0 masks, left padding, mask_min = -1e4, scale != 1, strided packed-QKV views, every
dq / dk / dv / do layout the C ABI takes, writes past the outputs, lse itself, and both sides of the causal tile-skip rule.

The reference is float64 CPU autograd of the reference's op chain (tests/test_attn_bwd_gpu.py:_ref_chain, with dropout
tests/test_attn_dropout_gpu.py:_ref_chain_drop) on the 16-bit-rounded inputs, the yardstick the same chain on the GPU in the storage dtype
(attention.unfused_core, softmax in fp32 as OPT's upcast, softmax_1 in _ref_chain's shifted form).  Per tensor:
    max|fused - ref64| <= 2 max|torch_op - ref64| + 1e-3 max|ref64|;
the same per query row (o, dq) and per key row (dk, dv) with each row's own maxima and the rounding terms of _rows_check; where the
reference is exactly zero by construction (keys hidden from every query by the mask, fully masked softmax_1 rows) the kernel must give
exactly zero.  OEH_TEST_REPORT=<file> records every err / limit ratio (tests/test_attn_gpu.py:_le)."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests.test_attn_bwd_gpu import SOFTMAX, _check, _copy_params, _grads, _ref_chain, _spec
from tests.test_attn_dropout_cpu import keep_mask
from tests.test_attn_dropout_gpu import SEEDS, _ref_chain_drop
from tests.test_attn_gpu import _le

pytestmark = pytest.mark.gpu

TAGS = ("o", "dq", "dk", "dv")
ROW_ULPS = 4    # per-row bound: storage ulps of the row's own max|ref64| (_rows_check)
LSE_TOL = 1e-6  # |lse - lse64| <= LSE_TOL (1 + |lse64|): fp32 scores and statistics against float64 (measured <= 2.3e-7 on the MI355X)


# ---------------------------------------------------------------- a case: description -> float64 mask + kernel arguments
def _softmax_spec(name):
    from outeffhop_amd.ops import SoftmaxSpec

    if name == "clipped+":  # gamma > 0: masked keys get probability gamma, the skip rule must be off
        return SoftmaxSpec(1, True, 0.02, 1.0)
    return _spec(name)


def _mask_value(mask_min, mdt):
    """mask_min as a mask of dtype mdt holds it (finfo(mdt).min where mask_min is beyond the dtype), read back as the kernel reads it."""
    v = torch.tensor(mask_min, dtype=torch.float64).to(mdt)
    if not torch.isfinite(v):
        v = torch.tensor(torch.finfo(mdt).min, dtype=mdt)
    return float(v.double())


def _inputs(c):
    """q, k, v, do (B,H,S,64) in the storage dtype; q/k/v strided views of packed (B,S,3,H,64) buffers when c['packed']."""
    B, H, Sq, Sk, dt = c["B"], c["H"], c["Sq"], c["Sk"], c["dt"]
    g = torch.Generator().manual_seed(c["seed"])
    if c["dist"] == "t3":
        t = torch.distributions.StudentT(3.0)
        torch.manual_seed(c["seed"])
        mk = lambda S: t.sample((B, H, S, 64)).clamp(-30, 30)  # noqa: E731
    else:
        mk = lambda S: torch.randn(B, H, S, 64, generator=g)  # noqa: E731
    q, k, v = mk(Sq) * 0.125, mk(Sk), mk(Sk)
    if c["dist"] == "neg150":  # q . k ~ -150 +- 1 on every key (tests/test_attn_gpu.py's left-padded long rows)
        u = torch.randn(64, generator=g)
        u = u / u.norm()
        q = 0.05 * torch.randn(B, H, Sq, 64, generator=g) + 12.5 * u
        k = 0.05 * torch.randn(B, H, Sk, 64, generator=g) - 12.0 * u
    do = torch.randn(B, H, Sq, 64, generator=g)
    q, k, v, do = (t.to(dt) for t in (q, k, v, do))
    return q, k, v, do


def _to_dev(c, q, k, v):
    if not c["packed"]:
        return q.cuda(), k.cuda(), v.cuda()
    B, H, Sq, Sk = c["B"], c["H"], c["Sq"], c["Sk"]
    if Sq == Sk:  # the modules' layout: one (B,S,3,H,64) projection output
        buf = torch.empty(B, Sq, 3, H, 64, dtype=q.dtype, device="cuda")
        for i, t in enumerate((q, k, v)):
            buf[:, :, i] = t.permute(0, 2, 1, 3).cuda()
        return tuple(buf[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    qb = torch.empty(B, Sq, 3, H, 64, dtype=q.dtype, device="cuda")
    kvb = torch.empty(B, Sk, 3, H, 64, dtype=q.dtype, device="cuda")
    qb[:, :, 2] = q.permute(0, 2, 1, 3).cuda()
    kvb[:, :, 0] = k.permute(0, 2, 1, 3).cuda()
    kvb[:, :, 1] = v.permute(0, 2, 1, 3).cuda()
    return qb[:, :, 2].permute(0, 2, 1, 3), kvb[:, :, 0].permute(0, 2, 1, 3), kvb[:, :, 1].permute(0, 2, 1, 3)


def _masks(c):
    """(add64 or None, kernel kwargs): the additive float64 mask of the reference chain and the fused call's mask arguments, both from
    the case's description and the values the mask dtype holds."""
    B, Sq, Sk, mdt, mm = c["B"], c["Sq"], c["Sk"], c["mdt"], c["mask_min"]
    mv = _mask_value(mm, mdt)
    causal = c["kind"] != "cross"
    add = torch.zeros(B, 1, Sq, Sk, dtype=torch.float64)
    kw = dict(causal=causal, mask_min=mm)
    if causal:  # (mask_min is an fp32 value: finfo.min of a 16-bit type or -1e4)
        qi, ki = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
        add = add + torch.where(ki > qi + (Sk - Sq), mm, 0.0).double()
    if c["mask"] in ("pad_right", "pad_left"):
        rng = random.Random(c["seed"] + 1)
        pad = torch.zeros(B, Sk, dtype=mdt)
        for b in range(B):
            n = rng.randint(0, Sk) if b < B - 1 or B == 1 else Sk  # the last sequence of a batch fully padded (B > 1): rows with no key
            if c["mask"] == "pad_right":
                pad[b, Sk - n:] = mv
            else:
                pad[b, :n] = mv
        if c["pad_shape"] == "expand":  # one row for every sequence, batch stride 0
            pad = pad[:1].expand(B, Sk)
        add = add + pad.double()[:, None, None, :]
        kw["key_pad_mask"] = (pad if c["pad_shape"] == "B" else pad[:, None, None, :]).cuda()
    if c["mask"] in ("full", "full_expand"):
        g = torch.Generator().manual_seed(c["seed"] + 2)
        rows = 1 if c["mask"] == "full_expand" else B
        full = torch.where(torch.rand(rows, 1, Sq, Sk, generator=g) < 0.25, mv, 0.0).to(mdt)
        full[..., min(3, Sq - 1), :] = mv  # one fully masked query row
        full = full.expand(B, 1, Sq, Sk)  # (full_expand: batch stride 0)
        add = add + full.double()
        kw["full_mask"] = full.cuda()
    if c["kind"] == "cross" and c["mask"] == "none":
        add = None
    return add, kw


def _stable_softmax(x, spec, dim=-1):
    """softmax.softmax_autograd with softmax_1 shifted by max(m, 0) as in _ref_chain: the same function, but its gradient stays finite on
    a fully masked row (the literal form's exp(-m) is inf there and its gradient NaN, in fp32 as in float64)."""
    from outeffhop_amd.softmax import softmax_autograd

    if spec.base == 0:
        return softmax_autograd(x, spec, dim)
    m = x.max(dim=dim, keepdim=True).values.clamp(min=0)
    e = torch.exp(x - m)
    p = e / (e.sum(dim=dim, keepdim=True) + torch.exp(-m))
    if spec.clip:
        p = torch.clip(p * (spec.eta - spec.gamma) + spec.gamma, 0, 1)
    return p


def _required_zeros(c, add):
    """{tag: (B,H,S) bool} rows the kernel must give as exact zeros: dk / dv of keys hidden (p = 0 in float64 and fp32 alike) from every
    query that has a visible key, when fully masked rows add nothing (softmax_1, or no such row) - dv not under a clip with gamma > 0,
    which gives hidden keys probability gamma; o / dq of fully masked softmax_1 rows (o again not with gamma > 0)."""
    B, H, Sq, Sk = c["B"], c["H"], c["Sq"], c["Sk"]
    spec = _softmax_spec(c["sm"])
    if add is None:
        hidden = torch.zeros(B, Sq, Sk, dtype=torch.bool)
    else:
        hidden = add[:, 0] <= -5000.0
    dead_row = hidden.all(-1)  # (B,Sq)
    gpos = bool(spec.clip) and spec.gamma > 0
    if spec.base == 1:
        key0 = hidden.all(1)
    else:
        key0 = (hidden | dead_row[:, :, None]).all(1) & ~dead_row.any(1, keepdim=True)
    row0 = dead_row & (spec.base == 1)
    ex = lambda t: t[:, None].expand(B, H, t.shape[1])  # noqa: E731
    z = torch.zeros(B, H, Sq, dtype=torch.bool)
    return {"o": z if gpos else ex(row0), "dq": ex(row0), "dk": ex(key0), "dv": ex(key0) & (not gpos)}


def _case_name(c):
    return ("B{B} H{H} Sq{Sq} Sk{Sk} {kind} {sm} mask={mask}/{pad_shape}/{mdtn} mask_min={mask_min:.3g} clamp={clamp} scale={scale}/div{scale_div} "
            "{dtn} packed={packed} dist={dist} p={p} seed={dseed}").format(mdtn=str(c["mdt"]).split(".")[-1], dtn=str(c["dt"]).split(".")[-1], **c)


def _dev_mask(add, dt):
    return None if add is None else add.clamp(min=torch.finfo(dt).min).to(dt).cuda()


def _run(c):
    """(fused, torch_op, ref64) lists of (o, dq, dk, dv), and the fused lse."""
    from outeffhop_amd import fused_attention, ops
    from outeffhop_amd.attention import unfused_core

    spec = _softmax_spec(c["sm"])
    q, k, v, do = _inputs(c)
    add, mkw = _masks(c)
    clamp = c["clamp"] and add is not None
    p, seed = c["p"], c["dseed"]
    sc, sd = c["scale"], c["scale_div"]
    if p > 0:
        keep = torch.from_numpy(keep_mask(c["B"], c["H"], c["Sq"], c["Sk"], p, seed))
        ref = _grads(lambda a, b, cc: _ref_chain_drop(a, b, cc, spec, sc, sd, add, clamp, c["mask_min"], keep, p), q.double(), k.double(),
                     v.double(), do.double())
        kd = keep.to(c["dt"]).cuda()
        drop = lambda t: t * kd / (1.0 - p)  # noqa: E731
    else:
        ref = _grads(lambda a, b, cc: _ref_chain(a, b, cc, spec, sc, sd, add, clamp, c["mask_min"]), q.double(), k.double(), v.double(),
                     do.double())
        drop = None
    qd, kd_, vd = _to_dev(c, q, k, v)
    fkw = dict(softmax=spec, scale=sc, scale_div=sd, clamp_min=clamp, dropout_p=p, dropout_seed=seed if p > 0 else None, **mkw)
    fused = _grads(lambda a, b, cc: fused_attention(a, b, cc, **fkw), qd, kd_, vd, do.cuda())
    fkw.pop("dropout_p"), fkw.pop("dropout_seed")
    _, lse = ops.attn_fwd_train(qd, kd_, vd, **fkw)
    am = _dev_mask(add, c["dt"])
    fn = lambda x, dim=-1: _stable_softmax(x.float(), spec, dim).to(c["dt"])  # noqa: E731
    top = _grads(lambda a, b, cc: unfused_core(a, b, cc, softmax_fn=fn, scale=sc, scale_div=sd, attention_mask=am, clamp_min=clamp,
                                               dropout=drop)[0],
                 q.cuda(), k.cuda(), v.cuda(), do.cuda())
    return fused, top, ref, lse.cpu(), add


def _rows_check(name, fused, torch_op, ref, zeros, dt, floor):
    """The yardstick per row (o / dq: query rows, dk / dv: key rows) with each row's own maxima,
        max_row|fused - ref64| <= 2 max_row|torch_op - ref64| + ROW_ULPS eps(dt) max_row|ref64| + 1e-3 max|ref64|,
    and exact zeros where required (_required_zeros).  The row term in storage ulps stands for the 16-bit rounding of the kernel's own
    operands (p, dX) where the torch-op path happens to round a row more luckily; the last term is the tensor bound's floor, below
    which a row is cancellation residue (a row with one visible key under vanilla softmax is 0 in float64, dY - rowsum(dO o O) in the
    kernel).  A dropped or misplaced tile moves a row by its own size and fails this at any magnitude above that floor.  floor: an extra
    per-row term {tag: (B,H,S)} (_delta_floor)."""
    worst = {}
    eps = torch.finfo(dt).eps
    for tag, f, t, r in zip(TAGS, fused, torch_op, ref):
        f, t, r = f.double().cpu(), t.double().cpu(), r.double().cpu()
        must = zeros[tag]
        nz = (f.abs().amax(-1) != 0) & must
        assert not bool(nz.any()), f"{name} {tag}: {int(nz.sum())} rows nonzero that must be exactly 0, first at {nz.nonzero()[0].tolist()}"
        assert not bool(((r.abs().amax(-1) != 0) & must).any()), f"{name} {tag}: the reference is not 0 where the test expects it"
        ef = (f - r).abs().amax(-1)  # (B,H,S): one value per row
        et = (t - r).abs().amax(-1)
        mr = r.abs().amax(-1)
        lim = 2 * et + ROW_ULPS * eps * mr + 1e-3 * float(r.abs().max()) + floor.get(tag, 0.0)
        ratio = torch.where(mr == 0, torch.zeros_like(ef), ef / lim.clamp(min=1e-300))
        worst[tag] = float(ratio.max())
        _le(worst[tag], 1.0, f"train_sweep rows {tag} [{name}]")
        bad = ratio > 1
        assert not bool(bad.any()), (f"{name} {tag}: {int(bad.sum())} rows over the per-row bound, worst {worst[tag]:.2f}x at "
                                     f"{(ratio == ratio.max()).nonzero()[0].tolist()}")
    return worst


def _delta_floor(c, o, do, q, k, add):
    """dq / dk rows: the kernel's row term delta_i = rowsum(dO o O) is formed from the STORED 16-bit o (FlashAttention's form), so it
    carries e_i <= eps(dt) sum_d |dO_i o_i| of rounding; dX_ij = p_ij (g_ij - delta_i) passes it on to dq_i = scale sum_j dX_ij k_j and
    dk_j = scale sum_i dX_ij q_i.  On a peaked row dX is a small difference and this term is most of what the kernel can be held to (the
    torch-op path sums p g instead).  Twice that bound, with p in float64."""
    spec = _softmax_spec(c["sm"])
    sc = 1.0 / c["scale_div"] if c["scale_div"] else c["scale"]
    e = torch.finfo(c["dt"]).eps * (do.double().abs() * o.double().cpu().abs()).sum(-1)  # (B,H,Sq)
    s = q.double() @ k.double().transpose(-1, -2)
    s = s * sc
    if add is not None:
        s = s + add
        if c["clamp"]:
            s = torch.clamp(s, min=c["mask_min"])
    lse = _lse_ref(q, k, add, spec, c["scale"], c["scale_div"], c["clamp"] and add is not None, c["mask_min"])
    p = torch.exp(s - lse[..., None])
    kmax = k.double().abs().amax(-1)  # (B,H,Sk)
    qmax = q.double().abs().amax(-1)  # (B,H,Sq)
    return {"dq": 2 * abs(sc) * e * (p * kmax[:, :, None, :]).sum(-1), "dk": 2 * abs(sc) * (p * (e * qmax)[..., None]).sum(-2)}


def _lse_ref(q, k, add, spec, sc, sd, clamp, mask_min):
    s = q.double() @ k.double().transpose(-1, -2)
    s = s / sd if sd else s * sc
    if add is not None:
        s = s + add
        if clamp:
            s = torch.clamp(s, min=mask_min)
    lse = torch.logsumexp(s, -1)
    return torch.logaddexp(torch.zeros_like(lse), lse) if spec.base == 1 else lse


# ---------------------------------------------------------------- a. the seeded random sweep
EDGES = (1, 2, 15, 16, 17, 63, 64, 65, 127, 129)


def _draw_S(rng):
    return rng.choice(EDGES) if rng.random() < 0.6 else rng.randint(3, 400)


def _sweep_cases(n=48, seed=20261016):
    rng = random.Random(seed)
    cases = []
    for i in range(n):
        kind = rng.choice(("cross", "causal", "causal_qgt"))
        Sq, Sk = _draw_S(rng), _draw_S(rng)
        if kind == "causal" and Sq > Sk:
            Sq, Sk = Sk, Sq
        if kind == "causal_qgt":
            if Sq == Sk:
                Sk = max(1, Sk - rng.randint(1, 40))
            if Sq < Sk:
                Sq, Sk = Sk, Sq
        dt = rng.choice((torch.float16, torch.bfloat16))
        mask = rng.choice(("none", "pad_right", "pad_left", "full", "full_expand"))
        mm_kind = rng.choice(("finfo", "finfo", "1e4"))
        mdt = rng.choice((torch.float32, torch.float16, torch.bfloat16))
        scale, scale_div = rng.choice(((1.0, 0.0), (1.0, 8.0), (0.3, 0.0), (1.0 / 3.0, 0.0)))
        dist = rng.choice(("normal", "normal", "t3", "neg150"))
        if dist == "neg150":
            scale, scale_div = 1.0, 0.0
            if mask == "none" or kind != "cross":
                mask = "pad_left"
        sm = rng.choice(list(SOFTMAX) + ["clipped+"])
        if Sk == 1 and sm in ("vanilla", "clipped"):  # one key: dq = dk = 0 exactly in the reference, only rounding in the kernel
            sm = "softmax1"
        cases.append(dict(
            B=rng.randint(1, 3), H=rng.randint(1, 4), Sq=Sq, Sk=Sk, kind="causal" if kind == "causal_qgt" else kind,
            sm=sm, mask=mask, pad_shape=rng.choice(("B", "B1", "expand")), mdt=mdt,
            mask_min=float(torch.finfo(dt).min) if mm_kind == "finfo" else -1e4,
            clamp=mm_kind == "finfo",  # OPT clamps at finfo.min; BERT's -1e4 masks are not clamped
            scale=scale, scale_div=scale_div, dt=dt, packed=rng.random() < 0.5, dist=dist,
            p=rng.choice((0.0, 0.0, 0.1)), dseed=rng.choice(SEEDS), seed=1000 + i))
    return cases


def _directed_cases():
    """What the sweep must reach whatever its draw: the skip-off causal forms against float64, ragged Sk % 4 != 0 with dropout, and
    the bf16 clamp ties (a vanilla row fully masked by ONE finfo.min term: its uniform p times the clamp's half gradient)."""
    base = dict(B=2, H=2, mask="none", pad_shape="B", mdt=torch.float32, clamp=True, scale=1.0, scale_div=0.0, packed=False, dist="normal",
                p=0.0, dseed=0, kind="causal")
    f16, b16 = float(torch.finfo(torch.float16).min), float(torch.finfo(torch.bfloat16).min)
    out = [
        dict(base, Sq=129, Sk=200, sm="clipped+", dt=torch.float16, mask_min=f16, seed=1),                       # clip gamma > 0, causal
        dict(base, Sq=150, Sk=150, sm="softmax1", dt=torch.float16, mask_min=-1e4, clamp=False, seed=2),        # mask_min = -1e4, causal
        dict(base, Sq=97, Sk=161, sm="vanilla", dt=torch.bfloat16, mask="pad_right", mask_min=b16, seed=3),     # vanilla causal + padding
        dict(base, Sq=77, Sk=197, sm="clippedsoftmax1", dt=torch.float16, mask_min=f16, p=0.1, dseed=SEEDS[2], seed=4),  # Sk % 4 != 0
        dict(base, Sq=259, Sk=5, sm="vanilla", dt=torch.float16, kind="cross", mask_min=f16, p=0.1, dseed=SEEDS[3], seed=5),
        dict(base, Sq=130, Sk=67, sm="vanilla", dt=torch.bfloat16, mask_min=b16, seed=6),                       # Sq > Sk: ties, causal alone
        dict(base, Sq=90, Sk=70, sm="vanilla", dt=torch.bfloat16, kind="cross", mask="pad_left", mask_min=b16, seed=7),  # ties, padding
        dict(base, Sq=65, Sk=65, sm="clipped", dt=torch.bfloat16, kind="cross", mask="full", mask_min=b16, seed=8),
        dict(base, Sq=1, Sk=1, sm="softmax1", dt=torch.bfloat16, mask_min=b16, seed=9),
        dict(base, Sq=17, Sk=1, sm="clippedsoftmax1", dt=torch.float16, mask="full_expand", mdt=torch.float16, mask_min=f16, p=0.1, dseed=1, seed=10),
    ]
    return out


SWEEP = _sweep_cases() + _directed_cases()


@pytest.mark.parametrize("i", range(len(SWEEP)))
def test_training_sweep(i):
    c = SWEEP[i]
    name = _case_name(c)
    fused, top, ref, lse, add = _run(c)
    rep = []
    try:
        _check(name, fused, top, ref, rep)
    finally:
        for _, tag, ef, et, _rel in rep:
            mr = float(ref[TAGS.index(tag)].abs().max())
            _le(ef / max(2 * et + 1e-3 * mr, 1e-300), 1.0, f"train_sweep tensor {tag} [{name}]")
    q, k, _, do = _inputs(c)
    _rows_check(name, fused, top, ref, _required_zeros(c, add), c["dt"], _delta_floor(c, fused[0], do, q, k, add))
    # lse of the same call against float64 (dropout leaves it alone)
    want = _lse_ref(q, k, add, _softmax_spec(c["sm"]), c["scale"], c["scale_div"], c["clamp"] and add is not None, c["mask_min"])
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(lse.double()), fin), name
    err = ((lse.double() - want).abs() / (1 + want.abs()))[fin]
    if err.numel():
        assert _le(float(err.max()), LSE_TOL, f"train_sweep lse [{name}]"), f"{name}: lse off by {float(err.max()):.2e}"


def test_sweep_reaches_the_edges():
    """The draw covers what it is there for (a changed seed or list must not quietly drop a class)."""
    got = {(c["Sq"] != c["Sk"]) for c in SWEEP}
    assert got == {True, False}
    assert any(c["kind"] == "causal" and c["Sq"] > c["Sk"] for c in SWEEP)
    assert any(c["kind"] == "causal" and c["Sq"] < c["Sk"] for c in SWEEP)
    assert any(min(c["Sq"], c["Sk"]) < 64 for c in SWEEP) and any(c["Sq"] == 1 or c["Sk"] == 1 for c in SWEEP)
    assert any(c["p"] > 0 and c["Sk"] % 4 for c in SWEEP) and any(c["packed"] for c in SWEEP)
    for key, vals in (("sm", set(SOFTMAX) | {"clipped+"}), ("mdt", {torch.float32, torch.float16, torch.bfloat16}),
                      ("mask", {"none", "pad_right", "pad_left", "full", "full_expand"}), ("dist", {"normal", "t3", "neg150"}),
                      ("dt", {torch.float16, torch.bfloat16})):
        assert {c[key] for c in SWEEP} == vals, key
    assert {c["mask_min"] for c in SWEEP} >= {-1e4, float(torch.finfo(torch.float16).min), float(torch.finfo(torch.bfloat16).min)}
    assert {(c["scale"], c["scale_div"]) for c in SWEEP} >= {(1.0, 8.0), (0.3, 0.0), (1.0, 0.0)}


# ---------------------------------------------------------------- b. the skip rule: both sides give the same bits
def _pair(sm, dt, Sq, Sk, p, mdt):
    from outeffhop_amd import ops

    g = torch.Generator().manual_seed(Sq * 1000 + Sk)
    B, H = 2, 3
    q = (torch.randn(B, H, Sq, 64, generator=g) * 0.125).to(dt).cuda()
    k, v = (torch.randn(B, H, Sk, 64, generator=g).to(dt).cuda() for _ in range(2))
    do = torch.randn(B, H, Sq, 64, generator=g).to(dt).cuda()
    mm = float(torch.finfo(dt).min)
    spec = _softmax_spec(sm)
    full = torch.triu(torch.full((Sq, Sk), mm, dtype=mdt), 1 + Sk - Sq)[None, None].expand(B, 1, Sq, Sk).cuda()
    drop = dict(dropout_p=p, dropout_seed=SEEDS[2] if p else None)
    res = []
    for kw in (dict(causal=True), dict(full_mask=full)):
        kw.update(softmax=spec, clamp_min=True, mask_min=mm, scale=0.7)
        o, lse = ops.attn_fwd_train(q, k, v, **kw, **drop)
        res.append([o, lse, *ops.attn_bwd(q, k, v, o, do, lse, **kw, **drop)])
    return res


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Sq,Sk", [(200, 200), (70, 250), (1, 130)])
@pytest.mark.parametrize("sm", ["softmax1", "clippedsoftmax1", "clipped", "vanilla"])
def test_skip_rule_both_sides_bitwise(sm, Sq, Sk, p):
    """Where the skip rule holds (softmax_1; clip gamma <= 0; vanilla without another mask; Sq <= Sk), analytic causal (tiles skipped) and
    the same mask as a full (B,1,Sq,Sk) mask of mask_min (every tile visited) give the same bits: score() forms the same x on both
    sides, so a hidden tile adds p = 0 (the clip maps 0 to 0 with a zero gate, alpha = 1) - exact zeros."""
    cases = [(torch.float16, torch.float32), (torch.float16, torch.float16), (torch.bfloat16, torch.float32)]
    for dt, mdt in cases:
        a, b = _pair(sm, dt, Sq, Sk, p, mdt)
        torch.cuda.synchronize()
        for tag, x, y in zip(("o", "lse", "dq", "dk", "dv"), a, b):
            assert torch.isfinite(x).all(), (tag, dt, mdt)
            assert torch.equal(x, y), f"{sm} Sq{Sq} Sk{Sk} p{p} {dt}/{mdt} {tag}: skip and no-skip differ by {float((x.float() - y.float()).abs().max()):.3e}"


# ---------------------------------------------------------------- c. layouts through the C ABI
def _abi_bwd(lib, d, q, k, v, o, do, lse, dq, dk, dv):
    from outeffhop_amd import ops

    st = lambda t: (C.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))  # noqa: E731
    work = torch.empty(max(1, lib.oeh_attn_bwd_work_bytes(C.byref(d)) // 4), dtype=torch.float32, device="cuda")
    rc = lib.oeh_attn_bwd(C.byref(d), ops._ptr(q), ops._ptr(k), ops._ptr(v), ops._ptr(o), ops._ptr(do), st(do), ops._ptr(lse), ops._ptr(dq),
                          st(dq), ops._ptr(dk), st(dk), ops._ptr(dv), st(dv), ops._ptr(work), ops._stream())
    assert rc == 0, rc


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_layouts_through_the_c_abi(dt):
    from outeffhop_amd import _lib, ops

    lib = _lib.load()
    B, H, S = 2, 3, 161
    g = torch.Generator().manual_seed(5)
    kw = dict(softmax=_spec("clippedsoftmax1"), causal=True, clamp_min=True)
    q, k, v = ((torch.randn(B, H, S, 64, generator=g) * s).to(dt).cuda() for s in (0.125, 1, 1))
    do = torch.randn(B, H, S, 64, generator=g).to(dt).cuda()
    o_ref, lse_ref = ops.attn_fwd_train(q, k, v, **kw)
    grads_ref = ops.attn_bwd(q, k, v, o_ref, do, lse_ref, **kw)
    # q / k / v as views of one packed (B,S,3,H,D) buffer
    pk = torch.stack([t.permute(0, 2, 1, 3) for t in (q, k, v)], 2).contiguous()
    qp, kp, vp = (pk[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    o = torch.empty(B, H, S, 64, dtype=dt, device="cuda")  # (B,H,S,D)-contiguous this time
    lse = torch.empty(B, H, S, dtype=torch.float32, device="cuda")
    d, keep = ops._train_desc(qp, kp, vp, o, kw["softmax"], 1.0, 0.0, None, None, True, True, None)
    assert lib.oeh_attn_fwd_train(C.byref(d), ops._ptr(qp), ops._ptr(kp), ops._ptr(vp), ops._ptr(o), ops._ptr(lse), ops._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    one = torch.randn(1, 1, 1, 64, generator=g).to(dt).cuda()
    dos = {"BSHD": do.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), "BHSD": do.contiguous(), "broadcast": one.expand(B, H, S, 64)}
    for dname, dov in dos.items():
        want = grads_ref if dname != "broadcast" else ops.attn_bwd(q, k, v, o_ref, dov.contiguous(), lse_ref, **kw)
        gp = torch.full((B, S, 3, H, 64), float("nan"), dtype=dt, device="cuda")  # one packed gradient buffer
        outs = {"packed": tuple(gp[:, :, i].permute(0, 2, 1, 3) for i in range(3)),
                "BHSD": tuple(torch.full((B, H, S, 64), float("nan"), dtype=dt, device="cuda") for _ in range(3))}
        for oname, (dq, dk, dv) in outs.items():
            _abi_bwd(lib, d, qp, kp, vp, o, dov, lse, dq, dk, dv)
            torch.cuda.synchronize()
            for tag, x, y in zip(("dq", "dk", "dv"), (dq, dk, dv), want):
                assert torch.equal(x, y), f"do {dname}, grads {oname}: {tag} differs"
    del keep


# ---------------------------------------------------------------- d. nothing written past the outputs
def _guarded(shape_bshd, dt, G=40):
    """A (B,H,S,D) view with row pitch D + 8 inside a flat buffer with G guard elements at each end, all of a NaN pattern."""
    B, S, H, D = shape_bshd
    n = B * S * H * (D + 8)
    pat = 0x7FC5  # a NaN in fp16 and in bf16
    buf = torch.full((n + 2 * G,), pat, dtype=torch.int16, device="cuda")
    t = buf.view(dt)[G:G + n].view(B, S, H, D + 8)[..., :D].permute(0, 2, 1, 3)
    return buf, t, pat


def _guard_intact(buf, t, pat, G=40):
    """Every element of buf outside the view t (which starts G elements in) still holds pat."""
    m = torch.ones_like(buf, dtype=torch.bool)
    idx = torch.arange(buf.numel(), device="cuda")
    m[torch.as_strided(idx[G:], t.shape, t.stride()).reshape(-1)] = False
    return bool((buf[m] == pat).all())


@pytest.mark.parametrize("Sq,Sk", [(1, 17), (17, 1), (65, 129), (130, 63)])
def test_writes_stay_inside_the_outputs(Sq, Sk):
    from outeffhop_amd import _lib, ops

    lib = _lib.load()
    B, H, dt, G = 2, 3, torch.float16, 40
    g = torch.Generator().manual_seed(Sq + Sk)
    q = (torch.randn(B, H, Sq, 64, generator=g) * 0.125).to(dt).cuda()
    k, v = (torch.randn(B, H, Sk, 64, generator=g).to(dt).cuda() for _ in range(2))
    do = torch.randn(B, H, Sq, 64, generator=g).to(dt).cuda()
    kw = dict(softmax=_spec("clipped"), causal=True, clamp_min=True)
    for p in (0.0, 0.1):
        bo, o, pat = _guarded((B, Sq, H, 64), dt)
        lbuf = torch.full((B * H * Sq + 2 * G,), 0x7FC0DEAD, dtype=torch.int32, device="cuda")
        lse = lbuf.view(torch.float32)[G:G + B * H * Sq].view(B, H, Sq)
        d, keep = ops._train_desc(q, k, v, o, kw["softmax"], 1.0, 0.0, None, None, True, True, None)
        drop = ops._dropout(p, 3)
        st = lambda t: (C.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))  # noqa: E731
        if drop is None:
            rc = lib.oeh_attn_fwd_train(C.byref(d), ops._ptr(q), ops._ptr(k), ops._ptr(v), ops._ptr(o), ops._ptr(lse), ops._stream())
        else:
            rc = lib.oeh_attn_fwd_train_dropout(C.byref(d), C.byref(drop), ops._ptr(q), ops._ptr(k), ops._ptr(v), ops._ptr(o), ops._ptr(lse),
                                                ops._stream())
        assert rc == 0
        (bq, dq, _), (bk, dk, _), (bv, dv, _) = _guarded((B, Sq, H, 64), dt), _guarded((B, Sk, H, 64), dt), _guarded((B, Sk, H, 64), dt)
        nw = lib.oeh_attn_bwd_work_bytes(C.byref(d)) // 4
        wbuf = torch.full((nw + 2 * G,), 0x7FC0DEAD, dtype=torch.int32, device="cuda")
        work = wbuf.view(torch.float32)[G:G + nw]
        args = (C.byref(d), ops._ptr(q), ops._ptr(k), ops._ptr(v), ops._ptr(o), ops._ptr(do), st(do), ops._ptr(lse), ops._ptr(dq), st(dq),
                ops._ptr(dk), st(dk), ops._ptr(dv), st(dv), ops._ptr(work), ops._stream())
        rc = lib.oeh_attn_bwd(*args) if drop is None else lib.oeh_attn_bwd_dropout(args[0], C.byref(drop), *args[1:])
        assert rc == 0
        torch.cuda.synchronize()
        for name, buf, t in (("o", bo, o), ("dq", bq, dq), ("dk", bk, dk), ("dv", bv, dv)):
            assert _guard_intact(buf, t, pat), f"p{p}: a write outside {name}"
            assert torch.isfinite(t).all(), f"p{p}: {name} not fully written"
        for name, buf, n in (("lse", lbuf, B * H * Sq), ("work", wbuf, nw)):
            assert bool((buf[:G] == 0x7FC0DEAD).all() and (buf[G + n:] == 0x7FC0DEAD).all()), f"p{p}: a write outside {name}"
            assert torch.isfinite(buf[G:G + n].view(torch.float32)).all(), f"p{p}: {name} not fully written"
        del keep


# ---------------------------------------------------------------- e. lse against float64
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_lse_against_float64(dt):
    from outeffhop_amd import ops

    B, H, Sq, Sk = 2, 2, 100, 143
    g = torch.Generator().manual_seed(8)
    q = (torch.randn(B, H, Sq, 64, generator=g) * 0.4).to(dt)
    k = torch.randn(B, H, Sk, 64, generator=g).to(dt)
    mm = float(torch.finfo(dt).min)
    full = torch.zeros(B, 1, Sq, Sk)
    full[:, :, 7] = mm  # fully masked rows
    full[0, :, :, 120:] = mm
    for sm in ("vanilla", "softmax1"):
        spec = _spec(sm)
        want = _lse_ref(q, k, full.double(), spec, 1.0, 0.0, True, mm)
        for p in (0.0, 0.1):
            _, lse = ops.attn_fwd_train(q.cuda(), k.cuda(), k.cuda(), softmax=spec, full_mask=full.cuda(), clamp_min=True, mask_min=mm,
                                        dropout_p=p, dropout_seed=11 if p else None)
            lse = lse.double().cpu()
            if p == 0.0:
                lse0 = lse
            else:
                assert torch.equal(lse, lse0), f"{sm}: dropout changed lse"
            rows = torch.ones(Sq, dtype=torch.bool)
            rows[7] = False
            err = ((lse - want).abs() / (1 + want.abs()))[:, :, rows]
            assert _le(float(err.max()), LSE_TOL, f"lse_f64 [{sm} {dt}]"), (sm, float(err.max()))
            if sm == "softmax1":  # log(1 + 0): exactly 0 on a fully masked row
                assert float(lse[:, :, 7].abs().max()) == 0.0
            else:  # mask_min + log(Sk), as float64 rounds it to fp32
                assert float(((lse[:, :, 7] - want[:, :, 7]).abs() / want[:, :, 7].abs()).max()) <= 1e-6


# ---------------------------------------------------------------- f. dropout at ragged key counts
@pytest.mark.parametrize("Sk", [1, 3, 5, 197, 259])
def test_dropout_mask_at_ragged_keys(Sk):
    from outeffhop_amd import ops

    for Sq in (1, 37, 130):
        for seed in SEEDS:
            got = ops.attn_dropout_mask(2, 3, Sq, Sk, 0.1, seed, "cuda").cpu().numpy()
            assert np.array_equal(got, keep_mask(2, 3, Sq, Sk, 0.1, seed)), (Sq, Sk, seed)


# ---------------------------------------------------------------- bf16 clamp ties (see test_fully_masked_rows)
def test_clamp_ties_split_the_gradient():
    """bf16 storage, clamp at finfo(bf16).min: x + mask_min IS the floor (fp32 and float64 alike), and autograd's max passes half the
    gradient at a tie.  A vanilla row masked by one such term is uniform; its dq / dk contribution must be the reference's (not twice)."""
    from outeffhop_amd import fused_attention

    dt = torch.bfloat16
    B, H, Sq, Sk = 1, 2, 70, 90
    g = torch.Generator().manual_seed(3)
    q = (torch.randn(B, H, Sq, 64, generator=g) * 0.125).to(dt)
    k, v = (torch.randn(B, H, Sk, 64, generator=g).to(dt) for _ in range(2))
    do = torch.randn(B, H, Sq, 64, generator=g).to(dt)
    mm = float(torch.finfo(dt).min)
    pad = torch.zeros(B, Sk)
    pad[:, 30:] = mm
    full = torch.zeros(B, 1, Sq, Sk)
    full[:, :, 4] = mm
    add = pad.double()[:, None, None, :] + full.double()
    ref = _grads(lambda a, b, c: _ref_chain(a, b, c, _spec("vanilla"), 1.0, 0.0, add, True, mm), q.double(), k.double(), v.double(), do.double())
    fused = _grads(lambda a, b, c: fused_attention(a, b, c, softmax=_spec("vanilla"), key_pad_mask=pad.cuda(), full_mask=full.cuda(),
                                                   clamp_min=True, mask_min=mm), q.cuda(), k.cuda(), v.cuda(), do.cuda())
    # row 4: keys < 30 masked once (ties, p uniform over them), keys >= 30 twice (below the floor in fp32: no gradient)
    r = ref[1][:, :, 4].abs().max()
    e = float((fused[1][:, :, 4].double().cpu() - ref[1][:, :, 4]).abs().max())
    assert e <= 2e-2 * float(r), f"dq of the tied row: {e:.3e} (max|ref| {float(r):.3e})"
    for f, rr, tag in zip(fused, ref, TAGS):
        err = float((f.double().cpu() - rr).abs().max())
        assert err <= 2e-2 * float(rr.abs().max()) + 1e-3, (tag, err)


# ---------------------------------------------------------------- 2. module level
def _module_run(make, run, dout_of, fused_calls=1, skip=()):
    """tests/test_attn_bwd_gpu.py:_module_case for any module call: run(mod, dtype) -> (output, [inputs that take a gradient]).  fp32
    torch-op path = reference, fp16 torch-op path = yardstick, fp16 fused path checked; the fused calls must have run.  skip: names of
    parameters left out of the comparison."""
    from outeffhop_amd import attention as A
    from outeffhop_amd import autograd_attention as AA

    torch.manual_seed(0)
    m16 = make().cuda().half().train()
    m32 = make().cuda().float().train()
    _copy_params(m32, m16)

    def grads(mod, dt):
        mod.zero_grad(set_to_none=True)
        out, ins = run(mod, dt)
        out.backward(dout_of(out))
        return [out.detach()] + [t.grad for t in ins] + [p.grad for n, p in mod.named_parameters() if n not in skip]

    prev = A.FUSED_BACKWARD
    try:
        A.set_fused_backward(False)
        ref = grads(m32, torch.float32)
        off = grads(m16, torch.float16)
        A.set_fused_backward(True)
        n0 = dict(AA.CALLS)
        on = grads(m16, torch.float16)
        ran = AA.CALLS["forward"] - n0["forward"], AA.CALLS["backward"] - n0["backward"]
    finally:
        A.set_fused_backward(prev)
    assert ran == (fused_calls, fused_calls), ran
    for i, (f, t, r) in enumerate(zip(on, off, ref)):
        f, t, r = f.double(), t.double(), r.double()
        ef, et, mr = float((f - r).abs().max()), float((t - r).abs().max()), float(r.abs().max())
        assert torch.isfinite(f).all(), i
        _le(ef / (2 * et + 1e-3 * mr), 1.0, f"train_module [{make.__name__} {i}]")
        assert ef <= 2 * et + 1e-3 * mr, (i, ef, et, mr)


def test_bert_cross_attention_trains_on_the_fused_kernels():
    from types import SimpleNamespace

    from outeffhop_amd import SOFTMAX_MAPPING, BertSelfAttentionWithExtras

    def bert_cross():
        cfg = SimpleNamespace(hidden_size=768, num_attention_heads=12, attention_probs_dropout_prob=0.0, position_embedding_type="absolute",
                              max_position_embeddings=512, is_decoder=False)
        return BertSelfAttentionWithExtras(cfg, softmax_fn=SOFTMAX_MAPPING["softmax1"])

    B, Sq, Sk = 2, 100, 173
    x = torch.randn(B, Sq, 768, device="cuda").half()
    enc = torch.randn(B, Sk, 768, device="cuda").half()
    dout = torch.randn(B, Sq, 768, device="cuda").half()

    def run(mod, dt):
        xx, ee = x.to(dt).clone().requires_grad_(True), enc.to(dt).clone().requires_grad_(True)
        em = torch.zeros(B, 1, 1, Sk, dtype=dt, device="cuda")
        em[1, ..., Sk - 50:] = torch.finfo(dt).min
        return mod(xx, encoder_hidden_states=ee, encoder_attention_mask=em)[0], [xx, ee]

    # key.bias: its gradient is sum_j dK_j = scale sum_i q_i sum_j dX_ij, and sum_j dX_ij is 0 under vanilla softmax and a residue under
    # softmax_1 - both paths measure their rounding of a near-zero sum there, not the attention
    _module_run(bert_cross, run, lambda out: dout.to(out.dtype), skip=("key.bias",))


def test_vit_trains_on_the_fused_kernels():
    from outeffhop_amd import SOFTMAX_MAPPING, ViTSelfAttentionWithExtras

    def vit():
        return ViTSelfAttentionWithExtras(768, num_heads=12, qkv_bias=True, softmax_fn=SOFTMAX_MAPPING["clippedsoftmax1(-.025:1)"])

    B, N = 2, 197
    x = torch.randn(B, N, 768, device="cuda").half()
    dout = torch.randn(B, N, 768, device="cuda").half()

    def run(mod, dt):
        xx = x.to(dt).clone().requires_grad_(True)
        return mod(xx), [xx]

    _module_run(vit, run, lambda out: dout.to(out.dtype))


def test_opt_left_padded_decoder_mask_trains_on_the_fused_kernels(monkeypatch):
    """A LEFT-padded decoder mask: classify_causal turns it into the analytic causal mask + a padding vector (softmax_1: the padded
    sequence's first rows see no key at all).  The torch-op runs take softmax_1 in _ref_chain's shifted form - the same function, whose
    gradient stays finite on those rows."""
    from outeffhop_amd import OPTAttentionWithExtras, SOFTMAX_MAPPING
    from outeffhop_amd import attention as A
    from outeffhop_amd import softmax as S

    orig = S.softmax_autograd
    monkeypatch.setattr(S, "softmax_autograd", lambda data, spec, dim=-1: orig(data, spec, dim) if spec.base == 0 else _stable_softmax(data, spec, dim))

    def opt():
        return OPTAttentionWithExtras(768, 12, dropout=0.0, is_decoder=True, softmax_fn=SOFTMAX_MAPPING["softmax1"])

    B, S = 2, 256
    x = torch.randn(B, S, 768, device="cuda").half()
    dout = torch.randn(B, S, 768, device="cuda").half()

    def mask(dt):
        fmin = torch.finfo(dt).min
        m = torch.triu(torch.full((S, S), fmin, dtype=dt, device="cuda"), 1)[None, None].expand(B, 1, S, S).clone()
        m[1, :, :, :40] = fmin
        return m

    m16 = mask(torch.float16)
    causal, pad = A.classify_causal(m16)
    assert causal and pad is not None and bool((pad[1, :40] != 0).all())

    def run(mod, dt):
        xx = x.to(dt).clone().requires_grad_(True)
        return mod(xx, attention_mask=m16 if dt == torch.float16 else mask(dt))[0], [xx]

    _module_run(opt, run, lambda out: dout.to(out.dtype))


def test_golden_train_toy_on_the_fused_kernels():
    """tests/golden/train_grads.npz (the reference's own gradients of a two-layer OPT -> BERT toy) with the modules in fp16 on the
    fused backward; the yardstick is the same fp16 toy on the torch-op path."""
    import json

    from outeffhop_amd import attention as A
    from outeffhop_amd import autograd_attention as AA
    from tests.conftest import load_golden
    from tests.test_host_cpu import run_train_toy

    g = load_golden("train_grads.npz")
    for cj in g["cases_json"]:
        case = json.loads(str(cj))
        name = case["name"]
        prev = A.FUSED_BACKWARD
        try:
            A.set_fused_backward(False)
            off = run_train_toy(g, case, "cuda", torch.float16)
            A.set_fused_backward(True)
            n0 = dict(AA.CALLS)
            on = run_train_toy(g, case, "cuda", torch.float16)
            assert (AA.CALLS["forward"] - n0["forward"], AA.CALLS["backward"] - n0["backward"]) == (2, 2), name
        finally:
            A.set_fused_backward(prev)

        def tensors(res):
            la, lb, x, z = res
            out = [("z", z), ("dx", x.grad)]
            for tag, mod in (("a", la), ("b", lb)):
                out += [(f"{tag}.{k}", p.grad) for k, p in mod.named_parameters() if bool(g[f"{name}.{tag}.hasgrad.{k}"])]
            return out

        for (what, f), (_, t) in zip(tensors(on), tensors(off)):
            key = {"z": f"{name}.z", "dx": f"{name}.dx"}.get(what, f"{name}.{what[0]}.g.{what[2:]}")
            r = torch.from_numpy(g[key]).double()
            f, t = f.detach().double().cpu(), t.detach().double().cpu()
            ef, et, mr = float((f - r).abs().max()), float((t - r).abs().max()), float(r.abs().max())
            assert torch.isfinite(f).all(), (name, what)
            _le(ef / (2 * et + 1e-3 * mr), 1.0, f"train_golden [{name} {what}]")
            assert ef <= 2 * et + 1e-3 * mr, (name, what, ef, et, mr)
