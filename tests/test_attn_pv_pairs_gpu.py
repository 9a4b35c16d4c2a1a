"""The probability pairs on an MI355X (include/oeh.h: oeh_attn_opts.pv_pairs): fp32 storage with the context to fp32 accuracy.
Off is bitwise off; with the pairs the one-pass and full-row kernels' fp32 forms are held to bounds derived from the arithmetic (the
operand pairs carry 22 bits, fp32 24): against float64, a small multiple of the fp32 oracle's own distance from float64."""
import numpy as np
import pytest

from oracle import oeh_oracle as O
from tests.conftest import load_golden
from tests.test_attn_gpu import SPECS, _attn_f64, _np32, _outlier_qkv, _spec

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FMIN = float(np.finfo(np.float32).min)
KINDS = ["normal", "student_t3", "channel", "last_tile_jump", "ascending"]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _f64_bound(e_oracle64, vmax):
    """(b): 4 x the fp32 oracle's own distance from float64 + 2^-20 max(1, |V|max)"""
    return 4.0 * e_oracle64 + 2.0 ** -20 * max(1.0, vmax)


def _bitwise(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("form", ["flash_plain", "flash_mq2", "flash_mq2_clip2p", "flash_pad", "flash_full", "flash_clip2p", "flash_clip2p_pad", "fast_plain", "fast_clip", "fast_pad"])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_off_is_bitwise_off(ops, form, D):
    """oeh_attn_fwd_ex with pv_pairs = 0 (and ops.attn_fwd(pv_pairs=False)) is oeh_attn_fwd, bit for bit, on every SRC32 form."""
    from outeffhop_amd import _lib
    import ctypes as C

    B, H = (8, 12) if "mq2" in form else (2, 3)   # (8 x 12 heads of 600 rows: two query blocks per wave where the head dim allows)
    S = {"flash_plain": 600, "flash_mq2": 600, "flash_mq2_clip2p": 600, "flash_pad": 600, "flash_full": 576, "flash_clip2p": 600, "flash_clip2p_pad": 600, "fast_clip": 200}.get(form, 100)
    g = torch.Generator().manual_seed(7 + D)
    q, k, v = (torch.randn(B, H, S, D, generator=g).cuda() for _ in range(3))
    kw = dict(softmax=_spec(ops, "clippedsoftmax1(-.025:1)" if "clip" in form else "softmax1"), scale=D ** -0.5, mask_min=FMIN)
    if form in ("flash_pad", "flash_clip2p_pad", "fast_pad"):
        m = torch.zeros(B, S)
        m[1, S - 70:] = FMIN
        kw["key_pad_mask"] = m.cuda()
    if form == "flash_full":
        fm = torch.zeros(B, 1, S, S)
        fm[:, :, :, S - 40:] = FMIN
        kw["full_mask"] = fm.cuda()
    if form in ("flash_plain", "flash_mq2", "flash_mq2_clip2p"):
        kw["causal"] = True
    var = ops.attn_variant(B, H, S, S, D, torch.float32, clip="clip" in form, causal=bool(kw.get("causal")), key_pad="key_pad_mask" in kw,
                           full_mask="full_mask" in kw, scale=D ** -0.5)
    assert var.startswith("flash16/" if form.startswith("flash") else "fast16/"), (form, var)
    assert ("MQ2" in var) == ("mq2" in form and D != 128), (form, var)
    a = ops.attn_fwd(q, k, v, **kw)
    box = []
    b = ops.attn_fwd(q, k, v, pv_pairs=False, _prepared=box, **kw)
    fn, args, _keep = box
    assert fn == _lib.load().oeh_attn_fwd
    b.zero_()
    d = args[0]
    rc = _lib.load().oeh_attn_fwd_ex(d, C.byref(_lib.oeh_attn_opts(pv_pairs=0)), *args[1:], None)
    torch.cuda.synchronize()
    assert rc == 0
    assert _bitwise(a, b), form
    c = ops.attn_fwd(q, k, v, pv_pairs=True, **kw)
    assert not _bitwise(a, c)   # (the pairs do change the result)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sm", ["softmax1", "clippedsoftmax1(-.025:1)", "vanilla"])
def test_outlier_regime_with_pairs(ops, kind, sm):
    """S = 512 causal, B=2 H=3 D=64, fp32 storage: softmax1 (one-pass), clippedsoftmax1 (full-row), vanilla - (a) against the fp32 oracle,
    (b) against float64, (c) against the same call without the pairs on the heavy-tailed kinds."""
    B, H, S, D = 2, 3, 512, 64
    q, k, v = (torch.from_numpy(a) for a in _outlier_qkv(kind, B, H, S, D, 4000 + len(kind)))
    qn, kn, vn = _np32(q), _np32(k), _np32(v)
    want = O.attn_core(qn, kn, vn, causal=True, clamp_min=True, **SPECS[sm])
    exact, _ = _attn_f64(qn, kn, vn, causal=True, **SPECS[sm])
    vmax = np.abs(vn).max(axis=(-1, -2))
    kw = dict(softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=FMIN)
    var = ops.attn_variant(B, H, S, S, D, torch.float32, clip=SPECS[sm]["clip"], causal=True, pv_pairs=True)
    assert var.endswith("+pv2"), var
    got = _np32(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), pv_pairs=True, **kw))
    off = _np32(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw))
    assert np.isfinite(got).all()
    scale = np.maximum(1.0, vmax)[..., None, None]
    err = np.abs(got - want)
    lim_a = 5e-5 * scale + 5e-5 * np.abs(want)
    e64, e_off64, e_or64 = float(np.abs(got - exact).max()), float(np.abs(off - exact).max()), float(np.abs(want - exact).max())
    bound_b = _f64_bound(e_or64, float(vmax.max()))
    print(f"pv2 outlier {kind:15s} {sm:25s} [{var}] |V|max {vmax.max():6.1f}: (a) vs oracle {err.max():.2e} (worst err/limit {float((err / lim_a).max()):.2f}); "
          f"(b) vs float64 {e64:.2e} <= {bound_b:.2e} (fp32 oracle {e_or64:.2e}); (c) without pairs {e_off64:.2e} (ratio {e64 / max(e_off64, 1e-30):.3f})")
    assert (err <= lim_a).all(), f"(a) {kind} {sm}: {err.max():.3e}, worst err/limit {float((err / lim_a).max()):.2f}"
    assert e64 <= bound_b, f"(b) {kind} {sm}: {e64:.3e} > {bound_b:.3e}"
    if kind in ("student_t3", "channel", "ascending"):
        assert e64 <= 0.25 * e_off64, f"(c) {kind} {sm}: {e64:.3e} vs {e_off64:.3e} without the pairs"


def _f64_masked(q, k, v, *, base, clip, gamma, eta, addmask):
    s = np.matmul(q.astype(np.float64), np.swapaxes(k.astype(np.float64), -1, -2)) + addmask
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    p = e / (e.sum(-1, keepdims=True) + (np.exp(-m) if base else 0.0))
    if clip:
        p = np.clip(p * (eta - gamma) + gamma, 0, 1)
    return np.matmul(p, v.astype(np.float64))


@pytest.mark.parametrize("case", ["clip_long_rows", "key_padding", "full_mask", "d32", "d128"])
def test_other_forms_against_float64(ops, case):
    """The (b) bound on the two-pass clipped one-pass form (rows > 512 keys), key padding, a (B,1,Sq,Sk) mask, head dims 32 and 128."""
    D = {"d32": 32, "d128": 128}.get(case, 64)
    B, H = 2, 2
    S = {"clip_long_rows": 768, "key_padding": 704, "full_mask": 640}.get(case, 512)
    sm = "clippedsoftmax1(-.025:1)" if case == "clip_long_rows" else "softmax1"
    q, k, v = (torch.from_numpy(a) for a in _outlier_qkv("student_t3", B, H, S, D, 4300 + S + D))
    qn, kn, vn = _np32(q), _np32(k), _np32(v)
    add = np.zeros((B, 1, S, S), np.float32)
    kw = dict(softmax=_spec(ops, sm), mask_min=FMIN, clamp_min=True)
    vk = dict(clip=SPECS[sm]["clip"])
    if case == "key_padding":
        pad = np.zeros((B, S), np.float32)
        pad[0, S - 100:] = FMIN
        pad[1, :30] = FMIN
        add += pad[:, None, None, :]
        kw["key_pad_mask"] = torch.from_numpy(pad).cuda()
        vk["key_pad"] = True
    elif case == "full_mask":
        rs = np.random.RandomState(11)
        add = np.where(rs.rand(B, 1, S, S) < 0.3, FMIN, 0.0).astype(np.float32)
        add[..., 0] = 0.0
        kw["full_mask"] = torch.from_numpy(add).cuda()
        vk["full_mask"] = True
    else:
        kw["causal"] = True
        vk["causal"] = True
        add = np.ascontiguousarray(np.broadcast_to(np.where(np.triu(np.ones((S, S), bool), 1), FMIN, 0.0).astype(np.float32), (B, 1, S, S)))
    var = ops.attn_variant(B, H, S, S, D, torch.float32, pv_pairs=True, **vk)
    assert var.startswith("flash16/") and var.endswith("+pv2"), var
    got = _np32(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), pv_pairs=True, **kw))
    off = _np32(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw))
    want = O.attn_core(qn, kn, vn, full_mask=add, clamp_min=True, **SPECS[sm])
    exact = _f64_masked(qn, kn, vn, addmask=np.maximum(add.astype(np.float64), -1e300), **SPECS[sm])
    vmax = float(np.abs(vn).max())
    e64, e_or64, e_off64 = float(np.abs(got - exact).max()), float(np.abs(want - exact).max()), float(np.abs(off - exact).max())
    bound = _f64_bound(e_or64, vmax)
    print(f"pv2 {case:14s} [{var}]: vs float64 {e64:.2e} <= {bound:.2e} (fp32 oracle {e_or64:.2e}, without pairs {e_off64:.2e})")
    assert e64 <= bound, f"{case}: {e64:.3e} > {bound:.3e}"


def test_fully_masked_softmax1_row_is_zero(ops):
    B, H, S, D = 2, 2, 704, 64
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B, H, S, D, generator=g).cuda() for _ in range(3))
    pad = torch.zeros(B, S)
    pad[1, :] = FMIN
    out = ops.attn_fwd(q, k, v, softmax=_spec(ops, "softmax1"), scale=0.125, key_pad_mask=pad.cuda(), mask_min=FMIN, pv_pairs=True)
    assert torch.count_nonzero(out[1]) == 0
    assert torch.isfinite(out).all() and torch.count_nonzero(out[0]) > 0


def test_reference_fixture_with_pairs(ops):
    """The reference's captured outputs (tests/golden/core_attn_long.npz): within 2e-5 max(1, |V|max) with the pairs (5e-4 without)."""
    from tests.golden import synth as sy

    g = load_golden("core_attn_long.npz")
    q, k, v = (torch.from_numpy(a) for a in sy.long_causal_qkv())
    lim = 2e-5 * max(1.0, float(v.abs().max()))
    for sm in ("softmax1", "clippedsoftmax1(-.025:1)", "vanilla"):
        want = g[f"opt512[{sm}].ctx"]
        kw = dict(softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=FMIN)
        got = _np32(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), pv_pairs=True, **kw))
        off = _np32(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw))
        e, e0 = float(np.abs(got - want).max()), float(np.abs(off - want).max())
        print(f"reference fixture S=512 causal {sm} fp32 + pairs: {e:.2e} (without {e0:.2e}), limit {lim:.2e}")
        assert e <= lim, (sm, e, lim)
    q, k, v = (torch.from_numpy(a) for a in sy.long_padded_qkv())
    pad = torch.from_numpy(sy.key_padding(sy.LONG_PAD_B, sy.LONG_PAD_S, sy.LONG_PAD_LEFT, sy.LONG_PAD_RIGHT)).cuda()
    lim = 2e-5 * max(1.0, float(v.abs().max()))
    for sm in ("softmax1", "vanilla"):
        want = g[f"bert704[{sm}].ctx"]
        kw = dict(softmax=_spec(ops, sm), scale_div=8.0, key_pad_mask=pad, mask_min=FMIN)
        got = _np32(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), pv_pairs=True, **kw))
        off = _np32(ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), **kw))
        e, e0 = float(np.abs(got - want).max()), float(np.abs(off - want).max())
        print(f"reference fixture 704 padded keys {sm} fp32 + pairs: {e:.2e} (without {e0:.2e}), limit {lim:.2e}")
        assert e <= lim, (sm, e, lim)


def test_determinism(ops):
    B, H, S, D = 2, 3, 512, 64
    q, k, v = (torch.from_numpy(a).cuda() for a in _outlier_qkv("channel", B, H, S, D, 4007))
    for sm in ("softmax1", "clippedsoftmax1(-.025:1)"):
        kw = dict(softmax=_spec(ops, sm), causal=True, clamp_min=True, mask_min=FMIN, pv_pairs=True)
        a = ops.attn_fwd(q, k, v, **kw)
        b = ops.attn_fwd(q, k, v, **kw)
        assert _bitwise(a, b), sm


@pytest.fixture
def oa():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import outeffhop_amd

    yield outeffhop_amd
    outeffhop_amd.attention.set_compensated_pv(False)


def _module_cases(oa):
    from tests.test_host_cpu import Cfg

    class CfgB(Cfg):
        attention_probs_dropout_prob = 0.0

    torch.manual_seed(0)
    opt = oa.OPTAttentionWithExtras(128, 2, is_decoder=True, softmax_fn=oa.SOFTMAX_MAPPING["softmax1"])
    bert = oa.BertSelfAttentionWithExtras(CfgB(), softmax_fn=oa.SOFTMAX_MAPPING["softmax1"])
    B, S = 2, 256
    g = torch.Generator().manual_seed(5)
    hidden = torch.randn(B, S, 128, generator=g)
    hidden[..., [3, 77]] *= 30.0   # outlier channels of the hidden state
    omask = torch.zeros(B, 1, S, S)
    omask += torch.triu(torch.full((S, S), FMIN), 1)
    omask[1, :, :, :20] = FMIN
    omask[1, :, torch.arange(20), torch.arange(20)] = 0.0   # (left padding: those rows see themselves only)
    bmask = torch.zeros(B, 1, 1, S)
    bmask[0, ..., S - 40:] = FMIN
    return [("OPT", opt, hidden, omask), ("BERT", bert, hidden, bmask)]


def _run(m, hidden, mask, **kw):
    with torch.no_grad():
        out = m(hidden, attention_mask=mask, **kw)
    return out[0]


def _module_f64(name, m, hidden, mask):
    """The module's softmax1 attention in float64 torch ops (OPT: q scaled, + mask, out_proj; BERT: / sqrt(d), + mask)."""
    lin = lambda l, x: torch.nn.functional.linear(x, l.weight.double(), None if l.bias is None else l.bias.double())  # noqa: E731
    h = hidden.double()
    if name == "OPT":
        H, d = m.num_heads, m.head_dim
        q, k, v = lin(m.q_proj, h) * m.scaling, lin(m.k_proj, h), lin(m.v_proj, h)
    else:
        H, d = m.num_attention_heads, m.attention_head_size
        q, k, v = lin(m.query, h), lin(m.key, h), lin(m.value, h)
    B, S = h.shape[:2]
    q, k, v = (t.view(B, S, H, d).transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2)
    if name != "OPT":
        s = s / np.sqrt(d)
    s = torch.maximum(s + mask.double(), torch.tensor(FMIN, dtype=torch.float64, device=s.device))
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    ctx = ((e / (torch.exp(-mx) + e.sum(-1, keepdim=True))) @ v).transpose(1, 2).reshape(B, S, H * d)
    return lin(m.out_proj, ctx) if name == "OPT" else ctx


def test_fp32_modules_closer_to_float64_with_the_switch(oa):
    for name, m, hidden, mask in _module_cases(oa):
        m = m.cuda().eval()
        with torch.no_grad():
            exact = _module_f64(name, m, hidden.cuda(), mask.cuda())
        h, mk = hidden.cuda(), mask.cuda()
        off = _run(m, h, mk)
        oa.attention.set_compensated_pv(True)
        on = _run(m, h, mk)
        on2 = _run(m, h, mk)
        oa.attention.set_compensated_pv(False)
        off2 = _run(m, h, mk)
        e_on, e_off = float((on.double() - exact).abs().max()), float((off.double() - exact).abs().max())
        print(f"{name} fp32 module vs float64: with the pairs {e_on:.2e}, without {e_off:.2e}")
        assert e_on < e_off, (name, e_on, e_off)
        assert _bitwise(off, off2) and _bitwise(on, on2), name
        assert not _bitwise(on, off), name


def test_quantised_modules_with_quantisers_on_are_unchanged(oa):
    from tests.test_modules_gpu import _qparams

    for name, m, hidden, mask in _module_cases(oa):
        dev = torch.device("cuda:0")
        cls = oa.QuantizedOPTAttentionWithExtras if name == "OPT" else oa.QuantizedBertSelfAttentionWithExtras
        qm = cls(m.to(dev), **_qparams(oa)).to(dev).eval()
        qm.set_quant_state(weight_quant=True, act_quant=True)
        h, mk = hidden.cuda(), mask.cuda()
        _run(qm, h, mk)   # calibration pass (estimate ranges)
        qm.fix_ranges()
        off = _run(qm, h, mk)
        oa.attention.set_compensated_pv(True)
        on = _run(qm, h, mk)
        oa.attention.set_compensated_pv(False)
        assert _bitwise(off, on), name
