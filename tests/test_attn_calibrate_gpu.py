"""Every branch of the attention calibration kernel (csrc/oeh_calib.hip: attn_calib_kernel, launch_attn_calibrate; include/oeh.h:
oeh_attn_calibrate) at the smallest shapes that reach it, and two cases oeh_percentile_ema lacked.  `-m gpu`.

Yardsticks (tests/_calib_ref.py; their soundness is checked without a GPU in tests/test_attn_calibrate_cpu.py):
  A  scores       the inputs make the score tensor EXACTLY known, so the percentile pair must equal np.percentile(scores32, (lo, hi))
                  bit for bit; the running average against its float64 formula at rtol 1e-15 (as tests/test_rows_gpu.py)
  B  probs        |got - np.percentile(p64, pair)| <= 4 err64 + one float64 spacing, err64 = max |oracle fp32 probs - float64 probs|
                  (order statistics are 1-Lipschitz in the max norm); the factor 4 covers the kernel's summation tree and 1-ulp exp
  C  context      |ctx - ctx64| <= 4 err64 (err64 from the oracle's context) elementwise.  With the probability quantiser: rows that
                  hold a probability within 4 err64_probs / scale of a rounding boundary are the tie band (<= 5 % of the rows, asserted
                  on the CPU); err64 is taken over the other rows (inside the band the oracle itself may sit on the other grid point),
                  band rows may differ by (band probabilities in the row) * scale * max|v| more
  D  percentile_ema  bit for bit against np.percentile
The ratios to err64 are printed (-s); the largest measured on an MI355X stand at the end of this docstring.

Which case reaches which branch (shapes are (Sq, Sk); selection cases are named family-SqxSk-layout, value cases as in
_calib_ref.VALUE_CASES):
  D = 32 / 64 / 128 x fp32 / fp16 / bf16     all nine template instances: every test below is parametrised or loops over them
  q / k / v strided views of a fused output  selection *-fused; context cases with an odd index in test_context_*
  partial last key tile (Sk % 16 != 0)       1x1, 1x45, 16x15, 63x17, 65x33, 150x150; Sk < 16: 1x1, 16x15; Sq < 16: 1x1, 1x45
  waves without rows                         1x1, 1x45, 16x15 (3 of 4 waves), 17x128 (2), 65x33 and 150x150 (last workgroup)
  lanes without rows (qvalid)                1x1, 1x45, 63x17, 65x33, 17x128, 150x150
  scale_div / scale / neither                selection cases rotate over the three; value cases scale-half, *-eighths
  pass 1 / pass 2 digit and prefix, W_NEXT   selector-*: scores that differ in their low mantissa bits, one-spacing neighbours
  tie branch cnt_le >= i + 2                 integer-* (a few dozen distinct scores) and the duplicate block of selector-*
  ranks at the very top (i + 1 >= n), n = 1  pair (0, 100) on every selection case; *-1x1-* has B = H = 1: n = 1
  frac exactly 0                             the fifth pair of every selection case (_calib_ref.frac0_pair)
  momentum 0 / 0.9 / 1, first = 0            every selection case makes two further calls with one of the three
  state is written, nothing around it        every statistics call: state is the middle of a 4-element tensor
  dirty work buffer on entry                 a percentile_ema call on other data precedes every statistics call
  masks / causal / clip leave scores alone   selection cases with extras "opt" (pad + causal + clamp_min), "bert" (full mask + clip)
  vanilla / softmax_1                        value cases alternate; clip: clip-025-sat-below (gamma -0.025), clip-003-sat-above
  score quantiser, n_bits != 8               sr of the value cases: saturating below / above / both (4 bits) / step 1/8 / none
  pad fp32 / fp16, full fp32 / row-strided   pad-f32-4bit, pad-f16-eighths, full-f32, full-strided, pad-and-full-eighths
  causal offset Sk - Sq, clamp_min           causal-pad-clamp-wide (17x128), causal-pad-clamp-tall (63x17: rows with every key masked)
  a sample with every key masked             masked-sample-clamp-vanilla (uniform rows), masked-sample-clamp-softmax1 (zero rows)
  probability quantiser                      test_context_* with _calib_ref.PROB_RANGES: (0, 1) and the saturating (0, 0.5)
  keys beyond Sk are never read              test_context_ignores_rows_beyond_sk
  percentile_ema second grid stride, cap     test_percentile_ema_beyond_the_block_cap (n = 2048 * 4096 + 4099, fp32 and fp16)
  fp32 subnormals                            test_percentile_ema_keeps_subnormals

MEASURED_B: 1.00 (largest |got - want| / err64 over the probability cases: "single", one element, err64 1e-10; the others <= 0.61)
MEASURED_C: 1.90 (largest |ctx - ctx64| / err64 over the context cases, quantised ones outside the tie band; D = 64 fp32)"""
import numpy as np
import pytest

from oracle import oeh_oracle as O
from tests import _calib_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
INSTANCES = [(D, st) for D in R.HEAD_DIMS for st in R.STORAGES]
VALUE_IDS = [c["name"] for c in R.VALUE_CASES]
GUARD = (1234.5, -77.25)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def dirty(ops):
    """A percentile_ema call on unrelated data: leaves the stream's shared work buffer (histograms, prefixes, counts) dirty."""
    x = torch.randn(5003, generator=torch.Generator().manual_seed(3)).cuda()
    st = torch.zeros(2, dtype=torch.float64, device="cuda")
    return lambda: ops.percentile_ema(x, 3.0, 60.0, st, first=True)


def _dev(a, storage=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if storage is None else t.to(DT[storage])).cuda()


def _heads(a, storage, layout, slot=0, noise_seed=0):
    """(B,H,S,D) numpy -> device tensor: contiguous, or slot `slot` of a fused (B,S,3*H*D) projection output viewed (B,H,S,D)."""
    B, H, S, D = a.shape
    if layout == "contiguous":
        return _dev(a, storage)
    fused = torch.randn(B, S, 3 * H * D, generator=torch.Generator().manual_seed(noise_seed)).to(DT[storage])
    fused[:, :, slot * H * D:(slot + 1) * H * D] = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 1, 3))).reshape(B, S, H * D).to(DT[storage])
    t = fused.cuda()[:, :, slot * H * D:(slot + 1) * H * D].view(B, S, H, D).permute(0, 2, 1, 3)
    assert t.stride(3) == 1 and (S == 1 or t.stride(2) == 3 * H * D)
    return t


def _range(r):
    return None if r is None else torch.tensor([float(r[0]), float(r[1])], dtype=torch.float64, device="cuda")


def _mask_kw(ops, base, clip, pad, full, full_strided=False):
    kw = dict(softmax=ops.SoftmaxSpec(base=base) if clip is None else ops.SoftmaxSpec(base=base, clip=True, gamma=clip[0], eta=clip[1]),
              mask_min=R.FMIN32)
    if pad is not None:
        kw["key_pad_mask"] = _dev(pad)
    if full is not None:
        if full_strided:  # rows of a wider allocation: read in place through the row stride
            wide = torch.full(full.shape[:3] + (full.shape[3] + 8,), 7.0)
            wide[..., :full.shape[3]] = torch.from_numpy(full)
            kw["full_mask"] = wide.cuda()[..., :full.shape[3]]
            assert not kw["full_mask"].is_contiguous()
        else:
            kw["full_mask"] = _dev(full)
    return kw


class _State:
    """float64[2] state as the middle of a 4-element tensor: the entry point writes those two elements and nothing around them."""

    def __init__(self):
        self.buf = torch.tensor([GUARD[0], 0.0, 0.0, GUARD[1]], dtype=torch.float64, device="cuda")
        self.state = self.buf[1:3]

    def read(self):
        b = self.buf.cpu().numpy()
        assert b[0] == GUARD[0] and b[3] == GUARD[1], f"the entry point wrote outside state[0..1]: {b}"
        return b[1:3].copy()


# ---- A. the selection, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,storage", INSTANCES)
def test_score_statistics_are_the_exact_order_statistics(ops, dirty, D, storage):
    for c in R.selection_cases(D, storage):
        q, k, want = R.selection_inputs(c)
        ex = R.selection_extras(c)
        tq, tk = _heads(q, storage, c["layout"], 0, 1), _heads(k, storage, c["layout"], 1, 2)
        kw = _mask_kw(ops, ex["base"], ex.get("clip"), ex.get("pad"), ex.get("full"))
        kw.update(scale=c["scale"], scale_div=c["scale_div"], causal=ex.get("causal", False), clamp_min=ex.get("clamp_min", False))
        flat = want.reshape(-1)
        st = _State()
        for pair in R.pairs_for(flat.size):
            dirty()
            ops.attn_calibrate(tq, tk, None, ops.CALIB_SCORES, q_lo=pair[0], q_hi=pair[1], first=True, state=st.state, **kw)
            got, exp = st.read(), np.percentile(flat, pair)
            assert got.dtype == np.float64 and np.array_equal(got, exp), (c["name"], D, storage, pair, got, exp)
        # the running average: two further calls on top of a first one
        m = c["momentum"]
        trail = ((0.1, 99.9), (25.0, 75.0), (0.0, 100.0))
        run = None
        for i, pair in enumerate(trail):
            dirty()
            ops.attn_calibrate(tq, tk, None, ops.CALIB_SCORES, q_lo=pair[0], q_hi=pair[1], momentum=m, first=i == 0, state=st.state, **kw)
            new = np.percentile(flat, pair)
            run = new if run is None else (1.0 - m) * new + m * run
            np.testing.assert_allclose(st.read(), run, rtol=1e-15, atol=0, err_msg=f"{c['name']} momentum {m} call {i}")


# ---- B. probabilities against float64 -------------------------------------------------------------------------------------------
def _value_call_kw(ops, c, x):
    kw = _mask_kw(ops, c["base"], c["clip"], x["pad"], x["full"], c["full"] == "strided")
    kw.update(scale=c["scale"], scale_div=c["scale_div"], causal=c["causal"], clamp_min=c["clamp_min"], scores_range=_range(c["sr"]), n_bits=c["n_bits"])
    return kw


@pytest.mark.parametrize("case", R.VALUE_CASES, ids=VALUE_IDS)
def test_probability_statistics_against_float64(ops, dirty, case):
    ci = VALUE_IDS.index(case["name"])
    worst = 0.0
    for D, storage in (INSTANCES[ci % 9], INSTANCES[(ci + 4) % 9]):
        x, r, p32, _ = R.value_refs(case, D, storage, O)
        e = R.err64(p32, r["probs"])
        layout = R.LAYOUTS[ci % 2]
        tq, tk = _heads(x["q"], storage, layout, 0, 1), _heads(x["k"], storage, layout, 1, 2)
        kw = _value_call_kw(ops, case, x)
        st = _State()
        for pair in R.VALUE_PAIRS:
            dirty()
            ops.attn_calibrate(tq, tk, None, ops.CALIB_PROBS, q_lo=pair[0], q_hi=pair[1], first=True, state=st.state, **kw)
            got, want = st.read(), np.percentile(r["probs"].reshape(-1), pair)
            diff = np.abs(got - want)
            ratio = float(diff.max() / e) if e > 0 else (0.0 if diff.max() == 0 else float("inf"))
            worst = max(worst, ratio)
            print(f"probs {case['name']} D{D} {storage} {pair}: got {got} want {want} err64 {e:.3e} ratio {ratio:.3f}")
            assert (diff <= 4.0 * e + np.spacing(np.abs(want))).all(), (case["name"], D, storage, pair, got, want, e, ratio)
    print(f"probs {case['name']}: largest ratio to err64 {worst:.3f}")


# ---- C. the context -------------------------------------------------------------------------------------------------------------
def _context(ops, case, x, storage, layout, probs_range, k=None, v=None):
    tq = _heads(x["q"], storage, layout, 0, 1)
    tk = _heads(x["k"], storage, layout, 1, 2) if k is None else k
    tv = _heads(x["v"], storage, layout, 2, 2) if v is None else v
    kw = _value_call_kw(ops, case, x)
    ctx = ops.attn_calibrate(tq, tk, tv, ops.CALIB_CONTEXT, probs_range=_range(probs_range), **kw)
    B, H, Sq, D = x["q"].shape
    assert ctx.dtype == torch.float32 and ctx.shape == (B, H, Sq, D) and ctx.permute(0, 2, 1, 3).is_contiguous()  # stored (B,Sq,H,D)
    return ctx


@pytest.mark.parametrize("D,storage", INSTANCES)
def test_context_against_float64(ops, D, storage):
    worst = 0.0
    for ci, case in enumerate(R.VALUE_CASES):
        for pr in (None,) + R.PROB_RANGES:
            x, r, p32, ctx32 = R.value_refs(case, D, storage, O, pr)
            got = _context(ops, case, x, storage, R.LAYOUTS[ci % 2], pr).cpu().numpy().astype(np.float64)
            diff = np.abs(got - r["ctx"])
            label = (case["name"], D, storage, pr)
            if pr is None:
                e = R.err64(ctx32, r["ctx"])
                lim = np.full(diff.shape[:3], 4.0 * e)
                rows = np.zeros(diff.shape[:3], dtype=bool)
            else:
                rows, count, scale = R.band_rows(r, p32, pr, case["n_bits"])
                assert rows.mean() <= R.MAX_BAND_ROWS, label
                e = R.err64(ctx32[~rows], r["ctx"][~rows])
                lim = 4.0 * e + count * scale * float(np.abs(x["v"]).max())
            ratio = float(diff[~rows].max() / e) if e > 0 else (0.0 if diff[~rows].max() == 0 else float("inf"))
            worst = max(worst, ratio)
            print(f"ctx {label}: err64 {e:.3e} ratio {ratio:.3f} band rows {int(rows.sum())} of {rows.size}")
            bad = diff > lim[..., None]
            assert not bad.any(), (label, int(bad.sum()), float(diff.max()), e, ratio)
    print(f"ctx D{D} {storage}: largest ratio to err64 {worst:.3f}")


@pytest.mark.parametrize("D,storage", INSTANCES)
def test_context_ignores_rows_beyond_sk(ops, D, storage):
    """Sk is no multiple of 16: the values of k and v rows beyond Sk, in a larger backing allocation, must not reach the context."""
    for name in ("vanilla", "clip-025-sat-below", "pad-f32-4bit"):
        case = R.VALUE_CASES[VALUE_IDS.index(name)]
        x = R.value_inputs(case, D, storage)
        B, H, Sq, Sk = case["B"], case["H"], case["Sq"], case["Sk"]
        assert Sk % 16 != 0
        back = []
        for a in (x["k"], x["v"]):
            t = torch.zeros(B, H, Sk + 16, D)
            t[:, :, :Sk] = torch.from_numpy(a)
            back.append(t.to(DT[storage]).cuda())
        views = [t[:, :, :Sk] for t in back]
        first = _context(ops, case, x, storage, "contiguous", (0.0, 1.0), *views).clone()
        for t, val in zip(back, (3.0e4, -2.5e4)):
            t[:, :, Sk:] = val
        second = _context(ops, case, x, storage, "contiguous", (0.0, 1.0), *views)
        assert torch.equal(first, second), (name, D, storage)


# ---- D. oeh_percentile_ema ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "fp16"])
def test_percentile_ema_beyond_the_block_cap(ops, storage):
    """n = 2048 * 4096 + 4099: the block count is capped at 2048, every thread of calib_hist_kernel / calib_next_kernel takes a second
    grid stride (and a few a third)."""
    n = 2048 * 4096 + 4099
    x = np.random.default_rng(11).standard_normal(n, dtype=np.float32) * np.float32(3.0)
    x = R.round_storage(x, storage)
    tx = _dev(x, storage)
    for pair in ((0.001, 99.999), (37.5, 50.0)):
        st = _State()
        ops.percentile_ema(tx, pair[0], pair[1], st.state, first=True)
        got, want = st.read(), np.percentile(x, pair)
        assert np.array_equal(got, want), (storage, pair, got, want)


def test_percentile_ema_keeps_subnormals(ops):
    """fp32 subnormals and the smallest normals: the ranks interpolate between two subnormals, whose difference numpy forms in float32 - a
    flush-to-zero anywhere in the selection or in b - a would show."""
    rs = np.random.RandomState(17)
    ints = rs.randint(-2 ** 24, 2 ** 24, size=70001)
    ints[:500] = 0
    ints[500:700] = ints[700]
    x = np.ldexp(ints.astype(np.float64), -149).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), np.ldexp(ints.astype(np.float64), -149))
    tiny = float(np.finfo(np.float32).tiny)
    tx = _dev(x)
    for pair in ((40.003, 60.0), (25.0, 75.0), (0.1, 99.9), (45.003, 50.0), (0.0, 100.0)):
        want = np.percentile(x, pair)
        if pair[0] in (40.003, 45.003):  # strictly between two subnormals: no float32 value
            assert 0.0 < abs(want[0]) < tiny and want[0] != float(np.float32(want[0])), (pair, want)
        st = _State()
        ops.percentile_ema(tx, pair[0], pair[1], st.state, first=True)
        got = st.read()
        assert np.array_equal(got, want), (pair, got, want)
