"""The yardsticks of tests/test_attn_calibrate_gpu.py, checked without a GPU on the very cases that file runs: the float64 restatement
(tests/_calib_ref.py) against the fp32 oracle, the order-statistic property every tolerance there rests on, the exactness of the
selector-query inputs, and the tie-band cap of the context cases with a probability quantiser.

Bounds of the reference against the oracle ("the oracle's own rounding"; u = 2^-24, Sk keys):
  scores         equal: both input families give scores that every summation order computes exactly
  probabilities  (Sk + 8) u: one rounding each for x - max, the exponential (1 ulp), the division, the clip's multiply and add, and at
                 most Sk u relative for the fp32 sum of Sk terms, all on values <= 1
  context        4 (Sk + 8) u max|v|: the probabilities' error against sum |v| p, the clip's absolute roundings summed over Sk keys,
                 the fp32 accumulation of P V - each at most (Sk + 8) u max|v| - and one such share for the quantiser's fp32 scale
                 multiply (rows of the tie band excepted: there the oracle itself may sit on the other grid point)
Measured over all cases: the order statistics move by at most 1.0 err64 (reached, by an extreme); the largest tie band holds 4.2 % of
a case's rows (cap: 5 %)."""
import numpy as np
import pytest

from oracle import oeh_oracle as O
from tests import _calib_ref as R

U = 2.0 ** -24
INSTANCES = [(D, st) for D in R.HEAD_DIMS for st in R.STORAGES]
VALUE_IDS = [c["name"] for c in R.VALUE_CASES]


def _oracle_kw(c, extras):
    kw = dict(base=extras.get("base", 1), pad_mask=extras.get("pad"), full_mask=extras.get("full"), causal=extras.get("causal", False),
              clamp_min=extras.get("clamp_min", False), mask_min=R.FMIN32)
    if extras.get("clip") is not None:
        kw.update(gamma=extras["clip"][0], eta=extras["clip"][1], clip=True)
    if c["scale_div"] != 0.0:
        kw.update(scale=c["scale_div"], scale_is_divisor=True)
    else:
        kw.update(scale=c["scale"])
    return kw


def test_helpers_restate_the_contract():
    """The score ranges of the value cases give grids with power-of-two steps; bf16 rounding is ties-to-even on the upper 16 bits; the frac-0 pairs
    really have frac 0 as the entry point computes it."""
    assert R.grid_from_range(-8.0, 247.0) == (1.0, 8.0, 255.0)
    assert R.grid_from_range(-250.0, 5.0) == (1.0, 250.0, 255.0)
    assert R.grid_from_range(-8.0, 7.0, 4) == (1.0, 8.0, 15.0)
    assert R.grid_from_range(-12.0, 19.875) == (0.125, 96.0, 255.0)
    assert R.grid_from_range(0.0, 1.0)[0] == float(np.float32(1.0 / 255.0))
    assert R.grid_from_range(0.25, 0.5)[:2] == (float(np.float32(0.5 / 255.0)), 0.0) and R.grid_from_range(-1.0, -0.5, eps=1e-8)[1] == 255.0
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -7, 1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=np.float32)
    assert np.array_equal(R.round_storage(x, "bf16"), np.array([1.0, 1.0, 1.0 + 2.0 ** -6, -1.0 - 2.0 ** -7, 1.0 + 2.0 ** -7], dtype=np.float32))
    for st in R.STORAGES:
        a = R.round_storage(np.array([0.3, -0.7, 1.0, -2.0, 1.999], dtype=np.float32), st)
        b = R.next_representable(a, st)
        assert np.array_equal(R.round_storage(b, st), b) and (b > a).all() and (b - a <= np.abs(a) * 2.0 ** -R.MANT_BITS[st]).all()
    for n in (1, 6, 270, 1440, 6426, 12870, 13056, 135000):
        for q in R.frac0_pair(n):
            assert 0.0 <= q <= 100.0 and R.virtual_index(n, q)[1] == 0.0
        i_lo, i_hi = R.virtual_index(n, R.frac0_pair(n)[0])[0], R.virtual_index(n, R.frac0_pair(n)[1])[0]
        assert n < 6 or 0 < i_lo < i_hi < n - 1


@pytest.mark.parametrize("D,storage", INSTANCES)
def test_selector_queries_are_exact(D, storage):
    """The selector-query (and small-integer) inputs hold values of their storage type, and the oracle's fp32 matmul reproduces the
    gather - the exactly known score tensor - bit for bit; so does the float64 restatement."""
    for c in R.selection_cases(D, storage):
        if c["layout"] != "contiguous":
            continue  # (the layout changes nothing on the host)
        q, k, want = R.selection_inputs(c)
        assert np.array_equal(R.round_storage(q, storage), q) and np.array_equal(R.round_storage(k, storage), k), c["name"]
        assert np.isfinite(want).all() and (c["family"] != "selector" or (np.abs(want[want != 0]) >= 2.0 ** -100).all())
        _, o = O.attn_core(q, k, k, want=("scores",), **_oracle_kw(c, {}))
        assert o["scores"].dtype == np.float32 and np.array_equal(o["scores"], want), c["name"]
        assert np.array_equal(R.attn64(q, k, scale=c["scale"], scale_div=c["scale_div"])["scores"], want.astype(np.float64)), c["name"]
        if c["family"] == "selector" and c["Sk"] >= 8:  # duplicates and one-spacing neighbours are really there
            flat = np.sort(want.reshape(-1))
            gaps = np.diff(flat)
            assert (gaps == 0).any() and (gaps[gaps > 0] <= np.spacing(np.abs(flat[:-1][gaps > 0])) * 2.0 ** (23 - R.MANT_BITS[storage])).any(), c["name"]
        if c["family"] == "integer" and c["Sq"] * c["Sk"] >= 1000:
            assert 20 <= len(np.unique(want)) <= 160, (c["name"], len(np.unique(want)))


@pytest.mark.parametrize("D,storage", INSTANCES)
def test_reference_agrees_with_the_oracle_on_the_selection_cases(D, storage):
    """The masked / clipped selection cases through the whole chain: probabilities within (Sk + 8) u of the oracle's."""
    for c in R.selection_cases(D, storage):
        if c["layout"] != "contiguous" or c["extras"] == "none":
            continue
        q, k, _ = R.selection_inputs(c)
        ex = R.selection_extras(c)
        r = R.attn64(q, k, scale=c["scale"], scale_div=c["scale_div"], **ex)
        _, o = O.attn_core(q, k, k, want=("probs",), **_oracle_kw(c, ex))
        assert R.err64(o["probs"], r["probs"]) <= (c["Sk"] + 8) * U, (c["name"], R.err64(o["probs"], r["probs"]))


@pytest.mark.parametrize("case", R.VALUE_CASES, ids=VALUE_IDS)
def test_reference_agrees_with_the_oracle_on_the_value_cases(case):
    """Probabilities and context of every value case, every head dim and storage type, with and without the probability quantiser."""
    for D, storage in INSTANCES:
        for pr in (None,) + R.PROB_RANGES:
            x, r, p32, ctx32 = R.value_refs(case, D, storage, O, pr)
            assert np.isfinite(r["probs"]).all() and np.isfinite(r["ctx"]).all()
            assert R.err64(p32, r["probs"]) <= (case["Sk"] + 8) * U, (case["name"], D, storage, R.err64(p32, r["probs"]))
            keep = slice(None)
            if pr is not None:
                keep = ~R.band_rows(r, p32, pr, case["n_bits"])[0]
            lim = 4 * (case["Sk"] + 8) * U * float(np.abs(x["v"]).max())
            assert R.err64(ctx32[keep], r["ctx"][keep]) <= lim, (case["name"], D, storage, pr, R.err64(ctx32[keep], r["ctx"][keep]), lim)


@pytest.mark.parametrize("case", R.VALUE_CASES, ids=VALUE_IDS)
def test_order_statistics_move_no_further_than_the_values(case):
    """Order statistics, and their linear interpolation, are 1-Lipschitz in the max norm: the percentiles of the oracle's fp32
    probabilities lie within err64 of the float64 reference's.  The GPU file's tolerance for the probability statistics rests on it."""
    for D, storage in INSTANCES:
        _, r, p32, _ = R.value_refs(case, D, storage, O)
        e = R.err64(p32, r["probs"])
        for pair in R.VALUE_PAIRS + ((0.0, 100.0), (0.1, 99.9)):
            got = np.percentile(p32.reshape(-1), pair)
            want = np.percentile(r["probs"].reshape(-1), pair)
            assert got.dtype == np.float64 and (np.abs(got - want) <= e).all(), (case["name"], D, storage, pair, got, want, e)


@pytest.mark.parametrize("case", R.VALUE_CASES, ids=VALUE_IDS)
def test_tie_band_stays_within_its_cap(case):
    """Context cases with the probability quantiser: the rows that hold a probability within 4 err64 / scale of a rounding boundary
    are at most 5 % of the (B,H,Sq) rows - a condition on the inputs, asserted on the two references alone."""
    for D, storage in INSTANCES:
        for pr in R.PROB_RANGES:
            _, r, p32, _ = R.value_refs(case, D, storage, O, pr)
            rows, _, _ = R.band_rows(r, p32, pr, case["n_bits"])
            assert rows.mean() <= R.MAX_BAND_ROWS, (case["name"], D, storage, pr, float(rows.mean()))
