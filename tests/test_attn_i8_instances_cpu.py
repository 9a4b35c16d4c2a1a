"""The registry and the staged model of tests/_i8_ref.py, checked without a GPU: the cases reach exactly the instances of oeh_attn_i8_kernel
that the library was built with, each at least twice; the ruler of the probability stage (ERR64) is the fp32 oracle's own distance from
float64 on these cases; every case saturates and ties as the registry says; the restated host constants are the float64 values rounded once;
the model agrees with the oracle on the dequantised values within the bound of the statistical tests (tests/test_attn_gpu.py:
test_int8_storage_*), which ties the new ruler to the old one; and the cases of every instance reject a kernel that is wrong in one term.

Power: the model with one thing wrong (`_i8_ref.MUTANTS`) plays the kernel - every stage computed from its own stage before - and its dumps
and output go through the acceptance check the GPU test applies (`_i8_ref.check_stages`).  For every instance and every mutant that is
meaningful for it, at least one of the instance's cases must reject it."""
import numpy as np
import pytest

from oracle import oeh_oracle as O
from tests import _i8_ref as R

F32, F64 = np.float32, np.float64


def test_the_cases_reach_exactly_the_built_instances():
    by, built = R.by_instance(), R.built_instances()
    assert len(built) == 60 and built == {("i8", nt, out, dump, cq2, pad) for nt in (8, 16, 32) for out, dump in ((0, 0), (1, 0), (2, 0), (2, 1), (3, 0))
                                          for cq2 in (0, 1) for pad in (0, 1)}
    assert set(by) == built, (sorted(built - set(by)), sorted(set(by) - built))   # none unreachable, nothing the library was not built with
    for inst, cases in by.items():
        assert len({c["name"] for c, _ in cases}) >= 2, inst
        assert all(R.group_of(c) == (inst[1], inst[4], inst[5]) for c, _ in cases), inst
    assert {R.group_of(c) for c in R.CASES} == set(R.GROUPS)
    for c in R.CASES:
        nt = R.group_of(c)[0]
        for form in R.FORMS:
            assert R.variant_name(c, form) == f"i8mfma/NT{nt}/D64/{'f32' if form == 'dump' else form}", (c["name"], form)
    print(f"{len(built)} instances, {len(R.CASES)} problems, {len(R.CASES) * len(R.FORMS)} launches of distinct (problem, form)")


def test_the_registry_holds_what_it_lists():
    """The shapes, layouts, zero points, masks and options the cases are there for: one assertion per item, so that a case cannot leave quietly."""
    cs = R.CASES
    for nt, want in ((8, {16, 48, 80, 128}), (16, {144, 208, 256}), (32, {272, 384, 400, 464, 512})):
        assert {c["Sk"] for c in cs if R.group_of(c)[0] == nt} == want
    assert any(c["Sq"] % 16 for c in cs) and any(c["Sq"] == 77 for c in cs)
    assert any(c["causal"] and c["Sq"] < c["Sk"] for c in cs) and any(c["causal"] and c["Sq"] == c["Sk"] == 512 for c in cs)
    assert {1, 6, 17} <= {c["B"] * c["H"] for c in cs}
    assert {c["layout"] for c in cs} == {"bshe", "bhsd"} and any(c["cache"] for c in cs) and any(c["guard"] for c in cs)
    assert {0.0, 255.0, 128.0, 97.0} <= {c["zq"] for c in cs}
    for z in ("zk", "zv"):
        vals = {c[z] for c in cs}
        assert {0.0, 255.0, 128.0} <= vals and any(0 < v < 128 for v in vals) and any(128 < v < 255 for v in vals)
    assert {c["zs"] for c in cs} == {100.0, 128.0, 140.0} and {c["zpp"] for c in cs} == {0.0, 7.0}
    for nt in (8, 16, 32):
        assert any(c["tie"] and R.prep(c)["k1"] == F32(2.0 ** -7) for c in cs if R.group_of(c)[0] == nt)
    assert {(c["pad"] is not None, c["causal"]) for c in cs} == {(False, False), (False, True), (True, False), (True, True)}
    pads = [c["pad"] for c in cs if c["pad"] is not None]
    assert {p[0] for p in pads} == {"f16", "f32"}
    rows = [r for p in pads for r in p[1]]
    assert {r[0] for r in rows} == {"none", "right", "left", "full"} and {R.FMIN32, R.FMIN16, -1.0e4} <= {r[2] for r in rows}
    assert any(r[0] in ("right", "left") and r[1] % 64 == 0 for r in rows)   # a whole 64-key tile padded
    assert {c["base"] for c in cs if c["pad"] is not None and any(r[0] == "full" for r in c["pad"][1])} == {0, 1}
    assert {(c["base"], c["clip"]) for c in cs} >= {(0, None), (1, None), (0, R.CLIP_A), (0, R.CLIP_B)}
    assert any(c["scale_div"] == 8.0 for c in cs) and any(c["scale_div"] == R.DIV for c in cs) and any(c["scale_div"] == 0.0 for c in cs)
    assert {c["gate"] for c in cs} == {None, "token", "head"}
    assert any(c["gc"] is None for c in cs) and any(c["gc"] and c["gate"] and c["before"] for c in cs) and any(c["gc"] and c["gate"] and not c["before"] for c in cs) and any(c["emit"] for c in cs)
    for c in cs:   # the slices stay inside their allocations: the geometry `descriptor` and the GPU test share
        assert c["cache"] >= 0 and c["guard"] in (0, 1)


def test_err64_band_share_saturation_and_ties():
    worst, share = 0.0, 0.0
    for c in R.CASES:
        p = R.prep(c)
        s_idx = R.stage1(c)
        pr, t, _ = R.stage2(c, s_idx)
        worst = max(worst, R.err64_of(c))
        band = float(R.band_of(c, t).mean())
        assert band <= R.BAND_SHARE, (c["name"], "share of the probability indices inside the band", band)
        share = max(share, band)
        lo, hi = float((s_idx == 0).mean()), float((s_idx == 255).mean())
        assert 0.005 <= lo <= 0.05 and 0.005 <= hi <= 0.05, (c["name"], "saturated scores at either end", lo, hi)
        tk = p["S"] * F64(p["k1"])
        ties = float((np.abs(tk - np.floor(tk)) == 0.5).mean())
        assert (0.005 <= ties <= 0.012) if c["tie"] else ties == 0.0, (c["name"], "exact ties S k1 = n + 1/2", ties)
        assert np.abs(tk).max() < 2 ** 22
    print(f"err64 {worst:.3e}, largest share of a case's probability indices inside the band {share:.2e}")
    # what the GPU test uses IS this number, and it is the size of a few fp32 roundings of a probability (<= 1): 2^-24 = 6e-8 each
    assert R.err64() == worst and 2.0 ** -24 <= worst <= 8 * 2.0 ** -24, (worst, R.err64())


def test_restated_host_constants():
    for c in R.CASES:
        g, p = R.grids(c), R.prep(c)
        mult = F64(F32(c["scale"])) if c["scale_div"] == 0.0 else 1.0 / F64(F32(c["scale_div"]))
        k64 = F64(F32(g["q"][0])) * F64(F32(g["k"][0])) * mult / F64(F32(g["s"][0]))
        assert abs(F64(p["k1"]) - k64) <= 2.0 ** -24 * k64, c["name"]
        s64 = F64(F32(g["p"][0])) * F64(F32(g["v"][0]))
        assert abs(F64(R.so_of(g["p"][0], g["v"][0])) - s64) <= 2.0 ** -24 * s64, c["name"]


def _deq(idx, step, zp):
    return ((idx.astype(F32) - F32(zp)) * F32(step)).astype(F32)


def test_model_agrees_with_the_oracle_on_dequantised_values():
    """The bound of tests/test_attn_gpu.py's INT8 tests: an output at most one context-grid step (times the gate) from the oracle's, and at most
    5e-4 of the outputs off it at all.  The share is taken over the registry as a whole: these cases are small (one row whose probabilities hold
    a tie between fp32 and float64 is 64 outputs, 2e-3 of the smallest case), the tests that bound was set on have 2e5 outputs each.  (Without a
    context quantiser the outputs are no grid points: they count for the share alone.)"""
    n_off, n_all, worst = 0, 0, (0.0, None)
    for c in R.CASES:
        p, g = R.prep(c), R.grids(c)
        Sk = c["Sk"]
        qd = _deq(p["qi"], *g["q"])
        kd, vd = _deq(p["ki"][:, :, :Sk], *g["k"]), _deq(p["vi"][:, :, :Sk], *g["v"])
        kw = dict(base=c["base"], causal=c["causal"], clamp_min=True, mask_min=R.FMIN32, fq_scores=g["s"], fq_probs=g["p"], fq_ctx=g["c"], ctx_quant_before_gate=c["before"])
        if c["scale_div"] != 0.0:
            kw.update(scale=c["scale_div"], scale_is_divisor=True)
        else:
            kw.update(scale=c["scale"])
        if c["clip"] is not None:
            kw.update(clip=True, gamma=c["clip"][0], eta=c["clip"][1])
        if p["pad"] is not None:
            kw["pad_mask"] = p["pad"].astype(F32)
        if p["gate"] is not None:
            kw["gate"] = p["gate"]
        want = O.attn_core(qd, kd, vd, **kw)
        got = R.run_model(dict(c, emit=False))[3]
        err = np.abs(got.astype(F64) - want.astype(F64))
        off = err > 1e-6 + 1e-5 * np.abs(want)
        n_off, n_all = n_off + int(off.sum()), n_all + off.size
        worst = max(worst, (float(off.mean()), c["name"]))
        if g["c"] is not None:
            step = g["c"][0] * (1.0 if p["gate"] is None or not c["before"] else float(p["gate"].max()))
            assert err.max() <= 1.01 * step + 1e-6, (c["name"], "more than one context step from the oracle", float(err.max()), step)
    print(f"outputs off the oracle's: {n_off} of {n_all} ({n_off / n_all:.2e}); largest share of one case {worst[0]:.2e} ({worst[1]})")
    assert n_off <= 5e-4 * n_all, (n_off, n_all)


def meaningful(inst):
    """The mutants an instance can be wrong in: what its template arguments compile in, and what its launches read at run time."""
    _, _, out, _, cq2, pad = inst
    m = set(R.MUTANTS)
    if not cq2:
        m.discard("cq2-64-added-once")
    if not pad:
        m -= {"pad-boundary-plus-1", "1e4-visible"}
    if out == 3:   # the int8 output is the context quantiser's integers: that quantiser is the last operation
        m.discard("ctx-quantiser-other-side")
    return m


@pytest.mark.parametrize("group", R.GROUPS, ids=R.GROUP_IDS)
def test_the_model_passes_its_own_check_and_every_meaningful_mutant_is_rejected(group):
    misses = []
    runs = {}

    def run(c, kind):
        key = (c["name"], c["emit"], kind)
        if key not in runs:
            runs[key] = R.run_model(c, kind)
        return runs[key]
    for inst, cases in sorted(R.by_instance().items()):
        if (inst[1], inst[4], inst[5]) != group:
            continue
        for c, form in cases:
            R.check_stages(R.form_case(c, form), *run(R.form_case(c, form), None))
        for kind in sorted(meaningful(inst)):
            tried, rejected = 0, False
            for c, form in cases:
                c = R.form_case(c, form)
                if not R.exercises(c, kind):
                    continue
                tried += 1
                try:
                    R.check_stages(c, *run(c, kind))
                except AssertionError:
                    rejected = True
                    break
            assert tried, (inst, kind, "no case of the instance exercises the term")
            if not rejected:
                misses.append((inst, kind))
    assert not misses, ("mutants that pass every case of an instance", misses)
