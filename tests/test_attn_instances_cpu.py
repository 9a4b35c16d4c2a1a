"""The registry of tests/_attn_inst.py, checked without a GPU: the cases reach exactly the instances of the one-pass, full-row and general
attention kernels that the library was built with, under the names they claim; the fp32 oracle meets the acceptance checks of every case
(the yardsticks tests/test_plan_instances_gpu.py applies to the kernels); and the cases of every instance have the power to reject a
kernel that is wrong in one term.

Power: the float64 chain with one thing wrong (MUTANTS), rounded to the storage type, is fed to the same acceptance check.  For every
instance and every mutant that is meaningful for it (`meaningful`), at least one of the instance's cases must reject it.  The mutants are
posed as inputs of the unchanged chain: a key is dropped by a mask entry, the causal limit and the padding boundary are moved in the masks,
softmax_1's "+1" is dropped by base 0 and doubled by one more key with a zero score and a zero value."""
import numpy as np
import pytest

from oracle import oeh_oracle as O
from tests import _attn_inst as I
from tests import _attn_ref as A

pytest.importorskip("torch")

MUTANTS = ("plus1-dropped", "plus1-doubled", "last-key-dropped", "tile-first-key-dropped", "causal-limit-plus-1", "causal-limit-minus-1",
           "pad-boundary-plus-1", "eta-minus-gamma-is-1", "gamma-is-0", "gate-not-applied", "ctx-quantiser-on-the-other-side-of-the-gate")
GROUPS, GROUP_IDS = I.GROUPS, I.GROUP_IDS


def meaningful(inst):
    """The mutants an instance can be wrong in: what its template arguments compile in, and what its launches read at run time."""
    fam = inst[0]
    m = set(MUTANTS[:6])
    clip = {"fast": lambda: inst[4], "flash": lambda: inst[7] == 1, "hot": lambda: 0, "mfma": lambda: 1}[fam]()
    pad = {"fast": lambda: inst[6] != 1, "flash": lambda: inst[4], "hot": lambda: 0, "mfma": lambda: inst[4] != 1}[fam]()
    fq = {"fast": lambda: inst[6], "flash": lambda: 2 if inst[7] == 2 else 0, "hot": lambda: 0, "mfma": lambda: inst[4]}[fam]()
    if pad:
        m.add("pad-boundary-plus-1")
    if clip:
        m |= {"eta-minus-gamma-is-1", "gamma-is-0"}
    m.add("gate-not-applied")  # (gate values are a run-time branch of every instance's epilogue; the in-kernel predictor's output likewise)
    if fq and not (fam == "fast" and fq == 2):
        m.add("ctx-quantiser-on-the-other-side-of-the-gate")
    return m


def test_the_cases_reach_exactly_the_built_instances():
    by = I.by_instance()
    built = I.built_instances()
    assert len({c["name"] for c in I.CASES}) == len(I.CASES)
    assert set(by) | set(I.UNREACHABLE) == built, (sorted(built - set(by) - set(I.UNREACHABLE)), sorted((set(by) | set(I.UNREACHABLE)) - built))
    assert not set(by) & set(I.UNREACHABLE)
    assert set(I.GROUPS) == {I.group_of(i) for i in built}
    for inst, cases in by.items():
        assert len(cases) >= 2, inst
        # causal and non-causal, base 0 and 1 (the one-pass INT8 chain takes padded keys under softmax_1 only: oeh_api.hip, flash_two_pass_can)
        assert {c["causal"] for c in cases} == {False, True}, inst
        assert {c["base"] for c in cases} == ({1} if inst[0] == "flash" and inst[4] and inst[7] == 2 else {0, 1}), inst
        assert all(c["B"] == 2 and c["H"] == 3 for c in cases)
        assert all(c["Sq"] < c["Sk"] for c in cases if c["causal"])
        if (inst[0] in ("fast", "flash") and inst[5]):
            assert {c["gate_units"] for c in cases} == {0, 48}, inst
    lay = {}
    for inst, cases in by.items():
        lay.setdefault(I.group_of(inst), set()).update(c["layout"] for c in cases)
    assert all(len(v) >= 3 for v in lay.values()), lay
    print(f"{len(built)} instances, {len(I.CASES)} cases, {len(I.UNREACHABLE)} unreachable")


def test_every_case_names_the_kernel_it_claims():
    lib = I._lib()
    for c in I.CASES:
        assert I.variant_name(lib, c) == c["kernel"], c["name"]


def test_every_census_name_of_the_three_families_occurs():
    import os

    names = set()
    with open(os.path.join(I.ROOT, "tests", "golden", "dispatch_census.txt")) as fh:
        for line in fh:
            for n in line.split(" | ")[1].split()[0].split(","):
                if n.startswith(("fast16/", "flash16/", "mfma16/")):
                    names.add(n)
    assert len(names) > 200
    assert names <= {c["kernel"] for c in I.CASES}, sorted(names - {c["kernel"] for c in I.CASES})


def _true_dumps(c, r):
    w = r["w"]
    if not (c["gs"] or c["gp"] or c["gc"]):
        return None
    return {k: None if w[k + "_idx"] is None else w[k + "_idx"].astype(np.uint8) for k in ("scores", "probs", "ctx")}


def _own_dumps(c, r):
    """The indices of the fp32 oracle's own values: what a run of the oracle would dump."""
    if not (c["gs"] or c["gp"] or c["gc"]):
        return None
    o, (gs, gp, gc) = r["o"], r["grids"]
    return {k: None if g is None else A.index64(o[key], *g).astype(np.uint8) for k, key, g in (("scores", "scores", gs), ("probs", "probs", gp), ("ctx", "ctx_pre", gc))}


def _accept(c, r, got, dumps):
    """The acceptance check tests/test_plan_instances_gpu.py applies to the case."""
    if dumps is not None and c["Sk"] > 512:
        return A.check_contract_long(c, r, got, dumps)
    return A.check_contract(c, r, got, dumps)


def _stored(c, a):
    """What a kernel would store of a: the storage type's rounding (fp32 output of 16-bit storage keeps the accumulators)."""
    return np.asarray(a, dtype=np.float64) if c["out32"] else A.R.round_storage(np.asarray(a, dtype=np.float32), c["storage"]).astype(np.float64)


@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_oracle_meets_the_yardsticks(group):
    """Conditions, not measurements: the fp32 oracle, rounded to the storage type, passes the acceptance check of every case against
    float64 with at most 10 % of a case's rows left out and at most 1 % of a dump inside a tie band."""
    worst = 0.0
    for inst, cases in sorted(I.by_instance().items()):
        if I.group_of(inst) != group:
            continue
        for c in cases:
            r = A.refs(c, O)
            for key in ("scores", "probs", "ctx_pre", "ctx"):
                assert not np.isnan(r["w"][key]).any(), (c["name"], key)
            if c["gs"] or c["gp"] or c["gc"]:
                A.conditions(c, r)
            got = _stored(c, r["o"]["ctx"])
            if c["gs"] or c["gp"] or c["gc"]:  # the rows and elements downstream of a tie band are what the conditions above leave out
                got = np.where(r["rows_p"][..., None] | r["band_c"], r["w"]["ctx"], got)
            ratio = _accept(c, r, got, _own_dumps(c, r))
            assert ratio <= 1.0, (c["name"], ratio)
            worst = max(worst, ratio)
    print(f"{group}: the oracle's largest share of a limit {worst:.3f}")


# ---- power ----------------------------------------------------------------------------------------------------------------------------
def _tile(c):
    return 16 if c["kernel"].startswith("mfma16/") else 64  # keys per tile of the kernel's key loop


def mutant(c, x, kind):
    """The output of the float64 chain with `kind` wrong, or None where the case does not exercise that term."""
    Sq, Sk, B = c["Sq"], c["Sk"], c["B"]
    mmin = float(np.float32(c["mask_min"]))
    q, k, v = x["q"], x["k"], x["v"]
    pad = None if x["pad"] is None else np.asarray(x["pad"], dtype=np.float32).astype(np.float64)
    full = None if x["full"] is None else np.asarray(x["full"], dtype=np.float32).astype(np.float64)
    kw = dict(gate=x["gate"], ctx_grid=A.grid(c, "gc"), ctx_before_gate=c["before"], ctx_emit_index=c["emit"], scores_grid=A.grid(c, "gs"),
              probs_grid=A.grid(c, "gp"), scale=c["scale"], scale_div=c["scale_div"], causal=c["causal"], clamp_min=c["clamp_min"],
              mask_min=c["mask_min"], base=c["base"], clip=c["clip"])

    def explicit_causal(shift, cols):
        i = np.arange(Sq)[:, None] + (Sk - Sq) + shift
        m = np.where(np.arange(cols)[None, :] > i, mmin, 0.0)
        m[:, Sk:] = 0.0
        return np.broadcast_to(m[None, None], (B, 1, Sq, cols)).copy()

    def add_full(extra):
        return extra if full is None else full + extra

    if kind in ("plus1-dropped", "plus1-doubled"):
        if c["base"] != 1:
            return None
        if kind == "plus1-dropped":
            kw["base"] = 0
        else:  # one more key with score 0 and value 0, visible to every row
            z = np.zeros(k.shape[:2] + (1, k.shape[3]), dtype=k.dtype)
            k, v = np.concatenate([k, z], axis=2), np.concatenate([v, z], axis=2)
            pad = None if pad is None else np.concatenate([pad, np.zeros((B, 1))], axis=1)
            full = None if full is None else np.concatenate([full, np.zeros((B, 1, Sq, 1))], axis=3)
            if c["causal"]:
                kw["causal"] = False
                full = add_full(explicit_causal(0, Sk + 1))
    elif kind in ("last-key-dropped", "tile-first-key-dropped"):
        j = Sk - 1 if kind == "last-key-dropped" else _tile(c) * ((Sk - 1) // _tile(c))
        extra = np.zeros((B, 1, Sq, Sk))
        extra[..., j] = -1.0e300
        full = add_full(extra)
    elif kind in ("causal-limit-plus-1", "causal-limit-minus-1"):
        if not c["causal"]:
            return None
        kw["causal"] = False
        full = add_full(explicit_causal(1 if kind.endswith("plus-1") else -1, Sk))
    elif kind == "pad-boundary-plus-1":
        if pad is None:
            return None
        pad = pad.copy()
        for b in range(B):
            hidden = np.nonzero(pad[b] != 0.0)[0]
            if hidden.size:
                pad[b, hidden[0]] = 0.0
    elif kind in ("eta-minus-gamma-is-1", "gamma-is-0"):
        if c["clip"] is None:
            return None
        g, e = c["clip"]
        kw["clip"] = (g, g + 1.0) if kind == "eta-minus-gamma-is-1" else (0.0, e - g)
    elif kind == "gate-not-applied":
        if x["gate"] is None:
            return None
        kw["gate"] = None
    elif kind == "ctx-quantiser-on-the-other-side-of-the-gate":
        if x["gate"] is None or c["gc"] is None or c["emit"]:
            return None
        kw["ctx_before_gate"] = not c["before"]
    return A.chain64(q, k, v, pad=pad, full=full, **kw)["ctx"]


@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_the_cases_of_every_instance_reject_every_meaningful_mutant(group):
    misses = []
    for inst, cases in sorted(I.by_instance().items()):
        if I.group_of(inst) != group:
            continue
        for kind in MUTANTS:
            if kind not in meaningful(inst):
                continue
            rejected, tried = False, 0
            for c in cases:
                r = A.refs(c, O)
                out = mutant(c, r["x"], kind)
                if out is None:
                    continue
                tried += 1
                try:
                    _accept(c, r, _stored(c, out), _true_dumps(c, r))
                except AssertionError as e:  # only the output check counts: a non-finite row or an index check is no rejection
                    if len(e.args[0]) > 1 and e.args[0][1] == "output":
                        rejected = True
                        break
            assert tried, (inst, kind, "no case of the instance exercises the term")
            if not rejected:
                misses.append((inst, kind, [c["name"] for c in cases]))
    assert not misses, ("mutants that pass every case of an instance", misses)
