"""The yardsticks of tests/test_attn_small_gpu.py and tests/test_attn_generic_gpu.py, checked without a GPU on the very cases those files run
(tests/_attn_ref.py): the fp32 oracle against the float64 chain per stage, the conditions on the quantiser cases, the acceptance checks
fed with the oracle's own results, the route table through oeh_attn_variant on the real descriptors, the any-shape kernel's LDS bound and
the two hook bits that switch the kernels of last resort off.

Bounds of the oracle against the chain (u = 2^-24; D head dims, Sk keys; |s| the largest score, |v| the largest value):
  scores         (D + 2) u |q|.|k| |scale|: the fp32 dot product and the scaling
  probabilities  (Sk + 8) u + 2 e_scores: as tests/test_attn_calibrate_cpu.py, plus the scores' own error through exp (a relative 2 e_scores
                 on values <= 1); the exponent range of softmax_1's exp(-m) term included
  context        the oracle's accumulation of P V and the probabilities' error against sum |v|: 4 (Sk + 8) u |v| + 2 Sk e_probs |v|
Measured over all cases: see the test's printout (-s); every bound holds with a factor of 2 or more to spare."""
import ctypes as C

import numpy as np
import pytest

from oracle import oeh_oracle as O
from tests import _attn_ref as A

torch = pytest.importorskip("torch")

ALL_CASES = A.SMALL_CASES + A.GENERIC_CASES + A.ROUTE_CASES
IDS = [c["name"] for c in ALL_CASES]


def test_case_names_are_unique_and_cover_the_lists():
    assert len(set(IDS)) == len(IDS)
    small = A.SMALL_CASES
    assert {(c["D"], c["Sk"] <= 32, c["storage"]) for c in small} == {(D, s, st) for D in (16, 32, 64) for s in (True, False) for st in A.R.STORAGES}
    assert {c["Sk"] for c in small} >= {1, 3, 5, 15, 16, 17, 31, 32, 33, 48, 63, 64} and {c["Sq"] for c in small} >= {1, 15, 16, 17, 32, 33, 49, 64}
    assert {c["H"] for c in small} >= {1, 3, 4} and all(c["Sq"] <= 64 and c["Sk"] <= 64 for c in small)
    # the launcher's three forms (csrc/oeh_attn_small.hip: launch_small_et_st): nqb == 1; a wave per block with nqb 2, 3, 4; whole problems, nqb > 1
    nqb = lambda c: (c["Sq"] + 15) // 16  # noqa: E731
    assert {nqb(c) for c in small if c["B"] * c["H"] < 2048} >= {1, 2, 3, 4} and any(c["B"] * c["H"] >= 2048 and nqb(c) > 1 for c in small)
    assert any(c["B"] * c["H"] == 1 and nqb(c) > 1 for c in small)
    assert any((c["B"] * c["H"] * nqb(c)) % 4 != 0 and nqb(c) > 1 for c in small) and any(c["B"] * c["H"] % 4 != 0 and c["B"] * c["H"] >= 2048 for c in small)
    assert {c["Sk"] for c in small if c["clip"] and c["clip"][0] > 0} >= {5, 17, 33}
    gen = A.GENERIC_CASES
    assert {c["storage"] for c in gen} == set(A.R.STORAGES) and {c["D"] for c in gen} >= {8, 48, 80, 127, 144, 200}
    assert {c["Sk"] for c in gen} >= {1, 5, 127, 128, 129, 300, 513, 700}
    assert all(c["Sk"] <= 130 for c in ALL_CASES if c["dumps"] and not c["name"].endswith(("long-peaked", "-513")))


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_oracle_against_the_float64_chain(case):
    c, r = case, A.refs(case, O)
    w, x = r["w"], r["x"]
    for key in ("scores", "probs", "ctx_pre", "ctx"):
        assert not np.isnan(w[key]).any(), (c["name"], key, "NaN in float64: outside the contract")
    u, Sk, D = A.U, c["Sk"], c["D"]
    mult = abs(1.0 / c["scale_div"] if c["scale_div"] != 0.0 else c["scale"])
    qk = float(np.max(np.matmul(np.abs(x["q"].astype(np.float64)), np.swapaxes(np.abs(x["k"].astype(np.float64)), -1, -2))))
    vmax = float(np.abs(x["v"]).max())
    gmax = 1.0 if x["gate"] is None else float(np.abs(x["gate"]).max())
    assert r["e_scores"] <= (D + 2) * u * qk * mult, (c["name"], r["e_scores"])
    assert r["e_probs"] <= (Sk + 8) * u + 2.0 * r["e_scores"], (c["name"], r["e_probs"], r["e_scores"])
    assert r["e_pre"] <= (4 * (Sk + 8) * u + 2.0 * Sk * r["e_probs"]) * vmax * gmax, (c["name"], r["e_pre"])
    print(f"{c['name']}: err64 scores {r['e_scores']:.2e} probs {r['e_probs']:.2e} ctx {r['e_pre']:.2e} out {r['e_out']:.2e}")
    if c["gs"] or c["gp"] or c["gc"]:
        print("   shares", A.conditions(c, r))
    # the acceptance check passes the oracle itself, with a ratio of at most 1 by construction
    o = r["o"]
    got = o["ctx"].astype(np.float64)
    exact = c["kernel"] == "generic" or c["kernel"].startswith("small/")
    if exact:
        assert A.check_exact(c, r, A.R.round_storage(got, c["storage"]).astype(np.float64)) <= 1.0
    else:
        dumps = None
        if c["gs"] or c["gp"] or c["gc"]:
            dumps = {k: None if w[k + "_idx"] is None else w[k + "_idx"].astype(np.uint8) for k in ("scores", "probs", "ctx")}
        assert A.check_contract(c, r, A.R.round_storage(got, c["storage"]).astype(np.float64), dumps) <= 1.0


def test_fully_masked_samples_and_rows():
    """A sample with every key padded under clamp_min: uniform rows (vanilla), exactly 0 (softmax_1); rows whose every key the causal
    mask hides (Sq > Sk) likewise."""
    by = {c["name"]: c for c in A.GENERIC_CASES}
    for name, uniform in (("generic-masked-sample-vanilla", True), ("generic-masked-sample-softmax1", False)):
        r = A.refs(by[name], O)
        p = r["w"]["probs"][1]
        assert np.array_equal(p, np.full(p.shape, 1.0 / by[name]["Sk"])) if uniform else not p.any()
    for name, uniform in (("generic-causal-tall-vanilla", True), ("generic-d64-hook-causal-tall", False)):
        c = by[name]
        p = A.refs(c, O)["w"]["probs"][:, :, :c["Sq"] - c["Sk"]]
        assert p.size and (np.array_equal(p, np.full(p.shape, 1.0 / c["Sk"])) if uniform else not p.any())


# ---- routes, on the real descriptors ------------------------------------------------------------------------------------------------
def _descriptor(ops, c, x):
    """The descriptor ops.attn_fwd builds for the case (the `_prepared` form hands it back and launches nothing), from CPU tensors: the checks
    that want a GPU are bypassed, no kernel runs."""
    DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DT[c["storage"]])  # noqa: E731
    sm = ops.SoftmaxSpec(base=c["base"]) if c["clip"] is None else ops.SoftmaxSpec(base=c["base"], clip=True, gamma=c["clip"][0], eta=c["clip"][1])
    kw = dict(softmax=sm, scale=c["scale"], scale_div=c["scale_div"], causal=c["causal"], clamp_min=c["clamp_min"], mask_min=c["mask_min"])
    if x["pad"] is not None:
        kw["key_pad_mask"] = torch.from_numpy(x["pad"])
    if x["full"] is not None:
        kw["full_mask"] = torch.from_numpy(x["full"])
    if x["gate"] is not None:
        kw["gate"] = torch.from_numpy(x["gate"])
    if c["gs"] or c["gp"] or c["gc"]:
        def spec(key):
            g = A.grid(c, key)
            return None if g is None else ops.FakeQuantSpec(g[0], g[1], g[2])
        kw["fq"] = ops.AttnFakeQuant(scores=spec("gs"), probs=spec("gp"), ctx=spec("gc"), ctx_before_gate=c["before"], ctx_emit_index=c["emit"])
    box = []
    ops.attn_fwd(t(x["q"]), t(x["k"]), t(x["v"]), _prepared=box, **kw)
    return box[2][0], box[2][1]


@pytest.fixture()
def host_ops(monkeypatch):
    from outeffhop_amd import ops

    monkeypatch.setattr(ops, "_need_gpu", lambda *ts, **kw: None)
    monkeypatch.setattr(ops, "_warn_if_any_shape_kernel", lambda *a, **kw: None)
    return ops


def _name(lib, d, fqd):
    n = lib.oeh_attn_variant(C.byref(d), None if fqd is None else C.byref(fqd))
    return None if n is None else n.decode()


def _with_dump_pointers(c, fqd):
    """The dumps are a route of their own (fast_can refuses them): their pointers, fake ones - nothing on the host dereferences them."""
    if c["dumps"] and fqd is not None:
        for f in (fqd.scores, fqd.probs, fqd.ctx):
            if f.enable:
                f.dump_idx = 0x10000000
    return fqd


@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_every_case_names_its_kernel(host_ops, case):
    """oeh_attn_variant on the descriptor ops.attn_fwd builds, under the case's hook mask: the kernel the GPU tests assert again on the device."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    c = case  # (a layout case is posed contiguous here: its strides exist on the device only, where the GPU test asserts the name again)
    d, fqd = _descriptor(host_ops, c, A.inputs(c))
    fqd = _with_dump_pointers(c, fqd)
    assert lib.oeh_debug_set_variant(c["hook"], 0) == 0
    try:
        assert _name(lib, d, fqd) == c["kernel"], c["name"]
    finally:
        lib.oeh_debug_set_variant(0, 0)


def test_hook_bits_switch_the_kernels_of_last_resort_off(host_ops):
    """include/oeh_debug.h: bit 3 the general kernel, bit 4 the any-shape kernel - and with both off a problem only they take has no name."""
    from outeffhop_amd import _lib, ops

    lib = _lib.load()
    probe = lambda **kw: ops.attn_variant(2, 2, 12, 80, 64, torch.float16, **kw)  # noqa: E731
    try:
        assert probe(scale=-0.125) == "mfma16/NT8/D64/f16"
        assert lib.oeh_debug_set_variant(1 << 3, 0) == 0
        assert probe(scale=-0.125) == "generic" and probe() == "fast16/NT8/D64/f16"
        lib.oeh_debug_set_variant(1 << 4, 0)
        assert probe(scale=-0.125) == "mfma16/NT8/D64/f16" and ops.attn_variant(2, 2, 12, 80, 144, torch.float16) is None
        lib.oeh_debug_set_variant((1 << 3) | (1 << 4), 0)
        assert probe(scale=-0.125) is None
        lib.oeh_debug_set_variant(A.GENERIC_ONLY, 0)
        assert probe() == "generic" and ops.attn_variant(2, 2, 512, 512, 64, torch.float32, clip=True) == "generic"
        # the probability pairs send the general kernel's problems to the any-shape kernel: the same bit switches that off
        lib.oeh_debug_set_variant(0, 0)
        assert ops.attn_variant(2, 2, 12, 80, 64, torch.float32, scale=-0.125, pv_pairs=True) == "generic"
        lib.oeh_debug_set_variant(1 << 4, 0)
        assert ops.attn_variant(2, 2, 12, 80, 64, torch.float32, scale=-0.125, pv_pairs=True) is None
    finally:
        lib.oeh_debug_set_variant(0, 0)


def test_any_shape_lds_bound():
    """The query row and the score row as fp32 in 64 KiB of LDS: D + Sk = 16384 names the kernel, one more key names nothing."""
    from outeffhop_amd import ops

    for D in (144, 8, 200):
        assert ops.attn_variant(1, 1, 2, 16384 - D, D, torch.float32) == "generic"
        assert ops.attn_variant(1, 1, 2, 16384 - D + 1, D, torch.float32) is None
    assert ops.attn_variant(1, 1, 2, 16384 - 64, 64, torch.float16, scale=-1.0) == "generic"
    assert ops.attn_variant(1, 1, 2, 16384 - 64 + 1, 64, torch.float16, scale=-1.0) is None
