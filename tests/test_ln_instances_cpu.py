"""The registry of tests/_ln_inst.py, checked without a GPU: the cases reach exactly the instances of oeh_resid_ln_kernel, oeh_embed_kernel,
oeh_ln_train_fwd_kernel and oeh_ln_train_bwd_kernel that the library was built with, each under the name the library gives it; the widths
the scan finds are the ones written down here, so that an edit of ln_plan (csrc/oeh_ln_row.h) fails this file and not silently; every
run-time branch value occurs in each kernel with each form; and the draws of the block tail's cases with an output quantiser meet the
tie-band condition of tests/_ln_ref.py with half the cap to spare.

The tie band is a condition on the inputs, not a measurement: `check_indices` requires that at most 1e-3 of the elements lie within
4 err64 / scale of a rounding tie.  Here each such case is evaluated on the CPU - torch's add in the storage type, the float64 fake-quant of
tests/_ln_ref.py, then `_cpu_case`'s float64 and fp32 LayerNorm - and must hold at most half of that.  A draw that does not gets another
seed (`_ln_inst.RESEED`); the cap stays.  The embedding front's cases take their draws through `_case` of tests/test_embed_gpu.py, which
asks the same condition (at the cap) of its yardsticks before the kernel runs and moves on to the next seed itself."""
import numpy as np
import pytest

from tests import _ln_inst as I
from tests import _ln_ref as R

torch = pytest.importorskip("torch")

DT = (torch.float16, torch.bfloat16, torch.float32)

# (form, CH) -> (first, last) width per dtype: the scan of the library's names must give exactly this
_SCALAR = {("scalar", 1): (1, 256), ("scalar", 4): (257, 1024), ("scalar", 16): (1025, 4096), ("scalar", 32): (4097, 8192)}
_BIT16 = {("wave", 1): (8, 512), ("wave", 2): (520, 1024), ("block", 1): (1032, 2048), ("block", 2): (2056, 4096), ("block", 4): (4104, 8192), **_SCALAR}
EXPECTED = {"f16": _BIT16, "bf16": _BIT16,
            "f32": {("wave", 1): (4, 256), ("wave", 2): (260, 512), ("wave", 4): (516, 1024), ("block", 2): (1028, 2048), ("block", 4): (2052, 4096),
                    ("block", 8): (4100, 8192), **_SCALAR}}
COUNTS = {"ln": 28, "embed": 84, "ln_train_fwd": 56, "ln_train_bwd": 56}


def test_the_cases_reach_exactly_the_built_instances():
    by, built, cases = I.by_instance(), I.built_instances(), I.cases()
    assert len({c["name"] for c in cases}) == len(cases)
    assert set(by) | set(I.UNREACHABLE) == built, (sorted(built - set(by) - set(I.UNREACHABLE)), sorted((set(by) | set(I.UNREACHABLE)) - built))
    assert not set(by) & set(I.UNREACHABLE)
    assert {k: sum(1 for i in built if i[0] == k) for k in I.KERNELS} == COUNTS
    for inst, cs in by.items():
        assert [c["which"] for c in cs] == ["first", "last"] and cs[0]["cols"] < cs[1]["cols"], inst
    print(f"{len(built)} instances, {len(cases)} cases, {len(I.UNREACHABLE)} unreachable")


def test_every_case_is_filed_under_the_instance_its_name_maps_to():
    for c in I.cases():
        name = I.variant_name(c)
        assert name is not None and I.key_of(name) == c["inst"], (c["name"], name)
        assert name.split("/")[0] == ("ln_train" if c["kernel"].startswith("ln_train") else c["kernel"])
        # the /drop of the name is the case's p, the Tn its number of lookups
        assert ("/drop" in name) == (c.get("p", 0.0) > 0.0) and (c["kernel"] != "embed" or f"/T{c['nt']}/" in name)


def test_groups_are_the_built_ones():
    assert len(I.GROUPS) == len(set(I.GROUPS)) == len(I.GROUP_IDS) == len(set(I.GROUP_IDS))
    assert set(I.GROUPS) == {I.group_of(i) for i in I.built_instances()}
    for g in I.GROUPS:  # each group: every NT / DROP value of its template, at both widths
        cs = I.cases_of(g)
        assert len(cs) == 2 * {"ln": 1, "embed": 3}.get(g[0], 2), g
        assert {c["inst"][4:] for c in cs} == {"ln": {()}, "embed": {(1,), (2,), (3,)}}.get(g[0], {(0,), (1,)}), g


def test_the_scan_finds_the_written_ranges():
    for IN, dt in enumerate(I.DTN):
        got = {(I.FORMS[f], ch): r for (f, ch), r in I.ranges(IN).items()}
        assert got == EXPECTED[dt], (dt, got)


def test_widths_and_strides_of_the_cases():
    for c in I.cases():
        nv = I.VEC[c["IN"]]
        lo, hi = I.ranges(c["IN"])[(c["form"], c["CH"])]
        assert c["cols"] == (lo if c["which"] == "first" else hi)
        if c["form"] == 2:  # element accesses: the first width is no vector multiple, the last one is and takes rows cols + 1 apart
            assert (c["cols"] % nv != 0 and c["stride"] == c["cols"]) if c["which"] == "first" else (c["cols"] % nv == 0 and c["stride"] == c["cols"] + 1), c["name"]
        else:
            assert c["cols"] % nv == 0 and c["stride"] == c["cols"]
        # first width: one chunk in the last access; last width: every access of every thread full
        threads, per = (64 if c["form"] == 0 else 256), (1 if c["form"] == 2 else nv)
        chunks = c["cols"] // per
        assert chunks <= threads * c["CH"]
        if c["which"] == "last":
            assert chunks == threads * c["CH"], c["name"]
        else:  # one chunk more than the range below takes (the workgroup form starts where the wave form's 1024 columns end)
            below = [r[1] for (f, ch), r in I.ranges(c["IN"]).items() if f == c["form"] and ch < c["CH"]]
            assert chunks == (max(below) // per + 1 if below else 1024 // nv + 1 if c["form"] == 1 else 1), c["name"]


def test_every_branch_value_occurs_in_each_kernel_with_each_form():
    seen = {}
    for c in I.cases():
        if c["kernel"] == "ln":
            flags = ("r", "beta", "sq", "oq", "sum")
        elif c["kernel"] == "embed":
            flags = ("tab", "id64", "ln") + (("mid",) if c["nt"] == 3 else ()) + (("last",) if c["nt"] >= 2 else ()) + (("beta", "oq") if c["ln"] else ())
        elif c["kernel"] == "ln_train_fwd":
            flags = ("r", "beta")
        else:
            flags = ("dsum", "dr", "dbeta")
        for f in flags:
            seen.setdefault((c["kernel"], c["form"], f), set()).add(c[f])
    assert len(seen) == 3 * (5 + 7 + 2 + 3)
    for (kernel, form, f), values in seen.items():
        assert values == ({"plain", "grid", "int8"} if f == "tab" else {False, True}), (kernel, I.FORMS[form], f, values)
    assert all(c["B"] * c["S"] == I.ROWS for c in I.cases() if c["kernel"] == "embed")


def test_every_training_case_has_a_usable_draw():
    """`train_draw` of tests/test_ln_instances_gpu.py runs on the CPU alone: every case of the two training kernels finds a draw whose unit
    (err64 of y) is at least half an fp32 ulp of the largest output, within a few seeds."""
    from tests.test_ln_instances_gpu import train_draw

    later, n = 0, 0
    for c in I.cases():
        if c["kernel"].startswith("ln_train"):
            seed, draw = train_draw(c)
            assert (seed - c["seed"]) % 7919 == 0 and (seed - c["seed"]) // 7919 < 8, c["name"]
            assert draw[0].shape == (I.ROWS, c["cols"])
            later, n = later + (seed != c["seed"]), n + 1
    assert n == 2 * (COUNTS["ln_train_fwd"] + COUNTS["ln_train_bwd"])
    print(f"{n} training cases, {later} on a later seed than their first")


def test_tie_band_of_the_block_tail_cases_is_within_half_the_cap():
    from tests.test_ln_gpu import _cpu_case, _inputs

    worst, n = 0.0, 0
    for c in I.cases():
        if c["kernel"] != "ln" or not c["oq"]:
            continue
        dtype = DT[c["IN"]]
        x, r, gamma, beta = _inputs(I.ROWS, c["cols"], dtype, c["seed"], device="cpu")
        s = torch.add(x, r) if c["r"] else x
        if c["sq"]:
            _, val = R.fake_quant64(s.float().numpy(), *R.grid_from_minmax(float(s.min()), float(s.max())))
            s = torch.from_numpy(val.astype(np.float32)).to(dtype)
        y64, err64, y32 = _cpu_case(s, gamma, beta if c["beta"] else None)
        scale, zp, qmax = R.grid_from_minmax(float(y32.min()), float(y32.max()))
        own = np.clip(np.rint(y64 / scale + zp), 0.0, qmax)
        try:
            share, _ = R.check_indices(own, y64, scale, zp, qmax, err64, max_band=0.5e-3)
        except AssertionError as e:
            raise AssertionError(f"{c['name']} (seed {c['seed']}): {e}: give it another seed in _ln_inst.RESEED") from None
        worst, n = max(worst, share), n + 1
    assert n >= 28
    print(f"{n} block-tail cases with an output quantiser: tie band <= {worst:.1e} of the elements (half the cap: 5e-4)")
