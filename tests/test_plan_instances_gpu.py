"""Every compiled instance of the one-pass, full-row and general attention kernels on the device, against the float64 chain of
tests/_attn_ref.py.  `-m gpu`.  The cases and what each instance is come from tests/_attn_inst.py; tests/test_attn_instances_cpu.py proves
without a GPU that the cases reach exactly the built instances and that they would reject a kernel wrong in one term.

(The file name sorts after test_modules_gpu.py on purpose: that file's mask-address test depends on every GPU allocation before it.)

One test per (family, head dim, storage, NT or MQ) walks the group's instances and their cases.  Each case asserts
  - the variant name on the real descriptor, and that the real descriptor gives the instance the registry claims (for the one-pass kernel's
    plain form also which launch form ran: oeh_debug_hot_launches);
  - a finite output, and a second call that equals the first bit for bit;
  - the contract against float64 (tests/_attn_ref.py: check_contract): fp16 1e-3 + half an fp16 ulp, bf16 2e-2 absolute + relative, fp32
    storage 5e-4 absolute + relative; with the probability pairs the bound of tests/test_attn_pv_pairs_gpu.py;
  - in-kernel gate predictor: the gate the kernel wrote (GatePredictor.out) within 2e-3 (fp16, fp32 storage) / 1.5e-2 (bf16) of the float64
    predictor, and the output against the chain with the kernel's own gate;
  - fake-quant, up to 512 keys: a second run through the general kernel with index dumps equals the instance's output bit for bit, and its
    dumps say which rows hold an index one off float64 (the full-row kernel's FQ = 3 form has no twin there - see `_run` - and may differ
    from that run in fewer than 2e-3 of the elements by one context grid step; those elements are left out, the others of its own output
    meet the contract); above 512 keys: the any-shape kernel's dumps are exact (check_exact's statement),
    and rows that hold a tie-band element or an index that differs from float64 are left out (check_contract_long);
  - layouts with guard rows (longkv, qslice: NaN behind k / v / q): no guard row was read - the output is finite.
Siblings: an O32 instance's output rounded to the storage type equals the 16-bit instance's output bit for bit; the hot-argument launch
equals the launch under hook bit 13 bit for bit."""
import numpy as np
import pytest

from oracle import oeh_oracle as O
from tests import _attn_inst as I
from tests import _attn_ref as A

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:outeffhop_amd.*any-shape HIP kernel:RuntimeWarning")]  # (the dumps of the long quantised rows)

GROUPS, GROUP_IDS = I.GROUPS, I.GROUP_IDS
GATE_TOL = {"fp16": 2e-3, "bf16": 1.5e-2, "fp32": 2e-3}
WORST = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _run(ops, inst, c):
    r = A.refs(c, O)
    info, again = {}, {}
    name, got, _ = A.pose(ops, torch, c, r["x"], info=info)
    assert name == c["kernel"], (c["name"], name)
    assert I.instance_from(name, info["desc"], info["fqd"], c["hook"]) == inst, (c["name"], inst)
    assert info["hot"] == (1 if inst[0] == "hot" else 0), (c["name"], "launch form", info["hot"])
    assert np.isfinite(got).all(), (c["name"], "non-finite output")
    A.pose(ops, torch, c, r["x"], info=again)
    assert torch.equal(_bits(info["raw"]), _bits(again["raw"])), (c["name"], "a second call differs")
    if c["gate_units"] is not None:  # the chain takes the gate the kernel wrote, which is held to the float64 predictor on its own
        g64 = r["x"]["gate64"][..., 0]
        gerr = float(np.abs(info["gate_out"] - g64).max())
        assert gerr < GATE_TOL[c["storage"]], (c["name"], "in-kernel gate against the float64 predictor", gerr)
        r = dict(r, w=dict(r["w"], ctx=r["w"]["ctx"] * (info["gate_out"] / g64)[..., None]))
    if c["gs"] or c["gp"] or c["gc"]:
        if c["Sk"] <= 512:
            c2 = dict(c, hook=I.NO_FLASH | I.NO_FAST, mq=0, dumps=True)
            name2, got2, dumps = A.pose(ops, torch, c2, r["x"])
            assert name2.startswith("mfma16/") and name2.endswith("/fq"), (c["name"], name2)
            differs = got != got2
            leave_out = None
            if c["pad_bool"] and c["gc"] and differs.any():
                # The full-row kernel's grid chain with a padding vector (FQ = 3) has no twin in the general kernel: launch_nt_d
                # (csrc/oeh_attn_mfma.inl) takes its grid chain only without a padding vector and runs the literal op order here, and the two
                # forms agree "up to rare single steps" (tests/test_attn_gpu.py: test_int8_grid_chain_with_key_padding).  So the bit equality
                # holds for FQ 1 and 2, and here a context index may land on the neighbouring grid point - rarer than FLIP_SHARE, one step (times
                # the gate) apart.  Those elements the dumps do not speak for: they are left out, every other element of the instance's OWN
                # output meets the contract.
                step = (1.0 if c["emit"] else r["grids"][2][0]) * (np.abs(r["x"]["gate"].astype(np.float64)) if c["before"] else 1.0)
                assert differs.sum() <= max(A.FLIP_SHARE * differs.size, 2.0), (c["name"], "elements that differ from the general kernel", int(differs.sum()))
                lim = (step + np.zeros(got.shape)) * (1.0 + 2.0 ** -A.R.MANT_BITS[c["storage"]]) + 2.0 * A.half_ulp(got2, c["storage"])
                assert (np.abs(got - got2)[differs] <= lim[differs]).all(), (c["name"], "more than one context grid step from the general kernel", float(np.abs(got - got2).max()))
                leave_out = differs
            else:
                assert not differs.any(), (c["name"], "differs from the general kernel's fake-quant chain", name2, float(np.abs(got - got2).max()))
            ratio = A.check_contract(c, r, got, dumps, leave_out)
        else:
            c2 = dict(c, hook=I.NO_FLASH, mq=0, dumps=True)
            name2, got2, dumps = A.pose(ops, torch, c2, r["x"])
            assert name2 == "generic", (c["name"], name2)
            ratio = A.check_contract_long(c, r, got, dumps)
    else:
        ratio = A.check_contract(c, r, got)
    if c["out32"]:  # "the same loop, only the epilogue's store differs" (csrc/oeh_attn_flash.inl, csrc/oeh_attn_fast.inl)
        sib = {}
        name16, _, _ = A.pose(ops, torch, dict(c, out32=False), r["x"], info=sib)
        assert name16 == name, (c["name"], name16)
        assert torch.equal(_bits(info["raw"].to(sib["raw"].dtype)), _bits(sib["raw"])), (c["name"], "the O32 output rounded to the storage type differs from the 16-bit instance's")
    if inst[0] == "hot":
        sib = {}
        A.pose(ops, torch, dict(c, hook=c["hook"] | I.NO_HOT), r["x"], info=sib)
        assert sib["hot"] == 0 and torch.equal(_bits(info["raw"]), _bits(sib["raw"])), (c["name"], "the hot-argument launch differs from the launch under hook bit 13")
    return ratio


@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_every_instance_against_float64(ops, group):
    worst, n_inst, n_case = (0.0, None), 0, 0
    for inst, cases in sorted(I.by_instance().items()):
        if I.group_of(inst) != group:
            continue
        n_inst += 1
        for c in cases:
            ratio = _run(ops, inst, c)
            n_case += 1
            assert ratio <= 1.0, (c["name"], ratio)
            worst = max(worst, (ratio, c["name"]))
    assert n_inst and n_case >= 2 * n_inst
    WORST[group] = worst
    print(f"{group}: {n_inst} instances, {n_case} cases, largest |got - want64| / limit {worst[0]:.3f} ({worst[1]})")


def test_report_the_largest_ratios_per_family(ops):
    """Recorded, not asserted beyond <= 1: the per-family maxima of the groups that ran in this process."""
    for fam in ("flash", "fast", "mfma"):
        got = [v for g, v in WORST.items() if g[0] == fam]
        if got:
            print(f"{fam}: largest |got - want64| / limit {max(got)[0]:.3f} ({max(got)[1]})")
