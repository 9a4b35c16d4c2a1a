"""Every compiled instance of the INT8-storage attention kernel (csrc/oeh_attn_i8.hip) on the device, held to the bit where its arithmetic is
exact and to a float64 tie band where it rounds.  `-m gpu`.  The cases, the staged model and what each instance is come from
tests/_i8_ref.py; tests/test_attn_i8_instances_cpu.py proves without a GPU that the cases reach exactly the 60 built instances and that they
reject a kernel wrong in one term.

One test per (NT, CQ2, PAD) group walks the group's problems; a problem fans out over its five output forms through `ops.attn_fwd_i8`.
Per problem:
  - the variant name and the instance, from the REAL descriptor of every launch;
  - the DUMP instance: stage 1 (score indices of every key < Sk of every row, exact), stage 2 (probability indices from the dumped score
    indices: equal to float64 outside the band, one step at most inside; the distance from float64 that the indices prove, over ERR64, is at
    most 4), stage 3 (context indices and fp32 output from the dumped probability indices, bit for bit, the sign of zero included);
  - siblings: the production fp32 instance equals the DUMP instance bit for bit (causal cases: skipped against unskipped key tiles); the f16 and
    bf16 instances equal the fp32 output rounded to nearest even; the int8 instance (ctx_emit_index) equals idx - 128 of the context dump of
    the same form's DUMP launch, its f16 form idx - zp; a second call of every instance is bitwise equal;
  - layouts: k and v_t are slices of longer caches whose bytes behind Sk are random; guard rows around the output keep their fill."""
import time

import numpy as np
import pytest

from tests import _i8_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WORST = {}
FILL = {torch.float32: 123.0, torch.float16: 123.0, torch.bfloat16: 123.0, torch.int8: 77}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.int8}[t.element_size()])


class _Device:
    """A problem's tensors on the device, laid out as `_i8_ref.descriptor` says."""

    def __init__(self, ops, c):
        p = R.prep(c)
        B, H, Sq, Sk, cache = c["B"], c["H"], c["Sq"], c["Sk"], c["cache"]
        dev = torch.device("cuda:0")
        cen = lambda a: ops.centre_indices(torch.from_numpy(a).to(dev))  # noqa: E731
        qc, kc = cen(p["qi"]), cen(p["ki"])                              # (B,H,S,64) centred
        if c["layout"] == "bshe":   # (B,S,H*64) storage, the heads as strided views
            self.q = qc.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
            self.k = kc.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)[:, :, :Sk]
        else:
            self.q, self.k = qc.contiguous(), kc.contiguous()[:, :, :Sk]
        self.vt = cen(p["vi"]).permute(0, 1, 3, 2).contiguous()[:, :, :, :Sk]   # (B,H,64,Sk) of a (B,H,64,Sk + cache) cache
        assert self.k.shape == (B, H, Sk, 64) and self.vt.shape == (B, H, 64, Sk) and self.vt.stride(2) == Sk + cache
        self.pad = None if p["pad"] is None else torch.from_numpy(p["pad"]).to(dev)
        self.gate = None if p["gate"] is None else torch.from_numpy(p["gate"]).to(dev)

    def launch(self, ops, c, form, dump=False):
        """One launch of form `form` of case c (c may be the problem's emit form).  Returns (instance key, output (B,H,Sq,64) on the host,
        [score, probability, context index dumps] or None)."""
        B, H, Sq, Sk, guard = c["B"], c["H"], c["Sq"], c["Sk"], c["guard"]
        g = R.grids(c)
        dt = {"dump": torch.float32, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "i8": torch.int8}[form]
        dumps = None
        if dump:
            dumps = [torch.full((B, H, Sq, Sk), 0, dtype=torch.uint8, device="cuda"), torch.full((B, H, Sq, Sk), 0, dtype=torch.uint8, device="cuda"),
                     torch.full((B, H, Sq, 64), 0, dtype=torch.uint8, device="cuda")]
        FQ = ops.FakeQuantSpec
        spec = lambda key, i: None if g[key] is None else FQ(g[key][0], g[key][1], 255.0, None if dumps is None else dumps[i])  # noqa: E731
        fq = ops.AttnFakeQuant(spec("s", 0), spec("p", 1), spec("c", 2), ctx_before_gate=c["before"], ctx_emit_index=c["emit"])
        store = torch.full((B, Sq + 2 * guard, H, 64), FILL[dt], dtype=dt, device="cuda")
        out = store[:, guard:guard + Sq].permute(0, 2, 1, 3)
        sm = ops.SoftmaxSpec(c["base"], c["clip"] is not None, *(c["clip"] or (0.0, 1.0)))
        grids = tuple(ops.QuantGrid(*g[k]) for k in ("q", "k", "v"))
        pa = ops.PreparedAttn(self.q, self.k, self.vt, i8_grids=grids, fq=fq, out_dtype=dt, softmax=sm, scale=c["scale"], scale_div=c["scale_div"], causal=c["causal"],
                              clamp_min=True, mask_min=R.FMIN32, gate=self.gate, out=out, key_pad_mask=self.pad)
        d, fqd = pa._keep[0], pa._keep[1]
        name = R._lib().oeh_attn_variant_ex(R.C.byref(d), None, R.C.byref(fqd)).decode()
        assert name == f"i8mfma/NT{R.group_of(c)[0]}/D64/{'f32' if form == 'dump' else form}", (c["name"], form, name)
        inst = R.instance_from(name, d, fqd)
        pa()
        torch.cuda.synchronize()
        if guard:
            assert bool((store[:, :guard] == FILL[dt]).all()) and bool((store[:, guard + Sq:] == FILL[dt]).all()), (c["name"], form, "a guard row of the output was written")
        return inst, out, dumps


def _twice(dv, ops, c, form, dump=False):
    inst, out, dumps = dv.launch(ops, c, form, dump)
    inst2, out2, dumps2 = dv.launch(ops, c, form, dump)
    assert inst == inst2 and torch.equal(_bits(out), _bits(out2)), (c["name"], form, "a second call differs")
    if dump:
        assert all(torch.equal(a, b) for a, b in zip(dumps, dumps2)), (c["name"], form, "a second call's dumps differ")
    return inst, out, dumps


def _run(ops, c, launched):
    nt, cq2, pad = R.group_of(c)
    dv = _Device(ops, c)
    # the DUMP instance: stages 1 - 3
    inst, o_dump, dumps = _twice(dv, ops, c, "dump", dump=True)
    assert inst == ("i8", nt, 2, 1, cq2, pad) == R.instance_of(c, "dump"), (c["name"], inst)
    launched.add(inst)
    s_idx, p_idx, c_idx = (t.cpu().numpy() for t in dumps)
    dist, share = R.check_stages(c, s_idx, p_idx, c_idx, o_dump.cpu().numpy())
    # siblings
    inst, o32, _ = _twice(dv, ops, c, "f32")
    assert inst == ("i8", nt, 2, 0, cq2, pad) == R.instance_of(c, "f32"), (c["name"], inst)
    launched.add(inst)
    assert torch.equal(_bits(o32), _bits(o_dump)), (c["name"], "the production fp32 instance differs from the DUMP instance", int((_bits(o32) != _bits(o_dump)).sum()))
    for form, dt, code in (("f16", torch.float16, 0), ("bf16", torch.bfloat16, 1)):
        inst, o16, _ = _twice(dv, ops, c, form)
        assert inst == ("i8", nt, code, 0, cq2, pad) == R.instance_of(c, form), (c["name"], inst)
        launched.add(inst)
        assert torch.equal(_bits(o16), _bits(o32.to(dt))), (c["name"], form, "differs from the fp32 output rounded to nearest even", int((_bits(o16) != _bits(o32.to(dt))).sum()))
    # the context quantiser's integers: the emit form of the problem, its own DUMP launch as the reference (stage 3 again, on its dumps)
    ce = R.emit_case(c)
    _, oe_dump, dumps_e = dv.launch(ops, ce, "dump", dump=True)
    assert torch.equal(dumps_e[0], dumps[0]) and torch.equal(dumps_e[1], dumps[1]), (c["name"], "the emit form's score / probability dumps differ")
    ce_idx = dumps_e[2].cpu().numpy()
    want_c, want_o = R.stage3(ce, p_idx)
    assert np.array_equal(ce_idx, want_c) and np.array_equal(oe_dump.cpu().numpy().view(np.int32), want_o.view(np.int32)), (c["name"], "stage 3 of the emit form")
    inst, o8, _ = _twice(dv, ops, ce, "i8")
    assert inst == ("i8", nt, 3, 0, cq2, pad) == R.instance_of(c, "i8"), (c["name"], inst)
    launched.add(inst)
    assert np.array_equal(o8.cpu().numpy().astype(np.int32), ce_idx.astype(np.int32) - 128), (c["name"], "the int8 instance is not idx - 128 of the context dump")
    _, oe16, _ = dv.launch(ops, ce, "f16")
    assert np.array_equal(oe16.float().cpu().numpy(), ce_idx.astype(np.float32) - np.float32(ce["gc"][1])), (c["name"], "the f16 emit form is not idx - zp")
    return dist, share


@pytest.mark.parametrize("group", R.GROUPS, ids=R.GROUP_IDS)
def test_every_instance_of_the_group(ops, group):
    t0 = time.time()
    launched, worst, share, n = set(), (-1.0, ""), (-1.0, ""), 0
    for c in R.CASES:
        if R.group_of(c) != group:
            continue
        dist, sh = _run(ops, c, launched)
        worst, share, n = max(worst, (dist, c["name"])), max(share, (sh, c["name"])), n + 1
    want = {inst for inst in R.built_instances() if (inst[1], inst[4], inst[5]) == group}
    assert launched == want and len(want) == 5 and n >= 2, (sorted(want - launched), n)
    WORST[group] = (worst, share)
    print(f"{R.GROUP_IDS[R.GROUPS.index(group)]}: {len(launched)} instances, {n} problems, largest probability distance from float64 / ERR64 {worst[0]:.2f} ({worst[1]}), "
          f"largest share of indices inside the band {share[0]:.2e} ({share[1]}), {time.time() - t0:.1f} s")


def test_report_the_largest_distance(ops):
    """Recorded, not asserted beyond <= 4: the maxima over the groups that ran in this process."""
    if WORST:
        print(f"INT8-storage instances: ERR64 {R.err64():.3e}, largest probability distance from float64 / ERR64 {max(w for w, _ in WORST.values())}, "
              f"largest band share {max(s for _, s in WORST.values())}, {len(WORST)} groups")
