"""The optimizer phase under fp16 loss scaling on the device (include/oeh.h: oeh_grad_norm_amp, oeh_adamw_step_amp, oeh_loss_scale_update;
outeffhop_amd/optim.py: FusedAdamW(amp=True), LossScaler).  As in test_optim_adamw_gpu.py every tensor is a slice of a larger buffer whose
other elements are canaries, and whole buffers are compared bit for bit - with the plain step (oeh_adamw_step) where the two must agree,
with the numpy restatement (tests/_adamw_amp_ref.py) elsewhere.  Tensors have at most 3 * 4096 + 5 elements."""
import copy
import gc
import math

import numpy as np
import pytest

from tests import _adamw_amp_ref as A
from tests import _adamw_ref as R

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DT = (torch.float32, torch.float16, torch.bfloat16)
PAD = 64         # canary elements around every tensor: a multiple of 16 bytes in every storage type
CANARY = -123.5  # exact in fp16 and bf16
SIZES = (1, 5, 4095, 4096, 4097, 3 * 4096 + 5)
# lr, beta1, beta2, eps, weight_decay, step: test_optim_adamw_gpu.py's - group 0 is a first step (zero state), group 1 has no weight decay
GROUPS = ((1e-3, 0.9, 0.999, 1e-8, 1e-2, 1), (6e-4, 0.9, 0.95, 1e-8, 0.0, 2), (5e-5, 0.8, 0.95, 1e-6, 0.1, 1000))
SLOT_CANARY = 77.0  # in the counters no record owns


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """test_modules_gpu.py's mask-address test passes only while the caching allocator hands a freed block straight back, which depends on
    every allocation made in the process before it.  This file is therefore named to be collected AFTER that one, and gives its cached
    blocks back when it is done (see test_optim_adamw_gpu.py)."""
    yield
    if torch.cuda.is_available():
        from outeffhop_amd import ops as _ops

        _ops._grad_norm_work.clear()
        _ops._adamw_amp_work.clear()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64 if t.dtype == torch.float64 else torch.int16).numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class Arena:
    """One host buffer of `dtype` full of canaries in which tensors are placed PAD elements apart, each on a 16-byte boundary plus `disp`
    elements; `upload` makes the device copy and `view(i)` the i-th tensor as a slice of it."""

    def __init__(self, dtype):
        self.dtype, self.parts, self.spans, self.cursor = dtype, [], [], PAD

    def add(self, values, disp=0):
        start = self.cursor + disp
        self.parts.append((start, values.to(self.dtype)))
        self.spans.append((start, start + values.numel()))
        self.cursor = -(-(start + values.numel() + PAD) // 16) * 16
        return len(self.spans) - 1

    def host(self):
        buf = torch.full((self.cursor + PAD,), CANARY, dtype=self.dtype)
        for start, v in self.parts:
            buf[start:start + v.numel()] = v
        return buf

    def upload(self):
        self.dev = self.host().cuda()
        assert self.dev.data_ptr() % 16 == 0
        return self.dev

    def view(self, i):
        a, b = self.spans[i]
        return self.dev[a:b]


class Case:
    """A tensor list in arenas - p, m, v in three fp32 arenas, g in one arena per storage type - and the step counters: one slot per
    tensor, handed out in REVERSE order, between counters that no record owns."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.P, self.M, self.V = Arena(torch.float32), Arena(torch.float32), Arena(torch.float32)
        self.G = {dt: Arena(dt) for dt in DT}
        self.items = []  # (index in P / M / V, g dtype, index in G[dtype], group, n)
        self.counts = []  # the counter of each tensor BEFORE the step

    def add(self, n, dt, group, gscale=1.0, disp=(0, 0, 0, 0), g=None, gmul=1.0):
        """gmul: the loss scale the stored gradient carries (a power of two: exact); g: the stored gradient's values instead"""
        p, g_, m, v = R.random_state(self.rng, n, gscale, first=GROUPS[group][5] == 1)
        g = g_ * np.float32(gmul) if g is None else np.asarray(g, dtype=np.float32)
        i = self.P.add(_t(p), disp[0])
        self.M.add(_t(m), disp[2])
        self.V.add(_t(v), disp[3])
        self.items.append((i, dt, self.G[dt].add(_t(g), disp[1]), group, n))
        self.counts.append(GROUPS[group][5] - 1)

    def upload(self):
        for a in (self.P, self.M, self.V, *self.G.values()):
            a.upload()
        n = len(self.items)
        self.slots = [2 * (n - 1 - i) + 1 for i in range(n)]
        steps = np.full(2 * n + 1, SLOT_CANARY, np.float32)
        steps[self.slots] = self.counts
        self.steps_host = steps
        self.steps = _t(steps).cuda()
        return self

    def lists(self):
        ps = [self.P.view(i) for i, *_ in self.items]
        ms = [self.M.view(i) for i, *_ in self.items]
        vs = [self.V.view(i) for i, *_ in self.items]
        gs = [self.G[dt].view(j) for _, dt, j, _, _ in self.items]
        return ps, gs, ms, vs, [grp for *_, grp, _ in self.items]

    def stored(self, k):
        """tensor k's gradient as stored, as fp32 numpy"""
        _, dt, j, _, _ = self.items[k]
        return self.G[dt].host()[slice(*self.G[dt].spans[j])].float().numpy()

    def expected(self, c, only=None):
        """The three fp32 arenas and the counters after one amp step with coefficient c (fp32): the restatement inside, canaries outside.
        only: the tensors that are stepped (default all)."""
        P, M, V = self.P.host(), self.M.host(), self.V.host()
        steps = self.steps_host.copy()
        for k, (i, dt, j, grp, n) in enumerate(self.items):
            if only is not None and k not in only:
                continue
            (a, b), (ma, mb), (va, vb) = self.P.spans[i], self.M.spans[i], self.V.spans[i]
            t = self.counts[k] + 1
            pn, mn, vn = A.step32_amp(P[a:b].numpy(), self.stored(k), M[ma:mb].numpy(), V[va:vb].numpy(), c, GROUPS[grp][:5], t)
            P[a:b], M[ma:mb], V[va:vb] = _t(pn), _t(mn), _t(vn)
            steps[self.slots[k]] = t
        return P, M, V, steps

    def snapshot(self):
        """every buffer on the device as bits: parameters, moments, gradients of every storage type, counters"""
        return [_bits(a.dev) for a in (self.P, self.M, self.V, *self.G.values())] + [_bits(self.steps)]

    def sumsq(self):
        g = np.concatenate([self.stored(k).astype(np.float64) for k in range(len(self.items))])
        return float(np.sum(g * g))


def _same(got, want, what=""):
    for k, (a, b) in enumerate(zip(got, want)):
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{what} buffer {k}: {bad.size} elements differ, first at {bad[:5]}"


def _groups(ops, with_step=True):
    return [ops.AdamWGroup(*g[:5], g[5] if with_step else 0) for g in GROUPS]


def _list(seed, dt=torch.float32, gmul=1.0, gscales=(1.0, 1e-3, 30.0)):
    """every size in each of the three groups' turn, and one tensor whose gradient is one element off its 16-byte boundary (the elem form)"""
    case = Case(seed)
    for k, n in enumerate(SIZES):
        case.add(n, dt, k % 3, gscale=gscales[k % 3], gmul=gmul)
    case.add(4096 + 5, dt, 1, gscale=0.1, disp=(0, 1, 0, 0), gmul=gmul)
    return case.upload()


def _f32(x, dev="cuda"):
    return torch.tensor([x], dtype=torch.float32, device=dev)


def test_scale_one_is_the_plain_step_and_the_device_forms_the_restatements_constants(ops):
    amp, plain = _list(1), _list(1)
    pa, pp = ops.mt_plan(*amp.lists()), ops.mt_plan(*plain.lists())
    assert pa.variants.count("elem") == 1 and pa.n_chunks == sum(-(-n // 4096) for n in SIZES) + 2
    o_plain = ops.grad_norm(pp, 1.0)
    ops.adamw_step(pp, _groups(ops), clip=o_plain)
    o_amp = ops.grad_norm_amp(pa, 1.0)
    work = ops.adamw_step_amp(pa, _groups(ops, with_step=False), o_amp, amp.steps, amp.slots)
    work = work.cpu().numpy()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(o_amp), _bits(o_plain)) and 0.0 < float(o_amp[2]) < 1.0 and float(o_amp[3]) == 0.0
    _same(amp.snapshot()[:-1], plain.snapshot()[:-1], "amp against plain:")
    P, M, V, steps = amp.expected(np.float32(float(o_amp[2])))
    _same(amp.snapshot(), [_bits(P), _bits(M), _bits(V)] + [_bits(a.host()) for a in amp.G.values()] + [steps.view(np.int32)], "amp against the restatement:")
    assert sorted(set(steps[amp.slots].tolist())) == [1.0, 2.0, 1000.0] and (steps[0::2] == SLOT_CANARY).all()
    # the device's double `/` and sqrt: the table the step read is the restatement's, bit for bit
    for k, (*_, grp, _) in enumerate(amp.items):
        lr, b1, b2 = GROUPS[grp][:3]
        want = np.array(A.amp_constants(lr, b1, b2, GROUPS[grp][5]), np.float32)
        assert np.array_equal(work[k].view(np.int32), want.view(np.int32)), (k, work[k], want)


@pytest.mark.parametrize("max_norm", [1.0, None])
def test_power_of_two_scale_is_exact_fp32(ops, max_norm):
    s = 2.0 ** 16
    scales = (0.15, 0.1, 0.16)  # |g| in [1e-3, 30], the x40 outliers included
    amp, plain = _list(2, gmul=s, gscales=scales), _list(2, gscales=scales)
    for k in range(len(amp.items)):
        g = np.abs(plain.stored(k))
        assert np.array_equal(amp.stored(k), plain.stored(k) * np.float32(s)) and g.min() >= 1e-3 and g.max() <= 30.0
    pa, pp = ops.mt_plan(*amp.lists()), ops.mt_plan(*plain.lists())
    o_plain = ops.grad_norm(pp, max_norm)
    ops.adamw_step(pp, _groups(ops), clip=o_plain if max_norm is not None else None)
    o_amp = ops.grad_norm_amp(pa, max_norm, grad_scale=_f32(s))
    ops.adamw_step_amp(pa, _groups(ops, with_step=False), o_amp, amp.steps, amp.slots)
    oa, op = o_amp.cpu().numpy(), o_plain.cpu().numpy()
    assert oa[0] == op[0] * s * s and oa[1] == op[1] and oa[2] * s == op[2] and oa[3] == 0.0  # the norm and clipc of oeh_grad_norm on g
    assert (op[2] < 1.0) == (max_norm is not None)
    got, want = amp.snapshot(), plain.snapshot()
    _same(got[:3], want[:3], "p, m, v against the plain clip + step on g:")
    _same(got[3:6], [_bits(a.host()) for a in amp.G.values()], "gradients:")
    assert np.array_equal(got[6], amp.expected(np.float32(1.0))[3].view(np.int32))


@pytest.mark.parametrize("dt,s", [(torch.float16, 2.0 ** 16), (torch.bfloat16, 2.0 ** 16), (torch.float32, 3.0 * 2 ** 10), (torch.float16, 3.0 * 2 ** 10)])
@pytest.mark.parametrize("max_norm", [0.25, None])
def test_scaled_gradients_against_the_restatement(ops, dt, s, max_norm):
    """16-bit gradients hold the scaled values rounded to their type (fp16 ones that overflowed are the next test's): the restatement starts
    from the values as stored.  The unscaled gradients are small enough for the scaled ones to fit fp16: |g| 2^16 < 65504, outliers included."""
    case = Case(3)
    for k, n in enumerate(SIZES):
        g = R.random_state(case.rng, n, (1e-3, 1e-5, 4e-3)[k % 3])[1].astype(np.float64) * s
        case.add(n, dt, k % 3, gscale=(1e-3, 1e-5, 4e-3)[k % 3], g=_t(g).to(dt).float().numpy())
    case.add(4096 + 5, dt, 1, gscale=1e-3, g=_t(R.random_state(case.rng, 4096 + 5, 1e-3)[1].astype(np.float64) * s).to(dt).float().numpy(), disp=(0, 1, 0, 0))
    case.upload()
    assert all(np.isfinite(case.stored(k)).all() for k in range(len(case.items)))
    plan = ops.mt_plan(*case.lists())
    assert "elem" in plan.variants
    out4 = ops.grad_norm_amp(plan, max_norm, grad_scale=_f32(s))
    ops.adamw_step_amp(plan, _groups(ops, with_step=False), out4, case.steps, case.slots)
    o = out4.cpu().numpy()
    n = sum(it[4] for it in case.items)
    want = case.sumsq()
    assert abs(o[0] - want) <= (n + 4) * 2.0 ** -52 * want
    ref = A.norm_amp(o[0], max_norm, s)  # sqrt and two quotients in double on the device: 2 ulp, the plain norm's allowance
    assert abs(o[1] - ref[1]) <= 2 * math.ulp(ref[1]) and abs(o[2] - ref[2]) <= 2 * math.ulp(ref[2]) and o[3] == 0.0
    assert (o[2] * s < 1.0) == (max_norm is not None)
    P, M, V, steps = case.expected(np.float32(o[2]))
    _same(case.snapshot(), [_bits(P), _bits(M), _bits(V)] + [_bits(a.host()) for a in case.G.values()] + [steps.view(np.int32)])


def _overflow_case():
    case = Case(4)
    case.add(4096, torch.float32, 0)                                  # 0: its first element
    case.add(4097, torch.float32, 1, gscale=1e-3)                     # 1: the last element of a ragged tail
    case.add(4096 + 5, torch.float32, 2, disp=(0, 1, 0, 0))           # 2: the elem form
    case.add(3 * 4096 + 5, torch.float16, 1)                          # 3: an fp16 gradient
    case.add(5, torch.bfloat16, 2)
    return case.upload()


def test_overflow_leaves_everything_alone(ops):
    case = _overflow_case()
    ps, gs, ms, vs, grp = case.lists()
    plan = ops.mt_plan(ps, gs, ms, vs, grp)
    assert plan.variants == ["vec16", "vec16", "elem", "vec16", "vec16"]
    clean = case.snapshot()
    groups = _groups(ops, with_step=False)
    scale = _f32(2.0 ** 16)
    runs = []
    for where, (k, at) in {"first element": (0, 0), "last of a ragged tail": (1, 4096), "elem form": (2, 2000), "fp16": (3, 3 * 4096 + 4)}.items():
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = gs[k][at].clone()
            gs[k][at] = bad
            before = case.snapshot()
            acc, out4 = _f32(0.0), torch.full((4,), -1.0, dtype=torch.float64, device="cuda")
            ops.grad_norm_amp(plan, 1.0, grad_scale=scale, found_acc=acc, out=out4)
            ops.adamw_step_amp(plan, groups, out4, case.steps, case.slots)
            runs.append((where, bad, before, case.snapshot(), out4.cpu().numpy(), float(acc)))
            gs[k][at] = keep
    for where, bad, before, after, o, acc in runs:
        _same(after, before, f"{where} {bad}:")
        assert o[3] == 1.0 and acc == 1.0 and not math.isfinite(o[0]), (where, bad, o)
        assert sum(int((a != b).sum()) for a, b in zip(before, clean)) == 1  # (the one poisoned element)
    _same(case.snapshot(), clean)
    # a flag raised elsewhere (torch's own check, another device) does the same with finite gradients; without found_acc nothing else is written
    out4 = ops.grad_norm_amp(plan, 1.0, grad_scale=scale, found_inf=_f32(1.0))
    ops.adamw_step_amp(plan, groups, out4, case.steps, case.slots)
    o = out4.cpu().numpy()
    assert o[3] == 1.0 and math.isfinite(o[0]) and o[2] == 2.0 ** -16  # (a norm far below max_norm once the scale is divided out)
    _same(case.snapshot(), clean, "found_inf:")
    # a scale that is no positive finite number skips as well; an accumulator that is already raised stays raised on a clean step
    for s in (0.0, float("inf"), float("nan"), -4.0):
        out4 = ops.grad_norm_amp(plan, 1.0, grad_scale=_f32(s))
        ops.adamw_step_amp(plan, groups, out4, case.steps, case.slots)
        assert float(out4[3]) == 1.0, s
    _same(case.snapshot(), clean, "bad scale:")
    acc = _f32(1.0)
    zero = _f32(0.0)
    out4 = ops.grad_norm_amp(plan, 1.0, grad_scale=scale, found_inf=zero, found_acc=acc)
    assert float(out4[3]) == 0.0 and float(acc) == 1.0 and float(zero) == 0.0
    acc = _f32(0.0)
    ops.grad_norm_amp(plan, 1.0, grad_scale=scale, found_acc=acc)
    assert float(acc) == 0.0  # a clean norm stores nothing there
    # and the step that follows a clean norm does step
    ops.adamw_step_amp(plan, groups, out4, case.steps, case.slots)
    P, M, V, steps = case.expected(np.float32(float(out4[2])))
    _same(case.snapshot(), [_bits(P), _bits(M), _bits(V)] + clean[3:6] + [steps.view(np.int32)], "the clean step after:")


def test_a_record_of_a_group_the_descriptor_lacks_keeps_its_counter(ops):
    import ctypes as C

    from outeffhop_amd import _lib

    case = _overflow_case()
    ps, gs, ms, vs, grp = case.lists()
    plan = ops.mt_plan(ps, gs, ms, vs, grp)  # groups 0, 1, 2, 1, 2
    slots = ops.mt_slots(plan, case.slots)
    out4 = ops.grad_norm_amp(plan, None)
    d = _lib.oeh_adamw_desc()
    d.n_groups = 1
    d.lr[0], d.beta1[0], d.beta2[0], d.eps[0], d.weight_decay[0] = GROUPS[0][:5]
    work = torch.zeros(2 * len(ps), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.load().oeh_adamw_step_amp(p(plan.table), plan.n_chunks, len(ps), C.byref(d), p(out4), p(case.steps), p(slots.table), p(work),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    P, M, V, steps = case.expected(np.float32(1.0), only={0})
    _same(case.snapshot()[:3] + case.snapshot()[-1:], [_bits(P), _bits(M), _bits(V), steps.view(np.int32)])
    assert steps[case.slots].tolist() == [1.0, 1.0, 999.0, 1.0, 999.0]
    assert (work[2:] == 0).all() and (work[:2] != 0).all()  # their constants are not formed either
    with pytest.raises(ValueError):
        ops.adamw_step_amp(plan, _groups(ops)[:1], out4, case.steps, slots)  # the Python layer refuses
    with pytest.raises(ValueError, match="distinct"):
        ops.mt_slots(plan, [1, 1, 3, 5, 7])
    with pytest.raises(ValueError, match="records"):
        ops.mt_slots(plan, [1, 3])
    with pytest.raises(ValueError, match="outside"):
        ops.adamw_step_amp(plan, _groups(ops), out4, case.steps, [0, 1, 2, 3, 11])
    with pytest.raises(ValueError):
        ops.adamw_step_amp(plan, _groups(ops), out4, case.steps.double(), slots)
    with pytest.raises(ValueError):
        ops.grad_norm_amp(plan, 1.0, grad_scale=torch.ones(1, dtype=torch.float64, device="cuda"))
    from outeffhop_amd import _lib as L
    with pytest.raises(L.OehError):
        ops.grad_norm_amp(plan, 1.0, grad_scale=torch.ones(1))
    _same(case.snapshot()[:3] + case.snapshot()[-1:], [_bits(P), _bits(M), _bits(V), steps.view(np.int32)])


def test_the_same_launches_twice_give_the_same_bits(ops):
    outs = []
    for _ in range(2):
        case = _list(8, dt=torch.float16)
        plan = ops.mt_plan(*case.lists())
        out4 = ops.grad_norm_amp(plan, 0.5, grad_scale=_f32(3.0 * 2 ** 10))
        ops.adamw_step_amp(plan, _groups(ops, with_step=False), out4, case.steps, case.slots)
        state = _f32(0.0).repeat(4)
        state[0] = 1024.0
        ops.loss_scale_update(state, 2.0, 0.5, 1)
        outs.append(case.snapshot() + [_bits(out4), _bits(state)])
    _same(outs[0], outs[1])
    assert outs[0][-1].view(np.float32).tolist() == [2048.0, 0.0, 0.0, 0.0]


def test_loss_scale_update_on_the_device_is_the_restatement(ops):
    top = float(np.float32(np.finfo(np.float32).max / 1.5))
    for start, interval, founds in ((65536.0, 2, [0, 0, 1, 0, 0, 1, 1, 0, 0, 0]), (top, 1, [0, 0, 1, 0, 0]), (3.0, 3, [0, 0, 0, 0, 1, 0, 0, 0])):
        state = torch.tensor([start, 0.0, 0.0, 0.0], device="cuda")
        want = np.array([start, 0, 0, 0], np.float32)
        got = []
        for f in founds:
            state[2] = float(f)
            ops.loss_scale_update(state, 2.0, 0.5, interval)
            got.append(state.clone())
        for f, g in zip(founds, got):
            want[2] = f
            want = A.scaler_update(want, 2.0, 0.5, interval)
            assert np.array_equal(_bits(g), want.view(np.int32)), (start, f, g, want)
        assert np.isfinite(want[0]) and want[3] == sum(founds)


class Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(37, 129)
        self.layer_norm = torch.nn.LayerNorm(129)


def _grouped(model, wd):
    no_decay = ["bias", "layer_norm.weight"]  # run_clm.py:443-458
    return [{"params": [p for n, p in model.named_parameters() if not any(nd in n for nd in no_decay)], "weight_decay": wd},
            {"params": [p for n, p in model.named_parameters() if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]


HYPER = dict(lr=6e-4, betas=(0.9, 0.95), eps=1e-8)


def _true_grads(gen, params, it):
    return [torch.randn(p.shape, generator=gen) * (3.0 if it % 2 else 0.002) for p in params]


@pytest.mark.parametrize("max_norm", [1.0, None])
def test_fused_adamw_amp_with_loss_scaler_seven_steps(ops, max_norm):
    """Seven steps with growth_interval 2, an inf in the third step's gradients and a parameter without a gradient on the fifth: parameters,
    moments, counters, scale and tracker against the restatement after every step.  Without clipping the parent's path - torch's GradScaler
    around a plain FusedAdamW - must give the same parameters bit for bit (fp32 gradients, a power-of-two scale: its unscale pass is exact)."""
    import outeffhop_amd as oa

    torch.manual_seed(5)
    model = Tiny().cuda()
    params = list(model.parameters())
    opt = oa.FusedAdamW(_grouped(model, 0.1), max_grad_norm=max_norm, amp=True, **HYPER)
    scaler = oa.LossScaler(init_scale=2.0 ** 16, growth_interval=2)
    wd = {id(p): g["weight_decay"] for g in opt.param_groups for p in g["params"]}
    twin = ts = None
    if max_norm is None:
        twin = Tiny().cuda()
        twin.load_state_dict(model.state_dict())
        topt = oa.FusedAdamW(_grouped(twin, 0.1), **HYPER)
        ts = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16, growth_interval=2)
        ts.scale(torch.zeros((), device="cuda"))  # (its state is made by the first scale())
    gen = torch.Generator().manual_seed(11)
    counts = [0] * len(params)
    state = np.array([2.0 ** 16, 0, 0, 0], np.float32)
    scales = []
    zeros = lambda p: np.zeros(p.shape, np.float32)  # noqa: E731
    for it in range(1, 8):
        s = scaler.get_scale()
        assert s == float(state[0])
        true = _true_grads(gen, params, it)
        grads = [(g * s).cuda() for g in true]  # what the backward of the scaled loss leaves: exact, s is a power of two
        if it == 3:
            grads[0].view(-1)[17] = float("inf")
        if it == 5:
            grads[1] = None
        for p, g in zip(params, grads):
            p.grad = g
        before = [(p.detach().cpu().numpy().copy(),) + tuple(opt.state[p][k].cpu().numpy().copy() if p in opt.state else zeros(p) for k in ("exp_avg", "exp_avg_sq"))
                  for p in params]
        scaler.step(opt)
        scaler.update()
        skipped = float(opt.step_skipped)
        assert skipped == (1.0 if it == 3 else 0.0)
        state[2] = skipped
        state = A.scaler_update(state, 2.0, 0.5, 2)
        assert np.array_equal(_bits(scaler._state), state.view(np.int32)), (it, scaler._state, state)
        scales.append(float(state[0]))
        c = np.float32(float(opt.clip_coef))
        if it != 3:
            norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g, h in zip(true, grads) if h is not None))
            assert abs(float(opt.grad_norm) - norm) <= 1e-12 * norm  # of the UNSCALED gradients
            assert (float(c) * s < 1.0) == (max_norm is not None and it % 2 == 1)
            if max_norm is None:
                assert float(c) == 1.0 / s
        for i, (p, g) in enumerate(zip(params, grads)):
            if g is not None and it != 3:
                counts[i] += 1
                want = A.step32_amp(before[i][0], g.cpu().numpy(), before[i][1], before[i][2], c, (HYPER["lr"], *HYPER["betas"], HYPER["eps"], wd[id(p)]), counts[i])
            else:
                want = before[i]
            if p in opt.state:
                got = (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
                assert all(np.array_equal(_bits(a), b.view(np.int32)) for a, b in zip(got, want)), (it, i)
                st = opt.state[p]["step"]
                assert float(st) == counts[i] and st.is_cuda and st.dim() == 0 and st.data_ptr() == opt._steps.data_ptr() + 4 * i
            if g is not None:
                assert torch.equal(p.grad, g) or it == 3  # the gradients are not written (nan != nan)
        if twin is not None:
            assert ts.get_scale() == s
            for p, g in zip(twin.parameters(), grads):
                p.grad = None if g is None else g.clone()
            ts.step(topt)
            ts.update()
            for a, b in zip(params, twin.parameters()):
                assert np.array_equal(_bits(a), _bits(b)), it
        opt.zero_grad(set_to_none=True)
    assert scales == [2.0 ** 16, 2.0 ** 17, 2.0 ** 16, 2.0 ** 16, 2.0 ** 17, 2.0 ** 17, 2.0 ** 18]  # up, back off, recover
    assert scaler.steps_skipped() == 1 and counts == [6, 5, 6, 6]
    assert scaler.state_dict() == {"scale": 2.0 ** 18, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2, "_growth_tracker": 0}
    if twin is not None:
        assert ts.state_dict() == scaler.state_dict()


def test_torch_grad_scaler_drives_the_amp_optimizer(ops):
    """torch's GradScaler (and accelerate through it) hands an optimizer with _step_supports_amp_scaling its scale and its own found_inf
    and calls step(): the unscale is folded in and the skip happens on the device."""
    import outeffhop_amd as oa

    torch.manual_seed(6)
    model = Tiny().cuda()
    params = list(model.parameters())
    opt = oa.FusedAdamW(_grouped(model, 0.1), max_grad_norm=1.0, amp=True, **HYPER)
    ts = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, growth_interval=2)
    ts.scale(torch.zeros((), device="cuda"))  # (its state is made by the first scale())
    gen = torch.Generator().manual_seed(12)
    for it in range(1, 4):
        s = ts.get_scale()
        for p, g in zip(params, _true_grads(gen, params, it)):
            p.grad = (g * s).cuda()
        if it == 2:
            params[2].grad[3] = float("nan")
        before = [p.detach().clone() for p in params]
        ts.step(opt)
        ts.update()
        assert float(opt.step_skipped) == (1.0 if it == 2 else 0.0)
        assert all(torch.equal(a, p) == (it == 2) for a, p in zip(before, params))
        assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    assert ts.get_scale() == 2.0 ** 9 and [float(opt.state[p]["step"]) for p in params] == [2.0] * 4


def test_the_steady_loop_does_not_synchronise(ops):
    import outeffhop_amd as oa

    model = Tiny().cuda()
    opt = oa.FusedAdamW(_grouped(model, 0.1), max_grad_norm=1.0, amp=True, **HYPER)
    scaler = oa.LossScaler(growth_interval=2)
    for p in model.parameters():
        p.grad = torch.full_like(p, 64.0)
    scaler.step(opt)  # the planning step: state is made, tables are copied
    scaler.update()
    x = torch.ones(3, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            scaler.step(opt)
            scaler.update()
        with pytest.raises(RuntimeError):  # the mode is live on this build: a deliberate read-back trips it
            x.sum().item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert opt.plan_builds == 1 and scaler.get_scale() == 2.0 ** 17 and [float(opt.state[p]["step"]) for p in model.parameters()] == [3.0] * 4


def test_state_moves_between_amp_plain_and_torch(ops):
    import outeffhop_amd as oa

    torch.manual_seed(9)
    model = Tiny().cuda()
    params = list(model.parameters())
    amp = oa.FusedAdamW(_grouped(model, 0.1), amp=True, **HYPER)
    gen = torch.Generator().manual_seed(13)
    for it in range(1, 4):
        for i, (p, g) in enumerate(zip(params, _true_grads(gen, params, it))):
            p.grad = None if (it == 2 and i == 3) else g.cuda()
        amp.step()  # no scaler: the scale is 1 and the flag is the norm's own
    counts = [3, 3, 3, 2]
    assert [float(amp.state[p]["step"]) for p in params] == counts and float(amp.step_skipped) == 0.0
    wd = {id(p): g["weight_decay"] for g in amp.param_groups for p in g["params"]}

    def twin_model():
        m2 = Tiny().cuda()
        m2.load_state_dict(model.state_dict())
        return m2
    grads = [g.cuda() for g in _true_grads(gen, params, 1)]
    # into a plain FusedAdamW: one step against the restatement of the plain step
    mp = twin_model()
    plain = oa.FusedAdamW(_grouped(mp, 0.1), **HYPER)
    plain.load_state_dict(copy.deepcopy(amp.state_dict()))
    for p, g in zip(mp.parameters(), grads):
        p.grad = g.clone()
    plain.step()
    for i, (p0, p1, g) in enumerate(zip(params, mp.parameters(), grads)):
        pn, mn, vn = R.step32(p0.detach().cpu().numpy(), g.cpu().numpy(), amp.state[p0]["exp_avg"].cpu().numpy(), amp.state[p0]["exp_avg_sq"].cpu().numpy(),
                              np.float32(1.0), (HYPER["lr"], *HYPER["betas"], HYPER["eps"], wd[id(p0)], counts[i] + 1))
        assert np.array_equal(_bits(p1), pn.view(np.int32)) and np.array_equal(_bits(plain.state[p1]["exp_avg_sq"]), vn.view(np.int32))
        st = plain.state[p1]["step"]
        assert float(st) == counts[i] + 1 and st.device.type == "cpu"
    # into torch's fused AdamW: loads and steps
    mt = twin_model()
    tfused = torch.optim.AdamW(_grouped(mt, 0.1), fused=True, **HYPER)
    tfused.load_state_dict(copy.deepcopy(amp.state_dict()))
    for group in tfused.param_groups:
        group["fused"] = True  # (the loaded groups carry FusedAdamW's fused=None)
    for p, g in zip(mt.parameters(), grads):
        p.grad = g.clone()
    tfused.step()
    assert [float(tfused.state[p]["step"]) for p in mt.parameters()] == [c + 1 for c in counts]
    assert all(torch.allclose(a, b, rtol=0.0, atol=1e-6) for a, b in zip(mt.parameters(), mp.parameters()))
    # a plain state into amp: the counters are copied into their slots once, and the step after plans nothing
    mb = twin_model()
    back = oa.FusedAdamW(_grouped(mb, 0.1), amp=True, **HYPER)
    back.load_state_dict(copy.deepcopy(plain.state_dict()))
    assert all(not back.state[p]["step"].is_cuda for p in mb.parameters())
    for p, g in zip(mb.parameters(), grads):
        p.grad = g.clone()
    snap = [(p.detach().clone(), back.state[p]["exp_avg"].clone(), back.state[p]["exp_avg_sq"].clone()) for p in mb.parameters()]
    back.step()
    views = [back.state[p]["step"] for p in mb.parameters()]
    assert back.plan_builds == 1 and all(v.is_cuda and v.data_ptr() == back._steps.data_ptr() + 4 * i for i, v in enumerate(views))
    assert [float(v) for v in views] == [c + 2 for c in counts]
    for i, ((p0, m0, v0), p1, g) in enumerate(zip(snap, mb.parameters(), grads)):
        pn, mn, vn = A.step32_amp(p0.cpu().numpy(), g.cpu().numpy(), m0.cpu().numpy(), v0.cpu().numpy(), np.float32(1.0),
                                  (HYPER["lr"], *HYPER["betas"], HYPER["eps"], wd[id(params[i])]), counts[i] + 2)
        assert np.array_equal(_bits(p1), pn.view(np.int32)) and np.array_equal(_bits(back.state[p1]["exp_avg"]), mn.view(np.int32))
    back.step()
    assert back.plan_builds == 1 and all(a is b for a, b in zip(views, [back.state[p]["step"] for p in mb.parameters()]))
    assert [float(v) for v in views] == [c + 3 for c in counts]


def test_amp_refusals_and_empty_parameters(ops):
    import outeffhop_amd as oa

    ps = [torch.nn.Parameter(torch.randn(6, device="cuda")) for _ in range(9)]
    for p in ps:
        p.grad = torch.ones_like(p)
    # nine step counts are one kernel group under amp; nine hyper-parameter sets are too many
    o = oa.FusedAdamW(ps, amp=True)
    o.step()
    ps[0].grad = None
    o.step()
    assert [float(o.state[p]["step"]) for p in ps] == [1.0] + [2.0] * 8
    ps[0].grad = torch.ones_like(ps[0])
    o = oa.FusedAdamW([{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(ps)], amp=True)
    with pytest.raises(ValueError, match="at most 8"):
        o.step()
    # an empty parameter has no plan record: it is neither stepped nor counted
    e = torch.nn.Parameter(torch.empty(0, device="cuda"))
    e.grad = torch.empty(0, device="cuda")
    ps[0].grad = torch.ones_like(ps[0])
    o = oa.FusedAdamW([ps[0], e, ps[1]], amp=True)
    o.step()
    assert [float(o.state[p]["step"]) for p in (ps[0], e, ps[1])] == [1.0, 0.0, 1.0]
    # a group added later gets slots behind the ones there are
    o.add_param_group({"params": [ps[2]]})
    o.step()
    assert [float(o.state[p]["step"]) for p in (ps[0], e, ps[1], ps[2])] == [2.0, 0.0, 2.0, 1.0]
    # capture still raises, before any state is made
    o = oa.FusedAdamW(ps[3:5], amp=True)
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError, match="captured"):
        with torch.cuda.graph(g):
            x += 1.0
            o.step()
    torch.cuda.synchronize()
    assert len(o.state) == 0
    with pytest.raises(TypeError):
        oa.LossScaler().step(oa.FusedAdamW(ps[:2]))
