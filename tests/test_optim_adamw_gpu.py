"""The fused optimizer step on the device (include/oeh.h: oeh_grad_norm, oeh_grad_scale, oeh_adamw_step; outeffhop_amd/optim.py): every
tensor is a slice of a larger buffer whose other elements are canaries, and whole buffers are compared bit for bit with what the numpy
restatement (tests/_adamw_ref.py) makes of the same inputs - parameters, both moments, the untouched gradients and every canary at once."""
import copy
import gc
import math

import numpy as np
import pytest

from tests import _adamw_ref as R

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DT = (torch.float32, torch.float16, torch.bfloat16)
PAD = 64         # canary elements around every tensor: a multiple of 16 bytes in every storage type
CANARY = -123.5  # exact in fp16 and bf16
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 5)
# lr, beta1, beta2, eps, weight_decay, step: group 0 is a first step (zero state), group 1 has no weight decay
GROUPS = ((1e-3, 0.9, 0.999, 1e-8, 1e-2, 1), (6e-4, 0.9, 0.95, 1e-8, 0.0, 2), (5e-5, 0.8, 0.95, 1e-6, 0.1, 1000))


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """test_modules_gpu.py's mask-address test passes only while the caching allocator hands a freed block straight back, which depends on
    every allocation made in the process before it.  This file is therefore named to be collected AFTER that one (the suite up to there runs
    exactly as it did without this file), and gives its cached blocks back when it is done."""
    yield
    if torch.cuda.is_available():
        from outeffhop_amd import ops as _ops

        _ops._grad_norm_work.clear()
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


class Arena:
    """One host buffer of `dtype` full of canaries in which tensors are placed PAD elements apart, each on a 16-byte boundary plus `disp`
    elements; `upload` makes the device copy and `view(i)` the i-th tensor as a slice of it."""

    def __init__(self, dtype):
        self.dtype, self.parts, self.spans, self.cursor = dtype, [], [], PAD

    def add(self, values: torch.Tensor, disp: int = 0) -> int:
        start = self.cursor + disp
        self.parts.append((start, values.to(self.dtype)))
        self.spans.append((start, start + values.numel()))
        self.cursor = -(-(start + values.numel() + PAD) // 16) * 16
        return len(self.spans) - 1

    def host(self) -> torch.Tensor:
        buf = torch.full((self.cursor + PAD,), CANARY, dtype=self.dtype)
        for start, v in self.parts:
            buf[start:start + v.numel()] = v
        return buf

    def upload(self):
        self.dev = self.host().cuda()
        assert self.dev.data_ptr() % 16 == 0
        return self.dev

    def view(self, i) -> torch.Tensor:
        a, b = self.spans[i]
        return self.dev[a:b]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class Case:
    """A tensor list in arenas: p, m, v in three fp32 arenas, g in one arena per storage type."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.P, self.M, self.V = Arena(torch.float32), Arena(torch.float32), Arena(torch.float32)
        self.G = {dt: Arena(dt) for dt in DT}
        self.items = []  # (index in P / M / V, g dtype, index in G[dtype], group, n)

    def add(self, n, dt, group, gscale=1.0, disp=(0, 0, 0, 0), g=None):
        """g: the gradient's values instead of random ones (exact in `dt`)"""
        p, g_, m, v = R.random_state(self.rng, n, gscale, first=GROUPS[group][5] == 1)
        g = g_ if g is None else np.asarray(g, dtype=np.float32)
        i = self.P.add(_t(p), disp[0])
        self.M.add(_t(m), disp[2])
        self.V.add(_t(v), disp[3])
        self.items.append((i, dt, self.G[dt].add(_t(g), disp[1]), group, n))

    def upload(self):
        for a in (self.P, self.M, self.V, *self.G.values()):
            a.upload()

    def lists(self):
        ps = [self.P.view(i) for i, *_ in self.items]
        ms = [self.M.view(i) for i, *_ in self.items]
        vs = [self.V.view(i) for i, *_ in self.items]
        gs = [self.G[dt].view(j) for _, dt, j, _, _ in self.items]
        return ps, gs, ms, vs, [grp for *_, grp, _ in self.items]

    def expected(self, c):
        """The three fp32 arenas after one step with coefficient c (fp32), as host tensors: the restatement inside, canaries outside."""
        P, M, V = self.P.host(), self.M.host(), self.V.host()
        G = {dt: a.host() for dt, a in self.G.items()}
        for i, dt, j, grp, n in self.items:
            (a, b), (ga, gb) = self.P.spans[i], self.G[dt].spans[j]
            (ma, mb), (va, vb) = self.M.spans[i], self.V.spans[i]
            g32 = G[dt][ga:gb].float().numpy()
            pn, mn, vn = R.step32(P[a:b].numpy(), g32, M[ma:mb].numpy(), V[va:vb].numpy(), c, GROUPS[grp])
            P[a:b], M[ma:mb], V[va:vb] = _t(pn), _t(mn), _t(vn)
        return P, M, V

    def sumsq(self):
        g = np.concatenate([self.G[dt].host()[slice(*self.G[dt].spans[j])].double().numpy() for _, dt, j, _, _ in self.items] or [np.zeros(0)])
        return float(np.sum(g * g)), g.size


def _groups(ops):
    return [ops.AdamWGroup(*g) for g in GROUPS]


@pytest.fixture(scope="module")
def big(ops):
    """ONE call of grad_norm + adamw_step over the whole list of the module's docstring; the tests below look at its pieces."""
    case = Case(20261020)
    k = 0
    for n in SIZES:
        for dt in DT:
            case.add(n, dt, k % 3, gscale=(1.0, 1e-3, 30.0)[k % 3])
            k += 1
    case.add(0, torch.float32, 0)
    # every fp16 subnormal, both signs, and the zeros: the 16-bit unpack must keep them (k 2^-24 is a normal fp32 number)
    sub = np.arange(-1023, 1024, dtype=np.float32) * np.float32(2.0 ** -24)
    case.add(sub.size, torch.float16, 1, g=sub)
    case.add(sub.size + 2, torch.float16, 2, g=np.concatenate([sub[::-1], [-0.0, 6.103515625e-05]]), disp=(0, 1, 0, 0))
    for i in range(300):
        case.add(1 + i % 9, DT[i % 3], (i // 3) % 3, gscale=0.1)
    for dt in DT:  # each of p, g, m, v one element off its 16-byte boundary, alone
        for which in range(4):
            disp = [0, 0, 0, 0]
            disp[which] = 1
            case.add(4096 + 5, dt, which % 3, disp=tuple(disp))
    case.upload()
    ps, gs, ms, vs, grp = case.lists()
    plan = ops.mt_plan(ps, gs, ms, vs, grp)
    out4 = ops.grad_norm(plan, 1.0)
    again = ops.grad_norm(plan, 1.0)
    g_before = {dt: _bits(a.dev) for dt, a in case.G.items()}
    ops.adamw_step(plan, _groups(ops), clip=out4)
    torch.cuda.synchronize()
    return case, plan, out4.cpu().numpy(), again.cpu().numpy(), g_before


def test_plan_of_the_list(big, ops):
    case, plan, *_ = big
    live = [it for it in case.items if it[4] > 0]
    assert plan.n_chunks == sum(-(-n // ops.MT_CHUNK) for *_, n in live) and plan.numel == sum(n for *_, n in live)
    assert len(plan.variants) == len(live)
    assert plan.variants[-12:] == ["elem"] * 12 and plan.variants[:-12].count("elem") == 1  # (the displaced subnormal list)


def test_step_is_the_restatement_bit_for_bit_with_canaries_and_gradients_intact(big):
    case, plan, out4, _, g_before = big
    assert 0.0 < out4[2] < 1.0  # the clip is active
    c = np.float32(out4[2])
    P, M, V = case.expected(c)
    for name, arena, want in (("p", case.P, P), ("exp_avg", case.M, M), ("exp_avg_sq", case.V, V)):
        got = _bits(arena.dev)
        bad = np.flatnonzero(got != _bits(want))
        assert bad.size == 0, f"{name}: {bad.size} elements differ, first at {bad[:5]}"
    assert np.isfinite(P.numpy()).all() and not torch.equal(P, case.P.host())
    for dt, arena in case.G.items():  # the clip is folded in: the gradients are not written
        assert np.array_equal(_bits(arena.dev), g_before[dt]) and np.array_equal(g_before[dt], _bits(arena.host())), dt


def test_norm_of_the_list(big):
    case, plan, out4, again, _ = big
    want, n = case.sumsq()
    assert n == plan.numel
    assert abs(out4[0] - want) <= (n + 4) * 2.0 ** -52 * want
    ulp = lambda x: math.ulp(x)  # noqa: E731
    norm = math.sqrt(out4[0])
    assert abs(out4[1] - norm) <= 2 * ulp(norm)
    coef = min(1.0, 1.0 / (out4[1] + 1e-6))
    assert abs(out4[2] - coef) <= 2 * ulp(coef) and out4[3] == 0.0
    assert np.array_equal(out4.view(np.int64), again.view(np.int64))  # two calls, the same bits


@pytest.fixture(scope="module")
def small(ops):
    """A shorter list for the calls that need fresh gradients: every storage type, full and ragged chunks, both access forms."""
    def make():
        case = Case(7)
        for k, (n, disp) in enumerate(((5, 0), (4096, 0), (4097, 0), (1025, 1), (4096 + 3, 1), (2 * 4096, 0))):
            for dt in DT:
                case.add(n, dt, 1, gscale=(1.0, 1e-2)[k % 2], disp=(0, disp, 0, 0))
        case.upload()
        return case
    return make


def test_norm_coefficients_and_nan(small, ops):
    case = small()
    ps, gs, ms, vs, grp = case.lists()
    plan = ops.mt_plan(ps, gs, ms, vs, grp)
    want, n = case.sumsq()
    outs = {mx: ops.grad_norm(plan, mx) for mx in (None, 0.0, float("inf"), 1e9, 0.5, -1.0)}
    normonly = ops.grad_norm(ops.mt_plan(None, gs), 0.5)  # the plan without p, m, v: the same chunks, the same sums
    gs[4].view(-1)[1000 if gs[4].numel() > 1000 else 0] = float("nan")
    nan = ops.grad_norm(plan, 0.5).cpu().numpy()
    outs = {k: v.cpu().numpy() for k, v in outs.items()}
    for mx, o in outs.items():
        assert abs(o[0] - want) <= (n + 4) * 2.0 ** -52 * want and abs(o[1] - math.sqrt(o[0])) <= 2 * math.ulp(o[1])
        assert o[0] == outs[None][0] and o[1] == outs[None][1]
        if mx != 0.5:
            assert o[2] == 1.0, mx  # None, 0, negative and inf: no clipping; 1e9: inactive, exactly 1
    coef = 0.5 / (outs[0.5][1] + 1e-6)
    assert coef < 1.0 and abs(outs[0.5][2] - coef) <= 2 * math.ulp(coef)
    assert np.array_equal(normonly.cpu().numpy().view(np.int64), outs[0.5].view(np.int64))
    assert math.isnan(nan[0]) and math.isnan(nan[1]) and math.isnan(nan[2])


def test_grad_scale_rounds_twice_in_every_storage_type(small, ops):
    case = small()
    _, gs, *_ = case.lists()
    plan = ops.mt_plan(None, gs)
    assert plan.norm_only and "elem" in plan.variants and "vec16" in plan.variants
    out4 = ops.grad_norm(plan, 0.37)
    ops.grad_scale_(plan, out4)
    c = torch.tensor(np.float32(out4.cpu().numpy()[2]))
    assert 0.0 < float(c) < 1.0
    for dt, arena in case.G.items():
        want = arena.host()
        for a, b in arena.spans:
            want[a:b] = (want[a:b].float() * c).to(dt)  # RN_dtype(fp32(g) * c): the product rounded to fp32 first
        bad = np.flatnonzero(_bits(arena.dev) != _bits(want))
        assert bad.size == 0, f"{dt}: {bad.size} elements differ, first at {bad[:5]}"
    with pytest.raises(ValueError):
        ops.adamw_step(plan, _groups(ops))  # a plan without moments is not stepped


def test_step_without_clip_and_empty_plans(small, ops):
    case = small()
    ps, gs, ms, vs, grp = case.lists()
    plan = ops.mt_plan(ps, gs, ms, vs, grp)
    ops.adamw_step(plan, _groups(ops))  # clip=None: coefficient 1, nothing read
    P, M, V = case.expected(np.float32(1.0))
    for arena, want in ((case.P, P), (case.M, M), (case.V, V)):
        assert np.array_equal(_bits(arena.dev), _bits(want))
    # nothing but empty tensors: no chunk, no launch of the chunk kernels, a norm of zero
    e = [torch.empty(0, device="cuda") for _ in range(4)]
    plan0 = ops.mt_plan(e[:1], e[1:2], e[2:3], e[3:])
    assert plan0.n_chunks == 0 and plan0.numel == 0
    out4 = ops.grad_norm(plan0, 1.0)
    ops.adamw_step(plan0, _groups(ops), clip=out4)
    ops.adamw_step(plan0, _groups(ops))
    ops.grad_scale_(plan0, out4)
    assert out4.cpu().tolist() == [0.0, 0.0, 1.0, 0.0]
    with pytest.raises(ValueError):
        ops.adamw_step(plan, _groups(ops)[:1])  # the list names group 1
    from outeffhop_amd import _lib
    with pytest.raises(_lib.OehError):
        ops.mt_plan([torch.zeros(4)], [torch.zeros(4)], [torch.zeros(4)], [torch.zeros(4)])


class Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(37, 129)
        self.layer_norm = torch.nn.LayerNorm(129)


def _grouped(model, wd):
    no_decay = ["bias", "layer_norm.weight"]  # run_clm.py:443-458
    return [{"params": [p for n, p in model.named_parameters() if not any(nd in n for nd in no_decay)], "weight_decay": wd},
            {"params": [p for n, p in model.named_parameters() if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]


def test_fused_adamw_four_steps(ops):
    import outeffhop_amd as oa

    torch.manual_seed(5)
    model = Tiny().cuda()
    params = list(model.parameters())
    hyper = dict(lr=6e-4, betas=(0.9, 0.95), eps=1e-8)
    o = oa.FusedAdamW(_grouped(model, 0.1), max_grad_norm=1.0, **hyper)
    wd = {id(p): g["weight_decay"] for g in o.param_groups for p in g["params"]}
    assert sorted(wd.values()) == [0.0, 0.0, 0.0, 0.1]
    gen = torch.Generator().manual_seed(11)
    steps = [0] * len(params)
    for it in range(1, 5):
        grads = [(torch.randn(p.shape, generator=gen) * (3.0 if it % 2 else 0.002)).cuda() for p in params]  # ~5000 elements: norms of ~210 and ~0.14
        if it == 3:
            grads[1] = None  # this parameter sits the step out and lags one behind from here on
        for p, g in zip(params, grads):
            p.grad = g
        before = [(p.detach().cpu().numpy().copy(),) + tuple(o.state[p][k].cpu().numpy().copy() if p in o.state else np.zeros(p.shape, np.float32)
                                                              for k in ("exp_avg", "exp_avg_sq")) for p in params]
        twins = [torch.nn.Parameter(torch.zeros_like(p)) for p, g in zip(params, grads) if g is not None]
        for t_, g in zip(twins, [g for g in grads if g is not None]):
            t_.grad = g.clone()
        o.step()
        total = oa.clip_grad_norm_(twins, 1.0)
        assert total.dtype == torch.float64 and total.dim() == 0 and _bits(total) == _bits(o.grad_norm)
        norm = float(o.grad_norm)
        assert abs(norm - math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads if g is not None))) <= 1e-12 * norm
        c = np.float32(float(o.clip_coef))
        assert (c < 1.0) == (it % 2 == 1)
        for t_, g in zip(twins, [g for g in grads if g is not None]):  # the stand-alone clip scaled its copies by the same coefficient
            assert torch.equal(t_.grad, g * torch.tensor(c, device="cuda"))
        for i, (p, g) in enumerate(zip(params, grads)):
            if g is None:
                assert np.array_equal(p.detach().cpu().numpy(), before[i][0])
                continue
            steps[i] += 1
            pn, mn, vn = R.step32(before[i][0], g.cpu().numpy(), before[i][1], before[i][2], c,
                                  (hyper["lr"], *hyper["betas"], hyper["eps"], wd[id(p)], steps[i]))
            assert np.array_equal(_bits(p), pn.view(np.int32)) and np.array_equal(_bits(o.state[p]["exp_avg"]), mn.view(np.int32))
            assert np.array_equal(_bits(o.state[p]["exp_avg_sq"]), vn.view(np.int32))
            assert torch.equal(p.grad, g)
        o.zero_grad(set_to_none=True)  # the next gradients get new addresses: the plan is rebuilt
    assert steps == [4, 3, 4, 4]
    for p, s in zip(params, steps):
        st = o.state[p]["step"]
        assert float(st) == s and st.device.type == "cpu" and st.dtype == torch.float32

    # the state into torch.optim.AdamW and into a second FusedAdamW (no clipping): one step of each, both against float64
    def twin_model():
        m2 = Tiny().cuda()
        m2.load_state_dict(model.state_dict())
        return m2
    ma, mb = twin_model(), twin_model()
    ta = torch.optim.AdamW(_grouped(ma, 0.1), **hyper)
    fb = oa.FusedAdamW(_grouped(mb, 0.1), **hyper)
    # (a copy each: load_state_dict keeps the CPU step tensors it is handed, and the in-place increment would be shared)
    ta.load_state_dict(copy.deepcopy(o.state_dict()))
    fb.load_state_dict(copy.deepcopy(o.state_dict()))
    grads = [torch.randn(p.shape, generator=gen).cuda() for p in params]
    worst = np.zeros(3)
    for mdl, opt in ((ma, ta), (mb, fb)):
        for p, g in zip(mdl.parameters(), grads):
            p.grad = g.clone()
        opt.step()
        for i, (p0, p1, g) in enumerate(zip(params, mdl.parameters(), grads)):
            got = tuple(x.detach().cpu().numpy() for x in (p1, opt.state[p1]["exp_avg"], opt.state[p1]["exp_avg_sq"]))
            assert float(opt.state[p1]["step"]) == steps[i] + 1
            r = R.bound_ratios(p0.detach().cpu().numpy(), g.cpu().numpy(), o.state[p0]["exp_avg"].cpu().numpy(), o.state[p0]["exp_avg_sq"].cpu().numpy(),
                               np.float32(1.0), (hyper["lr"], *hyper["betas"], hyper["eps"], wd[id(p0)], steps[i] + 1), got=got)
            worst = np.maximum(worst, r)
    print(f"torch.optim.AdamW and FusedAdamW from one state, worst |fp32 - float64| / bound: m' {worst[0]:.3f}  v' {worst[1]:.3f}  p' {worst[2]:.3f}")
    assert (worst <= 1.0).all(), worst
    assert fb.grad_norm is None  # no max_grad_norm: no norm


def test_fused_adamw_refusals_on_the_device(ops):
    import outeffhop_amd as oa

    ps = [torch.nn.Parameter(torch.randn(6, device="cuda")) for _ in range(9)]
    for p in ps:
        p.grad = torch.ones_like(p)
    o = oa.FusedAdamW([{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(ps)])
    with pytest.raises(ValueError, match="at most 8"):
        o.step()
    o = oa.FusedAdamW(ps[:8] + [torch.nn.Parameter(torch.zeros(3))])
    o.param_groups[0]["params"][-1].grad = torch.ones(3)
    from outeffhop_amd import _lib
    with pytest.raises(_lib.OehError):  # a CPU parameter among GPU ones
        o.step()
    # under stream capture the step refuses before it makes state or launches anything
    o = oa.FusedAdamW(ps[:2])
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(8, device="cuda")
    with pytest.raises(RuntimeError, match="captured"):
        with torch.cuda.graph(g):
            x += 1.0
            o.step()
    torch.cuda.synchronize()
    assert len(o.state) == 0
    o.step()  # and outside it steps
    assert float(o.state[ps[0]]["step"]) == 1.0


def test_a_tensor_of_a_group_the_descriptor_lacks_is_left_alone(small, ops):
    """At the C ABI the plan is device memory the host does not read: the kernel itself skips such a tensor (the Python layer refuses)."""
    import ctypes as C

    from outeffhop_amd import _lib

    case = small()  # every tensor in group 1
    ps, gs, ms, vs, grp = case.lists()
    grp[0] = 0
    plan = ops.mt_plan(ps, gs, ms, vs, grp)
    d = _lib.oeh_adamw_desc()
    d.n_groups = 1
    d.lr[0], d.beta1[0], d.beta2[0], d.eps[0], d.weight_decay[0], d.step[0] = GROUPS[0]
    rc = _lib.load().oeh_adamw_step(C.c_void_p(plan.table.data_ptr()), plan.n_chunks, C.byref(d), None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    P, M, V = case.P.host(), case.M.host(), case.V.host()
    i, dt, j, _, n = case.items[0]
    (a, b), (ma, mb), (va, vb), (ga, gb) = case.P.spans[i], case.M.spans[i], case.V.spans[i], case.G[dt].spans[j]
    pn, mn, vn = R.step32(P[a:b].numpy(), case.G[dt].host()[ga:gb].float().numpy(), M[ma:mb].numpy(), V[va:vb].numpy(), np.float32(1.0), GROUPS[0])
    P[a:b], M[ma:mb], V[va:vb] = _t(pn), _t(mn), _t(vn)
    for arena, want in ((case.P, P), (case.M, M), (case.V, V)):  # tensor 0 stepped, every other tensor and canary as before
        assert np.array_equal(_bits(arena.dev), _bits(want))


def test_cached_plan_frees_the_gradients_and_follows_their_addresses(ops):
    """The loop the reference runs is backward, step(), zero_grad() with torch's default set_to_none=True: the cached plan must not keep
    the old gradients alive, must be kept while every address is the same and rebuilt when one moves, and its table must come from
    pinned memory (an asynchronous copy: a pageable source would make step() wait for the stream)."""
    import outeffhop_amd as oa

    ps = [torch.nn.Parameter(torch.randn(n, device="cuda")) for n in (300_000, 70_001, 5)]
    o = oa.FusedAdamW(ps, lr=1e-3, max_grad_norm=1.0)
    grad_bytes = sum(4 * p.numel() for p in ps)

    def backward():
        for p in ps:
            p.grad = torch.full_like(p, 0.25)

    backward()
    o.step()
    assert o.plan_builds == 1 and o._plan.staging.is_pinned() and all(t[1] is None for t in o._plan.tensors)
    o.step()  # the same gradient tensors: nothing is planned
    assert o.plan_builds == 1
    addrs = [p.grad.data_ptr() for p in ps]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    o.zero_grad()  # set_to_none=True
    assert all(p.grad is None for p in ps)
    assert before - torch.cuda.memory_allocated() >= grad_bytes  # the plan did not hold them
    backward()
    builds = o.plan_builds
    same = [p.grad.data_ptr() for p in ps] == addrs
    o.step()
    assert o.plan_builds == builds + (0 if same else 1)
    # gradients that moved: the old ones are held here, so the new ones cannot have their addresses
    held = [p.grad for p in ps]
    backward()
    assert all(p.grad.data_ptr() != h.data_ptr() for p, h in zip(ps, held))
    builds, table, norm_view = o.plan_builds, o._plan.table.data_ptr(), o.grad_norm.data_ptr()
    before_p = [p.detach().clone() for p in ps]
    o.step()
    assert o.plan_builds == builds + 1 and all(not torch.equal(a, p) for a, p in zip(before_p, ps))
    # planning again wrote the table and the norm where they were: the step allocates nothing that would move the next gradients
    assert o._plan.table.data_ptr() == table and o.grad_norm.data_ptr() == norm_view
    assert [float(o.state[p]["step"]) for p in ps] == [4.0] * 3
    # and a rebuilt plan steps the right memory: one more step against the restatement from a snapshot
    m0 = [o.state[p]["exp_avg"].clone() for p in ps]
    v0 = [o.state[p]["exp_avg_sq"].clone() for p in ps]
    p0 = [p.detach().clone() for p in ps]
    o.step()
    c = np.float32(float(o.clip_coef))
    for p, a, m, v in zip(ps, p0, m0, v0):
        pn, mn, vn = R.step32(a.cpu().numpy(), p.grad.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), c, (1e-3, 0.9, 0.999, 1e-8, 1e-2, 5))
        assert np.array_equal(_bits(p), pn.view(np.int32)) and np.array_equal(_bits(o.state[p]["exp_avg_sq"]), vn.view(np.int32))
