"""The loss-scaling form of the optimizer phase without a GPU (include/oeh.h: oeh_grad_norm_amp, oeh_adamw_step_amp,
oeh_loss_scale_update): the numpy restatement (tests/_adamw_amp_ref.py) against tests/_adamw_ref.py, the float64 bounds of DESIGN.md
section 17 and torch's scale rule, and every refusal of the entry points through ctypes."""
import ctypes as C

import numpy as np
import pytest

from tests import _adamw_amp_ref as A
from tests import _adamw_ref as R

# lr, beta1, beta2 of test_optim_adamw_gpu.py's three GROUPS, and (4e-4, 0.9, 0.98)
HYPER = ((1e-3, 0.9, 0.999), (6e-4, 0.9, 0.95), (5e-5, 0.8, 0.95), (4e-4, 0.9, 0.98))
STEPS = list(range(1, 20001)) + [2 ** k for k in range(15, 24)] + [2 ** 24 - 1]
EINVAL, EALIGN, ENOTSUP = -22, -14, -95


def test_binary_exponentiation_gives_the_plain_steps_constants_bit_for_bit():
    """The precondition of every bit-equality between the amp step and the plain one: bc2 and ss from binary exponentiation in double equal
    the ones from libm's pow after the rounding to fp32, for every step number a counter of these tests can hold."""
    ts = np.array(STEPS, np.int64)
    differ = 0
    for lr, b1, b2 in HYPER:
        bc2, ss = A.amp_constants_many(lr, b1, b2, ts)
        want = np.array([R.constants32(lr, b1, b2, 1e-8, 0.0, int(t))[4::2] for t in STEPS], np.float32)
        differ += int((bc2.view(np.int32) != want[:, 0].view(np.int32)).sum() + (ss.view(np.int32) != want[:, 1].view(np.int32)).sum())
        for t in (1, 2, 3, 1000, 2 ** 24 - 1):  # the scalar form is the array form
            one = A.amp_constants(lr, b1, b2, t)
            i = STEPS.index(t)
            assert one[0].view(np.int32) == bc2[i].view(np.int32) and one[1].view(np.int32) == ss[i].view(np.int32)
    print(f"{differ} of {2 * len(HYPER) * len(STEPS)} constants differ")
    assert differ == 0
    assert A.amp_constants(1e-3, 0.9, 0.999, 0) == (0.0, 0.0)
    assert A.pw(0.0, 5) == 0.0 and A.pw(0.5, 0) == 1.0 and A.pw(0.5, 10) == 2.0 ** -10


def test_norm_finalize_restated():
    plain = A.norm_amp(9.0, 1.0)
    assert plain.tolist() == [9.0, 3.0, 1.0 / (3.0 + 1e-6), 0.0]
    for k in (16, -3):  # a power-of-two scale changes neither norm nor clip coefficient by a bit
        o = A.norm_amp(9.0 * 4.0 ** k, 1.0, 2.0 ** k)
        assert o[1] == plain[1] and o[2] * 2.0 ** k == plain[2] and o[3] == 0.0
    assert A.norm_amp(9.0, None, 3072.0)[2] == 1.0 / 3072.0 and A.norm_amp(9.0, -1.0, 4.0)[2] == 0.25
    assert A.norm_amp(float("inf"), 1.0)[3] == 1.0 and A.norm_amp(float("nan"), 1.0, 2.0)[3] == 1.0
    assert A.norm_amp(9.0, 1.0, 2.0, found_in=True)[3] == 1.0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert A.norm_amp(9.0, 1.0, bad)[3] == 1.0


@pytest.mark.parametrize("s", [1.0, 2.0 ** 16, 3.0 * 2 ** 10, 1e4])
def test_restated_step_stays_inside_the_float64_bounds(s):
    rng = np.random.default_rng(17)
    worst = np.zeros(3)
    for (lr, b1, b2, eps, wd, t), gscale in zip(((1e-3, 0.9, 0.999, 1e-8, 1e-2, 1), (6e-4, 0.9, 0.95, 1e-8, 0.0, 2), (5e-5, 0.8, 0.95, 1e-6, 0.1, 1000)),
                                               (1.0, 1e-3, 30.0)):
        p, g, m, v = R.random_state(rng, 3 * 4096 + 5, gscale, first=t == 1)
        stored = (g.astype(np.float64) * s).astype(np.float32)  # what a backward of the scaled loss leaves
        for max_norm in (None, 1.0):
            out4 = A.norm_amp(float(np.sum(stored.astype(np.float64) ** 2)), max_norm, s)
            c = np.float32(out4[2])
            got = A.step32_amp(p, stored, m, v, c, (lr, b1, b2, eps, wd), t)
            worst = np.maximum(worst, R.bound_ratios(p, stored, m, v, c, (lr, b1, b2, eps, wd, t), got=got))
    print(f"s = {s}: worst |fp32 - float64| / bound  m' {worst[0]:.3f}  v' {worst[1]:.3f}  p' {worst[2]:.3f}")
    assert (worst <= 1.0).all(), worst


def _run(state, founds, growth, backoff, interval):
    out = []
    for f in founds:
        state = np.array(state, np.float32)
        state[2] = f
        state = A.scaler_update(state, growth, backoff, interval)
        out.append(state.copy())
    return out


def test_scaler_rule_backs_off_grows_and_never_reaches_inf():
    founds = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0]
    seq = _run([65536.0, 0, 0, 0], founds, 2.0, 0.5, 2)
    assert [float(s[0]) for s in seq] == [65536.0, 131072.0, 65536.0, 65536.0, 131072.0, 131072.0, 65536.0, 32768.0, 32768.0, 65536.0]
    assert [int(s[1]) for s in seq] == [1, 0, 0, 1, 0, 1, 0, 0, 1, 0]  # the tracker is cleared on backoff and on growth
    assert [int(s[3]) for s in seq] == [0, 0, 1, 1, 1, 1, 2, 3, 3, 3] and all(s[2] == 0 for s in seq)
    top = np.float32(np.finfo(np.float32).max / 1.5)
    seq = _run([top, 0, 0, 0], [0] * 6, 2.0, 0.5, 1)
    assert all(s[0] == top and np.isfinite(s[0]) and s[1] == 0 for s in seq)  # 2 * top is inf: the scale stays, the tracker starts over


def test_scaler_rule_is_torchs():
    torch = pytest.importorskip("torch")
    try:
        torch._amp_update_scale_(torch.tensor([4.0]), torch.tensor([0], dtype=torch.int32), torch.tensor([0.0]), 2.0, 0.5, 2)
    except (RuntimeError, NotImplementedError) as e:
        pytest.skip(f"this torch build has no CPU kernel for _amp_update_scale_: {e}")
    rng = np.random.default_rng(3)
    for growth, backoff, interval, start in ((2.0, 0.5, 2, 65536.0), (2.0, 0.5, 3, 1.0), (2.0, 0.5, 1, float(np.finfo(np.float32).max / 1.5))):
        founds = (rng.random(40) < 0.3).astype(np.float32)
        scale, tracker = torch.tensor([start]), torch.tensor([0], dtype=torch.int32)
        state = np.array([start, 0, 0, 0], np.float32)
        for f in founds:
            torch._amp_update_scale_(scale, tracker, torch.tensor([float(f)]), growth, backoff, interval)
            state[2] = f
            state = A.scaler_update(state, growth, backoff, interval)
            assert state[0] == scale.item() and int(state[1]) == tracker.item()
        assert int(state[3]) == int(founds.sum())


def test_loss_scaler_state_dict_has_grad_scalers_keys():
    torch = pytest.importorskip("torch")
    import outeffhop_amd as oa

    # (GradScaler() names the GPU and disables itself with a warning where there is none - its state_dict() is then empty; "cpu" keeps it
    # enabled, and the keys do not depend on the device)
    theirs = torch.amp.GradScaler("cpu", init_scale=1024.0, growth_interval=7)
    ours = oa.LossScaler(init_scale=1024.0, growth_interval=7)
    assert ours.state_dict() == theirs.state_dict() and list(ours.state_dict()) == list(theirs.state_dict())
    assert len(ours.state_dict()) == 5
    ours.load_state_dict({**theirs.state_dict(), "scale": 8.0, "_growth_tracker": 3})
    assert ours.state_dict()["scale"] == 8.0 and ours.state_dict()["_growth_tracker"] == 3 and ours.steps_skipped() == 0
    theirs.load_state_dict(ours.state_dict())
    assert theirs.state_dict() == ours.state_dict()
    assert oa.LossScaler(enabled=False).state_dict() == {} and oa.LossScaler(enabled=False).get_scale() == 1.0
    with pytest.raises(TypeError):
        ours.step(torch.optim.SGD([torch.nn.Parameter(torch.zeros(2))], lr=0.1))
    with pytest.raises(TypeError):  # a plain FusedAdamW takes no part in the protocol
        ours.step(oa.FusedAdamW([torch.nn.Parameter(torch.zeros(2))]))
    assert oa.FusedAdamW([torch.nn.Parameter(torch.zeros(2))], amp=True)._step_supports_amp_scaling is True
    assert not hasattr(oa.FusedAdamW([torch.nn.Parameter(torch.zeros(2))]), "_step_supports_amp_scaling")
    for bad in (dict(growth_factor=0.0), dict(backoff_factor=float("inf")), dict(growth_interval=0)):
        with pytest.raises(ValueError):
            oa.LossScaler(**bad)


def _desc(_lib, n_groups=1):
    d = _lib.oeh_adamw_desc()
    d.n_groups = n_groups
    for i in range(max(n_groups, 0) if n_groups <= 8 else 0):
        d.lr[i], d.beta1[i], d.beta2[i], d.eps[i], d.weight_decay[i] = 1e-3, 0.9, 0.999, 1e-8, 1e-2
    return d


def test_refusals_of_the_three_entry_points_without_a_gpu():
    from outeffhop_amd import _lib

    lib = _lib.load()
    a8, a4, odd = C.c_void_p(4096), C.c_void_p(4100), C.c_void_p(4098)

    # oeh_grad_norm_amp: oeh_grad_norm's refusals ...
    norm = lib.oeh_grad_norm_amp
    assert norm(a8, 1, 1.0, None, None, None, a8, None, None) == EINVAL   # out4 NULL
    assert norm(a8, 1, 1.0, None, None, None, None, a8, None) == EINVAL   # work NULL with chunks
    assert norm(None, 1, 1.0, None, None, None, a8, a8, None) == EINVAL   # plan NULL with chunks
    assert norm(a8, -1, 1.0, None, None, None, a8, a8, None) == EINVAL    # n_chunks < 0
    assert norm(a8, 2 ** 31, 1.0, None, None, None, a8, a8, None) == ENOTSUP
    assert norm(a8, 1, 1.0, None, None, None, a4, a8, None) == EALIGN     # work off 8 bytes
    assert norm(a8, 1, 1.0, None, None, None, a8, a4, None) == EALIGN     # out4 off 8 bytes
    # ... and each of the three fp32 pointers off 4 bytes
    assert norm(a8, 1, 1.0, odd, None, None, a8, a8, None) == EALIGN
    assert norm(a8, 1, 1.0, a4, odd, None, a8, a8, None) == EALIGN
    assert norm(a8, 1, 1.0, a4, a4, odd, a8, a8, None) == EALIGN

    assert lib.oeh_adamw_amp_work_bytes(0) == 0 and lib.oeh_adamw_amp_work_bytes(3) == 24 and lib.oeh_adamw_amp_work_bytes(-1) == 0
    assert lib.oeh_adamw_amp_work_bytes(2 ** 31 - 1) == 8 * (2 ** 31 - 1)

    # oeh_adamw_step_amp: oeh_adamw_step's refusals without the step < 1 rule ...
    step = lib.oeh_adamw_step_amp
    ok = _desc(_lib)
    assert ok.step[0] == 0
    assert step(a8, 0, 0, C.byref(ok), a8, a4, a4, a4, None) == 0         # step[] is not read; no chunk: OEH_OK without a launch
    assert step(None, 0, 0, C.byref(ok), None, None, None, None, None) == 0
    assert step(a8, 1, 1, None, a8, a4, a4, a4, None) == EINVAL           # d NULL
    for n_groups in (0, 9, -1):
        assert step(a8, 1, 1, C.byref(_desc(_lib, n_groups)), a8, a4, a4, a4, None) == EINVAL
    d = _desc(_lib)
    d.reserved = 1
    assert step(a8, 1, 1, C.byref(d), a8, a4, a4, a4, None) == EINVAL
    for field, bad in (("lr", -1.0), ("lr", float("nan")), ("eps", -1e-8), ("eps", float("nan")), ("weight_decay", -0.1), ("weight_decay", float("nan")),
                       ("beta1", 1.0), ("beta1", -0.1), ("beta1", float("nan")), ("beta2", 1.0), ("beta2", -0.1), ("beta2", float("nan"))):
        d = _desc(_lib, 2)
        getattr(d, field)[1] = bad
        assert step(a8, 1, 1, C.byref(d), a8, a4, a4, a4, None) == EINVAL, (field, bad)
        d.n_groups = 1  # a column the descriptor does not use is not looked at
        assert step(a8, 0, 1, C.byref(d), a8, a4, a4, a4, None) == 0
    assert step(a8, -1, 1, C.byref(ok), a8, a4, a4, a4, None) == EINVAL
    assert step(None, 1, 1, C.byref(ok), a8, a4, a4, a4, None) == EINVAL
    assert step(a8, 2 ** 31, 1, C.byref(ok), a8, a4, a4, a4, None) == ENOTSUP
    # ... and its own
    assert step(a8, 1, -1, C.byref(ok), a8, a4, a4, a4, None) == EINVAL   # n_tensors < 0
    assert step(a8, 0, -1, C.byref(ok), a8, a4, a4, a4, None) == EINVAL
    for k in range(4):  # clip4, steps, slot, work: NULL with chunks
        args = [a8, a4, a4, a4]
        args[k] = None
        assert step(a8, 1, 1, C.byref(ok), *args, None) == EINVAL, k
    assert step(a8, 1, 1, C.byref(ok), a4, a4, a4, a4, None) == EALIGN    # clip4 off 8 bytes
    for k in range(1, 4):
        args = [a8, a4, a4, a4]
        args[k] = odd
        assert step(a8, 1, 1, C.byref(ok), *args, None) == EALIGN, k
        assert step(a8, 0, 1, C.byref(ok), *args, None) == EALIGN, k

    upd = lib.oeh_loss_scale_update
    assert upd(None, 2.0, 0.5, 2000, None) == EINVAL
    for growth, backoff, interval in ((0.0, 0.5, 1), (-2.0, 0.5, 1), (float("inf"), 0.5, 1), (float("nan"), 0.5, 1),
                                      (2.0, 0.0, 1), (2.0, -0.5, 1), (2.0, float("inf"), 1), (2.0, float("nan"), 1), (2.0, 0.5, 0), (2.0, 0.5, -3)):
        assert upd(a4, growth, backoff, interval, None) == EINVAL, (growth, backoff, interval)
    assert upd(odd, 2.0, 0.5, 2000, None) == EALIGN


def test_ops_refuse_cpu_tensors():
    torch = pytest.importorskip("torch")
    from outeffhop_amd import _lib, ops

    with pytest.raises(_lib.OehError):
        ops.loss_scale_update(torch.zeros(4), 2.0, 0.5, 2000)
    z = [torch.zeros(4)]
    with pytest.raises(_lib.OehError):
        ops.mt_plan(z, z, z, z)
