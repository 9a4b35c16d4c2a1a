"""Host side of the fused optimizer step (include/oeh.h: oeh_mt_plan, oeh_grad_norm, oeh_grad_scale, oeh_adamw_step;
outeffhop_amd/optim.py) without a GPU: the ABI, every refusal, the plan, the update's arithmetic against float64, and FusedAdamW's host logic."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _adamw_ref as R

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "oeh.h")
NEW = ("oeh_mt_plan_bytes", "oeh_mt_plan", "oeh_mt_variant", "oeh_grad_norm_work_bytes", "oeh_grad_norm", "oeh_grad_scale", "oeh_adamw_step")
EINVAL, ENOTSUP, EALIGN = -22, -95, -14
F16, BF16, F32 = 0, 1, 2


def test_header_binding_and_struct_layouts_agree(tmp_path):
    from outeffhop_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(oeh_[a-z0-9_]+)\s*\(", txt))
    assert set(NEW) <= declared and declared == set(_lib.EXPORTS)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW) and lib.oeh_abi_version() == 6
    for name in ("MT_CHUNK", "MT_MAX_GROUPS", "MT_ENTRY_BYTES", "MT_RECORD_BYTES"):
        assert int(re.search(rf"#define OEH_{name} (\d+)", txt).group(1)) == getattr(_lib, name), name
    assert (_lib.MT_CHUNK, _lib.MT_MAX_GROUPS) == (4096, 8)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HDR}"', "int main(void) {"]
    for st in (_lib.oeh_mt_tensor, _lib.oeh_adamw_desc):
        lines.append(f'  printf("{st.__name__}.size %zu\\n", sizeof({st.__name__}));')
        lines += [f'  printf("{st.__name__}.{f} %zu\\n", offsetof({st.__name__}, {f}));' for f, _ in st._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], check=True, capture_output=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for st in (_lib.oeh_mt_tensor, _lib.oeh_adamw_desc):
        assert int(out[f"{st.__name__}.size"]) == C.sizeof(st)
        for f, _ in st._fields_:
            assert int(out[f"{st.__name__}.{f}"]) == getattr(st, f).offset, f


def _tensors(rows):
    """rows: (p, g, m, v, n, g_dtype, group) with integer addresses"""
    from outeffhop_amd import _lib

    arr = (_lib.oeh_mt_tensor * max(len(rows), 1))()
    for a, (p, g, m, v, n, dt, grp) in zip(arr, rows):
        a.p, a.g, a.m, a.v, a.n, a.g_dtype, a.group = p, g, m, v, n, dt, grp
    return arr


BASE = (1 << 20, 2 << 20, 3 << 20, 4 << 20)  # p, g, m, v: 16-byte aligned dummies


def _row(n=100, dt=F32, grp=0, p=BASE[0], g=BASE[1], m=BASE[2], v=BASE[3]):
    return (p, g, m, v, n, dt, grp)


def _plan(rows, with_buffer=True):
    """(rc, n_chunks, entries [(tensor, count, offset)], records [(p, g, m, v, n, g_dtype, group, vec16, 0)])"""
    from outeffhop_amd import _lib

    lib = _lib.load()
    arr = _tensors(rows)
    nb = lib.oeh_mt_plan_bytes(arr, len(rows))
    nch = C.c_int64(-7)
    if nb < 0 or not with_buffer:
        return lib.oeh_mt_plan(arr, len(rows), None, C.byref(nch)), nch.value, None, None
    buf = np.zeros(max(nb // 8, 1), dtype=np.int64)
    rc = lib.oeh_mt_plan(arr, len(rows), C.c_void_p(buf.ctypes.data), C.byref(nch))
    assert nb == nch.value * _lib.MT_ENTRY_BYTES + len(rows) * _lib.MT_RECORD_BYTES
    raw = buf.view(np.uint8)
    ent = raw[:nch.value * 16].view(np.dtype([("tensor", "<i4"), ("count", "<i4"), ("off", "<i8")]))
    rec = raw[nch.value * 16:nb].view(np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("dt", "<i4"), ("grp", "<i4"),
                                               ("vec", "<i4"), ("zero", "<i4")]))
    return rc, nch.value, ent, rec


def test_plan_refusals():
    from outeffhop_amd import _lib

    lib = _lib.load()
    nch = C.c_int64()
    assert lib.oeh_mt_plan(None, 1, None, C.byref(nch)) == EINVAL and lib.oeh_mt_plan(None, -1, None, C.byref(nch)) == EINVAL
    assert lib.oeh_mt_plan(_tensors([_row()]), 1, None, None) == EINVAL
    assert lib.oeh_mt_plan_bytes(None, -1) == -1 and lib.oeh_mt_plan_bytes(None, 1) == -1
    for bad in (_row(n=-1), _row(grp=-1), _row(grp=8), _row(dt=3), _row(dt=-1), _row(dt=7), _row(p=0), _row(g=0), _row(m=0), _row(v=0)):
        assert _plan([_row(), bad])[0] == EINVAL, bad
        assert lib.oeh_mt_plan_bytes(_tensors([bad]), 1) == -1 and lib.oeh_mt_variant(_tensors([bad])) is None
    for name in ("p", "m", "v"):  # fp32: 4 bytes
        for off in (1, 2):
            assert _plan([_row(**{name: BASE[0] + off})])[0] == EALIGN, (name, off)
    assert _plan([_row(g=BASE[1] + 2)])[0] == EALIGN and _plan([_row(g=BASE[1] + 1, dt=F16)])[0] == EALIGN
    assert _plan([_row(g=BASE[1] + 2, dt=F16)])[0] == 0 and _plan([_row(g=BASE[1] + 2, dt=BF16)])[0] == 0
    assert _plan([_row(n=-1, p=BASE[0] + 1)])[0] == EINVAL  # the argument before the alignment
    assert _plan([_row(n=2 ** 43)], with_buffer=False)[0] == ENOTSUP  # 2^31 chunks
    assert lib.oeh_mt_plan(_tensors([_row()]), 1, C.c_void_p(4100), C.byref(nch)) == EALIGN  # the host buffer itself
    assert lib.oeh_mt_variant(None) is None
    # nothing to plan is no refusal
    assert lib.oeh_mt_plan(None, 0, None, C.byref(nch)) == 0 and nch.value == 0 and lib.oeh_mt_plan_bytes(None, 0) == 0


def test_plan_chunks_order_and_int64_offsets():
    sizes = [0, 1, 4095, 4096, 4097, 3 * 4096 + 5]
    want = [0, 1, 1, 1, 2, 4]
    rows = [_row(n=n, grp=i % 8, dt=(F32, F16, BF16)[i % 3], p=BASE[0] + 64 * i) for i, n in enumerate(sizes)]
    rc, nch, ent, rec = _plan(rows)
    assert rc == 0 and nch == sum(want)
    assert [int((ent["tensor"] == i).sum()) for i in range(len(sizes))] == want
    assert list(ent["tensor"]) == sorted(ent["tensor"])  # the tensors in the order given
    for i, n in enumerate(sizes):
        mine = ent[ent["tensor"] == i]
        assert list(mine["off"]) == [4096 * k for k in range(want[i])]
        assert list(mine["count"]) == [min(4096, n - 4096 * k) for k in range(want[i])] and int(mine["count"].sum()) == n
        assert (rec[i]["p"], rec[i]["n"], rec[i]["dt"], rec[i]["grp"], rec[i]["zero"]) == (BASE[0] + 64 * i, n, (F32, F16, BF16)[i % 3], i % 8, 0)
        assert (rec[i]["g"], rec[i]["m"], rec[i]["v"]) == BASE[1:]
    for n, c in zip(sizes, want):
        assert _plan([_row(n=n)], with_buffer=False)[1] == c
    # 2^33 elements: planned, never allocated; the offsets do not wrap at 2^31 or 2^32
    assert _plan([_row(n=2 ** 33)], with_buffer=False)[:2] == (0, 2 ** 21)
    rc, nch, ent, rec = _plan([_row(n=5), _row(n=2 ** 33 + 3), _row(n=1)])
    assert rc == 0 and nch == 1 + 2 ** 21 + 1 + 1
    big = ent[ent["tensor"] == 1]
    assert np.array_equal(big["off"], np.arange(2 ** 21 + 1, dtype=np.int64) * 4096) and int(big["off"][-1]) == 2 ** 33
    assert int(big["count"][-1]) == 3 and (big["count"][:-1] == 4096).all() and rec[1]["n"] == 2 ** 33 + 3
    assert ent[-1]["tensor"] == 2 and ent[0]["tensor"] == 0


def test_variant_follows_each_pointer():
    from outeffhop_amd import _lib

    lib = _lib.load()
    name = lambda **kw: lib.oeh_mt_variant(_tensors([_row(**kw)])).decode()  # noqa: E731
    for dt, eb in ((F32, 4), (F16, 2), (BF16, 2)):
        assert name(dt=dt) == "vec16"
        assert name(dt=dt, p=BASE[0] + 4) == "elem" and name(dt=dt, m=BASE[2] + 4) == "elem" and name(dt=dt, v=BASE[3] + 4) == "elem"
        assert name(dt=dt, g=BASE[1] + eb) == "elem"  # one element off
        assert name(dt=dt, g=BASE[1] + 8) == ("vec16" if eb == 2 else "elem")  # 8 bytes serve a 16-bit g where p needs 16
        assert name(dt=dt, g=BASE[1] + 16) == "vec16"
        rec = _plan([_row(dt=dt, g=BASE[1] + eb), _row(dt=dt)])[3]
        assert list(rec["vec"]) == [0, 1]


def _desc(n_groups=1, **kw):
    from outeffhop_amd import _lib

    d = _lib.oeh_adamw_desc()
    d.n_groups = n_groups
    for i in range(8):
        d.lr[i], d.beta1[i], d.beta2[i], d.eps[i], d.weight_decay[i], d.step[i] = 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1
    for k, (i, val) in kw.items():
        getattr(d, k)[i] = val
    return d


def test_step_norm_and_scale_refusals_without_gpu():
    from outeffhop_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(4096)
    step = lambda d, plan=one, n=0, clip=None: lib.oeh_adamw_step(plan, n, None if d is None else C.byref(d), clip, None)  # noqa: E731
    assert step(None) == EINVAL
    for ng in (0, -1, 9):
        assert step(_desc(ng)) == EINVAL
    d = _desc()
    d.reserved = 1
    assert step(d) == EINVAL
    nan = float("nan")
    for field, vals in (("step", (0, -3)), ("lr", (-1e-3, nan)), ("eps", (-1e-8, nan)), ("weight_decay", (-0.1, nan)),
                        ("beta1", (-0.1, 1.0, 1.5, nan)), ("beta2", (-0.1, 1.0, 1.5, nan))):
        for val in vals:
            assert step(_desc(1, **{field: (0, val)})) == EINVAL, (field, val)
            assert step(_desc(3, **{field: (2, val)})) == EINVAL, (field, val)
            assert step(_desc(2, **{field: (2, val)})) == 0  # a column that is not in use is not looked at
    assert step(_desc(), plan=None, n=1) == EINVAL and step(_desc(), n=-1) == EINVAL and step(_desc(), n=2 ** 31) == ENOTSUP
    assert step(_desc(), clip=C.c_void_p(4100)) == EALIGN
    # nothing to do: no launch, no device needed - with and without a plan, with every edge of the hyper-parameters that is allowed
    assert step(_desc()) == 0 and step(_desc(), plan=None) == 0 and step(_desc(8), clip=one) == 0
    assert step(_desc(1, lr=(0, 0.0), eps=(0, 0.0), weight_decay=(0, 0.0), beta1=(0, 0.0), beta2=(0, 0.0))) == 0
    # the norm
    norm = lambda plan=one, n=1, work=one, out=one: lib.oeh_grad_norm(plan, n, 1.0, work, out, None)  # noqa: E731
    assert norm(out=None) == EINVAL and norm(work=None) == EINVAL and norm(plan=None) == EINVAL and norm(n=-1) == EINVAL
    assert norm(n=2 ** 31) == ENOTSUP and norm(work=C.c_void_p(4100)) == EALIGN and norm(out=C.c_void_p(4100)) == EALIGN
    assert lib.oeh_grad_norm_work_bytes(0) == 0 and lib.oeh_grad_norm_work_bytes(5) == 40 and lib.oeh_grad_norm_work_bytes(-1) == 0
    # the stand-alone clip
    scale = lambda plan=one, n=1, clip=one: lib.oeh_grad_scale(plan, n, clip, None)  # noqa: E731
    assert scale(clip=None) == EINVAL and scale(plan=None) == EINVAL and scale(n=-1) == EINVAL and scale(n=2 ** 31) == ENOTSUP
    assert scale(clip=C.c_void_p(4100)) == EALIGN and scale(n=0) == 0 and scale(plan=None, n=0) == 0


HYPERS = [(1e-3, 0.9, 0.999, 1e-8, 1e-2), (6e-4, 0.9, 0.95, 1e-8, 0.1), (5e-5, 0.9, 0.95, 1e-6, 0.0), (1e-2, 0.8, 0.999, 1e-8, 1e-2)]


def test_restatement_against_float64_within_the_counted_roundings():
    """Measured here (worst ratio to the bound over 4 x 6 x 7 x 5 states of 4096 elements): m' 0.205, v' 0.326, p' 0.776."""
    rng = np.random.default_rng(20261020)
    worst = np.zeros(3)
    for hyper in HYPERS:
        for t in (1, 2, 3, 10, 1000, 2000):
            for gscale in (1e-6, 1e-4, 1e-2, 0.3, 1.0, 7.0, 30.0):
                for c in (1e-3, 0.0625, 0.7, 1.0, 3.1):
                    p, g, m, v = R.random_state(rng, 4096, gscale, first=(t == 1))
                    if c != 1.0:  # the cancellation stretch follows the coefficient
                        m[:1024] = (g[:1024] * np.float32(c)) * (1 + rng.integers(-3, 4, 1024) * 2.0 ** -23).astype(np.float32)
                        m = m if t > 1 else np.zeros_like(m)
                    worst = np.maximum(worst, R.bound_ratios(p, g, m, v, np.float32(c), hyper + (t,)))
    print(f"worst |fp32 - float64| / bound: m' {worst[0]:.3f}  v' {worst[1]:.3f}  p' {worst[2]:.3f}")
    assert (worst <= 1.0).all(), worst
    assert worst.min() > 0.05  # the bounds are not vacuous: the worst case uses a fair share of each


def test_restatement_constants_and_edges():
    d, k1, b2, k2, bc2, eps, ss = R.constants32(1e-3, 0.9, 0.999, 1e-8, 1e-2, 1)
    assert all(x.dtype == np.float32 for x in (d, k1, b2, k2, bc2, eps, ss))
    lr, b1, b2f = float(np.float32(1e-3)), float(np.float32(0.9)), float(np.float32(0.999))
    assert ss == np.float32(lr / (1.0 - b1)) and bc2 == np.float32((1.0 - b2f) ** 0.5) and d == np.float32(1.0 - lr * float(np.float32(1e-2)))
    # weight_decay 0 leaves p1 = p; a zero state and c = 1 give m' = g k, v' = g^2 k2 in two roundings each
    p, g, m, v = R.random_state(np.random.default_rng(1), 64, 1.0, first=True)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1)
    pn, mn, vn = R.step32(p, g, m, v, np.float32(1.0), hyper)
    assert np.array_equal(mn, g * R.constants32(*hyper)[1]) and np.array_equal(vn, (g * g) * R.constants32(*hyper)[3])
    assert R.constants32(*hyper)[0] == 1.0
    # lr 0: nothing moves but the moments
    pn, mn, vn = R.step32(p, g, m, v, np.float32(1.0), (0.0, 0.9, 0.999, 1e-8, 0.3, 5))
    assert np.array_equal(pn, p) and not np.array_equal(mn, m)


# ---- FusedAdamW's host side
def _params(*shapes, device="cpu"):
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(*s, generator=g).to(device)) for s in shapes]


def test_fused_adamw_construction_and_refusals():
    import outeffhop_amd as oa
    from outeffhop_amd import optim

    assert oa.FusedAdamW is optim.FusedAdamW and oa.clip_grad_norm_ is optim.clip_grad_norm_
    ps = _params((4, 3), (5,))
    o = oa.FusedAdamW(ps)
    g = o.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"]) == (1e-3, (0.9, 0.999), 1e-8, 1e-2, False)
    assert o.max_grad_norm is None and o.grad_norm is None and len(o.state) == 0  # state is made at the first step
    assert set(g) == set(torch.optim.AdamW(ps).param_groups[0])
    o = oa.FusedAdamW([{"params": ps[:1], "weight_decay": 0.1}, {"params": ps[1:], "weight_decay": 0.0}], lr=6e-4, betas=(0.9, 0.95), max_grad_norm=1.0)
    assert [g["weight_decay"] for g in o.param_groups] == [0.1, 0.0] and o.max_grad_norm == 1.0
    with pytest.raises(ValueError):
        oa.FusedAdamW(ps, amsgrad=True)
    with pytest.raises(TypeError):
        oa.FusedAdamW(ps, lr=torch.tensor(1e-3))
    for kw in ({"lr": -1.0}, {"eps": -1e-8}, {"betas": (1.0, 0.9)}, {"betas": (0.9, -0.1)}, {"weight_decay": -0.1}, {"max_grad_norm": float("nan")}):
        with pytest.raises(ValueError):
            oa.FusedAdamW(ps, **kw)
    with pytest.raises(TypeError):
        oa.FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    with pytest.raises(ValueError):
        oa.FusedAdamW([torch.nn.Parameter(torch.zeros(4, 6).t())])  # not contiguous
    o = oa.FusedAdamW(ps[:1])
    with pytest.raises(TypeError):
        o.add_param_group({"params": [torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))]})
    with pytest.raises(ValueError):
        o.add_param_group({"params": ps[1:], "amsgrad": True})


def test_fused_adamw_step_without_gpu():
    import outeffhop_amd as oa
    from outeffhop_amd import _lib

    ps = _params((4, 3), (5,))
    o = oa.FusedAdamW(ps, max_grad_norm=1.0)
    assert o.step() is None  # no gradient anywhere: nothing to do, as in torch
    assert o.step(lambda: torch.tensor(2.5)) == 2.5  # a closure is honoured
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(_lib.OehError):
        o.step()
    assert len(o.state) == 0
    ps[0].grad = torch.ones(4, 6)[:, ::2]
    with pytest.raises(ValueError):
        o.step()
    ps[0].grad_dtype = None  # (torch otherwise holds a gradient to its parameter's dtype)
    ps[0].grad = torch.ones(4, 3, dtype=torch.float64)
    with pytest.raises(TypeError):
        o.step()
    e = torch.nn.Embedding(4, 3, sparse=True)
    e(torch.tensor([1])).sum().backward()
    with pytest.raises(ValueError):
        oa.FusedAdamW(e.parameters()).step()
    o = oa.FusedAdamW(_params((3,)))
    o.param_groups[0]["lr"] = torch.tensor(1e-3)  # a tensor lr written in later is seen at the step
    with pytest.raises(TypeError):
        o.step()


def test_state_dict_travels_to_torch_adamw_and_back():
    import outeffhop_amd as oa

    ps = _params((4, 3), (5,))
    groups = lambda: [{"params": ps[:1], "weight_decay": 0.1}, {"params": ps[1:], "weight_decay": 0.0}]  # noqa: E731
    t = torch.optim.AdamW(groups(), lr=6e-4, betas=(0.9, 0.95))
    for p in ps:
        p.grad = torch.ones_like(p)
    t.step()
    t.step()
    o = oa.FusedAdamW(groups(), lr=1.0)
    o.load_state_dict(t.state_dict())
    sd = o.state_dict()
    assert [g["lr"] for g in sd["param_groups"]] == [6e-4, 6e-4] and [g["betas"] for g in sd["param_groups"]] == [(0.9, 0.95)] * 2
    for i, p in enumerate(ps):
        st = o.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 2.0
        assert torch.equal(st["exp_avg"], t.state[p]["exp_avg"]) and torch.equal(st["exp_avg_sq"], t.state[p]["exp_avg_sq"])
    t2 = torch.optim.AdamW(groups(), lr=1.0)
    t2.load_state_dict(sd)
    before = [p.detach().clone() for p in ps]
    t2.step()
    assert all(float(t2.state[p]["step"]) == 3.0 for p in ps) and not torch.equal(before[0], ps[0])
    assert t2.param_groups[1]["weight_decay"] == 0.0 and t2.param_groups[0]["lr"] == 6e-4


def test_clip_grad_norm_on_cpu_is_torchs():
    from outeffhop_amd import optim

    a, b = _params((4, 3), (5,)), _params((4, 3), (5,))
    for x, y in zip(a, b):
        x.grad = torch.full_like(x, 0.75)
        y.grad = torch.full_like(y, 0.75)
    n1 = optim.clip_grad_norm_(a, 0.5)
    n2 = torch.nn.utils.clip_grad_norm_(b, 0.5)
    assert torch.equal(n1, n2) and all(torch.equal(x.grad, y.grad) for x, y in zip(a, b))
    assert torch.equal(optim.clip_grad_norm_(a[0], 1.0, norm_type=float("inf")), torch.nn.utils.clip_grad_norm_(b[0], 1.0, norm_type=float("inf")))
    assert float(optim.clip_grad_norm_([torch.nn.Parameter(torch.zeros(2))], 1.0)) == 0.0  # no gradient at all
