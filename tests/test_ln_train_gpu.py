"""Every launch branch of the training block tail (csrc/oeh_ln_train.hip; include/oeh.h: oeh_drop_resid_ln_fwd / oeh_drop_resid_ln_bwd) at
the smallest shape that reaches it, and the autograd function and modules on top (outeffhop_amd/layers.py).  `-m gpu`.

Yardsticks.  Exact: the keep mask against the numpy restatement of Philox (tests/_ln_train_ref.py); the stored sum against the torch
expression (where(keep, x.float() * inv32, 0) + r.float()).to(dtype) on the GPU with the kernel's own mask; with p == 0, sum and y against
ops.resid_ln_quant without quantisers; dropped positions of dx are exactly zero; two calls, and each documented alias, give the same bits.
Against float64: y, dx, dr, dgamma, dbeta are compared with a float64 evaluation on the stored sum and the same mask, with the distance
of CPU fp32 torch (F.layer_norm and its autograd on that sum, the mask and 1 / (1 - p) applied behind it) from float64 on the same call
(err64, per output) as the unit:  |value - f64| <= 4 err64  (+ half an ulp of a 16-bit storage type for y, dx, dr).  The factor 4 is the
project's (tests/test_ln_gpu.py): a different summation tree and the two extra roundings of rstd.  With dsum, dr is checked against
float64's ds + dsum, and in fp32 - where RN is the identity - dr - (dr of the call without dsum) against dsum, both by the same rule.
In 16-bit storage that difference is one of two stored values, so it gets half an ulp of the storage type at each of them on top of 4 err64.
mean and rstd by the same rule, no ulp term: their CPU fp32 side is torch.native_layer_norm - what F.layer_norm runs -, which returns the
two statistics next to y.  The measured ratios are printed (-s).

mean, rstd, dgamma and dbeta: the kernels form them in float64 - the backward with row statistics it forms again for its two column sums -
and round once, so each value is the fp32 number next to float64's and no fp32 evaluation can be nearer: their ratio is at most 1 whatever
the CPU's rounding happens to be in a call of one or three rows (a single mean; an entry of dgamma that is one product).  
Worst ratios measured on an MI355X: y 3.65, dx 1.37, dr 1.45, dr - dr0 1.60, mean 1.00, rstd 1.00, dgamma 1.00, dbeta 1.00.

Launch forms (oeh_ln_row.h: ln_plan; VEC = 4 fp32 / 8 16-bit elements): cols 8, 72, 768, 1024 one wave per row; 1032, 2048, 8192 one
workgroup per row; 1, 770, a row stride that is no multiple of VEC and a base pointer one element off a 16-byte boundary element accesses.
The backward's slab loop (ops.drop_resid_ln_variant(..., backward=True) ends in G<workgroups>x<rows per slab>): one workgroup; several
workgroups of one row-step each; more rows than the grid bound takes in one step, with a ragged last slab; and the workgroup counts
around the column kernel's 32 slices (test_column_kernel_slice_split).
The column list reaches the first and the last CH of each 16-byte form and CH = 1 and 4 with elements (CH = 16 through the stride tests at
1032 columns), every one with p = 0.1 - not fp32 wave CH = 2, not the workgroup form's middle CH, not CH = 32 with elements, and the backward
without dropout at 72 columns only (39 of the forward's 56 instances and 22 of the backward's in a kernel trace).
tests/test_ln_instances_gpu.py runs every compiled instance of both row kernels, with and without dropout, at both ends of its range, from
the registry of tests/_ln_inst.py."""
import re

import numpy as np
import pytest

from tests import _ln_ref as R
from tests import _ln_train_ref as T

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
F = torch.nn.functional

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
COLS = (1, 8, 72, 768, 770, 1024, 1032, 2048, 8192)
ROWS = (1, 3, 5, 64)
EPS = 1e-5
P = 0.1
KEYS = ("y", "mean", "rstd", "dx", "dr", "dgamma", "dbeta")


@pytest.fixture(autouse=True)
def _fused_on():
    """The fused path, whatever the default of layers.FUSED_LN_TRAIN is."""
    from outeffhop_amd import layers

    prev = layers.set_fused_ln_train(True)
    yield
    layers.set_fused_ln_train(prev)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _f64(t):
    return t.detach().cpu().float().numpy().astype(np.float64)


def _name(dtype):
    return str(dtype).split(".")[-1]


def _inputs(rows, cols, dtype, seed, device="cuda"):
    """x, r ~ N(0, 1) with the x40 and x-25 outlier channels of tests/test_ln_gpu.py (where the row has them), gamma around 1, beta around
    0, and the two incoming gradients dy, dsum ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    r = torch.randn(rows, cols, generator=g)
    if cols >= 8:
        x[:, 3] *= 40.0
        x[:, cols - 2] *= -25.0
    gamma = 1.0 + 0.25 * torch.randn(cols, generator=g)
    beta = 0.1 * torch.randn(cols, generator=g)
    dy = torch.randn(rows, cols, generator=g)
    dsum = torch.randn(rows, cols, generator=g)
    return tuple(t.to(device) for t in (x.to(dtype), r.to(dtype), gamma, beta, dy.to(dtype), dsum.to(dtype)))


def _reference(s, gamma, beta, dy, dsum, keep, inv, eps=EPS):
    """name -> (float64 value, err64 = max distance of CPU fp32 torch from it) on the stored sum s; "ds32": CPU fp32's ds without dsum."""
    s32 = s.detach().cpu().float().requires_grad_()
    if beta is None:  # (y + 0 is y in every evaluation; dbeta does not depend on beta)
        beta = torch.zeros_like(gamma)
    g32, b32 = gamma.detach().cpu().float().requires_grad_(), beta.detach().cpu().float().requires_grad_()
    dy32 = dy.detach().cpu().float()
    y32, mean32, rstd32 = torch.native_layer_norm(s32, (s32.shape[-1],), g32, b32, eps)  # F.layer_norm, with its two statistics
    (y32 * dy32).sum().backward()
    ds32 = s32.grad if dsum is None else s32.grad + dsum.detach().cpu().float()
    keep_c = torch.from_numpy(keep)
    dx32 = torch.where(keep_c, ds32 * torch.tensor(np.float32(inv)), torch.zeros(()))
    got32 = dict(y=y32, mean=mean32.reshape(-1), rstd=rstd32.reshape(-1), dx=dx32, dr=ds32, dgamma=g32.grad, dbeta=b32.grad)
    sn, gn, bn = s32.detach().numpy(), g32.detach().numpy(), b32.detach().numpy()
    mean64, rstd64 = T.stats64(sn, eps)
    dx64, dr64, dg64, db64 = T.backward64(dy32.numpy(), sn, gn, eps, keep, inv, None if dsum is None else dsum.detach().cpu().float().numpy())
    want = dict(y=T.forward64(sn, gn, bn, eps), mean=mean64, rstd=rstd64, dx=dx64, dr=dr64, dgamma=dg64, dbeta=db64)
    out = {k: (want[k], float(np.abs(got32[k].detach().numpy().astype(np.float64) - want[k]).max())) for k in want}
    out["ds32"] = s32.grad
    return out


def _check_case(ops, x, r, gamma, beta, dy, dsum, p, seed, label, want_dr=True, want_dbeta=True):
    """One forward and one backward call on the given tensors (any views), checked against every yardstick.  Returns name -> ratio.  r, beta
    and dsum may be None; without want_dr / want_dbeta the backward returns None for that output and the others are checked."""
    dtype, (rows, cols) = x.dtype, x.shape
    s, y, mean, rstd = ops.drop_resid_ln_fwd(x, r, gamma, beta, EPS, p=p, seed=seed)
    assert s.shape == x.shape and y.shape == x.shape and s.dtype == dtype and y.dtype == dtype and mean.shape == (rows,) and rstd.dtype == torch.float32
    keep_t = ops.drop_resid_ln_mask(rows, cols, p, seed, x.device)
    keep = keep_t.cpu().numpy()
    assert np.array_equal(keep, T.keep_mask(rows, cols, p, seed)), f"{label}: the mask differs from the numpy restatement"
    inv = T.inv_keep(p)
    d = torch.where(keep_t, x.float() * torch.tensor(inv, device=x.device), torch.zeros((), device=x.device))
    s_want = (d if r is None else d + r.float()).to(dtype)
    assert np.array_equal(_bits(s), _bits(s_want)), f"{label}: the sum differs from the torch expression"
    dx, dr, dgamma, dbeta = ops.drop_resid_ln_bwd(dy, s, gamma, mean, rstd, dsum=dsum, p=p, seed=seed, want_dr=want_dr, want_dbeta=want_dbeta)
    assert dx.dtype == dtype and dgamma.dtype == torch.float32 and dgamma.shape == (cols,)
    assert (dr.dtype == dtype and dr.shape == x.shape) if want_dr else dr is None
    assert (dbeta.dtype == torch.float32 and dbeta.shape == (cols,)) if want_dbeta else dbeta is None
    assert not _f64(dx)[~keep].any(), f"{label}: a dropped position of dx is not zero"
    ref = _reference(s, gamma, beta, dy, dsum, keep, inv)
    got = dict(y=y, mean=mean, rstd=rstd, dx=dx, dr=dr, dgamma=dgamma, dbeta=dbeta)
    ratios = {}
    for k in KEYS:
        if got[k] is None:
            continue
        stored = _name(dtype) if k in ("y", "dx", "dr") else "float32"
        try:
            ratios[k] = R.check_values(_f64(got[k]), *ref[k], stored)
        except AssertionError as e:
            raise AssertionError(f"{label} {k}: {e}") from None
    if dsum is not None and want_dr:
        _, dr0, _, _ = ops.drop_resid_ln_bwd(dy, s, gamma, mean, rstd, p=p, seed=seed)
        ds32 = ref["ds32"]  # CPU fp32: one add, then the exact difference
        err = float(np.abs(((ds32 + dsum.cpu().float()).double() - ds32.double()).numpy() - _f64(dsum)).max())
        diff = np.abs((_f64(dr) - _f64(dr0)) - _f64(dsum))
        if dtype != torch.float32:  # two stored values: half an ulp of the storage type at each
            dr64 = ref["dr"][0]
            diff = np.maximum(diff - 0.5 * R.ulp_of(np.abs(dr64) + 4.0 * err, _name(dtype)) - 0.5 * R.ulp_of(np.abs(dr64 - _f64(dsum)) + 4.0 * err, _name(dtype)), 0.0)
        assert (diff <= 4.0 * err).all(), f"{label} dr - dr0: {int((diff > 4.0 * err).sum())} values beyond 4 x err64 = {4.0 * err:.3e}: {diff.max():.3e}"
        ratios["dr-dr0"] = float(diff.max() / err) if err > 0 else 0.0
    return ratios


def _merge(worst, ratios):
    for k, v in ratios.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _show(title, worst):
    print(f"\n{title}: max |value - f64| / err64 (limit 4): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cols", COLS)
def test_every_form_and_row_count(ops, cols, dt):
    dtype = DTYPES[dt]
    worst = {}
    for rows in ROWS:
        x, r, gamma, beta, dy, dsum = _inputs(rows, cols, dtype, 9100 + 7 * cols + rows)
        with_dsum = rows in (3, 64)
        _merge(worst, _check_case(ops, x, r, gamma, beta, dy, dsum if with_dsum else None, P, 1000 * cols + rows, f"{rows}x{cols} {dt}"))
    _show(f"{ops.drop_resid_ln_variant(64, cols, dtype, p=P)} | {ops.drop_resid_ln_variant(64, cols, dtype, backward=True, p=P)} cols {cols} {dt}", worst)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cols", (8, 1032))
def test_backward_slab_loop(ops, cols, dt):
    """Row counts read from the plan: one workgroup; several workgroups of one row-step each; more rows than the grid bound takes in one
    step (every slab several rows, the last one ragged)."""
    from outeffhop_amd import _lib

    dtype = DTYPES[dt]
    per_step = 4 if cols <= 1024 else 1  # rows a workgroup takes in one step: a wave each in the wave form
    bound = _lib.LN_TRAIN_MAX_GROUPS * per_step
    worst = {}
    for kind, rows in (("one", per_step - 1 if per_step > 1 else 1), ("steps", 3 * per_step), ("slabs", 2 * bound + (4 if per_step > 1 else 3))):
        name = ops.drop_resid_ln_variant(rows, cols, dtype, backward=True, p=P)
        wgs, per_slab = (int(v) for v in re.search(r"/G(\d+)x(\d+)$", name).groups())
        if kind == "one":
            assert (wgs, per_slab) == (1, 1)
        elif kind == "steps":
            assert wgs == 3 and per_slab == 1
        else:
            assert per_slab == 3 and rows % per_slab != 0 and wgs <= _lib.LN_TRAIN_MAX_GROUPS and wgs * per_step * per_slab >= rows
        x, r, gamma, beta, dy, dsum = _inputs(rows, cols, dtype, 9300 + cols + rows)
        _merge(worst, _check_case(ops, x, r, gamma, beta, dy, dsum, P, 77 + rows, f"{rows}x{cols} {dt} {name}"))
    _show(f"slab loop cols {cols} {dt}", worst)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cols", (8, 1032))
def test_column_kernel_slice_split(ops, cols, dt):
    """The column kernel cuts the list of workgroup partials into 32 slices of ceil(workgroups / 32): 2 and 31 partials (slices of one, the
    rest empty), 32 (every slice one), 33 (slices of two: slice 16 holds one partial, 17 .. 31 none), 64 and 65.  The counts are read back
    from the plan's name; the wave form's last workgroup has one row and three waves that add nothing.  dgamma and dbeta against float64
    by the rule of `_check_case`, with dbeta and without."""
    dtype = DTYPES[dt]
    per_step = 4 if cols <= 1024 else 1
    worst = {}
    for wgs in (2, 31, 32, 33, 64, 65):
        rows = per_step * (wgs - 1) + 1
        name = ops.drop_resid_ln_variant(rows, cols, dtype, backward=True, p=P)
        assert tuple(int(v) for v in re.search(r"/G(\d+)x(\d+)$", name).groups()) == (wgs, 1), name
        x, r, gamma, beta, dy, dsum = _inputs(rows, cols, dtype, 9400 + cols + rows)
        for want_dbeta in (True, False):
            _merge(worst, _check_case(ops, x, r, gamma, beta, dy, dsum if wgs % 2 else None, P, 55 + rows, f"{rows}x{cols} {dt} {name}", want_dbeta=want_dbeta))
    _show(f"column kernel slices cols {cols} {dt}", worst)


def _mask_through_forward(ops, rows, cols, dtype, p, seed, how):
    """The mask as the forward applies it in the launch form `how` reaches: x = 1, no residual, so the sum is inv where kept and 0 where dropped."""
    w = torch.ones(cols, device="cuda")
    if how == "aligned":
        x = torch.ones(rows, cols, dtype=dtype, device="cuda")
    elif how == "stride":  # a row stride that is no multiple of the 16-byte vector
        x = torch.ones(rows, cols + 1, dtype=dtype, device="cuda")[:, :cols]
    else:  # a base pointer one element off a 16-byte boundary
        x = torch.ones(rows * cols + 1, dtype=dtype, device="cuda")[1:].view(rows, cols)
    s, _, _, _ = ops.drop_resid_ln_fwd(x, None, w, None, EPS, p=p, seed=seed)
    return (s != 0).cpu().numpy()


@pytest.mark.parametrize("dt", list(DTYPES))
def test_mask_is_the_generators_in_every_form(ops, dt):
    dtype = DTYPES[dt]
    seed, rows = 0xC0FFEE1234567, 37
    for cols in (72, 1032):  # one wave per row / one workgroup per row when aligned
        want = T.keep_mask(rows, cols, 0.25, seed)
        assert np.array_equal(ops.drop_resid_ln_mask(rows, cols, 0.25, seed, "cuda").cpu().numpy(), want)
        for how in ("aligned", "stride", "offset"):
            assert np.array_equal(_mask_through_forward(ops, rows, cols, dtype, 0.25, seed, how), want), (cols, how)


def test_mask_rate_and_seeds(ops):
    rows, cols = 64, 1032
    n = rows * cols
    for p in (0.1, 0.5):
        share = float(ops.drop_resid_ln_mask(rows, cols, p, 123456789, "cuda").float().mean())
        assert abs(share - (1.0 - p)) <= 5.0 * np.sqrt(p * (1.0 - p) / n), (p, share)
    a = ops.drop_resid_ln_mask(rows, cols, 0.5, 1, "cuda")
    b = ops.drop_resid_ln_mask(rows, cols, 0.5, 2, "cuda")
    c = ops.drop_resid_ln_mask(rows, cols, 0.5, 1 << 32, "cuda")  # the key's second word
    assert not torch.equal(a, b) and not torch.equal(a, c) and torch.equal(a, ops.drop_resid_ln_mask(rows, cols, 0.5, 1, "cuda"))
    assert bool(ops.drop_resid_ln_mask(5, 9, 0.0, 7, "cuda").all())


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cols", COLS)
def test_without_dropout_it_is_the_inference_kernel(ops, cols, dt):
    dtype = DTYPES[dt]
    x, r, gamma, beta, _, _ = _inputs(5, cols, dtype, 9500 + cols)
    s0, y0 = ops.resid_ln_quant(x, r, gamma, beta, EPS, want_sum=True)
    s, y, _, _ = ops.drop_resid_ln_fwd(x, r, gamma, beta, EPS)
    assert np.array_equal(_bits(s), _bits(s0)) and np.array_equal(_bits(y), _bits(y0))
    y1 = ops.resid_ln_quant(x, None, gamma, None, EPS)
    s2, y2, _, _ = ops.drop_resid_ln_fwd(x, None, gamma, None, EPS)
    assert np.array_equal(_bits(s2), _bits(x)) and np.array_equal(_bits(y2), _bits(y1))


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("cols", (72, 770, 1032))
def test_reproducible_and_aliases(ops, cols, dt):
    dtype = DTYPES[dt]
    x, r, gamma, beta, dy, dsum = _inputs(9, cols, dtype, 9700 + cols)
    seed = 424242
    s, y, mean, rstd = ops.drop_resid_ln_fwd(x, r, gamma, beta, EPS, p=P, seed=seed)
    ra, xa = r.clone(), x.clone()
    s2, y2, mean2, rstd2 = ops.drop_resid_ln_fwd(xa, ra, gamma, beta, EPS, p=P, seed=seed, sum_out=ra, out=xa)  # sum_out is r, y is x
    assert s2 is ra and y2 is xa
    for a, b in ((s, s2), (y, y2), (mean, mean2), (rstd, rstd2)):
        assert np.array_equal(_bits(a), _bits(b))
    first = ops.drop_resid_ln_bwd(dy, s, gamma, mean, rstd, dsum=dsum, p=P, seed=seed)
    again = ops.drop_resid_ln_bwd(dy, s, gamma, mean, rstd, dsum=dsum, p=P, seed=seed)
    dya, dsa = dy.clone(), dsum.clone()
    alias = ops.drop_resid_ln_bwd(dya, s, gamma, mean, rstd, dsum=dsa, p=P, seed=seed, dx=dya, dr=dsa)  # dx is dy, dr is dsum
    assert alias[0] is dya and alias[1] is dsa
    for other in (again, alias):
        for a, b in zip(first, other):
            assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("cols", (72, 1032))
def test_strided_rows_and_unaligned_base(ops, cols, dt):
    dtype = DTYPES[dt]
    rows = 6
    x, r, gamma, beta, dy, dsum = _inputs(rows, cols, dtype, 9900 + cols)
    worst = {}
    for pad in (16, 1):  # a row stride above cols: still a multiple of the vector / no multiple of it (element accesses)
        wide = lambda t: torch.cat([t, torch.full((rows, pad), 7.0, dtype=dtype, device="cuda")], dim=1)[:, :cols]  # noqa: E731
        _merge(worst, _check_case(ops, wide(x), wide(r), gamma, beta, wide(dy), wide(dsum), P, 5 + pad, f"{rows}x{cols} {dt} stride +{pad}"))
    off = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(rows, cols)  # noqa: E731
    assert off(x).data_ptr() % 16 != 0
    _merge(worst, _check_case(ops, off(x), off(r), gamma, beta, off(dy), off(dsum), P, 99, f"{rows}x{cols} {dt} base + 1 element"))
    _show(f"strided / unaligned cols {cols} {dt}", worst)


# ---- autograd and modules (outeffhop_amd/layers.py)
@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_autograd_with_both_outputs_in_the_loss(ops, dt):
    from outeffhop_amd import layers as L

    dtype = DTYPES[dt]
    rows, cols, seed = 10, 72, 31337
    x, r, gamma, beta, wy, ws = _inputs(rows, cols, dtype, 8800)
    x3, r3 = x.view(2, 5, cols).requires_grad_(), r.view(2, 5, cols).requires_grad_()
    gamma, beta = gamma.requires_grad_(), beta.requires_grad_()
    before = dict(L.CALLS)
    s, y = L.dropout_add_layer_norm(x3, r3, gamma, beta, p=P, eps=EPS, want_sum=True, dropout_seed=seed)
    assert s.shape == x3.shape and y.requires_grad and s.requires_grad
    ((y.float() * wy.view_as(y).float()).sum() + (s.float() * ws.view_as(s).float()).sum()).backward()
    assert L.CALLS["forward"] == before["forward"] + 1 and L.CALLS["backward"] == before["backward"] + 1 and L.CALLS["torch"] == before["torch"]
    keep = ops.drop_resid_ln_mask(rows, cols, P, seed, "cuda").cpu().numpy()
    assert np.array_equal(keep, T.keep_mask(rows, cols, P, seed))
    ref = _reference(s.detach().view(rows, cols), gamma, beta, wy, ws, keep, T.inv_keep(P))
    got = dict(y=y.view(rows, cols), dx=x3.grad.view(rows, cols), dr=r3.grad.view(rows, cols), dgamma=gamma.grad, dbeta=beta.grad)
    assert gamma.grad.dtype == gamma.dtype and x3.grad.dtype == dtype
    ratios = {k: R.check_values(_f64(v), ref[k][0], ref[k][1], _name(dtype) if k in ("y", "dx", "dr") else "float32") for k, v in got.items()}
    assert not _f64(got["dx"])[~keep].any()
    _show(f"dropout_add_layer_norm want_sum {dt}", ratios)
    # the same seed gives the same result; without want_sum the sum carries no gradient
    s2, y2 = L.dropout_add_layer_norm(x3.detach(), r3.detach(), gamma.detach(), beta.detach(), p=P, eps=EPS, want_sum=True, dropout_seed=seed)
    assert np.array_equal(_bits(s2), _bits(s)) and np.array_equal(_bits(y2), _bits(y))
    xg = x3.detach().clone().requires_grad_()
    y3 = L.dropout_add_layer_norm(xg, r3.detach(), gamma.detach(), beta.detach(), p=P, eps=EPS, dropout_seed=seed)
    (y3.float() * wy.view_as(y3).float()).sum().backward()
    ref3 = _reference(s.detach().view(rows, cols), gamma, beta, wy, None, keep, T.inv_keep(P))
    R.check_values(_f64(xg.grad.view(rows, cols)), ref3["dx"][0], ref3["dx"][1], _name(dtype))
    # parameters of another dtype get their gradients in it
    gh, bh = gamma.detach().to(dtype).requires_grad_(), beta.detach().to(dtype).requires_grad_()
    L.dropout_add_layer_norm(x3.detach(), None, gh, bh, p=0.0, eps=EPS).float().sum().backward()
    assert gh.grad.dtype == dtype and bh.grad.dtype == dtype and gh.grad.shape == gh.shape


def test_manual_seed_reproduces_a_drawn_seed_and_the_switch(ops):
    from outeffhop_amd import layers as L

    x, r, gamma, beta, _, _ = _inputs(8, 72, torch.float16, 8900)
    torch.manual_seed(11)
    a = L.dropout_add_layer_norm(x, r, gamma, beta, p=0.5)
    b = L.dropout_add_layer_norm(x, r, gamma, beta, p=0.5)
    torch.manual_seed(11)
    c = L.dropout_add_layer_norm(x, r, gamma, beta, p=0.5)
    assert np.array_equal(_bits(a), _bits(c)) and not np.array_equal(_bits(a), _bits(b))
    e = L.dropout_add_layer_norm(x, r, gamma, beta, p=0.5, training=False)
    assert np.array_equal(_bits(e), _bits(ops.resid_ln_quant(x, r, gamma, beta, 1e-5)))  # evaluation: no dropout, the inference kernel's bits
    L.set_fused_ln_train(False)  # (the fixture puts the setting back)
    before = dict(L.CALLS)
    t = L.dropout_add_layer_norm(x, r, gamma.half(), beta.half(), p=0.0)
    assert L.CALLS["torch"] == before["torch"] + 1 and L.CALLS["forward"] == before["forward"]
    assert torch.equal(t, F.layer_norm(x + r, (72,), gamma.half(), beta.half(), 1e-5))


def test_fused_bert_self_output_against_the_plain_composition(ops):
    import types

    from outeffhop_amd import layers as L
    from outeffhop_amd.autograd_attention import draw_seed

    cfg = types.SimpleNamespace(hidden_size=72, intermediate_size=144, layer_norm_eps=1e-12, hidden_dropout_prob=P)
    torch.manual_seed(5)
    m = L.FusedBertSelfOutput(cfg).cuda().train()
    with torch.no_grad():
        m.LayerNorm.weight.normal_(1.0, 0.25)
        m.LayerNorm.bias.normal_(0.0, 0.1)
    hs, inp = torch.randn(2, 6, 72, device="cuda"), torch.randn(2, 6, 72, device="cuda", requires_grad=True)
    wy = torch.randn(2, 6, 72, device="cuda")
    torch.manual_seed(21)
    seed = draw_seed()
    torch.manual_seed(21)
    before = dict(L.CALLS)
    kept = []

    def keep_output(mod, args, out):  # the dense layer's output: its gradient is the fused call's dx
        out.retain_grad()
        kept.append(out)

    hook = m.dense.register_forward_hook(keep_output)
    y = m(hs, inp)
    hook.remove()
    (y * wy).sum().backward()
    assert L.CALLS["forward"] == before["forward"] + 1 and L.CALLS["backward"] == before["backward"] + 1
    # dense -> mask -> add -> LayerNorm with the kernel's mask
    keep_t = ops.drop_resid_ln_mask(12, 72, P, seed, "cuda")
    keep = keep_t.cpu().numpy()
    h = m.dense(hs).detach()
    s = torch.where(keep_t.view(2, 6, 72), h * torch.tensor(T.inv_keep(P), device="cuda"), torch.zeros((), device="cuda")) + inp.detach()
    ref = _reference(s.view(12, 72), m.LayerNorm.weight, m.LayerNorm.bias, wy.view(12, 72), None, keep, T.inv_keep(P), eps=1e-12)
    got = dict(y=y.view(12, 72), dx=kept[0].grad.view(12, 72), dr=inp.grad.view(12, 72), dgamma=m.LayerNorm.weight.grad, dbeta=m.LayerNorm.bias.grad)
    ratios = {k: R.check_values(_f64(v), ref[k][0], ref[k][1], "float32") for k, v in got.items()}
    assert not _f64(got["dx"])[~keep].any() and m.dense.weight.grad is not None
    _show("FusedBertSelfOutput hidden 72 fp32", ratios)


def test_no_rows(ops):
    from outeffhop_amd import layers as L

    x = torch.zeros(0, 72, device="cuda", requires_grad=True)
    w, b = torch.ones(72, device="cuda", requires_grad=True), torch.zeros(72, device="cuda", requires_grad=True)
    s, y = L.dropout_add_layer_norm(x, torch.zeros(0, 72, device="cuda"), w, b, p=P, want_sum=True, dropout_seed=3)
    assert s.shape == (0, 72) and y.shape == (0, 72)
    (y.sum() + s.sum()).backward()
    assert x.grad.shape == (0, 72) and not w.grad.any() and not b.grad.any() and w.grad.shape == (72,)
    s, y, mean, rstd = ops.drop_resid_ln_fwd(x.detach(), None, w, b)
    assert mean.shape == (0,) and y.shape == (0, 72)
