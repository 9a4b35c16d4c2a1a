"""The fused gate training kernels on the GPU (ops.gate_apply_fwd / ops.gate_apply_bwd; include/oeh.h: oeh_gate_apply_fwd / oeh_gate_apply_bwd).  `-m gpu`.

Exact: gate_out has the bits of ops.gate_fwd(scaling=1); out and dctx have the bits of the torch expression on the GPU formed from the
kernel's own gate_out (fp32 product with gate_out * scaling, one rounding to the storage type); two calls give the same bits; a hidden unit
that a large negative b1 keeps dead gets exactly zero dW1[j], db1_j and dw2_j; a token whose dout row is zero gets exactly zero dhidden;
dhidden=None leaves the other outputs' bits unchanged; a permuted dctx and a padded dhidden of the caller's hold the contiguous outputs' bits;
the four launches captured into a graph replay to the eager calls' bits.

Against float64 (tests/_gate_train_ref.py: backward64 on the stored inputs), per output tensor of dhidden, dw1, db1, dw2, db2:
|value - f64| <= 4 err64, err64 = the largest distance of the CPU fp32 torch chain (gate_autograd's per-head loop, ctx * (gate * s),
autograd) from float64 on the same call; dhidden gets half an ulp of a 16-bit storage type on top.  The factor 4 is the project's
(tests/test_ln_train_gpu.py).  Precondition, asserted: in float64 no ReLU pre-activation of an input lies within 1e-3 of zero (the
inputs are drawn that way on the CPU), so no tolerance hides a unit taken for dead or alive.

Shapes: d 32 / 64; units 0, 1, 5, 16, 64 (Linear; the layouts for 16, 32 and 64 units, full and partly filled); H 1, 3, 12; B T = 1, 63, 64,
65, 130 tokens (one lane, a ragged tile, a full tile, two tiles, B = 2 across a tile boundary); a token count taken from
ops.gate_apply_variant at which a workgroup walks two tiles and the last tile is ragged; and the workgroup counts around the reduce
kernel's 16 slices.  Layouts: ctx contiguous (B,H,T,d) and a permuted view of (B,T,H,d); hidden with a padded batch stride.

Worst ratios measured on an MI355X over all cases here (max |value - f64| / err64, limit 4): dhidden 1.43, dw1 0.96, db1 1.00, dw2 1.00,
db2 1.00 - the parameter gradients are summed in float64 from values formed in float64 and rounded once, so no fp32 evaluation is nearer.
(With the per-token chain in fp32 and only the sums in float64 the same cases gave db1 up to 6.97, dw2 up to 64, db2 4.42: DESIGN.md 20.)"""
import re

import numpy as np
import pytest

from tests import _gate_train_ref as G
from tests import _ln_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
NAMES = {torch.float32: "float32", torch.float16: "float16", torch.bfloat16: "bfloat16"}
UNITS = (0, 1, 5, 16, 64)
HEADS = (1, 3, 12)
TOKENS = ((1, 1), (1, 63), (1, 64), (1, 65), (2, 65))  # (B, T): B T = 1, 63, 64, 65, 130
GRADS = ("dhidden", "dw1", "db1", "dw2", "db2")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops

    return ops


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


def _f64(t):
    return t.detach().cpu().double().numpy()


def _to_gpu(case, ctx_layout="contig", hidden_pad=0):
    """The case's tensors on the GPU in the layout asked for: ctx contiguous or a permuted view of (B,T,H,d); hidden with `hidden_pad`
    extra token rows per batch (a padded batch stride)."""
    dev = torch.device("cuda")
    ctx = case["ctx"].to(dev)
    if ctx_layout == "permuted":
        ctx = ctx.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        assert not ctx.is_contiguous()
    hidden = case["hidden"].to(dev)
    if hidden_pad:
        B, T, E = hidden.shape
        buf = torch.full((B, T + hidden_pad, E), float("nan"), dtype=hidden.dtype, device=dev)
        buf[:, :T] = hidden
        hidden = buf[:, :T]
        assert hidden.stride(0) == (T + hidden_pad) * E
    g = lambda t: None if t is None else t.to(dev)  # noqa: E731
    return dict(ctx=ctx, hidden=hidden, dout=case["dout"].to(dev), w1=g(case["w1"]), b1=g(case["b1"]), w2=g(case["w2"]), b2=g(case["b2"]), s=case["s"])


def _call(ops, t, want_dhidden=True):
    out, pi = ops.gate_apply_fwd(t["ctx"], t["hidden"], t["w1"], t["b1"], t["w2"], t["b2"], t["s"])
    dctx, dhidden, dw1, db1, dw2, db2 = ops.gate_apply_bwd(t["dout"], t["ctx"], t["hidden"], pi, t["w1"], t["b1"], t["w2"], t["b2"], t["s"],
                                                          want_dhidden=want_dhidden)
    return dict(out=out, pi=pi, dctx=dctx, dhidden=dhidden, dw1=dw1, db1=db1, dw2=dw2, db2=db2)


def _check_case(ops, case, label, **layout):
    """One forward and one backward call, checked against every yardstick.  Returns name -> max |value - f64| / err64."""
    t = _to_gpu(case, **layout)
    B, H, T, d = t["ctx"].shape
    dtype = t["ctx"].dtype
    assert G.kink_clear(case, H), f"{label}: a pre-activation lies within {G.KINK} of zero"
    got = _call(ops, t)
    units = 0 if case["w2"] is None else case["w1"].shape[1]
    assert got["out"].shape == (B, T, H * d) and got["out"].dtype == dtype and got["pi"].shape == (B, H, T) and got["pi"].dtype == torch.float32
    assert got["dctx"].shape == (B, H, T, d) and got["dctx"].dtype == dtype and got["dhidden"].shape == (B, T, H * d) and got["dhidden"].dtype == dtype
    assert got["dw1"].shape == case["w1"].shape and got["db1"].shape == case["b1"].shape and got["dw1"].dtype == torch.float32
    assert (got["dw2"] is None and got["db2"] is None) if units == 0 else (got["dw2"].shape == (H, units) and got["db2"].shape == (H,))
    # ---- exact
    with torch.no_grad():
        pi_want = ops.gate_fwd(t["hidden"], H, t["w1"], t["b1"], t["w2"], t["b2"], scaling=1.0)[..., 0]
        g = (got["pi"] * t["s"])[..., None]
        out_want = (t["ctx"].float() * g).to(dtype).permute(0, 2, 1, 3).reshape(B, T, H * d)
        dctx_want = (t["dout"].view(B, T, H, d).permute(0, 2, 1, 3).float() * g).to(dtype)
    assert np.array_equal(_bits(got["pi"]), _bits(pi_want)), f"{label}: gate_out differs from ops.gate_fwd(scaling=1)"
    assert np.array_equal(_bits(got["out"]), _bits(out_want)), f"{label}: out differs from the torch expression"
    assert np.array_equal(_bits(got["dctx"]), _bits(dctx_want)), f"{label}: dctx differs from the torch expression"
    # ---- float64
    args = (case["dout"], case["ctx"], case["hidden"], case["w1"], case["b1"], case["w2"], case["b2"])
    want = G.backward64(*[None if a is None else _f64(a) for a in args], case["s"])
    t32 = G.torch_chain(*args, case["s"], dtype=torch.float32)
    ratios = {}
    for k in GRADS:
        if want[k] is None:
            continue
        err64 = float(np.abs(_f64(t32[k]) - want[k]).max())
        try:
            ratios[k] = R.check_values(_f64(got[k]), want[k], err64, NAMES[dtype] if k == "dhidden" else "float32")
        except AssertionError as e:
            raise AssertionError(f"{label} {k}: {e}") from None
    return ratios


def _merge(worst, ratios):
    for k, v in ratios.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _show(title, worst):
    print(f"\n{title}: max |value - f64| / err64 (limit 4): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("d", (32, 64))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_every_shape(ops, dt, d):
    worst, seed = {}, 1000 * d + 100 * list(DTYPES).index(dt)
    for units in UNITS:
        for H in HEADS:
            for B, T in TOKENS:
                seed += 1
                case = G.make_case(B, T, H, d, units, DTYPES[dt], seed)
                _merge(worst, _check_case(ops, case, f"{dt} d{d} m{units} H{H} B{B} T{T}"))
    _show(f"gate_train {dt} d{d}", worst)


@pytest.mark.parametrize("units", (0, 16))
@pytest.mark.parametrize("dt", list(DTYPES))
def test_layouts(ops, dt, units):
    """ctx as a permuted view of (B,T,H,d) and hidden with a padded batch stride, alone and together; scaling 1."""
    worst = {}
    for i, layout in enumerate((dict(ctx_layout="permuted"), dict(hidden_pad=3), dict(ctx_layout="permuted", hidden_pad=1))):
        case = G.make_case(2, 65, 3, 64, units, DTYPES[dt], 7000 + 10 * units + i, scaling=1.0)
        _merge(worst, _check_case(ops, case, f"{dt} m{units} {layout}", **layout))
    _show(f"gate_train layouts {dt} m{units}", worst)


@pytest.mark.parametrize("dt,d,units", (("fp16", 32, 5), ("fp32", 64, 16)))
def test_a_workgroup_walks_several_tiles(ops, dt, d, units):
    """More tiles than the bound on workgroups leaves one workgroup per tile: the slab loop, with a ragged last tile and a last workgroup that
    walks fewer tiles than the others."""
    H, ntok = 16, 70 * 64 - 54  # 1024 // 16 = 64 workgroups per head at the most; 70 tiles
    name = ops.gate_apply_variant(1, ntok, H, d, units, DTYPES[dt], backward=True)
    m = re.search(r"/G(\d+)x(\d+)$", name)
    groups, per = int(m.group(1)), int(m.group(2))
    tiles = -(-ntok // 64)
    assert per == 2 and groups == 35 and ntok % 64 != 0 and groups * per >= tiles, name
    case = G.make_case(1, ntok, H, d, units, DTYPES[dt], 8100 + d)
    _show(f"gate_train {name}", _check_case(ops, case, name))
    # ... and with a last workgroup of one tile: 69 tiles over 35 workgroups, B = 2 across the tiles
    ntok = 69 * 32 - 7
    name = ops.gate_apply_variant(2, ntok, H, d, units, DTYPES[dt], backward=True)
    assert name.endswith("/G35x2") and -(-2 * ntok // 64) == 69, name
    case = G.make_case(2, ntok, H, d, units, DTYPES[dt], 8200 + d)
    _show(f"gate_train {name} (odd tiles)", _check_case(ops, case, name))


@pytest.mark.parametrize("units", (0, 5))
def test_reduce_kernel_slice_split(ops, units):
    """The reduce kernel adds the workgroup list in 16 slices: fewer workgroups than slices, exactly 16, one more, and around 32."""
    worst = {}
    for groups in (2, 15, 16, 17, 31, 32, 33):
        ntok = groups * 64 - 3
        name = ops.gate_apply_variant(1, ntok, 1, 32, units, torch.float32, backward=True)
        assert name.endswith(f"/G{groups}x1"), name
        case = G.make_case(1, ntok, 1, 32, units, torch.float32, 8300 + groups + units)
        _merge(worst, _check_case(ops, case, name))
    _show(f"gate_train reduce split m{units}", worst)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_same_bits_twice_and_without_dhidden(ops, dt):
    for units in (0, 16):
        t = _to_gpu(G.make_case(2, 100, 3, 64, units, DTYPES[dt], 8400 + units))
        a, b, c = _call(ops, t), _call(ops, t), _call(ops, t, want_dhidden=False)
        assert c["dhidden"] is None
        for k, v in a.items():
            if v is None:
                continue
            assert np.array_equal(_bits(v), _bits(b[k])), f"{dt} m{units} {k}: two calls differ"
            if k != "dhidden":
                assert np.array_equal(_bits(v), _bits(c[k])), f"{dt} m{units} {k}: differs without dhidden"


@pytest.mark.parametrize("dt", list(DTYPES))
def test_dead_unit_and_zero_rows_are_exact_zeros(ops, dt):
    B, T, H, d, units = 2, 70, 3, 64, 5
    zero = ((0, 0), (0, 69), (1, 33))
    case = G.make_case(B, T, H, d, units, DTYPES[dt], 8500, dead_unit=(1, 2), zero_tokens=zero)
    got = _call(ops, _to_gpu(case))
    assert not _f64(got["dw1"])[1, 2].any() and _f64(got["db1"])[1, 2] == 0.0 and _f64(got["dw2"])[1, 2] == 0.0
    assert _f64(got["dw1"])[1, 1].any() and _f64(got["dw1"])[0, 2].any()  # (the neighbours are alive)
    dh = _f64(got["dhidden"])
    for b, t in zero:
        assert not dh[b, t].any(), (b, t)
    assert dh[0, 1].any() and np.isfinite(dh).all()
    _check_case(ops, case, f"{dt} dead unit")
    # Linear predictors: the zero rows
    case = G.make_case(B, T, H, d, 0, DTYPES[dt], 8501, zero_tokens=zero)
    dh = _f64(_call(ops, _to_gpu(case))["dhidden"])
    for b, t in zero:
        assert not dh[b, t].any(), (b, t)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_outputs_with_strides_of_their_own(ops, dt):
    """dctx as a permuted view of (B,T,H,d) and dhidden with a padded batch stride: the same bits as the contiguous outputs, nothing
    written outside them."""
    for units in (0, 5):
        t = _to_gpu(G.make_case(2, 70, 3, 32, units, DTYPES[dt], 8700 + units))
        B, H, T, d = t["ctx"].shape
        want = _call(ops, t)
        store_c = torch.full((B, T, H, d), 7.0, dtype=DTYPES[dt], device="cuda")
        store_h = torch.full((B, T + 2, H * d), 7.0, dtype=DTYPES[dt], device="cuda")
        dctx, dhidden = store_c.permute(0, 2, 1, 3), store_h[:, :T]
        assert not dctx.is_contiguous() and dhidden.stride(0) == (T + 2) * H * d
        got = ops.gate_apply_bwd(t["dout"], t["ctx"], t["hidden"], want["pi"], t["w1"], t["b1"], t["w2"], t["b2"], t["s"], dctx=dctx, dhidden=dhidden)
        assert got[0] is dctx and got[1] is dhidden
        assert np.array_equal(_bits(dctx), _bits(want["dctx"])) and np.array_equal(_bits(dhidden), _bits(want["dhidden"]))
        assert bool((store_h[:, T:] == 7.0).all()), "the padding rows of dhidden were written"
        for k, v in zip(("dw1", "db1", "dw2", "db2"), got[2:]):
            assert (v is None and want[k] is None) or np.array_equal(_bits(v), _bits(want[k])), k


@pytest.mark.parametrize("units", (0, 16))
def test_the_chain_of_launches_replays_from_a_graph(ops, units):
    """The four launches of one forward + backward - no allocation outside the capture's pool, no host synchronisation - captured into a
    graph on a side stream (ops._scratch's capture branch hands out the work buffer) and replayed: the bits of the eager calls, twice."""
    t = _to_gpu(G.make_case(2, 100, 3, 64, units, torch.float16, 8800 + units))
    want = _call(ops, t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call(ops, t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = _call(ops, t)
    for _ in range(2):
        for v in got.values():
            if v is not None:
                v.fill_(3.0)
        g.replay()
        torch.cuda.synchronize()
        for k, v in want.items():
            assert (v is None and got[k] is None) or np.array_equal(_bits(got[k]), _bits(v)), f"m{units} {k}: the replay differs from the eager call"


def test_refusals_return_their_codes(ops):
    from outeffhop_amd import _lib

    def code(fn):
        with pytest.raises(_lib.OehError) as e:
            fn()
        return e.value.code

    dev = torch.device("cuda")
    mk = lambda B, T, H, d, m: _to_gpu(G.make_case(B, T, H, d, m, torch.float16, 8600))  # noqa: E731
    t = mk(1, 8, 2, 64, 5)
    t48 = dict(t, ctx=torch.zeros(1, 2, 8, 48, dtype=torch.float16, device=dev), hidden=torch.zeros(1, 8, 96, dtype=torch.float16, device=dev),
               w1=torch.zeros(2, 5, 48, device=dev))
    assert code(lambda: ops.gate_apply_fwd(t48["ctx"], t48["hidden"], t48["w1"], t["b1"], t["w2"], t["b2"])) == -95  # d = 48
    wide = dict(w1=torch.zeros(2, 65, 64, device=dev), b1=torch.zeros(2, 65, device=dev), w2=torch.zeros(2, 65, device=dev), b2=t["b2"])
    assert code(lambda: ops.gate_apply_fwd(t["ctx"], t["hidden"], **wide)) == -95  # 65 hidden units
    assert code(lambda: ops.gate_apply_fwd(t["ctx"], t["hidden"], t["w1"], t["b1"], t["w2"], t["b2"], float("inf"))) == -22
    off = torch.zeros(8 * 128 + 4, dtype=torch.float16, device=dev)[4:].view(1, 8, 128)  # rows 8 bytes off
    assert code(lambda: ops.gate_apply_fwd(t["ctx"], off, t["w1"], t["b1"], t["w2"], t["b2"])) == -14
    out, pi = ops.gate_apply_fwd(t["ctx"], t["hidden"], t["w1"], t["b1"], t["w2"], t["b2"])
    assert code(lambda: ops.gate_apply_bwd(off, t["ctx"], t["hidden"], pi, t["w1"], t["b1"], t["w2"], t["b2"])) == -14
    assert code(lambda: ops.gate_apply_bwd(t["dout"], t["ctx"], t["hidden"], pi, t["w1"], t["b1"], t["w2"], t["b2"], float("nan"))) == -22
    with pytest.raises(_lib.OehError):  # no CPU path
        ops.gate_apply_fwd(t["ctx"].cpu(), t["hidden"].cpu(), t["w1"].cpu(), t["b1"].cpu(), t["w2"].cpu(), t["b2"].cpu())
