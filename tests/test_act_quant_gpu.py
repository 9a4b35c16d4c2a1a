"""`ops.act_quant` (include/oeh.h: oeh_act_quant) on the GPU.  `-m gpu`.

NONE and RELU are compared bit for bit with the kernels that compute the same chain in separate passes (`ops.quantize_heads_i8`,
`torch.relu` + `ops.fake_quant`); GELU by the index interval of tests/_act_quant_ref.py around a float64 evaluation.

Shapes: one chunk, a few chunks, a long row, a row stride above the row length, more rows than a workgroup covers, and - the launch deals
16-column chunks over at most 2048 workgroups of 256 threads - (2052, 4096), the smallest-by-rows 4096-column shape above 2048 * 256 chunks,
for the branch in which a thread takes a second chunk ("loop" in `ops.act_quant_variant`)."""
import numpy as np
import pytest

from tests import _act_quant_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, None), (3, 48, None), (17, 3072, None), (64, 768, 800), (4099, 64, None)]
LOOP_SHAPE = (2052, 4096, None)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
IBITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _rows(rows, cols, stride, dtype, seed, sigma=2.0, specials=False):
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(rows, stride or cols, generator=g) * sigma).to(dtype).cuda()
    x = base[:, :cols]
    if specials:
        x[0, :8] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 1e-30, -1e-30, 65504.0], dtype=dtype)
        x[rows - 1, cols - 4:] = torch.tensor([float("-inf"), float("nan"), -0.0, float("inf")], dtype=dtype)
    return x


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.is_floating_point():
        a, b = a.contiguous().view(IBITS[a.dtype]), b.contiguous().view(IBITS[b.dtype])
    return torch.equal(a, b)


def _bias(cols, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(cols, generator=g).cuda()


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES + [LOOP_SHAPE], ids=lambda s: f"{s[0]}x{s[1]}" + (f"s{s[2]}" if s[2] else ""))
def test_none_equals_the_separate_quantiser_kernels(ops, shape, dname):
    rows, cols, stride = shape
    dtype = DTYPES[dname]
    x = _rows(rows, cols, stride, dtype, 11, specials=True)
    assert ops.act_quant_variant(rows, cols, dtype, row_stride=stride, want_index=True).endswith("loop" if shape == LOOP_SHAPE else "once")
    for sp in (ops.FakeQuantSpec(0.05, 0.0), ops.FakeQuantSpec(0.031, 37.0)):
        y, idx = ops.act_quant(x, sp, want_index=True)
        assert y.shape == x.shape and y.dtype == dtype and idx.dtype == torch.int8 and idx.is_contiguous() and y.is_contiguous()
        yf, uf = ops.fake_quant(x, sp, want_idx=True)  # (on a dense copy of x)
        assert _same(y, yf) and _same(idx, ops.centre_indices(uf))
        if cols % 64 == 0:
            H = cols // 64
            for alpha, bias in ((1.0, None), (0.37, _bias(cols, 5))):
                y, idx = ops.act_quant(x, sp, alpha=alpha, bias=bias, want_index=True)
                hi, hy = ops.quantize_heads_i8(x.unsqueeze(0), sp, H, want_values=True, alpha=alpha, bias=bias)
                assert _same(y, hy[0]) and _same(idx, hi[0].permute(1, 0, 2).reshape(rows, cols))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES + [LOOP_SHAPE], ids=lambda s: f"{s[0]}x{s[1]}" + (f"s{s[2]}" if s[2] else ""))
def test_relu_equals_relu_then_fake_quant(ops, shape, dname):
    rows, cols, stride = shape
    dtype = DTYPES[dname]
    x = _rows(rows, cols, stride, dtype, 12, specials=True)
    for sp in (ops.FakeQuantSpec(0.02, 0.0), ops.FakeQuantSpec(0.031, 37.0)):
        y, idx = ops.act_quant(x, sp, act="relu", want_index=True)
        yf, uf = ops.fake_quant(torch.relu(x), sp, want_idx=True)
        assert _same(y, yf) and _same(idx, ops.centre_indices(uf))
        # values only, indices only, and the same call again
        assert _same(ops.act_quant(x, sp, act="relu"), y)
        assert _same(ops.act_quant(x, sp, act="relu", want_values=False, want_index=True), idx)
        y2, idx2 = ops.act_quant(x, sp, act="relu", want_index=True)
        assert _same(y2, y) and _same(idx2, idx)
        if dtype == torch.float32:
            # a raw accumulator: alpha a power of two, so that alpha * x + bias is the kernel's fused multiply-add bit for bit
            bias = _bias(cols, 6)
            v = torch.add(bias, x, alpha=0.25)
            y, idx = ops.act_quant(x, sp, act="relu", alpha=0.25, bias=bias, want_index=True)
            yf, uf = ops.fake_quant(torch.relu(v), sp, want_idx=True)
            assert _same(y, yf) and _same(idx, ops.centre_indices(uf))
    torch.cuda.synchronize()


def test_nan_and_saturation_indices(ops):
    """What the documentation says of the edge values: NaN takes index 0 (behind ReLU as well: it stays NaN), +inf the top, -inf and -0 the
    zero point's side."""
    x = torch.zeros(1, 16, device="cuda")
    x[0, :5] = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 1e38])
    for zp in (0.0, 37.0):
        sp = ops.FakeQuantSpec(0.1, zp)
        for act in ("none", "relu"):
            y, idx = ops.act_quant(x, sp, act=act, want_index=True)
            u = (idx.view(torch.uint8) ^ 128)[0, :5].tolist()
            assert u == [0, 255, 0 if act == "none" else int(zp), int(zp), 255], (zp, act, u)
            assert torch.isfinite(y).all() and not torch.signbit(y[0, 3])


@pytest.mark.parametrize("dname", list(DTYPES))
def test_gelu_indices_inside_the_float64_interval(ops, dname):
    """v ~ N(0, 2^2), grid = percentiles (0.001, 99.999) of gelu(v).  The kernel's index lies in the oracle's interval and y is that index's
    grid point.  From the oracle alone: over all shapes of the dtype at most 1e-3 of the elements are ambiguous (the two smallest shapes
    hold 16 and 144 elements - a share of one case means nothing there, so the elements are pooled), and no interval is wider than a step."""
    dtype = DTYPES[dname]
    amb = total = 0
    for rows, cols, stride in SHAPES:
        x = _rows(rows, cols, stride, dtype, 13)
        v = x.float().cpu().numpy().astype(np.float64)
        a = R.gelu64(v)
        delta, zf = R.percentile_grid(a)
        sp = ops.FakeQuantSpec.from_delta(delta, zf)
        lo, hi, _ = R.gelu_index_interval(v, sp.scale, sp.zero_point, dname)
        assert (hi - lo).max() <= 1
        amb, total = amb + int((lo != hi).sum()), total + lo.size
        y, idx = ops.act_quant(x, sp, act="gelu", want_index=True)
        u = (idx.view(torch.uint8) ^ 128).cpu().numpy().astype(np.float64)
        inside = (u >= lo) & (u <= hi)
        print(f"\n{dname} {rows}x{cols}: ambiguous {int((lo != hi).sum())} of {lo.size}, outside {int((~inside).sum())}, index 0: {float((u == 0).mean()):.2f}")
        assert inside.all(), f"{int((~inside).sum())} indices outside the interval, first at {np.argwhere(~inside)[:4].tolist()}"
        want = torch.from_numpy(R.dequant32(u, sp.scale, sp.zero_point)).to(dtype)
        assert _same(y.cpu(), want)
        assert _same(ops.act_quant(x, sp, act="gelu"), y) and _same(ops.act_quant(x, sp, act="gelu", want_values=False, want_index=True), idx)
        y2, idx2 = ops.act_quant(x, sp, act="gelu", want_index=True)
        assert _same(y2, y) and _same(idx2, idx)
    print(f"{dname}: ambiguous share {amb / total:.1e} of {total}")
    assert amb <= 1e-3 * total


def test_refusals_raise(ops):
    from outeffhop_amd import _lib

    sp = ops.FakeQuantSpec(0.1, 0.0)
    with pytest.raises(_lib.OehError):
        ops.act_quant(torch.zeros(4, 72, device="cuda"), sp)  # cols % 16
    with pytest.raises(_lib.OehError):
        ops.act_quant(torch.zeros(4, 72, device="cuda")[:, 2:66], sp)  # rows off the 16-byte grid
    with pytest.raises(ValueError):
        ops.act_quant(torch.zeros(4, 64, device="cuda"), sp, want_values=False)
    with pytest.raises(ValueError):
        ops.act_quant(torch.zeros(4, 64, device="cuda"), sp, act="tanh")
    assert ops.act_quant(torch.zeros(0, 64, device="cuda"), sp).shape == (0, 64)
