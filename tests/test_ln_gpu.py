"""Every launch branch of the block-tail kernel (csrc/oeh_ln.hip; include/oeh.h: oeh_resid_ln_quant) at the smallest shape that
reaches it.  `-m gpu`.

Yardsticks: the residual sum, its quantised values and its indices are compared BIT FOR BIT with torch's add in the storage type on the
GPU followed by the existing `ops.fake_quant`; the LayerNorm output with a float64 evaluation of the stored sum (tests/_ln_ref.py), with
the distance of CPU fp32 F.layer_norm from float64 on the same case (err64) as the unit:
  no output quantiser   |y - f64| <= 4 err64                     (+ half an ulp of a 16-bit storage type at |y|)
  output quantiser      outside the tie band |frac(y64 / scale + zp) - 1/2| <= 4 err64 / scale every index is float64's; inside it an
                        index may differ by one step; the band holds <= 1e-3 of the elements; every value is scale * (idx - zp)
The factor 4 covers the kernel's different summation tree and the two extra roundings of rstd.  The measured ratios are printed (-s).

Launch forms (oeh_ln_row.h: ln_plan; VEC = 4 fp32 / 8 16-bit elements):
  cols 8, 72, 768, 1024   one wave per row (cols <= 1024, cols % VEC == 0): CH = 1 and 4 accesses per lane in fp32, 1 and 2 in 16 bits;
                          rows 1, 3, 5 leave waves of the last workgroup without a row, 64 rows are 16 workgroups
  cols 1032, 2048, 8192   one workgroup per row (cols <= 8192): CH = 2 and 8 in fp32, 1 and 4 in 16 bits
  cols 1, 770             element accesses (cols % VEC != 0), CH = 1, 4; also: a row stride that is no multiple of VEC, a base pointer one
                          element off a 16-byte boundary (CH = 1, 4, 16, 32 over test_row_strides_and_offset_base's column list)
This list does not reach every CH of a form - fp32 wave CH = 2 (256 < cols <= 512) and the workgroup form's middle CH (2048 < cols <=
4096) are not in it.  tests/test_ln_instances_gpu.py runs every compiled instance at both ends of its range, from the registry of
tests/_ln_inst.py; this file keeps the row counts, the optional parts, the 16-bit grid, aliasing, offsets and refusals."""
import numpy as np
import pytest

from tests import _ln_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
COLS = (1, 8, 72, 768, 770, 1024, 1032, 2048, 8192)
ROWS = (1, 3, 5, 64)
EPS = 1e-5


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


def _round_storage(dtype):
    return None if dtype == torch.float32 else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy())


def _inputs(rows, cols, dtype, seed, device="cuda"):
    """x, r ~ N(0, 1) with a x40 and a x-25 outlier channel (where the row has them), gamma around 1, beta around 0."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=g)
    r = torch.randn(rows, cols, generator=g)
    if cols >= 8:
        x[:, 3] *= 40.0
        x[:, cols - 2] *= -25.0
    gamma = 1.0 + 0.25 * torch.randn(cols, generator=g)
    beta = 0.1 * torch.randn(cols, generator=g)
    return x.to(dtype).to(device), r.to(dtype).to(device), gamma.to(device), beta.to(device)


def _spec_of(ops, t, n_bits=8):
    lo, hi = float(t.min()), float(t.max())
    return ops.FakeQuantSpec(*R.grid_from_minmax(lo, hi, n_bits))


def _cpu_case(s, gamma, beta):
    """(float64 result, err64 = max distance of CPU fp32 F.layer_norm from it) on the stored sum `s`."""
    s32 = s.detach().cpu().float()
    g32, b32 = gamma.detach().cpu().float(), None if beta is None else beta.detach().cpu().float()
    y64 = R.layer_norm64(s32.numpy(), g32.numpy(), None if b32 is None else b32.numpy(), EPS)
    y32 = torch.nn.functional.layer_norm(s32, (s32.shape[-1],), g32, b32, EPS).numpy().astype(np.float64)
    return y64, float(np.abs(y32 - y64).max()), y32


def _yardstick_sum(ops, x, r, spec):
    s = x if r is None else torch.add(x, r)
    if spec is None:
        return s, None
    return ops.fake_quant(s, spec, want_idx=True)


def _check_call(ops, x, r, gamma, beta, with_sum_q, with_out_q, label, n_bits_out=8, want_sum=True, out=None, sum_out=None):
    """One fused call with everything dumped, checked against the yardsticks.  Returns (ratio, band share, flipped share).  out, sum_out:
    where the call writes (views of the caller's allocations).  want_sum=False: the call without the sum output, which has no dumps, runs
    as well and gives the checked call's y bit for bit."""
    dtype = x.dtype
    fq_sum = _spec_of(ops, x if r is None else torch.add(x, r)) if with_sum_q else None
    s_want, sidx_want = _yardstick_sum(ops, x, r, fq_sum)
    y64, err64, y32 = _cpu_case(s_want, gamma, beta)
    fq_out = ops.FakeQuantSpec(*R.grid_from_minmax(float(y32.min()), float(y32.max()), n_bits_out)) if with_out_q else None
    dump = n_bits_out <= 8
    if dump:
        s, y, sidx, yidx = ops.resid_ln_quant(x, r, gamma, beta, EPS, fq_sum=fq_sum, fq_out=fq_out, want_idx=True, out=out, sum_out=sum_out)
    else:
        (s, y), sidx, yidx = ops.resid_ln_quant(x, r, gamma, beta, EPS, fq_sum=fq_sum, fq_out=fq_out, want_sum=True, out=out, sum_out=sum_out), None, None
    if not want_sum:
        y_only = ops.resid_ln_quant(x, r, gamma, beta, EPS, fq_sum=fq_sum, fq_out=fq_out)
        assert torch.is_tensor(y_only) and np.array_equal(_bits(y_only), _bits(y)), f"{label}: y differs without the sum output"
    assert s.shape == x.shape and y.shape == x.shape and s.dtype == dtype and y.dtype == dtype
    assert np.array_equal(_bits(s), _bits(s_want)), f"{label}: the sum differs from torch add + ops.fake_quant"
    if with_sum_q and dump:
        assert np.array_equal(sidx.cpu().numpy(), sidx_want.cpu().numpy()), f"{label}: sum indices differ from ops.fake_quant"
    else:
        assert sidx is None
    if not with_out_q:
        assert yidx is None
        ratio = R.check_values(_f64(y), y64, err64, _name(dtype))
        return ratio, 0.0, 0.0
    if dump:
        idx = yidx.cpu().numpy().astype(np.float64)
    else:  # a 16-bit grid has no uint8 dump: the index is read back from the fp32 value, which sits on the grid exactly
        assert dtype == torch.float32
        idx = np.rint(_f64(y) / fq_out.scale) + fq_out.zero_point
    # (the band's width is 8 err64 / scale of a step: the 1e-3 condition is stated for 8-bit grids, and a 16-bit grid's step is 257 times finer)
    share, flipped = R.check_indices(idx, y64, fq_out.scale, fq_out.zero_point, fq_out.qmax, err64, max_band=1e-3 * fq_out.qmax / 255.0)
    R.check_on_grid(y.detach().cpu().float().numpy(), idx, fq_out.scale, fq_out.zero_point, _round_storage(dtype))
    return 0.0, share, flipped


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cols", COLS)
def test_every_form_and_row_count(ops, cols, dt):
    dtype = DTYPES[dt]
    worst, band, flip = 0.0, 0.0, 0.0
    for rows in ROWS:
        x, r, gamma, beta = _inputs(rows, cols, dtype, 9000 + 7 * cols + rows)
        ratio, _, _ = _check_call(ops, x, r, gamma, beta, True, False, f"{rows}x{cols} {dt} plain")
        _, share, flipped = _check_call(ops, x, r, gamma, beta, True, True, f"{rows}x{cols} {dt} quantised")
        worst, band, flip = max(worst, ratio), max(band, share), max(flip, flipped)
    print(f"\nresid_ln_quant {ops.resid_ln_variant(64, cols, dtype)} cols {cols} {dt}: max |y - f64| / err64 = {worst:.2f} (limit 4), "
          f"tie band <= {band:.1e} of the elements, indices that differ from float64 <= {flip:.1e}")


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("cols", (72, 770, 1032))
def test_every_combination_of_optional_parts(ops, cols, dt):
    dtype = DTYPES[dt]
    rows = 5
    x, r, gamma, beta = _inputs(rows, cols, dtype, 9100 + cols)
    for mask in range(16):
        with_r, with_beta, with_sq, with_oq = bool(mask & 1), bool(mask & 2), bool(mask & 4), bool(mask & 8)
        _check_call(ops, x, r if with_r else None, gamma, beta if with_beta else None, with_sq, with_oq, f"{cols} {dt} parts {mask:04b}")
    # without sum_out the result is the same y, and nothing else is returned
    fq_sum, fq_out = _spec_of(ops, torch.add(x, r)), ops.FakeQuantSpec(0.05, 120.0)
    s, y = ops.resid_ln_quant(x, r, gamma, beta, EPS, fq_sum=fq_sum, fq_out=fq_out, want_sum=True)
    y_only = ops.resid_ln_quant(x, r, gamma, beta, EPS, fq_sum=fq_sum, fq_out=fq_out)
    assert torch.is_tensor(y_only) and np.array_equal(_bits(y_only), _bits(y))


def test_sixteen_bit_output_grid(ops):
    """The OPT final LayerNorm's 16-bit quantiser (qmax 65535): values only - a uint8 dump of that grid is refused."""
    from outeffhop_amd import _lib

    for cols in (768, 2048, 770):
        x, r, gamma, beta = _inputs(5, cols, torch.float32, 9200 + cols)
        _check_call(ops, x, r, gamma, beta, True, True, f"{cols} 16-bit grid", n_bits_out=16)
    with pytest.raises(_lib.OehError) as e:
        ops.resid_ln_quant(x, r, gamma, beta, EPS, fq_out=ops.FakeQuantSpec(1e-4, 30000.0, 65535.0), want_idx=True)
    assert e.value.code == -95


def _same_case(ops, got, want, y64, err64, fq_out, dtype, label):
    """Another launch form on the same values: the sum and its indices bit for bit; the LayerNorm's sums run in another order, so its
    indices by the tie-band rule - and within one step of the first form's."""
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[2].cpu().numpy(), want[2].cpu().numpy()), label
    idx = got[3].cpu().numpy().astype(np.float64)
    R.check_indices(idx, y64, fq_out.scale, fq_out.zero_point, fq_out.qmax, err64)
    R.check_on_grid(got[1].detach().cpu().float().numpy(), idx, fq_out.scale, fq_out.zero_point, _round_storage(dtype))
    assert np.abs(idx - want[3].cpu().numpy().astype(np.float64)).max() <= 1.0, label


@pytest.mark.parametrize("dt", list(DTYPES))
def test_row_strides_and_offset_base(ops, dt):
    dtype = DTYPES[dt]
    rows = 5
    for cols in (72, 1024, 2048, 4104, 8192):  # (4104 elements: 17 per thread -> the 32-access element form)
        x, r, gamma, beta = _inputs(rows, cols, dtype, 9300 + cols)
        fq_sum = _spec_of(ops, torch.add(x, r))
        y64, err64, y32 = _cpu_case(ops.fake_quant(torch.add(x, r), fq_sum), gamma, beta)
        fq_out = ops.FakeQuantSpec(*R.grid_from_minmax(float(y32.min()), float(y32.max())))
        want = ops.resid_ln_quant(x, r, gamma, beta, EPS, fq_sum=fq_sum, fq_out=fq_out, want_idx=True)
        _same_case(ops, want, want, y64, err64, fq_out, dtype, (cols, "dense"))
        for pad in (16, 3):  # a row stride above cols: a multiple of VEC (the 16-byte forms stay), and not one (element accesses)
            def strided(t):
                big = torch.full((rows, cols + pad), 7.0, dtype=dtype, device="cuda")
                big[:, :cols] = t
                return big, big[:, :cols]
            (bx, vx), (br, vr) = strided(x), strided(r)
            big_out = torch.full((rows, cols + pad), -3.0, dtype=dtype, device="cuda")
            big_sum = torch.full((rows, cols + pad), -5.0, dtype=dtype, device="cuda")
            got = ops.resid_ln_quant(vx, vr, gamma, beta, EPS, fq_sum=fq_sum, fq_out=fq_out, want_idx=True, out=big_out[:, :cols], sum_out=big_sum[:, :cols])
            assert got[1].data_ptr() == big_out.data_ptr() and got[0].data_ptr() == big_sum.data_ptr()
            _same_case(ops, got, want, y64, err64, fq_out, dtype, (cols, pad))
            if pad == 16:  # the same launch form on the same values: the same bits throughout
                assert np.array_equal(_bits(got[1]), _bits(want[1]))
            assert (big_out[:, cols:] == -3.0).all() and (big_sum[:, cols:] == -5.0).all() and (bx[:, cols:] == 7.0).all()  # nothing beyond a row's end
        def offset(t):  # the same values one element off a 16-byte boundary
            buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
            v = buf[1:1 + t.numel()].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 != 0
            return v
        for which in range(4):
            args = [x, r, gamma, beta]
            args[which] = offset(args[which])
            got = ops.resid_ln_quant(*args, EPS, fq_sum=fq_sum, fq_out=fq_out, want_idx=True)
            _same_case(ops, got, want, y64, err64, fq_out, dtype, (cols, "offset", which))
    # leading dimensions: (B, S, N) views collapse to rows; a transposed batch does not and is copied
    x, r, gamma, beta = _inputs(6, 72, dtype, 9399)
    want = ops.resid_ln_quant(x, r, gamma, beta, EPS)
    assert np.array_equal(_bits(ops.resid_ln_quant(x.view(2, 3, 72), r.view(2, 3, 72), gamma, beta, EPS).view(6, 72)), _bits(want))
    xt = x.view(2, 3, 72).transpose(0, 1)
    got = ops.resid_ln_quant(xt, r.view(2, 3, 72).transpose(0, 1), gamma, beta, EPS)
    assert got.shape == xt.shape and np.array_equal(_bits(got.transpose(0, 1).reshape(6, 72)), _bits(want))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cols", (72, 770, 2048))
def test_constant_row_gives_beta(ops, cols, dt):
    dtype = DTYPES[dt]
    x, r, gamma, beta = _inputs(5, cols, dtype, 9400 + cols)
    x[2] = 1.5  # sums of 1.5 are exact in fp32 up to 8192 terms: mean = 1.5, var = 0
    y = ops.resid_ln_quant(x, None, gamma, beta, EPS)
    assert np.array_equal(_bits(y[2]), _bits(beta.to(dtype)))
    y64, err64, _ = _cpu_case(x, gamma, beta)
    R.check_values(_f64(y), y64, err64, _name(dtype))
    y0 = ops.resid_ln_quant(x, None, gamma, None, EPS)
    assert (y0[2] == 0).all()


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("cols", (768, 770, 1032))
def test_aliasing(ops, cols, dt):
    """sum_out == r, sum_out == x and y == x: a thread has loaded all it needs of a row before its first store to it."""
    dtype = DTYPES[dt]
    x, r, gamma, beta = _inputs(64, cols, dtype, 9500 + cols)
    fq_sum, fq_out = _spec_of(ops, torch.add(x, r)), ops.FakeQuantSpec(0.04, 128.0)
    kw = dict(fq_sum=fq_sum, fq_out=fq_out)
    s_want, y_want = ops.resid_ln_quant(x, r, gamma, beta, EPS, want_sum=True, **kw)
    rc = r.clone()
    s, y = ops.resid_ln_quant(x, rc, gamma, beta, EPS, sum_out=rc, **kw)
    assert s.data_ptr() == rc.data_ptr() and np.array_equal(_bits(rc), _bits(s_want)) and np.array_equal(_bits(y), _bits(y_want))
    xc = x.clone()
    s, y = ops.resid_ln_quant(xc, r, gamma, beta, EPS, sum_out=xc, **kw)
    assert np.array_equal(_bits(xc), _bits(s_want)) and np.array_equal(_bits(y), _bits(y_want))
    xc = x.clone()
    y = ops.resid_ln_quant(xc, r, gamma, beta, EPS, out=xc, **kw)
    assert y.data_ptr() == xc.data_ptr() and np.array_equal(_bits(xc), _bits(y_want))
    xc, rc = x.clone(), r.clone()
    s, y = ops.resid_ln_quant(xc, rc, gamma, beta, EPS, out=xc, sum_out=rc, **kw)  # the decoder layer's in-place use
    assert np.array_equal(_bits(rc), _bits(s_want)) and np.array_equal(_bits(xc), _bits(y_want))


def test_two_calls_are_bitwise_equal(ops):
    for cols, dtype in ((768, torch.float32), (8192, torch.float32), (770, torch.float16), (2048, torch.bfloat16)):
        x, r, gamma, beta = _inputs(64, cols, dtype, 9600 + cols)
        a = ops.resid_ln_quant(x, r, gamma, beta, EPS, want_sum=True)
        b = ops.resid_ln_quant(x, r, gamma, beta, EPS, want_sum=True)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_refusals_on_the_device(ops):
    from outeffhop_amd import _lib

    x, r, gamma, beta = _inputs(3, 72, torch.float32, 9700)
    with pytest.raises(_lib.OehError):
        ops.resid_ln_quant(x.cpu(), None, gamma.cpu(), beta.cpu())
    with pytest.raises(_lib.OehError):
        ops.resid_ln_quant(x, r.cpu(), gamma, beta)
    wide = torch.zeros(2, 8200, device="cuda")
    with pytest.raises(_lib.OehError) as e:
        ops.resid_ln_quant(wide, None, torch.ones(8200, device="cuda"))
    assert e.value.code == -95
    with pytest.raises(_lib.OehError) as e:
        ops.resid_ln_quant(x, r, gamma, beta, -1.0)
    assert e.value.code == -22
    with pytest.raises(ValueError):
        ops.resid_ln_quant(x, r[:, :8], gamma, beta)
    with pytest.raises(ValueError):
        ops.resid_ln_quant(x, r, gamma, beta, out=torch.empty(72, 3, device="cuda").t())  # no contiguous last dimension
    assert ops.resid_ln_quant(x[:0], None, gamma, beta).shape == (0, 72)
