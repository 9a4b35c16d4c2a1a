"""Every launch branch of the row, quantiser, gate and min/max kernels (csrc/oeh_rows.hip and the stand-alone half of
csrc/oeh_calib.hip) against plain numpy references computed from the exact values the kernels read.  `-m gpu`.

Each parametrisation carries a table `case -> kernel instantiation -> host condition` to be checked against the launch function.
A misaligned pointer is an offset view of a flat buffer (`buf[1:1 + n].view(shape)`): ops.* call .contiguous(), which keeps the
view's storage offset.  VEC is the 16-byte vector: 4 fp32 or 8 16-bit elements."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32 = np.float32
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _vec(dtype):
    return 4 if dtype == torch.float32 else 8


def _f64(t):
    """A tensor's values as float64, exactly (16-bit -> fp32 -> float64 are exact upcasts)."""
    return t.detach().cpu().float().numpy().astype(np.float64)


def _bits(t):
    """The storage bits of a 16- or 32-bit float tensor (so that -0.0 != +0.0 and nothing hides behind a NaN)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _misaligned(t):
    """The same values one element off a 16-byte boundary (torch allocations are at least 256-byte aligned)."""
    flat = t.reshape(-1)
    buf = torch.empty(flat.numel() + 8, dtype=t.dtype, device="cuda")
    buf[1:1 + flat.numel()].copy_(flat)
    v = buf[1:1 + flat.numel()].view(t.shape)
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    return v


def _tile_rows(pattern, rows):
    """`rows` rows that repeat the (P, K) pattern: P is prime, so a row read or written at a wrong index shows."""
    P = pattern.shape[0]
    return pattern.repeat((rows + P - 1) // P, 1)[:rows].contiguous()


# =====================================================================================================================
# 1. softmax rows
# =====================================================================================================================
SPECS = [(0, False, 0.0, 1.0), (1, False, 0.0, 1.0), (0, True, -0.025, 1.0), (1, True, -0.025, 1.1)]
ROW_KINDS = ("randn*3", "mask minimum throughout", "one dominant element (+40)", "shifted by -95")


def _softmax_ref(x64, base, clip, gamma, eta):
    """float64: m = max; e = exp(x - m); den = sum e (+ exp(-m) for softmax_1; an overflow to inf makes the row 0, as in fp32);
    p = e / den; clip(p * w + g, 0, 1) with the fp32 w = RN(eta - gamma) and g = RN(gamma) the library is handed."""
    m = x64.max(axis=-1, keepdims=True)
    with np.errstate(over="ignore"):
        e = np.exp(x64 - m)
        den = e.sum(axis=-1, keepdims=True)
        if base:
            den = den + np.exp(-m)
        p = e / den
    if clip:
        p = np.clip(p * np.float64(F32(eta - gamma)) + np.float64(F32(gamma)), 0.0, 1.0)
    return p


def _softmax_rows_input(kinds, cols, dtype, g):
    x = torch.randn(len(kinds), cols, generator=g) * 3.0
    for r, kind in enumerate(kinds):
        if kind == 1:
            x[r] = torch.finfo(dtype).min  # what the reference's masks add: the dtype's most negative finite value
        elif kind == 2:
            x[r, (7 * r + cols // 2) % cols] += 40.0
        elif kind == 3:
            x[r] -= 95.0  # exp(-m) of softmax_1 crosses exp_acc's clamp (90) / the fp32 overflow; 1/den reaches the fp32 subnormals
    return x.to(dtype)


def _softmax_bar(ref, cols, dtype):
    """fp32: the project's bar rtol = 2e-6 (3e-6 for rows longer than 4096), atol = 1e-7.  16-bit outputs are that fp32 result
    rounded to nearest even: + u |ref| + s with u = 2^-11, s = 2^-25 (half the smallest subnormal) for fp16, u = 2^-8, s = 0 for bf16."""
    bar = (3e-6 if cols > 4096 else 2e-6) * np.abs(ref) + 1e-7
    if dtype == torch.float16:
        bar = bar + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25
    elif dtype == torch.bfloat16:
        bar = bar + 2.0 ** -8 * np.abs(ref)
    return bar


def _check_softmax(ops, x, what, out=None):
    x64 = _f64(x)
    cols = x.shape[-1]
    for (base, clip, gamma, eta) in SPECS:
        spec = ops.SoftmaxSpec(base=base, clip=clip, gamma=gamma, eta=eta)
        got = ops.softmax_rows(x, spec) if out is None else ops.softmax_rows(x, spec, out=out)
        assert got.dtype == x.dtype and got.shape == x.shape
        ref = _softmax_ref(x64, base, clip, gamma, eta)
        err = np.abs(_f64(got) - ref)  # (a NaN fails the comparison below)
        bar = _softmax_bar(ref, cols, x.dtype)
        ok = err <= bar
        print(f"softmax {what} spec={(base, clip, gamma, eta)}: max err/bar {np.nanmax(err / bar):.3f}")
        assert ok.all(), (what, (base, clip, gamma, eta), int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), float(np.nanmax(err / bar)))


# case (dtype, cols) -> kernel                               -> condition in launch_softmax_rows / launch_softmax_rows_wave
# fp32 4, 252, 256   -> oeh_softmax_rows_wave_kernel<F32, 1> -> cols % 4 == 0, aligned, nchunk = cols / 4 <= 64
# fp32 260, 512      -> <F32, 2>                             -> 64 < nchunk <= 128
# fp32 516, 1024     -> <F32, 4>                             -> 128 < nchunk <= 256
# fp32 1028, 2048    -> <F32, 8>                             -> 256 < nchunk <= 512
# fp32 2052          -> oeh_softmax_rows_kernel<F32, true>   -> nchunk = 513 > 512; cols <= 15872: staged
# fp32 255, 2047     -> oeh_softmax_rows_kernel<F32, true>   -> cols % 4 != 0
# 16-bit 8, 512      -> wave <IN, 1>                         -> cols % 8 == 0, nchunk = cols / 8 <= 64
# 16-bit 520, 1024   -> wave <IN, 2>;  1032, 2048 -> <IN, 4>;  2056, 4096 -> <IN, 8>
# 16-bit 4104        -> oeh_softmax_rows_kernel<IN, true>    -> nchunk = 513
# 16-bit 511         -> oeh_softmax_rows_kernel<IN, true>    -> cols % 8 != 0
# Row counts 1, 3, 5, 9: the wave kernel packs four rows per workgroup, so 1, 3 and 5 leave the last workgroup partly empty.  Every
# row count sees all four row contents (ROW_KINDS): 5 and 9 rows in one matrix, 3 rows in two matrices, 1 row in four.
SOFTMAX_COLS = [("fp32", c) for c in (4, 252, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 255, 2047)] + \
               [(d, c) for d in ("fp16", "bf16") for c in (8, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 511)]


@pytest.mark.parametrize("dt,cols", SOFTMAX_COLS, ids=[f"{d}-{c}" for d, c in SOFTMAX_COLS])
def test_softmax_rows_every_chunk_count(ops, dt, cols):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(1000 + cols)
    for rows in (1, 3, 5, 9):
        for k in range((len(ROW_KINDS) + rows - 1) // rows):
            kinds = [(k * rows + r) % len(ROW_KINDS) for r in range(rows)]
            x = _softmax_rows_input(kinds, cols, dtype, g).cuda()
            _check_softmax(ops, x, f"{dt} {rows}x{cols} kinds={kinds}")


# case                       -> kernel                                 -> condition
# fp32 5 x 2048, x misaligned -> oeh_softmax_rows_kernel<F32, true>     -> (x | y) & 15 != 0 in launch_softmax_rows_wave
# fp32 65539 x 5              -> <F32, true>, grid = 65536              -> rows > 65536: rows 65536.. are a second trip of the row loop (red[] reused)
# fp32 2 x 15872              -> <F32, true>                            -> cols <= 15872
# fp32 2 x 15876, 2 x 15873   -> oeh_softmax_rows_kernel<F32, false>    -> cols > 15872 (a multiple of 4 and not)
# out=                        -> wave <F32, 8>, written into the caller's tensor
def test_softmax_rows_misaligned_input_takes_the_staged_kernel(ops):
    g = torch.Generator().manual_seed(11)
    x = _misaligned(_softmax_rows_input([0, 1, 2, 3, 0], 2048, torch.float32, g).cuda())
    _check_softmax(ops, x, "fp32 5x2048 misaligned")


def test_softmax_rows_more_rows_than_the_staged_grid(ops):
    g = torch.Generator().manual_seed(12)
    rows = 65539
    x = _softmax_rows_input([r % 4 if r % 97 == 0 or r >= 65536 else 0 for r in range(rows)], 5, torch.float32, g).cuda()
    _check_softmax(ops, x, "fp32 65539x5")


@pytest.mark.parametrize("cols", [15872, 15876, 15873])
def test_softmax_rows_staged_limit(ops, cols):
    g = torch.Generator().manual_seed(cols)
    for kinds in ([0, 1], [2, 3]):
        _check_softmax(ops, _softmax_rows_input(kinds, cols, torch.float32, g).cuda(), f"fp32 2x{cols} kinds={kinds}")


def test_softmax_rows_out_tensor(ops):
    g = torch.Generator().manual_seed(13)
    x = _softmax_rows_input([0, 1, 2, 3, 0], 2048, torch.float32, g).cuda()
    out = torch.full_like(x, float("nan"))
    _check_softmax(ops, x, "fp32 5x2048 out=", out=out)
    assert ops.softmax_rows(x, ops.SoftmaxSpec(1), out=out).data_ptr() == out.data_ptr()


# =====================================================================================================================
# 2. fake-quantisers, bit for bit
# =====================================================================================================================
def _fq_ref(x32, scale, zp, qmax):
    """The reference formula in numpy float32 (every operation correctly rounded, as the kernels' are):
    idx = clamp(round_half_even(x / scale) + zp, 0, qmax), x_q = scale * (idx - zp)."""
    x32 = np.asarray(x32, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(x32 / F32(scale))
        idx = np.clip(r + F32(zp), F32(0.0), F32(qmax))
        y = F32(scale) * (idx - F32(zp))
    assert y.dtype == F32 and idx.dtype == F32
    return y, idx


def _as_dtype_bits(y32, dtype):
    """fp32 values cast to `dtype` with round-to-nearest-even, as bits."""
    return _bits(torch.from_numpy(np.ascontiguousarray(y32)).to(dtype))


def _range_grid(lo, hi, n_bits, eps):
    """set_quant_range in float64, as fake_quant_range_kernel derives it on the device."""
    qmax = float(2 ** n_bits - 1)
    x_min, x_max = min(lo, 0.0), max(hi, eps)
    delta = (x_max - x_min) / qmax
    zero = -x_min / delta
    return float(F32(max(delta, eps))), float(min(max(np.rint(zero), 0.0), qmax)), qmax


# grids: (n_bits, scale, zero point).  2^-5 puts 16-bit inputs on exact .5 ties; zp = 0 and zp = qmax are the one-sided grids.
FQ_GRIDS = [(4, 0.61, 7.0), (8, 0.0371, 121.0), (8, 0.03125, 0.0), (8, 0.0433, 255.0), (16, 1.73e-4, 30000.0)]


def _check_fake_quant(ops, x, what):
    x32 = x.detach().cpu().float().numpy()
    for (n_bits, scale, zp) in FQ_GRIDS:
        qmax = float(2 ** n_bits - 1)
        spec = ops.FakeQuantSpec(float(F32(scale)), zp, qmax)
        want_y, want_idx = _fq_ref(x32, spec.scale, zp, qmax)
        want_bits = _as_dtype_bits(want_y, x.dtype)
        y = ops.fake_quant(x, spec)
        bad = _bits(y) != want_bits
        assert not bad.any(), (what, n_bits, "values", int(bad.sum()), np.argwhere(bad)[:4].tolist())
        if qmax <= 255.0:  # (the index output is uint8: 16-bit grids run without it)
            y2, idx = ops.fake_quant(x, spec, want_idx=True)
            bad = idx.cpu().numpy() != want_idx.astype(np.uint8)
            assert not bad.any(), (what, n_bits, "indices", int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert np.array_equal(_bits(y2), want_bits), (what, n_bits, "values next to indices")


# case (per dtype)                      -> kernel                        -> condition in launch_fake_quant
# n = 3                                 -> oeh_fake_quant_vec_kernel     -> aligned; nvec = 0: one block, the tail loop does all of it
# n = 1000 VEC + VEC - 1                -> oeh_fake_quant_vec_kernel     -> aligned; vector body + the (n % VEC) tail by thread 0 of block 0
# n = 4096 * 256 VEC + 5 VEC + 3        -> oeh_fake_quant_vec_kernel     -> blocks capped at 4096: the grid-stride loop's second trip, + a tail
# n = 1000 VEC + VEC - 1, misaligned x  -> oeh_fake_quant_kernel         -> x & 15 != 0
# n_bits = 16 (qmax = 65535, no idx)    -> the same two kernels          -> idx == nullptr keeps the vector kernel at qmax > 255
@pytest.mark.parametrize("size", ["below_vec", "tail", "past_block_cap", "misaligned"])
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_fake_quant_vector_and_scalar_kernels_bit_exact(ops, dt, size):
    dtype = DTYPES[dt]
    V = _vec(dtype)
    n = {"below_vec": 3, "tail": 1000 * V + V - 1, "past_block_cap": 4096 * 256 * V + 5 * V + 3, "misaligned": 1000 * V + V - 1}[size]
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(n, generator=g) * 3.0).to(dtype).cuda()
    if size == "misaligned":
        x = _misaligned(x)
    _check_fake_quant(ops, x, f"{dt} {size}")


def _saturating(dt):
    """Inputs whose quotient by the step overflows fp32 (or simply leaves the grid), spread over vector body and tail, among ordinary ones."""
    big = {"fp32": [np.inf, -np.inf, 3e38, -3e38], "bf16": [np.inf, -np.inf, 3e38, -3e38], "fp16": [np.inf, -np.inf, 65504.0, -65504.0]}[dt]
    V = _vec(DTYPES[dt])
    x = torch.randn(4 * V + 3, generator=torch.Generator().manual_seed(22)) * 3.0
    pos = [1, V + 2, 2 * V, 3 * V + 3, 4 * V, 4 * V + 1, 4 * V + 2, 0]  # the last three before 0 are the tail
    for i, p in enumerate(pos):
        x[p] = big[i % 4]
    return x.to(DTYPES[dt]), pos


def _check_saturated(what, x, pos, idx, y, scale, zp, qmax=255.0):
    """Positive saturating inputs: index qmax, value scale (qmax - zp); negative: index 0.  (idx / y may be None.)"""
    xs = x.detach().cpu().float().numpy().reshape(-1)
    for p in pos:
        want_i = qmax if xs[p] > 0 else 0.0
        if idx is not None:
            assert float(idx.reshape(-1)[p]) == want_i, (what, p, float(xs[p]), float(idx.reshape(-1)[p]), want_i)
        if y is not None:
            want_v = F32(scale) * (F32(want_i) - F32(zp))
            got_v = float(y.reshape(-1)[p])
            assert got_v == float(torch.tensor(want_v).to(y.dtype)), (what, p, float(xs[p]), got_v, float(want_v))


# case                          -> kernel                                      -> what makes |x| / scale overflow
# fake_quant, aligned           -> oeh_fake_quant_vec_kernel (body and tail)   -> +-inf, +-3e38 (fp32, bf16); fp16: +-inf (+-65504 merely saturate)
# fake_quant, misaligned        -> oeh_fake_quant_kernel (divides)             -> the same tensor: both kernels must give the same bits
# fake_quant, scale = 1e-9      -> both kernels, fp32                          -> +-1e30 * RN(1e9) = inf
# fake_quant_range              -> fake_quant_range_kernel                     -> the same tensor
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_fake_quant_saturating_inputs(ops, dt):
    x, pos = _saturating(dt)
    scale, zp = float(F32(0.0371)), 100.0
    spec = ops.FakeQuantSpec(scale, zp)
    want_y, want_idx = _fq_ref(x.float().numpy(), scale, zp, 255.0)
    for name, xx in (("aligned", x.cuda()), ("misaligned", _misaligned(x.cuda()))):
        y, idx = ops.fake_quant(xx, spec, want_idx=True)
        print(f"saturating {dt} {name}: x = {x.float()[pos].tolist()} -> idx {idx.cpu()[pos].tolist()}, y {y.float().cpu()[pos].tolist()}")
        _check_saturated(f"{dt} {name}", x, pos, idx.cpu(), y.cpu(), scale, zp)
        assert np.array_equal(idx.cpu().numpy(), want_idx.astype(np.uint8)), (dt, name)
        assert np.array_equal(_bits(y), _as_dtype_bits(want_y, x.dtype)), (dt, name)
    # the grid derived on the device from a range
    lo, hi, eps = -3.71, 5.7505, 1e-12
    rs, rz, qmax = _range_grid(lo, hi, 8, eps)
    got = ops.fake_quant_range(x.cuda(), torch.tensor([lo, hi], dtype=torch.float64, device="cuda"), 8, eps)
    print(f"saturating {dt} fake_quant_range: y {got.float().cpu()[pos].tolist()}")
    _check_saturated(f"{dt} range", x, pos, None, got.cpu(), rs, rz)
    assert np.array_equal(_bits(got), _as_dtype_bits(_fq_ref(x.float().numpy(), rs, rz, qmax)[0], x.dtype)), dt
    if dt == "fp32":  # a fine grid: 1e30 / 1e-9
        x2 = torch.randn(x.numel(), generator=torch.Generator().manual_seed(222)) * 3e-8  # (ordinary elements: some tens of steps)
        for i, p in enumerate(pos):
            x2[p] = (1e30, -1e30)[i % 2]
        s2, z2 = float(F32(1e-9)), 77.0
        want_y, want_idx = _fq_ref(x2.numpy(), s2, z2, 255.0)
        for name, xx in (("aligned", x2.cuda()), ("misaligned", _misaligned(x2.cuda()))):
            y, idx = ops.fake_quant(xx, ops.FakeQuantSpec(s2, z2), want_idx=True)
            print(f"saturating fp32 scale=1e-9 {name}: idx {idx.cpu()[pos].tolist()}")
            _check_saturated(f"1e30 {name}", x2, pos, idx.cpu(), y.cpu(), s2, z2)
            assert np.array_equal(idx.cpu().numpy(), want_idx.astype(np.uint8)) and np.array_equal(_bits(y), _bits(torch.from_numpy(want_y))), name
        rs, rz, qmax = _range_grid(-77e-9, 178e-9, 8, eps)
        got = ops.fake_quant_range(x2.cuda(), torch.tensor([-77e-9, 178e-9], dtype=torch.float64, device="cuda"), 8, eps)
        _check_saturated("1e30 range", x2, pos, None, got.cpu(), rs, rz)
        assert np.array_equal(_bits(got), _bits(torch.from_numpy(_fq_ref(x2.numpy(), rs, rz, qmax)[0])))


# case                    -> kernel                                 -> condition in launch_quantize_heads_i8
# transpose=False         -> quantize_rows_kernel<IN, true>         -> y != nullptr
# transpose=True          -> quantize_heads_t_kernel<IN, true>      -> y != nullptr
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_quantize_heads_i8_saturating_inputs(ops, dt):
    xs, pos = _saturating(dt)
    B, S, H = 2, 16, 1
    x = (torch.randn(B * S * H * 64, generator=torch.Generator().manual_seed(23)) * 3.0).to(DTYPES[dt])
    where = [64 * 3 + 5 + 17 * i for i in range(len(pos))]
    for w, p in zip(where, pos):
        x[w] = xs[p]
    x = x.view(B, S, H * 64)
    scale, zp = float(F32(0.0371)), 100.0
    want_y, want_idx = _fq_ref(x.float().numpy(), scale, zp, 255.0)
    want_c = (want_idx.astype(np.int32) - 128).astype(np.int8).reshape(B, S, H, 64)
    for transpose in (False, True):
        idx, y = ops.quantize_heads_i8(x.cuda(), ops.FakeQuantSpec(scale, zp), H, transpose=transpose, want_values=True)
        got_c = idx.cpu().numpy() if not transpose else idx.permute(0, 1, 3, 2).cpu().numpy()  # -> (B, H, S, 64)
        print(f"saturating {dt} quantize_heads_i8 transpose={transpose}: idx {(got_c.transpose(0, 2, 1, 3).reshape(-1)[where].astype(int) + 128).tolist()}")
        _check_saturated(f"{dt} heads transpose={transpose}", x, where, got_c.transpose(0, 2, 1, 3).astype(np.int32) + 128, y.cpu(), scale, zp)
        assert np.array_equal(got_c, want_c.transpose(0, 2, 1, 3)), (dt, transpose)
        assert np.array_equal(_bits(y), _as_dtype_bits(want_y, x.dtype)), (dt, transpose)


def test_proj_quant_i8_accumulator_far_beyond_the_grid(ops):
    """The projection GEMM's epilogue quantiser (oeh_gemm.hip) on alpha * acc + bias ten orders of magnitude beyond the grid (segment 0:
    row-major indices + values, segment 1: transposed indices, segment 2: row-major indices only).  The quotient stays inside fp32 here;
    the epilogue still uses fq_rel / fq_quot and shares their defect where alpha * acc / scale itself overflows fp32 (oeh_common.h)."""
    g = torch.Generator().manual_seed(24)
    B, S, K, H = 2, 16, 32, 1
    E = 64 * H
    a = torch.randint(-8, 9, (B * S, K), generator=g).to(torch.float16)
    w = torch.randint(-8, 9, (3 * E, K), generator=g).to(torch.float16)
    bias = torch.randn(3 * E, generator=g)
    scale, zp = float(F32(0.0371)), 100.0   # the grid spans [-3.7, 5.8]
    alphas = [1e10, 1e10, -1e10]
    spec = ops.FakeQuantSpec(scale, zp)
    res = ops.proj_quant_i8(a.cuda(), w.cuda(), bias.cuda(), B, S, [(alphas[0], spec, False, True), (alphas[1], spec, True, False), (alphas[2], spec, False, False)], pairs=False)
    acc = a.double().numpy() @ w.double().numpy().T  # small integers: exact
    for n in range(3):
        with np.errstate(over="ignore"):
            v = (acc[:, n * E:(n + 1) * E] * np.float64(F32(alphas[n])) + bias[n * E:(n + 1) * E].double().numpy()).astype(F32)
        want_y, want_idx = _fq_ref(v, scale, zp, 255.0)
        sat = acc[:, n * E:(n + 1) * E] != 0
        assert sat.mean() > 0.8 and ((want_idx == 0) | (want_idx == 255))[sat].all()
        idx = res[n][0] if n == 0 else res[n]
        got = idx.cpu().numpy().astype(np.int32) + 128      # (B, H, S, 64) or (B, H, 64, S)
        got = (got.transpose(0, 3, 1, 2) if n == 1 else got.transpose(0, 2, 1, 3)).reshape(B * S, E)
        bad = (got != want_idx) & sat   # (where acc == 0 the value is the bias itself: an ordinary element, one rounding of the fma apart)
        print(f"proj_quant_i8 alpha={alphas[n]:g}: {int(bad.sum())} of {int(sat.sum())} saturating indices differ; got {sorted(set(got[sat].tolist()))}")
        assert not bad.any(), (n, int(bad.sum()), got[bad][:8].tolist(), want_idx[bad][:8].tolist())
        if n == 0:
            y = res[n][1].cpu().numpy().reshape(B * S, E)
            assert np.array_equal(y[sat], want_y[sat]), n


# case                   -> kernel                     -> condition
# bf16, n = 8 k + 5      -> fake_quant_range_kernel<BF16> (element loop: the "tail" is simply the last partial block)
# n_bits = 16            -> qmax = 65535 in the device-derived grid
@pytest.mark.parametrize("dt,n_bits", [("bf16", 8), ("bf16", 16), ("fp16", 16), ("fp32", 16), ("fp32", 4)])
def test_fake_quant_range_bf16_tail_and_16_bit_grid(ops, dt, n_bits):
    g = torch.Generator().manual_seed(25)
    x = (torch.randn(256 * 8 * 3 + 8 * 11 + 5, generator=g) * 3.0).to(DTYPES[dt])
    for (lo, hi) in ((-3.2187, 4.000123), (0.0, 0.99871), (-7.5, -1.0)):
        s, z, qmax = _range_grid(lo, hi, n_bits, 1e-8)
        got = ops.fake_quant_range(x.cuda(), torch.tensor([lo, hi], dtype=torch.float64, device="cuda"), n_bits, 1e-8)
        want = _as_dtype_bits(_fq_ref(x.float().numpy(), s, z, qmax)[0], x.dtype)
        bad = _bits(got) != want
        assert not bad.any(), (dt, n_bits, lo, hi, int(bad.sum()), np.argwhere(bad)[:4].tolist())


# case                              -> kernel                               -> condition in launch_quantize_heads_i8
# S = 16 / 80, transpose=False      -> quantize_rows_kernel<IN, WANT_Y>     -> !transpose
# S = 16 / 80, transpose=True       -> quantize_heads_t_kernel<IN, WANT_Y>  -> transpose; S = 80: the second 64-key tile holds 16 keys
# B S E / 16 = 8192 * 256 + 4 * 7   -> quantize_rows_kernel<F16, false>     -> blocks capped at 8192: the grid-stride loop's second trip
@pytest.mark.parametrize("S", [16, 80])
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
def test_quantize_heads_i8_layouts_values_and_partial_tiles(ops, dt, S):
    g = torch.Generator().manual_seed(26 + S)
    B, H = 2, 3
    x = (torch.randn(B, S, H * 64, generator=g) * 2.0).to(DTYPES[dt])
    for (scale, zp) in ((0.031, 131.0), (0.03125, 0.0), (0.05, 255.0)):
        scale = float(F32(scale))
        want_y, want_idx = _fq_ref(x.float().numpy(), scale, zp, 255.0)
        want_c = (want_idx.astype(np.int32) - 128).astype(np.int8).reshape(B, S, H, 64)
        want_bits = _as_dtype_bits(want_y, x.dtype)
        for transpose in (False, True):
            for want_values in (False, True):
                r = ops.quantize_heads_i8(x.cuda(), ops.FakeQuantSpec(scale, zp), H, transpose=transpose, want_values=want_values)
                idx, y = r if want_values else (r, None)
                assert idx.shape == ((B, H, 64, S) if transpose else (B, H, S, 64))
                assert np.array_equal(idx.cpu().numpy(), want_c.transpose(0, 2, 3, 1) if transpose else want_c.transpose(0, 2, 1, 3)), (dt, S, transpose, want_values)
                if want_values:
                    assert np.array_equal(_bits(y), want_bits), (dt, S, transpose)


def test_quantize_heads_i8_rows_past_the_block_cap(ops):
    g = torch.Generator().manual_seed(27)
    P, S = 4099, 8192 * 256 // 4 + 16  # E = 64: four 16-element chunks per row; S % 16 == 0
    pat = (torch.randn(P, 64, generator=g) * 2.0).half()
    scale, zp = float(F32(0.031)), 131.0
    want_idx = _fq_ref(pat.float().numpy(), scale, zp, 255.0)[1]
    want_c = torch.from_numpy((want_idx.astype(np.int32) - 128).astype(np.int8)).cuda()
    x = _tile_rows(pat.cuda(), S).view(1, S, 64)
    got = ops.quantize_heads_i8(x, ops.FakeQuantSpec(scale, zp), 1)
    assert got.shape == (1, 1, S, 64) and torch.equal(got.reshape(S, 64), _tile_rows(want_c, S))


def _rn16(v64):
    """float64 -> fp16, round to nearest even, saturating at +-65504 (the kernels run with the fp16 overflow clamp)."""
    with np.errstate(over="ignore"):
        h = np.asarray(v64, dtype=np.float64).astype(np.float16)
    return np.clip(h, np.float16(-65504.0), np.float16(65504.0))


def _split_ref(x32):
    """hi = RN16(x), lo = RN16((x - hi) 2^11), and the triple's 2^-5 scalings, in float64 from the fp32 input."""
    x64 = x32.astype(np.float64)
    hi = _rn16(x64)
    lo = _rn16((x64 - hi.astype(np.float64)) * 2048.0)
    hs = _rn16(hi.astype(np.float64) * 2.0 ** -5)
    ls = _rn16(lo.astype(np.float64) * 2.0 ** -5)
    return hi, lo, hs, ls


def _split_input(rows, K, g):
    """Magnitudes log-uniform over 1e-6 .. 6e4, random signs; two values beyond the fp16 range."""
    mag = torch.exp(torch.rand(rows, K, generator=g) * (np.log(6e4) - np.log(1e-6)) + np.log(1e-6))
    x = mag * (torch.randint(0, 2, (rows, K), generator=g).float() * 2.0 - 1.0)
    x[rows // 2, 3] = 1.0e5
    x[rows - 1, K - 2] = -7.0e4
    return x


def _triple_row(hi, hs, ls):
    tail = np.zeros((hi.shape[0], 8), dtype=np.float16)
    tail[:, 0], tail[:, 1] = 1.0, 2.0 ** -5
    return np.concatenate([hi, hs, ls, tail], axis=1)


# case                                        -> kernel               -> condition
# K = 8 / 776, contiguous and column slice    -> split_pairs_kernel / split_triples_kernel (x_sr = K or the wider matrix's row length)
# rows = 16384 * 256 + 77, K = 8              -> split_pairs_kernel   -> blocks capped at 16384 (one chunk per row): second trip of the loop
# rows = 8192 * 128 + 77, K = 8               -> split_triples_kernel -> blocks capped at 8192 (two chunks per row: data and constant tail)
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("K", [8, 776])
def test_split_pairs_and_triples_exact(ops, K, strided):
    g = torch.Generator().manual_seed(28 + K)
    rows = 37
    x = _split_input(rows, K, g)
    if strided:
        wide = torch.randn(rows, K + 24, generator=g)
        wide[:, 8:8 + K] = x
        xg = wide.cuda()[:, 8:8 + K]
        assert xg.stride(0) == K + 24 and not xg.is_contiguous()
    else:
        xg = x.cuda()
    hi, lo, hs, ls = _split_ref(x.numpy())
    pairs = ops.split_pairs(xg).cpu().numpy()
    assert np.isfinite(pairs).all()
    assert np.array_equal(pairs[:, :K].view(np.int16), hi.view(np.int16)), "hi"
    bad = pairs[:, K:].view(np.int16) != lo.view(np.int16)
    assert not bad.any(), ("lo", int(bad.sum()), x.numpy()[bad][:4].tolist(), pairs[:, K:][bad][:4].tolist(), lo[bad][:4].tolist())
    tri = ops.split_triples(xg).cpu().numpy()
    want = _triple_row(hi, hs, ls)
    assert tri.shape == (rows, 3 * K + 8)
    bad = tri.view(np.int16) != want.view(np.int16)
    assert not bad.any(), ("triples", int(bad.sum()), np.argwhere(bad)[:4].tolist())


def test_split_pairs_and_triples_past_their_block_caps(ops):
    """One chunk of split_pairs is 32 bytes in and 32 bytes out, so crossing its 16384-block cap takes 134 MB each way."""
    g = torch.Generator().manual_seed(29)
    P, K = 4099, 8
    pat = _split_input(P, K, g)
    hi, lo, hs, ls = _split_ref(pat.numpy())
    rows = 8192 * 128 + 77
    want = torch.from_numpy(_triple_row(hi, hs, ls).view(np.int16)).cuda()
    got = ops.split_triples(_tile_rows(pat.cuda(), rows))
    assert torch.equal(got.view(torch.int16), _tile_rows(want, rows))
    del got
    rows = 16384 * 256 + 77
    want = torch.from_numpy(np.concatenate([hi, lo], axis=1).view(np.int16)).cuda()
    got = ops.split_pairs(_tile_rows(pat.cuda(), rows))
    assert torch.equal(got.view(torch.int16), _tile_rows(want, rows))


# =====================================================================================================================
# 3. gate predictors
# =====================================================================================================================
def _gate_ref(hid64, H, w1, b1, w2, b2, scaling, pool):
    """float64 sigmoid(logit) * scaling and the a-priori bar
         scaling / 4 * (d + m + 8) 2^-22 A + 2^-22 |gate|,   A = sum_j |w2_j| (sum_k |x_k w1_jk| + |b1_j|) + |b2|   (linear: sum_k |x_k w_k| + |b|)
    (the sigmoid's slope is at most 1/4; 2^-22 per operation is what the operand-pair MFMA path claims, the fp32 FMA kernels sit well
    inside).  Pooled: the logit term is the mean over t of the per-token one, + (T / 64 + 8) 2^-24 mean_t |logit| for the mean itself."""
    B, T, E = hid64.shape
    d = E // H
    x = hid64.reshape(B * T, H, d).transpose(1, 0, 2)  # (H, N, d)
    w1, b1 = _f64(w1), _f64(b1)
    if w2 is None:
        m = 0
        logit = np.einsum("hnd,hd->hn", x, w1) + b1[:, None]
        A = np.einsum("hnd,hd->hn", np.abs(x), np.abs(w1)) + np.abs(b1)[:, None]
    else:
        w2, b2 = _f64(w2), _f64(b2)
        m = w1.shape[1]
        pre = x @ w1.transpose(0, 2, 1) + b1[:, None, :]  # (H, N, m)
        logit = (np.maximum(pre, 0.0) * w2[:, None, :]).sum(-1) + b2[:, None]
        A = ((np.abs(x) @ np.abs(w1).transpose(0, 2, 1) + np.abs(b1)[:, None, :]) * np.abs(w2)[:, None, :]).sum(-1) + np.abs(b2)[:, None]
    logit = logit.reshape(H, B, T).transpose(1, 0, 2)  # (B, H, T)
    err = (d + m + 8) * 2.0 ** -22 * A.reshape(H, B, T).transpose(1, 0, 2)
    if pool:
        err = err.mean(-1, keepdims=True) + (T / 64.0 + 8.0) * 2.0 ** -24 * np.abs(logit).mean(-1, keepdims=True)
        logit = logit.mean(-1, keepdims=True)
    gate = scaling / (1.0 + np.exp(-logit))
    return gate[..., None], (scaling / 4.0 * err + 2.0 ** -22 * np.abs(gate))[..., None]


def _gate_params(H, d, m, g):
    if m == 0:
        return torch.randn(H, d, generator=g) / d ** 0.5, torch.randn(H, generator=g) * 0.3, None, None
    return (torch.randn(H, m, d, generator=g) / d ** 0.5, torch.randn(H, m, generator=g) * 0.3,
            torch.randn(H, m, generator=g) / m ** 0.5, torch.randn(H, generator=g) * 0.3)


def _run_gate(ops, dt, d, m, H=3, B=3, T=37, layout="plain", pool=False, scaling=1.5, seed=0, outliers=False):
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(3000 + 131 * d + 7 * m + H + T + seed)
    E = H * d
    hid = torch.randn(B, T, E, generator=g).to(dtype)
    hot = None
    if outliers:  # hidden values beyond the fp16 range: the MFMA path saturates them under fp16_overflow_clamp
        hot = [(0, 3, 5), (1, 20, E - 2), (2, 36, d + 1)]
        for (b, t, e) in hot:
            hid[b, t, e] = 1.0e5
    w1, b1, w2, b2 = _gate_params(H, d, m, g)
    if layout == "strided":
        wide = torch.randn(B, T, E + 64, generator=g).to(dtype).cuda()
        wide[..., :E] = hid.cuda()
        hg = wide[..., :E]
        assert hg.stride() == (T * (E + 64), E + 64, 1)
    elif layout == "misaligned":
        hg = _misaligned(hid.cuda())
    else:
        hg = hid.cuda()
    c = lambda t: None if t is None else t.cuda()  # noqa: E731
    got = ops.gate_fwd(hg, H, c(w1), c(b1), c(w2), c(b2), per_head_pool=pool, scaling=scaling)
    want, bar = _gate_ref(_f64(hid), H, w1, b1, w2, b2, scaling, pool)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape == ((B, H, 1, 1) if pool else (B, H, T, 1))
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    if hot is not None:  # those tokens: finite is all that is asked
        for (b, t, e) in hot:
            err[b, :, t] = 0.0
    print(f"gate {dt} d={d} m={m} H={H} T={T} {layout} pool={pool}: max err/bar {float((err / bar).max()):.3f}")
    ok = err <= bar
    assert ok.all(), (dt, d, m, layout, pool, int((~ok).sum()), float((err / bar).max()), np.argwhere(~ok)[:4].tolist())


# case                          -> kernel                                -> condition in launch_gate_fast / launch_gate
# fp16 / fp32, d 32 / 64 / 128,  -> oeh_gate_mfma_kernel<IN, d, 1>       -> not bf16, aligned, d in {32, 64, 128}, m <= 64, groups * H = 2 * 3 < 4096
#   m 0, 1, 5, 16, 17, 48, 64      (m = 0: Linear, unit 0 only; 1, 5, 17: a partial 16-unit tile; 64: all four tiles; 3 * 37 = 111 tokens: a partial group)
MFMA_CASES = [(dt, d, m) for dt in ("fp16", "fp32") for d in (32, 64, 128) for m in (0, 1, 5, 16, 17, 48, 64)]


@pytest.mark.parametrize("dt,d,m", MFMA_CASES, ids=[f"{a}-d{b}-m{c}" for a, b, c in MFMA_CASES])
def test_gate_mfma_one_group_per_workgroup(ops, dt, d, m):
    _run_gate(ops, dt, d, m)


# fp16, d 32, m 0 / 20, H = 64,  -> oeh_gate_mfma_kernel<F16, 32, 4>      -> groups = ceil(4131 / 64) = 65, 65 * 64 >= 4096: grid x = 17, the last workgroup
#   B = 3, T = 1377                                                          takes group 64 (35 live tokens) and breaks at group 65
@pytest.mark.parametrize("m", [0, 20])
def test_gate_mfma_four_groups_per_workgroup(ops, m):
    _run_gate(ops, "fp16", 32, m, H=64, B=3, T=1377)


# fp16 / fp32, d 64, m 65        -> oeh_gate_logit_fast_kernel<IN, 64, 4> -> m > 64 leaves the MFMA branch (goto element_kernel); m >= 4: NW = 4
# bf16, d 64, m 0, 1, 3          -> oeh_gate_logit_fast_kernel<BF16, 64, 1> -> bf16 never takes the MFMA branch; m < 4: NW = 1 (remainder loop only)
# bf16, d 64, m 4, 7             -> <BF16, 64, 4>: remainder loop only (j + 12 < m never holds)
# bf16, d 64, m 16               -> <BF16, 64, 4>: the four-unit unrolled loop only;  m 19: unrolled once, then waves 0..2 take units 16..18
# bf16, d 32 / 128, m 16         -> <BF16, 32, 4> / <BF16, 128, 4>
FAST_CASES = [("fp16", 64, 65), ("fp32", 64, 65)] + [("bf16", 64, m) for m in (0, 1, 3, 4, 7, 16, 19)] + [("bf16", 32, 16), ("bf16", 128, 16)]


@pytest.mark.parametrize("dt,d,m", FAST_CASES, ids=[f"{a}-d{b}-m{c}" for a, b, c in FAST_CASES])
def test_gate_fast_kernel(ops, dt, d, m):
    _run_gate(ops, dt, d, m)


# all three dtypes, d 48, m 0 / 6 -> oeh_gate_logit_kernel<IN>            -> launch_gate_fast's switch (d) has no case 48
# fp16, d 64, m 16, misaligned    -> oeh_gate_logit_kernel<F16>           -> hidden & 15 != 0
ELEMENT_CASES = [(dt, 48, m, "plain") for dt in ("fp32", "fp16", "bf16") for m in (0, 6)] + [("fp16", 64, 16, "misaligned")]


@pytest.mark.parametrize("dt,d,m,layout", ELEMENT_CASES, ids=[f"{a}-d{b}-m{c}-{e}" for a, b, c, e in ELEMENT_CASES])
def test_gate_element_kernel(ops, dt, d, m, layout):
    _run_gate(ops, dt, d, m, layout=layout)


# hidden = wide[..., :E] of (B, T, E + 64): hs_t = E + 64, hs_b = T (E + 64)  -> the MFMA kernel (fp16) and the fast kernel (bf16) with row strides wider than E
@pytest.mark.parametrize("dt,d,m", [("fp16", 64, 16), ("fp32", 32, 5), ("bf16", 64, 19)])
def test_gate_strided_hidden(ops, dt, d, m):
    _run_gate(ops, dt, d, m, layout="strided")


# per_head_pool: the kernel writes logits (apply_sigmoid = 0) and oeh_gate_pool_kernel reduces them over T; T = 37 (< one 64-lane pass) and 200
# fp16 d 64 m 16 -> MFMA;  bf16 d 64 m 19 -> fast;  fp32 d 48 m 6 -> element;  + the Linear predictor (m = 0) of each
POOL_CASES = [(dt, d, m, T) for (dt, d, m) in (("fp16", 64, 16), ("fp16", 64, 0), ("bf16", 64, 19), ("bf16", 64, 0), ("fp32", 48, 6), ("fp32", 48, 0)) for T in (37, 200)]


@pytest.mark.parametrize("dt,d,m,T", POOL_CASES, ids=[f"{a}-d{b}-m{c}-T{e}" for a, b, c, e in POOL_CASES])
def test_gate_per_head_pool(ops, dt, d, m, T):
    _run_gate(ops, dt, d, m, T=T, pool=True)


def test_gate_hidden_values_beyond_fp16_stay_finite(ops):
    _run_gate(ops, "fp32", 64, 16, outliers=True)


# =====================================================================================================================
# 4. min / max
# =====================================================================================================================
def _check_minmax(ops, x, what):
    ref = x.detach().cpu().float().numpy().reshape(-1)
    got = ops.minmax(x).cpu().numpy()
    assert got.dtype == np.float32 and got[0] == ref.min() and got[1] == ref.max(), (what, got.tolist(), float(ref.min()), float(ref.max()))


# case (per dtype)                          -> kernel                 -> condition in launch_minmax
# n = 5                                     -> oeh_minmax_vec_kernel  -> aligned; nvec <= 1: everything (fp32: one vector + 1) in one block
# n = 1000 VEC + VEC - 1, extremes in tail  -> oeh_minmax_vec_kernel  -> the (n % VEC) tail is read by thread 0 of block 0 alone
# the same, misaligned                      -> oeh_minmax_kernel      -> x & 15 != 0
# n = 2048 * 1024 VEC + 5 VEC + VEC - 1     -> oeh_minmax_vec_kernel  -> vb capped at 2048: the four-vector loop runs, then the single-vector remainder
# all negative / signed zeros               -> both kernels (the int key order: -0.0 < +0.0; compared with ==)
@pytest.mark.parametrize("size", ["five", "tail", "misaligned", "past_block_cap"])
@pytest.mark.parametrize("dt", ["fp32", "fp16", "bf16"])
def test_minmax_every_branch(ops, dt, size):
    dtype = DTYPES[dt]
    V = _vec(dtype)
    n = {"five": 5, "tail": 1000 * V + V - 1, "misaligned": 1000 * V + V - 1, "past_block_cap": 2048 * 1024 * V + 5 * V + V - 1}[size]
    g = torch.Generator().manual_seed(41)
    x = torch.randn(n, generator=g).to(dtype)
    x[n - 1], x[n - 2] = -123.5, 77.5  # both in the tail
    xg = _misaligned(x.cuda()) if size == "misaligned" else x.cuda()
    _check_minmax(ops, xg, f"{dt} {size}")
    got = ops.minmax(xg).cpu().numpy()
    assert got[0] == -123.5 and got[1] == 77.5
    if size != "past_block_cap":
        neg = (-torch.rand(n, generator=g) - 1.0).to(dtype)  # all negative: the maximum must not stay at an initial 0 or -inf
        _check_minmax(ops, _misaligned(neg.cuda()) if size == "misaligned" else neg.cuda(), f"{dt} {size} negative")
        for sign in (1.0, -1.0):   # zeros of both signs as the minimum (sign = 1) or the maximum (sign = -1)
            z = (sign * (torch.rand(n, generator=g) + 0.5)).to(dtype)
            z[0], z[n - 1] = 0.0, -0.0
            _check_minmax(ops, _misaligned(z.cuda()) if size == "misaligned" else z.cuda(), f"{dt} {size} zeros {sign}")
