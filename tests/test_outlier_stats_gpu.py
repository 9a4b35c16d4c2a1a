"""Outlier statistics on the GPU (include/oeh.h: oeh_outlier_stats; outeffhop_amd/csrc/oeh_stats.hip) against float64 numpy on the exact
values the kernel read.  V = elements of a 16-byte vector (4 fp32, 8 fp16 / bf16), W = ops.STATS_WAVE_COLS, C = ops.STATS_CHUNK.

  case                                         kernel / path                                   host condition
  -------------------------------------------  ----------------------------------------------  ------------------------------------
  cols 1, 2, 3, V-1                            wave kernel, one partial slot                   cols <= W
  cols V, 63, 64, W (dense, 16-byte rows)      wave kernel, whole slots only (+ empty ones)    cols <= W, row address % 16 == 0
  cols V+1, 65, W-1                            wave kernel, whole slots + a partial last slot  cols <= W
  any cols <= W, offset base / odd stride      wave kernel, partial FIRST and last slot        row address % 16 != 0
  cols W+1 ... C-8 (any start)                 chunk kernel, ONE edge chunk + merge kernel     W < cols, cols + 7 <= C
  cols C-7 ... C (dense)                       one edge chunk + an EMPTY second chunk          C < cols + 7, row starts on 16 bytes
  cols C-1, C (offset base)                    two edge chunks                                 row address % 16 != 0
  cols C (dense)                               chunk kernel, the all-whole-slots body (FULL)   a chunk lies inside the row
  cols C+1, 2C, 2C+V+3, 5C+1                   FULL chunks + an edge chunk, pairwise merge     nch = ceil((cols + 7) / C) = 2, 3, 3, 6
  rows 1, 3, 7, 67                             4 rows per workgroup of the wave / merge        rows % 4 != 0: waves beyond the last row
                                               kernels; rows * nch workgroups of the chunk one
  padding NaN / 1e30 behind every row          no load beyond a row's last element             row_stride > cols
  row 2 at element 2^31 + 2 (byte 2^32 + 4)    64-bit row offsets                              rows * row_stride >= 2^31
  meter, accumulate 1 / 2 / 3                  one-wave meter kernel, rows > 64: second round  accumulate != 0
  NaN, +-inf, constant rows, cols = 1          integer max of |x| bits; min == max bits        -

Limits (derived, not measured): inf_norm bit for bit; kurtosis and std relative 4e-6; mean 2e-6 (|mean| + std).  M2 and M4 are sums
of non-negative fp32 terms over a tree of depth 8 + 2 + 6 + 2 = 18 <= 20, so <= 20 * 2^-24 = 1.2e-6 each, the kurtosis is M4 / M2^2,
and the float64 merge adds nothing visible.  Every test prints the largest error it saw (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_outlier_stats_cpu import KINDS as GOLDEN_KINDS
from tests.test_outlier_stats_cpu import f64_stats, long_input

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outlier_stats.npz")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
KINDS = ("normal", "student_t3", "outlier_columns", "large_mean", "tiny")
LAYOUTS = ("dense", "offset1", "padded", "odd_stride")
ROWS = (1, 3, 7, 67)
REL, MEAN_REL = 4e-6, 2e-6


def _consts():
    from outeffhop_amd import ops

    return ops.STATS_WAVE_COLS, ops.STATS_CHUNK


def _vec(dtype):
    return 16 // torch.empty(0, dtype=dtype).element_size()


def all_cols(dtype):
    W, Cc = _consts()
    V = _vec(dtype)
    return [1, 2, 3, V - 1, V, V + 1, 63, 64, 65, W - 1, W, W + 1, Cc - 1, Cc, Cc + 1, 2 * Cc, 2 * Cc + V + 3, 5 * Cc + 1]


def draw(gen, kind, rows, cols, dtype):
    """(rows, cols) CPU tensor of `dtype`: the values the kernel will read."""
    if kind == "student_t3":
        z = torch.randn(rows, cols, generator=gen, dtype=torch.float64)
        chi = (torch.randn(3, rows, cols, generator=gen, dtype=torch.float64) ** 2).sum(0)
        x = z / torch.sqrt(chi / 3.0)
    else:
        x = torch.randn(rows, cols, generator=gen, dtype=torch.float64)
    if kind == "outlier_columns":
        x[:, ::97] *= 60.0
    if kind == "large_mean":
        x = x + 1000.0 if dtype == torch.float32 else x * 0.5 + 100.0
    if kind == "tiny":
        x = x * 1e-3
    return x.to(dtype)


def place(x, layout):
    """The CPU tensor on the GPU in one of the layouts; returns the (rows, cols) GPU view."""
    rows, cols = x.shape
    if layout == "dense":
        return x.cuda()
    if layout == "offset1":  # base pointer one element past a 16-byte boundary
        buf = torch.empty(rows * cols + 1, dtype=x.dtype, device="cuda")
        v = buf[1:].view(rows, cols)
        v.copy_(x)
        assert v.data_ptr() % 16 == x.element_size()
        return v
    V = _vec(x.dtype)
    stride = cols + 2 * V if layout == "padded" else cols + 3 + (cols % 2)  # (odd_stride: an odd number of elements)
    assert layout == "padded" or stride % 2 == 1
    buf = torch.empty(rows, stride, dtype=x.dtype, device="cuda")
    buf[:, 0::2] = float("nan")
    buf[:, 1::2] = 1e30 if x.dtype != torch.float16 else 6e4
    v = buf[:, :cols]
    v.copy_(x)
    return v


def run(v, eps=1e-6, meter=None, accumulate=0):
    """oeh_outlier_stats on the 2-D view `v` AS IT LIES in memory (its own pointer and row stride), stats and work pre-filled with NaN."""
    from outeffhop_amd import _lib, ops

    lib = _lib.load()
    rows, cols = v.shape
    assert v.stride(1) == 1 or cols == 1
    stats = torch.full((rows, 4), float("nan"), dtype=torch.float32, device="cuda")
    nbytes = lib.oeh_outlier_stats_work_bytes(rows, cols)
    work = torch.full((max(nbytes // 8, 1),), float("nan"), dtype=torch.float64, device="cuda")
    rc = lib.oeh_outlier_stats(C.c_void_p(v.data_ptr()), rows, cols, v.stride(0) if rows > 1 else cols, ops._DT[v.dtype], eps, C.c_void_p(stats.data_ptr()),
                               C.c_void_p(meter.data_ptr() if meter is not None else 0), accumulate, C.c_void_p(work.data_ptr() if nbytes else 0),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return stats


class Worst:
    def __init__(self):
        self.kurt = self.std = self.mean = 0.0

    def __str__(self):
        return f"largest errors: kurtosis {self.kurt:.2e}, std {self.std:.2e} (limit {REL:.0e}), mean {self.mean:.2e} of |mean| + std (limit {MEAN_REL:.0e})"


def check(stats, x_cpu, worst, what, eps=1e-6):
    """stats (rows, 4) against float64 numpy on the values of x_cpu (the tensor in its storage type)."""
    got = stats.cpu().numpy().astype(np.float64)
    inf, kurt, mean, std = f64_stats(x_cpu.double().numpy(), eps)
    assert np.array_equal(stats[:, 0].cpu().numpy(), inf.astype(np.float32)), f"{what}: inf_norm"
    if x_cpu.shape[1] == 1:
        assert np.isnan(got[:, 1]).all() and np.isnan(got[:, 3]).all(), f"{what}: cols = 1"
        assert np.array_equal(got[:, 2], x_cpu.double().numpy()[:, 0])
        return
    flat = std == 0  # (a row of equal values: two or three draws on a coarse 16-bit grid) - zeros, exactly
    assert (got[flat, 3] == 0).all() and (got[flat, 1] == 0).all() and np.array_equal(got[flat, 2], mean[flat]), f"{what}: constant rows"
    got, kurt, mean, std = got[~flat], kurt[~flat], mean[~flat], std[~flat]
    if not len(std):
        return
    ek = np.abs(got[:, 1] - kurt) / np.abs(kurt)
    es = np.abs(got[:, 3] - std) / np.abs(std)
    em = np.abs(got[:, 2] - mean) / (np.abs(mean) + std)
    worst.kurt, worst.std, worst.mean = max(worst.kurt, ek.max()), max(worst.std, es.max()), max(worst.mean, em.max())
    assert ek.max() <= REL, f"{what}: kurtosis {ek.max():.3e}"
    assert es.max() <= REL, f"{what}: std {es.max():.3e}"
    assert em.max() <= MEAN_REL, f"{what}: mean {em.max():.3e}"


def bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_every_shape_class(dtype, layout):
    """Every column count of the list with every row count, the input kinds taken in turn."""
    gen = torch.Generator().manual_seed(1234 + 17 * DTYPES.index(dtype) + LAYOUTS.index(layout))
    worst, n = Worst(), 0
    for cols in all_cols(dtype):
        for rows in ROWS:
            kind = KINDS[n % len(KINDS)]
            n += 1
            x = draw(gen, kind, rows, cols, dtype)
            check(run(place(x, layout)), x, worst, f"{kind} ({rows}, {cols}) {layout}")
    print(f"\n{dtype} {layout}: {worst}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_every_input_kind(dtype, kind):
    """Each kind at the wave form's longest row, one chunk + 1, the three-chunk and the six-chunk shape, dense and one element off."""
    W, Cc = _consts()
    gen = torch.Generator().manual_seed(99 + KINDS.index(kind))
    worst = Worst()
    for cols in (777, W, Cc + 1, 2 * Cc + _vec(dtype) + 3, 5 * Cc + 1):
        x = draw(gen, kind, 3, cols, dtype)
        for layout in ("dense", "offset1"):
            check(run(place(x, layout)), x, worst, f"{kind} (3, {cols}) {layout}")
    print(f"\n{dtype} {kind}: {worst}")


@pytest.mark.parametrize("layout", ("dense", "offset1", "odd_stride"))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_planted_value_at_every_boundary(dtype, layout):
    """One value of magnitude 50 among N(0, 1): at element 0, at the last one, and around every vector and chunk boundary - one row per
    position.  A dropped (or doubly counted) boundary element shows in inf_norm (or in the moments)."""
    W, Cc = _consts()
    V = _vec(dtype)
    gen = torch.Generator().manual_seed(7)
    worst = Worst()
    for cols in (W, 2 * Cc + V + 3):
        pos = {0, 1, cols - 1, cols - 2}
        for b in [V, 2 * V, 64 * V, cols - V] + [k * Cc for k in (1, 2) if k * Cc < cols + V]:
            pos |= {b + d for d in range(-V - 1, V + 1)}
        pos = sorted(p for p in pos if 0 <= p < cols)
        x = draw(gen, "normal", len(pos), cols, dtype).clamp_(-6, 6)
        for r, p in enumerate(pos):
            x[r, p] = 50.0 if r % 2 else -50.0
        stats = run(place(x, layout))
        assert (stats[:, 0] == 50.0).all(), [pos[i] for i in torch.nonzero(stats[:, 0].cpu() != 50.0).flatten().tolist()]
        check(stats, x, worst, f"planted ({len(pos)}, {cols}) {layout}")
    print(f"\n{dtype} {layout}: {worst}")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_special_values(dtype):
    W, Cc = _consts()
    V = _vec(dtype)
    gen = torch.Generator().manual_seed(5)
    worst = Worst()
    nan, inf = float("nan"), float("inf")
    for cols in (V + 1, W, Cc + 1, 2 * Cc + V + 3):
        clean = draw(gen, "normal", 7, cols, dtype)
        x = clean.clone()
        x[1, :] = 0.1            # constant rows (0.1 is rounded to the storage type: still one value)
        x[3, :] = -3.5
        x[5, :] = 0.0
        for layout in ("dense", "offset1"):
            s = run(place(x, layout))
            ref = run(place(clean, layout))
            assert (s[[1, 3, 5], 3] == 0).all() and (s[[1, 3, 5], 1] == 0).all(), "constant rows: std == 0 and kurtosis == 0 exactly"
            assert torch.equal(s[[1, 3, 5], 0], x[[1, 3, 5], 0].float().abs().cuda()) and torch.equal(s[[1, 3, 5], 2], x[[1, 3, 5], 0].float().cuda())
            assert np.array_equal(bits(s[[0, 2, 4, 6]]), bits(ref[[0, 2, 4, 6]])), "neighbours of constant rows"
            check(s[[0, 2, 4, 6]], clean[[0, 2, 4, 6]], worst, f"neighbours ({cols})")
        for value, where, want_inf in ((nan, cols - 1, nan), (inf, cols - 1, inf), (-inf, cols // 2, inf), (inf, 0, inf)):
            x = clean.clone()
            x[2, where] = value
            x[4, where] = value
            if value != value:
                x[4, 0] = inf    # a NaN and an infinity in one row: NaN
            elif cols > 2:
                x[4, 1] = -value  # both infinities: still +inf
            s = run(place(x, "dense"))
            for r in (2, 4):
                assert (torch.isnan(s[r, 0]) if want_inf != want_inf else s[r, 0] == inf), (value, where, r, s[r])
                assert torch.isnan(s[r, 1]), (value, where, r, s[r])
            ref = run(place(clean, "dense"))
            assert np.array_equal(bits(s[[0, 1, 3, 5, 6]]), bits(ref[[0, 1, 3, 5, 6]])), "neighbours of non-finite rows"
    # cols = 1: inf_norm = |x|, std and kurtosis NaN
    x = draw(gen, "normal", 7, 1, dtype)
    for layout in ("dense", "odd_stride"):
        check(run(place(x, layout)), x, worst, "cols = 1")
    print(f"\n{dtype}: {worst}")


@pytest.mark.parametrize("cols_kind", ("wave", "chunks"))
def test_rows_beyond_two_to_the_31_elements(cols_kind):
    """Three fp16 rows 2^30 + 1 elements apart: row 2 starts at element 2^31 + 2, byte 2^32 + 4 (a 32-bit row offset would wrap)."""
    W, Cc = _consts()
    cols = 100 if cols_kind == "wave" else Cc + 9
    stride = (1 << 30) + 1
    buf = torch.empty(2 * stride + cols, dtype=torch.float16, device="cuda")
    v = buf.as_strided((3, cols), (stride, 1))
    x = draw(torch.Generator().manual_seed(3), "normal", 3, cols, torch.float16)
    x[2, cols - 1] = 50.0
    v.copy_(x)
    worst = Worst()
    check(run(v), x, worst, f"(3, {cols}) stride 2^30 + 1")
    print(f"\n{worst}")


def test_bitwise_reproducible_and_graph_capture():
    from outeffhop_amd import ops

    W, Cc = _consts()
    gen = torch.Generator().manual_seed(11)
    for cols, dtype in ((W, torch.float16), (2 * Cc + 11, torch.float32), (5 * Cc + 1, torch.bfloat16)):
        x = draw(gen, "student_t3", 7, cols, dtype).cuda()
        a, b = run(x), run(x)
        assert np.array_equal(bits(a), bits(b))
        eager = ops.outlier_stats(x)
        assert np.array_equal(bits(eager), bits(a)), "ops.outlier_stats is the same call"
        meter = torch.zeros(4, dtype=torch.float64, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = ops.outlier_stats(x, meter=meter, accumulate=3)
        meter.zero_()
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(eager)), "graph replay"
        want = torch.zeros(4, dtype=torch.float64, device="cuda")
        ops.outlier_stats(x, meter=want, accumulate=3)
        ops.outlier_stats(x, meter=want, accumulate=3)
        assert torch.equal(meter, want) and meter[1] == 14


def test_ops_reads_strided_views_in_place_and_copies_the_rest():
    from outeffhop_amd import kurtosis, inf_norm, ops

    gen = torch.Generator().manual_seed(12)
    x = draw(gen, "normal", 5, 4 * 96, torch.float16)
    padded = place(x, "padded")
    s = ops.outlier_stats(padded)
    assert np.array_equal(bits(s), bits(run(x.cuda())))
    x4 = x.cuda().view(5, 4, 96)
    assert np.array_equal(bits(ops.outlier_stats(x4)), bits(s))                                   # (B, S, E) is viewed as (B, S * E)
    t = x4.transpose(1, 2)                                                                        # rows no longer dense: copied
    assert np.array_equal(bits(ops.outlier_stats(t)), bits(run(t.contiguous().view(5, -1))))
    k, n = kurtosis(x.cuda()), inf_norm(x.cuda())
    assert k.dtype == torch.float32 and n.dtype == torch.float32 and k.shape == (5,) and n.shape == (5,)
    assert torch.equal(k, s[:, 1]) and torch.equal(n, s[:, 0])
    with pytest.raises(ValueError):
        ops.outlier_stats(torch.zeros(5, device="cuda"))


@pytest.mark.parametrize("cols_kind", ("wave", "chunks"))
def test_meter_is_the_sequential_float64_sum(cols_kind):
    """Three calls with different row counts, accumulate = 3, then 1, then 2: the meter is the Python-order float64 sum of the returned
    fp32 values (what AverageMeter.update(v.item()) forms), with ==.  130 rows: more than one round of the meter kernel's 64 lanes."""
    W, Cc = _consts()
    cols = 100 if cols_kind == "wave" else Cc + 5
    gen = torch.Generator().manual_seed(21)
    meter = torch.zeros(4, dtype=torch.float64, device="cuda")
    want = [0.0, 0.0, 0.0, 0.0]
    for rows, acc in ((5, 3), (130, 1), (9, 2)):
        x = draw(gen, "student_t3", rows, cols, torch.float32).cuda()
        s = run(x, meter=meter, accumulate=acc).cpu().numpy()
        if acc & 1:
            for v in s[:, 0]:
                want[0] += float(v)
            want[1] += rows
        if acc & 2:
            for v in s[:, 1]:
                want[2] += float(v)
            want[3] += rows
    assert meter.cpu().tolist() == want
    untouched = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
    run(x, meter=untouched, accumulate=0)
    assert torch.isnan(untouched).all()


def test_recorded_reference_values():
    """The reference's own kurtosis(x) and x.norm(p=inf) (tests/golden/outlier_stats.npz): within 4e-6 plus the reference's recorded
    distance from float64."""
    g = np.load(GOLDEN)
    worst = 0.0
    for kind in GOLDEN_KINDS:
        for tag in ("short", "long"):
            x = g[f"short_{kind}"] if tag == "short" else long_input(g["long_base"], kind)
            s = run(torch.from_numpy(x).cuda()).cpu().numpy()
            assert np.array_equal(s[:, 0], g[f"inf_{tag}_{kind}"])
            ref = g[f"kurt_{tag}_{kind}"].astype(np.float64)
            rel = np.abs(s[:, 1].astype(np.float64) - ref) / np.abs(ref)
            worst = max(worst, (rel - g[f"kurt_err_{tag}_{kind}"]).max())
            assert (rel <= REL + g[f"kurt_err_{tag}_{kind}"]).all(), (kind, tag, rel, g[f"kurt_err_{tag}_{kind}"])
    print(f"\nlargest distance from the reference beyond its own recorded error: {worst:.2e}")


def test_outlier_meter_on_a_module(monkeypatch):
    from outeffhop_amd import OutlierMeter

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(64, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 64)).cuda()
    names = ["0", "2"]
    seen = {"0": [], "2": [], "2.input": []}

    def keep_first(m, a, o):  # (a forward hook that returns something replaces the output)
        seen["0"].append(o.detach().clone())

    def keep_last(m, a, o):
        seen["2"].append(o.detach().clone())
        seen["2.input"].append(a[0].detach().clone())

    hooks = [model[0].register_forward_hook(keep_first), model[2].register_forward_hook(keep_last)]
    meter = OutlierMeter(model, names, inputs=["2"], kurtosis_batches=2)

    def no_sync(*a, **k):
        raise AssertionError("torch.cuda.synchronize called before summary()")

    monkeypatch.setattr(torch.cuda, "synchronize", no_sync)
    with torch.no_grad():
        for _ in range(3):
            model(torch.randn(5, 64, device="cuda") * 3.0)
    monkeypatch.undo()
    got = meter.summary(layer_names=["2"], ffn_substr="0")

    # the same metrics from the hooked tensors: per-sample values rounded to fp32 as the kernel returns them, Python sum / count
    from outeffhop_amd import ops

    inf_avg, kurt_avg = {}, {}
    for key in ("0", "2", "2.input"):
        s_inf = s_kurt = 0.0
        n_inf = n_kurt = 0
        for b, t in enumerate(seen[key]):
            stats = ops.outlier_stats(t).cpu().numpy()
            inf64, kurt64, _, _ = f64_stats(t.double().cpu().numpy())
            assert np.array_equal(stats[:, 0], inf64.astype(np.float32))
            assert (np.abs(stats[:, 1] - kurt64) <= REL * np.abs(kurt64)).all()
            for v in stats[:, 0]:
                s_inf += float(v)
                n_inf += 1
            if b < 2 and not key.endswith(".input"):
                for v in stats[:, 1]:
                    s_kurt += float(v)
                    n_kurt += 1
        inf_avg[key] = s_inf / n_inf
        if n_kurt:
            kurt_avg[key] = s_kurt / n_kurt
    assert n_inf == 15
    want = [("0", inf_avg["0"]), ("2", inf_avg["2"]), ("2.input", inf_avg["2.input"]), ("max_inf_norm", max(inf_avg.values())),
            ("max_ffn_inf_norm", inf_avg["0"]), ("max_layer_inf_norm", inf_avg["2"]), ("avg_kurtosis", (kurt_avg["0"] + kurt_avg["2"]) / 2),
            ("max_kurtosis", max(kurt_avg.values())), ("max_kurtosis_layers", kurt_avg["2"])]
    assert list(got.items()) == want
    meter.reset()
    assert meter.summary() == {}
    meter.remove()
    for h in hooks:
        h.remove()
    with torch.no_grad():
        model(torch.randn(5, 64, device="cuda"))
    assert list(meter.summary()) == []
