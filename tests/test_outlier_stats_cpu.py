"""CPU-side checks of the outlier statistics (include/oeh.h: oeh_outlier_stats): every refusal through ctypes without a GPU, the size
of the work buffer, the float64 statement of the formula against the reference's recorded values (tests/golden/outlier_stats.npz, made
by tests/golden/make_outlier_golden.py), no CPU fallback, and the metrics dict of `OutlierMeter.summarize` against the recorded
AverageMeter scenario."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outlier_stats.npz")
KINDS = ("normal", "student_t3", "outlier_columns", "large_mean", "tiny", "planted")
LONG = (3, 40000)


def long_input(base, kind):
    """tests/golden/make_outlier_golden.py: the (3, 40000) input of a kind from the fixture's one stored N(0, 1) draw `long_base`
    (additions, products, quotients and square roots in float64, rounded to fp32 once: the same bits everywhere)."""
    z = base.astype(np.float64)
    if kind == "student_t3":
        a, b, c = np.roll(z, 1, axis=0), np.roll(z, 2, axis=0), np.roll(z, 1, axis=1)
        z = z / np.sqrt((a * a + b * b + c * c) / 3.0)
    if kind == "large_mean":
        z = z + 1000.0
    if kind == "tiny":
        z = z * 1e-3
    x = z.astype(np.float32)
    if kind == "outlier_columns":
        x[:, ::97] *= np.float32(60.0)
    if kind == "planted":
        x[-1, -1] = np.float32(-50.0)
    return x


def f64_stats(x, eps=1e-6):
    """(inf_norm, kurtosis, mean, std) per row in float64: kurtosis = mean((x - mu)^4) / (std^4 + eps), std unbiased."""
    x = np.asarray(x, dtype=np.float64)
    mu = x.mean(axis=1, keepdims=True)
    d = x - mu
    with np.errstate(all="ignore"):
        std = np.sqrt((d * d).sum(axis=1) / (x.shape[1] - 1))
        kurt = (d ** 4).mean(axis=1) / (std ** 4 + eps)
    return np.abs(x).max(axis=1), kurt, mu[:, 0], std


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lib():
    from outeffhop_amd import _lib

    return _lib.load()


def test_every_refusal_happens_on_the_host(lib):
    p16, p8, p4 = C.c_void_p(4096), C.c_void_p(4096 + 8), C.c_void_p(4096 + 4)
    W, big = 2040, 2041

    def call(x=p16, rows=2, cols=8, stride=8, dtype=2, eps=1e-6, stats=p16, meter=None, acc=0, work=None):
        return lib.oeh_outlier_stats(x, rows, cols, stride, dtype, eps, stats, meter, acc, work, None)

    assert call(x=None) == -22 and call(stats=None) == -22
    assert call(rows=0) == -22 and call(rows=-1) == -22 and call(cols=0, stride=0) == -22 and call(cols=-3) == -22
    assert call(cols=8, stride=7) == -22
    assert call(dtype=3) == -22 and call(dtype=-1) == -22 and call(dtype=7) == -22
    assert call(eps=-1e-9) == -22 and call(eps=float("nan")) == -22
    assert call(acc=4, meter=p16) == -22 and call(acc=-1, meter=p16) == -22
    assert call(acc=1) == -22 and call(acc=2) == -22 and call(acc=3) == -22            # a meter to add to is missing
    assert call(cols=big, stride=big) == -22                                          # long rows need the work buffer
    assert call(cols=W, stride=W, stats=p8) == -14                                    # stats: 16 bytes
    assert call(stats=p4) == -14
    assert call(meter=p4, acc=1) == -14 and call(meter=p4, acc=0) == -14              # meter: 8 bytes
    assert call(cols=big, stride=big, work=p4) == -14                                 # work: 8 bytes
    assert call(x=C.c_void_p(4098)) == -14 and call(x=C.c_void_p(4097), dtype=0) == -14  # x: its own element


def test_work_bytes(lib):
    from outeffhop_amd import _lib, ops

    W, Cc = ops.STATS_WAVE_COLS, ops.STATS_CHUNK
    assert (W, Cc) == (_lib.STATS_WAVE_COLS, _lib.STATS_CHUNK) and W < Cc
    wb = lib.oeh_outlier_stats_work_bytes
    for rows in (1, 3, 67):
        for cols in (1, 2, 64, W - 1, W):
            assert wb(rows, cols) == 0
        for cols in (W + 1, Cc - 1, Cc, Cc + 1, 5 * Cc + 1):
            assert wb(rows, cols) > 0 and wb(rows, cols) % _lib.STATS_RECORD_BYTES == 0
    assert wb(0, 5) == 0 and wb(5, 0) == 0 and wb(-1, 100000) == 0
    cols = [1, 63, W, W + 1, Cc - 8, Cc - 7, Cc, Cc + 1, 2 * Cc, 2 * Cc + 11, 5 * Cc + 1, 393216, 1 << 24]
    for rows in (1, 2, 7, 67, 8192):
        sizes = [wb(rows, c) for c in cols]
        assert sizes == sorted(sizes)
        assert all(wb(rows, c) <= wb(rows + 1, c) for c in cols)
    # a row that starts up to 7 elements past a 16-byte boundary still fits its chunks
    assert wb(1, Cc - 7) == _lib.STATS_RECORD_BYTES and wb(1, Cc - 6) == 2 * _lib.STATS_RECORD_BYTES


@pytest.mark.parametrize("tag", ("short", "long"))
@pytest.mark.parametrize("kind", KINDS)
def test_float64_formula_reproduces_the_reference(golden, kind, tag):
    """The float64 numpy statement above against the reference's own fp32 evaluation (transformers_language/utils.py:9-20 on torch CPU
    tensors), relative 2e-6, and x.norm(p=inf) exactly.

    The `large_mean` kind (mean 1000, std 1) is the one near the limit, and not through the statement: the reference's fp32 `mean` is off
    by 3e-5 ... 9e-5 there (half an ulp of the data), which moves its fourth moment: 1.36e-6 on the short input and 1.14e-6 on the long
    one.  Every other kind is at 4e-8 ... 3.2e-7."""
    x = golden[f"short_{kind}"] if tag == "short" else long_input(golden["long_base"], kind)
    inf, kurt, _, _ = f64_stats(x)
    ref = golden[f"kurt_{tag}_{kind}"].astype(np.float64)
    rel = np.abs(ref - kurt) / np.abs(kurt)
    print(f"{kind} {tag}: reference vs float64 statement, max relative {rel.max():.3e} (recorded {golden[f'kurt_err_{tag}_{kind}'].max():.3e})")
    assert np.array_equal(inf.astype(np.float32), golden[f"inf_{tag}_{kind}"])
    np.testing.assert_allclose(rel, golden[f"kurt_err_{tag}_{kind}"], rtol=0, atol=1e-12)  # (the script's float64 evaluation is this one)
    assert rel.max() <= 2e-6


def test_no_cpu_fallback():
    import torch

    import outeffhop_amd as oa
    from outeffhop_amd import _lib, ops

    x = torch.randn(3, 50)
    for fn in (ops.outlier_stats, oa.kurtosis, oa.inf_norm):
        with pytest.raises(_lib.OehError):
            fn(x)
    model = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 8))
    meter = oa.OutlierMeter(model, ["0", "1"], inputs=["1"])
    with pytest.raises(_lib.OehError):
        model(torch.randn(2, 8))
    meter.remove()
    model(torch.randn(2, 8))  # hooks gone
    with pytest.raises(KeyError):
        oa.OutlierMeter(model, ["nope"])
    with pytest.raises(ValueError):
        oa.OutlierMeter(model, ["0"], inputs=["1"])


def test_summary_from_hand_filled_meters_is_the_recorded_metrics_dict(golden):
    from outeffhop_amd import OutlierMeter

    keys = [str(k) for k in golden["scenario_keys"]]
    want = OrderedDict((str(k), float(v)) for k, v in zip(golden["scenario_metric_keys"], golden["scenario_metric_values"]))
    got = OutlierMeter.summarize(keys, golden["scenario_meters"], layer_names=keys[1:], ffn_substr=".fc")
    assert list(got.items()) == list(want.items())
    assert list(got)[-6:] == ["max_inf_norm", "max_ffn_inf_norm", "max_layer_inf_norm", "avg_kurtosis", "max_kurtosis", "max_kurtosis_layers"]
    # the scenario's sums are the Python sums of the recorded fp32 values, sample by sample
    sums = {k: [0.0, 0, 0.0, 0] for k in keys}
    for b, fed in enumerate(golden["scenario_batches"]):
        for k, kind in zip(keys, fed):
            for v in golden[f"inf_short_{kind}"]:
                sums[k][0] += float(v)
                sums[k][1] += 1
            if b <= 1:
                for v in golden[f"kurt_short_{kind}"]:
                    sums[k][2] += float(v)
                    sums[k][3] += 1
    assert np.array_equal(np.array([sums[k] for k in keys], dtype=np.float64), golden["scenario_meters"])
    # a meter that never saw a kurtosis (an ".input" key) is listed with its inf-norm only, and an empty selection leaves its key out
    got = OutlierMeter.summarize(["a", "a.input"], [[6.0, 4, 2.0, 4], [10.0, 4, 0.0, 0]])
    assert list(got.items()) == [("a", 1.5), ("a.input", 2.5), ("max_inf_norm", 2.5), ("max_layer_inf_norm", 2.5), ("avg_kurtosis", 0.5),
                                 ("max_kurtosis", 0.5), ("max_kurtosis_layers", 0.5)]
