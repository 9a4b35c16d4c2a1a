"""CPU-side checks of the MSE range estimator (outeffhop_amd.quantization.MSE_Estimator, include/oeh.h: oeh_quant_mse) against the
reference's recorded behaviour (tests/golden/mse_ranges.npz, made by tests/golden/make_mse_golden.py): the chosen ranges of every grid
search bit for bit, the loss arrays within the error of the reference's fp32 sums, golden section within scipy's own tolerance, the
constructor / enum / config surface, and every host-side refusal of the entry point through ctypes without a GPU."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mse_ranges.npz")
GRID_CASES = ("sym_two_sided_8", "sym_two_sided_4", "sym_one_sided_8", "asym_one_sided_8", "asym_two_sided_2d")
GOLDEN_CASES = ("golden_sym", "golden_asym")
XATOL = 1e-5  # scipy.optimize.minimize_scalar(method="Bounded"): the default absolute termination tolerance on x


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def make_estimator(golden, name):
    from outeffhop_amd.quantization import AsymmetricUniformQuantizer, MSE_Estimator, OptMethod, SymmetricUniformQuantizer

    i = list(golden["cases"]).index(name)
    qcls = SymmetricUniformQuantizer if str(golden["case_quantizer"][i]) == "symmetric" else AsymmetricUniformQuantizer
    return MSE_Estimator(num_candidates=int(golden["case_num_candidates"][i]), opt_method=OptMethod[str(golden["case_opt_method"][i])],
                         quantizer=qcls(n_bits=int(golden["case_n_bits"][i])))


def test_fixture_states_its_own_condition(golden):
    """Six cases (the golden-section one for both quantisers), and the condition on the inputs that makes exact equality of the
    chosen ranges a fair demand: the two smallest accumulated losses are more than 1e-5 apart (relative) in every grid case."""
    assert tuple(golden["cases"]) == GRID_CASES + GOLDEN_CASES
    for name in GRID_CASES:
        assert golden[f"x_{name}"].shape == (2, 4096) and (golden[f"margin_{name}"] > 1e-5).all()


@pytest.mark.parametrize("name", GRID_CASES)
def test_grid_search_reproduces_the_reference(golden, name):
    """After each of the two batches: (xmin, xmax) equal the reference's float32 values exactly; the accumulated loss array is within
    (log2 n + 2) * 2^-24 relative of the reference's - the bound on torch's pairwise fp32 sum of n non-negative terms, which the
    reference forms and this code (float64 sums of the same fp32 terms) does not; candidate 0 stays +inf."""
    est = make_estimator(golden, name)
    x = golden[f"x_{name}"]
    bound = (math.log2(x.shape[1]) + 2) * 2.0 ** -24
    for b in range(2):
        lo, hi = est(torch.from_numpy(x[b]))
        assert lo.dtype == torch.float32 and hi.dtype == torch.float32 and lo.shape == (1,) and hi.shape == (1,)
        assert float(lo) == float(golden[f"xmin_{name}"][b]) and float(hi) == float(golden[f"xmax_{name}"][b])
        got, want = est.loss_array[0].numpy(), golden[f"loss_{name}"][b]
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.isinf(got[0]).all() and np.isinf(want[0]).all() and np.isfinite(got[1:]).all()
        rel = np.abs(got[1:] - want[1:]) / want[1:]
        print(f"{name} batch {b}: loss array max rel {rel.max():.2e} (bound {bound:.2e})")
        assert (rel <= bound).all()
    assert est.one_sided_dist == (str(golden["case_kind"][list(golden["cases"]).index(name)]) == "softmax")


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_section_is_within_scipys_tolerance(golden, name):
    """scipy's bounded search stops within xatol = 1e-5 of a minimum; the reference's fp32-summed loss moves what it finds by the
    recorded distance f64dist (its own search rerun with float64 sums), so the margin is xatol + 2 * f64dist per batch and bound."""
    pytest.importorskip("scipy")
    est = make_estimator(golden, name)
    for b in range(2):
        lo, hi = est(torch.from_numpy(golden[f"x_{name}"][b]))
        d = golden[f"f64dist_{name}"][b]
        e_lo, e_hi = abs(float(lo) - float(golden[f"xmin_{name}"][b])), abs(float(hi) - float(golden[f"xmax_{name}"][b]))
        print(f"{name} batch {b}: |xmin - ref| {e_lo:.2e} (margin {XATOL + 2 * d[0]:.2e}), |xmax - ref| {e_hi:.2e} (margin {XATOL + 2 * d[1]:.2e})")
        assert e_lo <= XATOL + 2 * d[0] and e_hi <= XATOL + 2 * d[1]
    assert est.loss_array is not None and "golden_section" in repr(est) and "num_candidates" not in repr(est)


def test_constructor_enum_and_registry_match_the_reference(golden):
    import outeffhop_amd as oa
    from outeffhop_amd.quantization import MSE_Estimator, OptMethod, RangeEstimators, SymmetricUniformQuantizer

    params = list(inspect.signature(MSE_Estimator.__init__).parameters.values())
    assert [p.name for p in params] == [str(s) for s in golden["signature_names"]]
    assert [p.kind.name for p in params] == [str(s) for s in golden["signature_kinds"]]
    defaults = ["<empty>" if p.default is inspect.Parameter.empty else (p.default.name if isinstance(p.default, OptMethod) else str(p.default)) for p in params]
    assert defaults == [str(s) for s in golden["signature_defaults"]]
    assert OptMethod.list_names() == [str(s) for s in golden["opt_method_names"]] == ["grid", "golden_section"]
    assert RangeEstimators.MSE.cls is MSE_Estimator and RangeEstimators.list_names() == ["current_minmax", "running_minmax", "MSE"]
    assert oa.MSE_Estimator is MSE_Estimator and oa.OptMethod is OptMethod
    q = SymmetricUniformQuantizer(n_bits=8)
    est = RangeEstimators.MSE(quantizer=q)
    assert (est.num_candidates, est.opt_method, est.range_margin, est.per_channel, est.max_int_skew) == (100, OptMethod.grid, 0.5, False, 64)
    assert repr(est) == "MSE_Estimator(opt_method=grid ,num_candidates=100)"
    with pytest.raises(NotImplementedError):
        MSE_Estimator()                              # no quantiser
    with pytest.raises(NotImplementedError):
        MSE_Estimator(per_channel=True, quantizer=q)  # per-channel ranges stay refused by RangeEstimatorBase


def test_val_qparams_carries_the_weight_range_options():
    from outeffhop_amd.quantization import MSE_Estimator, OptMethod, RangeEstimators, get_quant_config, val_qparams

    cfg = get_quant_config()
    assert val_qparams(cfg)["weight_range_options"] == {}
    cfg.quant.weight_quant_method = RangeEstimators.MSE
    cfg.quant.weight_opt_method = OptMethod.grid
    qp = val_qparams(cfg)
    assert qp["weight_range_method"] is MSE_Estimator and qp["weight_range_options"] == {"opt_method": OptMethod.grid}
    cfg.quant.num_candidates = 40
    assert val_qparams(cfg)["weight_range_options"] == {"opt_method": OptMethod.grid, "num_candidates": 40}


def test_quant_linear_estimates_fixes_and_quantises_on_cpu():
    """Weights quantised before .to(device): the estimator's CPU path (fp32 terms by torch ops, float64 sums) under QuantLinear."""
    from outeffhop_amd.quantization import MSE_Estimator, OptMethod, QuantLinear, SymmetricUniformQuantizer

    torch.manual_seed(5)
    lin = QuantLinear(24, 16, method=SymmetricUniformQuantizer, weight_range_method=MSE_Estimator, weight_range_options=dict(opt_method=OptMethod.grid), n_bits=4)
    with torch.no_grad():
        lin.weight[3, 5] = 1.5  # one outlier weight: the MSE range clips it, min-max would not
    est = lin.weight_quantizer.range_estimator
    assert isinstance(est, MSE_Estimator) and est.quantizer is lin.weight_quantizer.quantizer
    lin.quantized_weights()
    wq = lin.weight_quantizer(lin.weight).detach()
    lo, hi = est.current_xmin, est.current_xmax
    assert float(hi) == -float(lo) and 0 < float(hi) < 1.5 + 0.5 and float(hi) != float(lin.weight.detach().max())
    lin.fix_ranges()
    assert lin.weight_quantizer.is_fixed
    before = est.loss_array.clone()
    wq2 = lin.weight_quantizer(lin.weight).detach()
    assert torch.equal(wq, wq2) and torch.equal(est.loss_array, before)  # fixed: no further estimation
    scale = float(lin.weight_quantizer.quantizer.scale)
    idx = wq / scale
    assert torch.equal(idx, torch.round(idx)) and idx.min() >= -8 and idx.max() <= 7 and wq.unique().numel() <= 16
    # the chosen range is the candidate of least error, so it is no worse than the full min-max range (the grid's last candidates)
    w = lin.weight.detach()
    mse = float(((w - wq) ** 2).sum())
    s_mm = float(w.abs().max()) / 7.0
    mm = float(((w - s_mm * torch.clamp(torch.round(w / s_mm), -8, 7)) ** 2).sum())
    assert mse < mm


def test_reset_clears_the_loss_array(golden):
    est = make_estimator(golden, "sym_two_sided_8")
    x = torch.from_numpy(golden["x_sym_two_sided_8"])
    est(x[0])
    first = est.loss_array.clone()
    est(x[1])
    assert not torch.equal(est.loss_array, first)  # accumulated without momentum
    est.reset()
    assert est.loss_array is None and est.current_xmin is None and est.current_xmax is None
    est(x[0])
    assert torch.equal(est.loss_array, first)


def test_both_thresholds_zero_fall_through_to_the_current_range(golden):
    """`if x_min or x_max` of the reference's quantize(): thresholds of exactly (0, 0) leave the copied quantiser on its current range,
    and without one that is QuantizerNotInitializedError."""
    from outeffhop_amd.quantization import QuantizerNotInitializedError

    est = make_estimator(golden, "asym_one_sided_8")
    x = torch.from_numpy(golden["x_asym_one_sided_8"][0])
    with pytest.raises(QuantizerNotInitializedError):
        est.loss_fx(x, 0, 0.0)
    est.quantizer.set_quant_range(-0.25, 0.75)
    assert est.loss_fx(x, 0, 0.0) == est.loss_fx(x, -0.25, 0.75) != est.loss_fx(x, 0, 1e-8)
    rows = est.candidate_rows([0.0, -0.25], [0.0, 0.75])
    assert torch.equal(rows[0], rows[1]) and rows.shape == (2, 4) and rows.dtype == torch.float32


def test_entry_point_refuses_on_the_host():
    from outeffhop_amd import _lib, ops

    lib = _lib.load()
    assert (ops.QMSE_CHUNK, ops.QMSE_SLICE, ops.QMSE_MAX_BLOCKS) == (_lib.QMSE_CHUNK, _lib.QMSE_SLICE, _lib.QMSE_MAX_BLOCKS) == (8192, 256, 1024)
    p16, p8, p4 = C.c_void_p(4096), C.c_void_p(4096 + 8), C.c_void_p(4096 + 4)

    def call(x=p16, n=100, dtype=2, cand=p16, K=3, loss=p8, acc=0, work=p8):
        return lib.oeh_quant_mse(x, n, dtype, cand, K, loss, acc, work, None)

    assert lib.oeh_quant_mse(None, 1, 0, None, 1, None, 0, None, None) == -22
    assert call(x=None) == -22 and call(cand=None) == -22 and call(loss=None) == -22 and call(work=None) == -22
    assert call(n=0) == -22 and call(n=-5) == -22 and call(K=0) == -22 and call(K=-1) == -22
    assert call(dtype=3) == -22 and call(dtype=-1) == -22 and call(dtype=7) == -22
    assert call(cand=p8) == -14 and call(loss=p4) == -14 and call(work=p4) == -14
    assert call(x=C.c_void_p(4098)) == -14 and call(x=C.c_void_p(4097), dtype=0) == -14
    wb = lib.oeh_quant_mse_work_bytes
    Cc, S, B = ops.QMSE_CHUNK, ops.QMSE_SLICE, ops.QMSE_MAX_BLOCKS
    assert wb(0, 5) == 0 and wb(5, 0) == 0 and wb(-1, -1) == 0
    assert wb(1, 1) == 8 and wb(Cc - 7, 100) == 800 and wb(Cc - 6, 100) == 1600  # (7 elements of room for a misaligned start)
    assert wb(3 * Cc + 17, S + 1) == 4 * S * 8 and wb(100, 3 * S + 5) == S * 8    # a slice at a time
    assert wb(B * Cc - 7, 2) == B * 16 and wb(B * Cc + Cc + 5, 2) == (B // 2 + 1) * 16  # above B chunks a workgroup takes several


def test_no_cpu_fallback_behind_the_op():
    from outeffhop_amd import _lib, ops

    with pytest.raises(_lib.OehError):
        ops.quant_mse(torch.randn(64), ops.quant_grid_candidates([0.1], [-128.0], [127.0]))
