"""Quantisation-error search on the GPU (include/oeh.h: oeh_quant_mse; outeffhop_amd/csrc/oeh_qmse.hip) against numpy on the exact values
the kernel read: fp32 terms, float64 sum.  C = ops.QMSE_CHUNK, S = ops.QMSE_SLICE, B = ops.QMSE_MAX_BLOCKS, F = ops.QMSE_F64_K.

  case                                    kernel / path                                              host condition
  --------------------------------------  ---------------------------------------------------------  ------------------------------
  n 1, 3, 255, C - 1 (16-byte start)      one edge chunk (element loads), a second, EMPTY chunk      n + 7 > C
                                          from C - 6 on
  n C (16-byte start)                     the whole-slot body + an empty chunk                       a chunk lies inside the array
  n C + 1, 3C + 17                        whole-slot chunks + an edge chunk, merge over workgroups
  x[1:]                                   edge FIRST chunk: nothing before the view is read          address % 16 != 0
  n B * C + C + 5                         two chunks per workgroup, float64 slots added in LDS       more than B chunks
  n 2^31 + 4099                           257 chunks per workgroup, 64-bit element offsets
  K 1, 2                                  float64 sums from the first term                           K <= F
  K 7, 100                                32 terms pairwise in fp32, then float64                    F < K <= S
  K S + 1, 3S + 5                         2 / 4 slices: a pass and a merge each, `work` reused       K > S

Limit: |loss - L64| <= 6 * 2^-24 * L64 (include/oeh.h), L64 the float64 sum of the fp32 terms; exact 0 where every term is 0.
Every test prints the largest error it saw (pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.test_mse_estimator_cpu import GOLDEN_CASES, GRID_CASES, XATOL, make_estimator

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mse_ranges.npz")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
KINDS = ("normal", "student_t3", "outlier_columns")
BOUND = 6 * 2.0 ** -24


def consts():
    from outeffhop_amd import ops

    return ops.QMSE_CHUNK, ops.QMSE_SLICE, ops.QMSE_MAX_BLOCKS, ops.QMSE_F64_K


def draw(gen, kind, n, dtype):
    """n values of `dtype` as a CPU tensor: what the kernel will read."""
    x = torch.randn(n, generator=gen, dtype=torch.float64)
    if kind == "student_t3":
        x = x / torch.sqrt((torch.randn(3, n, generator=gen, dtype=torch.float64) ** 2).sum(0) / 3.0)
    if kind == "outlier_columns":
        x[3::16] *= 60.0
    return x.to(dtype)


def candidates(K, seed=0):
    """K grids, as (K, 4) float32: the seven kinds below in turn, with scales that vary from one to the next."""
    rs = np.random.RandomState(seed)
    rows = []
    for k in range(K):
        s = np.float32(0.004 * (1.0 + 3.0 * rs.rand()))
        kind = k % 7
        if kind == 0:
            rows.append((s * 8, -128.0, 127.0))          # symmetric, signed
        elif kind == 1:
            rows.append((s * 4, 0.0, 255.0))             # symmetric, unsigned
        elif kind == 2:
            zp = float(rs.randint(1, 255))
            rows.append((s * 6, -zp, 255.0 - zp))        # asymmetric with a zero point
        elif kind == 3:
            rows.append((s * 100, -8.0, 7.0))            # 4 bits
        elif kind == 4:
            rows.append((s / 64, -32768.0, 32767.0))     # 16 bits
        elif kind == 5:
            rows.append((1e-9, -128.0, 127.0))           # saturating: every index at a limit
        else:
            rows.append((1e6 * (1 + k), 0.0, 65535.0))   # far above the data: every index 0, the loss is sum x^2
    return np.array([r + (0.0,) for r in rows], dtype=np.float32)


def oracle(x, cand):
    """x: CPU tensor of the storage dtype; the fp32 terms of include/oeh.h, one candidate after the other, summed in float64."""
    x = x.float().numpy()
    out = np.empty(len(cand), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k, (s, lo, hi, _) in enumerate(cand):
            y = s * np.clip(np.rint(x / s), lo, hi)
            d = x - y
            out[k] = (d * d).astype(np.float64).sum()
    return out


def run(v, cand, loss=None, accumulate=0):
    """oeh_quant_mse on the 1-D view `v` AS IT LIES in memory; loss (unless given) and work pre-filled with NaN."""
    from outeffhop_amd import _lib, ops

    lib = _lib.load()
    K = len(cand)
    c = torch.from_numpy(np.ascontiguousarray(cand)).cuda()
    if loss is None:
        loss = torch.full((K,), float("nan"), dtype=torch.float64, device="cuda")
    nbytes = lib.oeh_quant_mse_work_bytes(v.numel(), K)
    work = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda")
    assert v.is_contiguous() and nbytes >= 8
    rc = lib.oeh_quant_mse(C.c_void_p(v.data_ptr()), v.numel(), ops._DT[v.dtype], C.c_void_p(c.data_ptr()), K, C.c_void_p(loss.data_ptr()), accumulate,
                           C.c_void_p(work.data_ptr()), ops._stream())
    assert rc == 0, rc
    return loss


def check(got, want, what):
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), what
    err = np.abs(got - want) / np.where(want > 0, want, 1.0)
    assert (err <= BOUND).all() and (got[want == 0] == 0).all(), (what, float(err.max()))
    return float(err.max())


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f16", "bf16"))
def test_every_size_against_float64(dtype):
    """Both summation forms (K = 2 and K = 7) at every size class and for a view that starts one element past a 16-byte boundary."""
    Cc, S, B, F = consts()
    gen = torch.Generator().manual_seed(1)
    worst = 0.0
    for i, n in enumerate((1, 3, 255, Cc - 1, Cc, Cc + 1, 3 * Cc + 17)):
        x = draw(gen, KINDS[i % 3], n + 1, dtype)
        xg = x.cuda()
        for K in (2, 7):
            cand = candidates(K, seed=n)
            assert (K <= F) == (K == 2)
            worst = max(worst, check(run(xg[:n].clone(), cand), oracle(x[:n], cand), (n, K)))
            v = xg[1:]
            assert v.data_ptr() % 16 == x.element_size()
            worst = max(worst, check(run(v, cand), oracle(x[1:], cand), (n, K, "offset")))
    print(f"quant_mse {dtype}: max rel err {worst:.2e} (limit {BOUND:.2e})")


@pytest.mark.parametrize("kind", KINDS)
def test_every_candidate_count_against_float64(kind):
    """K = 1 ... 3S + 5 (one to four slices) on two chunks and a bit, every grid kind in turn."""
    Cc, S, B, F = consts()
    gen = torch.Generator().manual_seed(2)
    dtype = DTYPES[KINDS.index(kind)]
    x = draw(gen, kind, Cc + 1001, dtype) * (300.0 if kind == "normal" else 1.0)  # (normal: |x| ~ 1e3 against the saturating scale 1e-9)
    xg = x.cuda()
    worst = 0.0
    for K in (1, 2, 100, S + 1, 3 * S + 5):
        cand = candidates(K, seed=K)
        want = oracle(x, cand)
        worst = max(worst, check(run(xg, cand), want, (kind, K)))
        if K >= 7:  # the far-too-large scale: every index is 0 and the loss is the sum of squares
            assert np.isclose(want[6], (x.double() ** 2).sum().item(), rtol=1e-6)
    print(f"quant_mse {kind} {dtype}: max rel err {worst:.2e} (limit {BOUND:.2e})")


def test_zero_losses_are_exact_and_inf_propagates():
    Cc, S, B, F = consts()
    n = 2 * Cc + 77
    for K in (3, 9):
        cand = candidates(K, seed=5)
        z = torch.zeros(n, dtype=torch.float16, device="cuda")
        assert (run(z, cand) == 0).all()
        # every element on one point of every grid: 96 * scale_k is not one value, so one candidate at a time
        for k in range(K):
            s, lo, hi, _ = cand[k]
            point = np.float32(s) * np.float32(min(max(5.0, lo), hi))
            xs = torch.full((n,), float(point), dtype=torch.float32, device="cuda")
            assert (run(xs, cand[k:k + 1].repeat(K, 0)) == 0).all()
    # one +inf element: every loss is inf (no grid reaches it), the call returns normally
    gen = torch.Generator().manual_seed(3)
    x = draw(gen, "normal", n, torch.float32)
    x[Cc + 5] = float("inf")
    for K in (2, 9):
        got = run(x.cuda(), candidates(K, seed=6))
        assert torch.isinf(got).all() and (got > 0).all()
    x[7] = float("nan")
    assert torch.isnan(run(x.cuda(), candidates(9, seed=6))).all()


def test_many_chunks_per_workgroup():
    """More than B chunks: a workgroup takes two chunks and adds them in its float64 LDS slots (every element random)."""
    Cc, S, B, F = consts()
    n = B * Cc + Cc + 5
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, generator=gen, dtype=torch.float32).to(torch.float16)
    x[3::16] *= 60.0
    xg = x.cuda()
    for K in (2, 5):
        cand = candidates(K, seed=8)
        print(f"quant_mse n = {n}, K = {K}: max rel err {check(run(xg, cand), oracle(x, cand), (n, K)):.2e}")


def test_elements_beyond_2_to_the_31():
    """4.3 GB of fp16: zeros, except 4099 random elements from 2^31 on.  Their terms are the whole loss of a grid that contains 0."""
    Cc, S, B, F = consts()
    n, tail = 2 ** 31 + 4099, 4099
    gen = torch.Generator().manual_seed(5)
    t = draw(gen, "student_t3", tail, torch.float16)
    x = torch.zeros(n, dtype=torch.float16, device="cuda")
    x[n - tail:] = t.cuda()
    for K in (1, 7):
        cand = candidates(K, seed=9)
        print(f"quant_mse n = 2^31 + {tail}, K = {K}: max rel err {check(run(x, cand), oracle(t, cand), (n, K)):.2e}")
    del x
    torch.cuda.empty_cache()


def bits(t):
    return t.cpu().numpy().view(np.int64)


def test_accumulate_overwrite_reproducible_and_graph_capture():
    from outeffhop_amd import ops

    Cc, S, B, F = consts()
    gen = torch.Generator().manual_seed(6)
    for n, dtype, K in ((3 * Cc + 17, torch.float16, S + 1), (Cc + 1, torch.float32, 2), (255, torch.bfloat16, 100)):
        x1, x2 = draw(gen, "student_t3", n, dtype).cuda(), draw(gen, "outlier_columns", n, dtype).cuda()
        cand = candidates(K, seed=n)
        a, a2, b = run(x1, cand), run(x1, cand), run(x2, cand)
        assert np.array_equal(bits(a), bits(a2)), "two calls, bitwise"
        loss = torch.full((K,), 1e300, dtype=torch.float64, device="cuda")
        run(x1, cand, loss=loss)                      # without accumulate the prior contents are overwritten
        assert np.array_equal(bits(loss), bits(a))
        run(x2, cand, loss=loss, accumulate=1)        # one float64 add
        assert np.array_equal(bits(loss), bits(a + b))
        cg = torch.from_numpy(cand).cuda()
        eager = ops.quant_mse(x1, cg)
        assert np.array_equal(bits(eager), bits(a)), "ops.quant_mse is the same call"
        acc = torch.zeros(K, dtype=torch.float64, device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = ops.quant_mse(x1, cg)
            ops.quant_mse(x2, cg, acc, accumulate=True)
        acc.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(a)) and np.array_equal(bits(acc), bits(b)), "graph replay"
    # a view that is not dense is made contiguous; a dense one is read where it lies
    x = draw(gen, "normal", 2 * 777, torch.float32).cuda().view(777, 2)
    cg = torch.from_numpy(candidates(5)).cuda()
    assert np.array_equal(bits(ops.quant_mse(x[:, 0], cg)), bits(ops.quant_mse(x[:, 0].contiguous(), cg)))
    assert np.array_equal(bits(ops.quant_mse(x.view(-1)[1:], cg)), bits(run(x.view(-1)[1:], candidates(5))))
    with pytest.raises(ValueError):
        ops.quant_mse(x, cg[:, :3])


# ---- the estimator on GPU tensors
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", GRID_CASES)
def test_grid_search_on_the_gpu_chooses_the_reference_ranges(golden, name):
    """The recorded fp32 batches on the GPU: the reference's (xmin, xmax) exactly after each batch, the loss array within the
    kernel's contract of the CPU path's (float64 sums of the same terms); then the fp16 and bf16 roundings of the same batches: the
    ranges of this package's CPU path on the same 16-bit data."""
    x = torch.from_numpy(golden[f"x_{name}"])
    est, ref = make_estimator(golden, name), make_estimator(golden, name)
    for b in range(2):
        lo, hi = est(x[b].cuda())
        ref(x[b])
        assert lo.is_cuda and lo.dtype == torch.float32 and lo.shape == (1,)
        assert float(lo) == float(golden[f"xmin_{name}"][b]) and float(hi) == float(golden[f"xmax_{name}"][b])
        got, want = est.loss_array[0].cpu().numpy().reshape(-1), ref.loss_array[0].numpy().reshape(-1)
        assert est.loss_array.is_cuda and np.array_equal(np.isinf(got), np.isinf(want))
        fin = np.isfinite(want)
        assert (np.abs(got[fin] - want[fin]) <= BOUND * want[fin]).all()
    for dtype in (torch.float16, torch.bfloat16):
        est, ref = make_estimator(golden, name), make_estimator(golden, name)
        for b in range(2):
            x16 = x[b].to(dtype)
            lo, hi = est(x16.cuda())
            rlo, rhi = ref(x16)
            assert float(lo) == float(rlo) and float(hi) == float(rhi), (name, dtype, b)


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_section_on_the_gpu_matches_the_cpu_path(golden, name):
    pytest.importorskip("scipy")
    x = torch.from_numpy(golden[f"x_{name}"])
    est, ref = make_estimator(golden, name), make_estimator(golden, name)
    for b in range(2):
        lo, hi = est(x[b].cuda())
        rlo, rhi = ref(x[b])
        print(f"{name} batch {b}: GPU vs CPU path |dxmin| {abs(float(lo) - float(rlo)):.2e} |dxmax| {abs(float(hi) - float(rhi)):.2e}")
        assert abs(float(lo) - float(rlo)) <= XATOL and abs(float(hi) - float(rhi)) <= XATOL


def test_attention_module_calibrates_with_mse_ranges():
    """A small quantised OPT attention (E = 64, H = 2, S = 32): weights by RangeEstimators.MSE / grid, activations by RangeEstimators.MSE /
    golden section.  Calibration on two batches takes the observable path (the fused calibration serves percentile estimators only),
    fix_ranges, and the evaluation runs the fused path; its outputs lie on the output quantiser's grid.  For every quantiser the error
    of the MSE range on the data it saw last is no larger than the error of that data's min-max range.

    Weights and activations are quantised to 4 bits, and the weights are N(0, 0.05) with every 97th entry x 6: at 16 levels the clipped
    range wins by a wide margin (loss ratios 0.2 ... 0.9 over six seeds of the same tensors by the CPU path).  At 8 bits on these 2048 ...
    4096 samples the two losses lie within 2 % of each other and either can be the smaller: the bounded search stops in a local minimum of
    a piecewise loss (ratios 0.985 ... 1.019 over four seeds), and for uniformly distributed weights no candidate of the 100-step grid,
    spaced (max |w| + 0.5) / 100 apart, beats the min-max range, which is not a candidate itself (measured 3.2702e-4 against 3.2691e-4).
    No attention mask: the masked scores hold finfo.min, whose squared error is not finite in fp32 - in the reference as here."""
    pytest.importorskip("scipy")
    import outeffhop_amd as oa
    from outeffhop_amd.quantization import MSE_Estimator, OptMethod, QuantizationManager, RangeEstimators

    E, H, S, Bt = 64, 2, 32, 2
    torch.manual_seed(21)
    dev = torch.device("cuda:0")
    org = oa.OPTAttentionWithExtras(E, H, is_decoder=True, softmax_fn=oa.SOFTMAX_MAPPING["softmax1"])
    with torch.no_grad():
        for lin in (org.q_proj, org.k_proj, org.v_proj, org.out_proj):
            w = torch.randn(E, E) * 0.05
            w.view(-1)[::97] *= 6.0
            lin.weight.copy_(w)
    cfg = oa.get_quant_config()
    cfg.quant.n_bits = cfg.quant.n_bits_act = 4
    cfg.quant.weight_quant_method = RangeEstimators.MSE
    cfg.quant.weight_opt_method = OptMethod.grid
    cfg.act_quant.quant_method = RangeEstimators.MSE
    cfg.act_quant.options = dict(opt_method=OptMethod.golden_section)
    qm = oa.QuantizedOPTAttentionWithExtras(org.to(dev), **{**oa.val_qparams(cfg), "quant_dict": {}}).to(dev).eval()
    qm.set_quant_state(weight_quant=True, act_quant=True)
    mgrs = {n: m for n, m in qm.named_modules() if isinstance(m, QuantizationManager)}
    assert len(mgrs) == 11 and all(isinstance(m.range_estimator, MSE_Estimator) and m.n_bits == 4 for m in mgrs.values())
    seen = {}
    hooks = [m.register_forward_pre_hook(lambda mod, args, n=n: seen.__setitem__(n, args[0].detach().clone())) for n, m in mgrs.items()]
    with torch.no_grad():
        for _ in range(2):
            x = torch.randn(Bt, S, E, device=dev)
            x[..., 7] *= 12.0
            qm(x)
        assert qm.__dict__.get("_fused_calib_calls", 0) == 0, "MSE estimators need the tensors: the observable path"
        for h in hooks:
            h.remove()
        qm.fix_ranges()
        assert qm._fq(True) is not None, "the three attention quantisers are fixed: the evaluation is the fused kernel"
        out = qm(x)[0]
    oq = qm.out_proj.activation_quantizer.quantizer
    idx = out.float() / float(oq.scale)
    assert float((idx - torch.round(idx)).abs().max()) < 1e-3 and idx.max() - idx.min() <= 15  # the outputs lie on the output grid
    assert {"attn_scores_act_quantizer", "attn_probs_act_quantizer", "context_act_quantizer"} <= {n.split(".")[0] for n in seen}
    assert sum(n.endswith("weight_quantizer") for n in seen) == 4
    for n, data in seen.items():
        est = mgrs[n].range_estimator
        lo, hi = float(est.current_xmin), float(est.current_xmax)
        rows = est.candidate_rows([lo, float(data.min())], [hi, float(data.max())]).numpy()
        mse, minmax = oracle(data.reshape(-1).cpu(), rows)
        print(f"{n}: range ({lo:.4g}, {hi:.4g}) of data in ({float(data.min()):.4g}, {float(data.max()):.4g}): loss {mse:.4g} against min-max {minmax:.4g}")
        assert mse <= minmax, n
