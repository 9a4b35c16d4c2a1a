"""Every branch of the small-shape attention kernel (csrc/oeh_attn_small.hip: oeh_attn_small_kernel and its launcher's three forms)
against the float64 chain of tests/_attn_ref.py, at problems of at most 64 x 64.  `-m gpu`.

The kernel is forced with hook bit 10 (include/oeh_debug.h) and every case asserts the name small/ST{2,4}/D{16,32,64}/{f32,f16,bf16} on
the descriptor it launches.  Limit: |got - want64| <= 4 err64 (+ half a 16-bit ulp of want64 in 16-bit storage), err64 = max |fp32 oracle -
float64| of the case (tests/test_attn_fallback_cpu.py shows the oracle's own distance and runs these very cases without a GPU).  The ratios
are printed (-s).

Which case reaches which branch (names as in _attn_ref.SMALL_CASES, without the "small-" prefix; shapes are Sq x Sk):
  18 template instances D x ST x storage     inst0 .. inst17 (D = 16: 0-5, 32: 6-11, 64: 12-17; even: Sk <= 32 / ST2, odd: ST4; storage
                                             fp32, fp16, bf16 in pairs)
  Sk 1 3 5 15 16 17 31 32 | 33 48 63 64      inst0 2 4 6 8 10 12 14 (16: Sk 5 again) | inst1 3 5 7 (9 11 13 15 again, 17: Sk 48); Sk < 4: inst0,
                                             inst2; Sk % 4 != 0: inst0 2 4 6 10 12 and the odd ones with 33 / 63
  Sq 1 15 16 17 32 33 49 64                  instN has Sq = (1 15 16 17 32 33 49 64)[3 N % 8]: inst0 8 16 / 3 11 / 6 14 / 1 9 17 / 4 12 / 7 15 /
                                             2 10 / 5 13
  launcher form 1 (nqb == 1)                 inst0 3 6 8 11 14 16 (Sq <= 16), layout-longkv, layout-off4-f16, gamma-pos-17, cold30
  launcher form 2 (a wave per 16-row block)  nqb 2: form2-nqb2-one-problem (B H = 1), inst1 4 9 12 17; nqb 3: form2-nqb3-nine-waves (the
                                             inexact magic 2^32 / 3), inst7 15, layout-outslice; nqb 4: form2-nqb4, inst2 5 10 13, gate-head
  launcher form 3 (whole problems, nqb > 1)  form3-512x4-gamma-pos (2048 problems), form3-683x3-gate (2049); 33 x 5, D = 16: the q0 loop
                                             runs three times
  waves past the last problem                form 1: inst0 (2 waves) inst3 (9) 8 14 16; form 2: form2-nqb2-one-problem (2), form2-nqb3-nine-waves
                                             (9), inst7 (15) inst12 (18) inst17 (30); form 3: form3-683x3-gate (2049)
  H 1 3 4 (magic_h)                          inst0 5 7 9 14 16 / inst1 3 8 10 12 17 / inst2 4 6 11 13 15; form3-683x3-gate H = 3
  scale / scale = 1 / scale_div = 3          instN: N % 3 = 0 / 1 / 2; layout-fused divides too; hot60 scale = 1
  vanilla / softmax_1 / clipped / clipped softmax_1   inst0 3 8 11 16 / inst1 6 9 14 17 / inst4 7 12 15 / inst2 5 10 13
  gamma = +0.05 on padded key slots          Sk 5: form3-512x4-gamma-pos; Sk 17: gamma-pos-17; Sk 33: gamma-pos-33 (the p = 0 line: a padded key
                                             would otherwise carry gamma into the product)
  gate per token / per head (stride 0)       gate-token-ragged (17 rows: Sq % 16 != 0), form3-683x3-gate (33 rows) / gate-head (49 rows),
                                             layout-off4-bf16 (33 rows)
  (B,L,H,E) views                            layout-blhe
  k / v the first Sk rows of a longer buffer layout-longkv (the other rows are NaN: the clamped loads of key slots past Sk stay inside Sk)
  out inside a larger tensor                 layout-outslice, layout-off4-* (every element around the view keeps its guard value)
  16-bit rows 8-byte, not 16-byte aligned    layout-off4-f16, layout-off4-bf16
  q, k, v one tensor                         layout-fused
  scores near +60, exponentials underflow    hot60 (scores ~ N(0, 24^2) under softmax_1)
  scores near -30 under softmax_1            cold30 (exp(-m) ~ 1e13 dominates the denominator)

MEASURED_SMALL: 1.90 (largest |got - want64| / err64 over all cases, beyond the storage rounding: layout-blhe, D = 64 fp32; 16-bit storage <= 0.43)"""
import pytest

from oracle import oeh_oracle as O
from tests import _attn_ref as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

IDS = [c["name"] for c in A.SMALL_CASES]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


@pytest.mark.parametrize("case", A.SMALL_CASES, ids=IDS)
def test_small_shape_kernel_against_float64(ops, case):
    r = A.refs(case, O)
    name, got, _ = A.pose(ops, torch, case, r["x"])
    assert name == case["kernel"], (case["name"], name)
    ratio = A.check_exact(case, r, got)
    print(f"{case['name']} {name}: err64 {r['e_out']:.3e} ratio {ratio:.3f}")
