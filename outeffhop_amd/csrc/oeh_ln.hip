// The tail of a quantised transformer block in one pass over its rows: residual add -> sum quantiser -> LayerNorm -> output quantiser
// (quantized_bert.py:541-606 QuantizedBertSelfOutput / QuantizedBertOutput, quantized_opt.py:277-384 QuantizedOPTDecoderLayer, with
// QuantLayerNorm of autoquant_utils.py:64-72 / hijacker.py:78-134).  The reference runs it as four eager ops, about nine passes over a
// (B * S, E) tensor; here a row is read once, kept in registers as fp32, and written once (twice with the sum).  HBM-bound.
//
// Arithmetic per row, every operation rounded on its own (-ffp-contract=off), in this order (include/oeh.h: oeh_resid_ln_quant):
//   s = RN_storage(x + r)                                       one fp32 add, rounded once to the storage type (torch's add in that type)
//   s = RN_storage(scale * fq_rel_sat(s))                       the arithmetic of oeh_fake_quant (oeh_rows.hip) - the LayerNorm reads THIS s
//   mean = sum(s) / N;  var = sum((s - mean)^2) / N             two passes over the registers; wave butterflies, then the fixed four-wave step
//   rstd = 1 / sqrt(var + eps)                                  correctly rounded square root and division, once per row
//   y = ((s - mean) * rstd) * gamma + beta                      then the output quantiser, then RN_storage
// Three launch forms (ln_plan, oeh_launch.h): one wave per row with four rows per workgroup (rows of up to 1024 elements), one workgroup per
// row (up to 8192), both with 16-byte accesses; and one workgroup per row with element accesses for whatever is not 16-byte aligned.
// In every form thread t owns the elements of its own chunks and has loaded all of them (x and r) before its first store, and no thread
// reads an element another one writes: sum_out may be r or x, and y may be x (same row stride).
#include "oeh_ln_row.h"  // the row arithmetic behind the loads, shared with oeh_embed.hip

namespace oeh {

template <int IN, int CH, int FORM>
__global__ __launch_bounds__(256) void oeh_resid_ln_kernel(const LnArgs p) {
  typedef LnForm<IN, FORM> Fm;
  constexpr int NV = Fm::NV;  // elements per access
  constexpr int T = Fm::T;    // threads per row
  typedef typename In<IN>::elem E;
  __shared__ float red[8];
  const int t = Fm::thread();
  const long row = Fm::row();
  if (FORM == LN_WAVE && row >= p.rows) return;  // (wave-uniform; this form has no workgroup barrier)
  const int nchunk = p.cols / NV;
  const E* xr = reinterpret_cast<const E*>(p.x) + row * p.x_stride;
  const E* rr = p.r != nullptr ? reinterpret_cast<const E*>(p.r) + row * p.r_stride : nullptr;
  E* sr = p.sum != nullptr ? reinterpret_cast<E*>(p.sum) + row * p.sum_stride : nullptr;
  E* yr = reinterpret_cast<E*>(p.y) + row * p.y_stride;

  // ---- the row into registers: every load of this thread before its first store
  float v[CH][NV];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = t + T * c;
    if (ch < nchunk) {
      if constexpr (FORM == LN_SCALAR) v[c][0] = In<IN>::to_f32(xr[ch]);
      else Vec16<IN>::load(xr + (long)ch * NV, v[c]);
    }
  }
  if (rr != nullptr) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = t + T * c;
      if (ch < nchunk) {
        float w[NV];
        if constexpr (FORM == LN_SCALAR) w[0] = In<IN>::to_f32(rr[ch]);
        else Vec16<IN>::load(rr + (long)ch * NV, w);
#pragma unroll
        for (int i = 0; i < NV; ++i) v[c][i] = round_storage<IN>(v[c][i] + w[i]);
      }
    }
  }

  const float acc = ln_sum_stage<IN, CH, FORM>(v, t, row, p.cols, nchunk, p.fq_sum, p.sum_idx, sr);
  ln_norm_stage<IN, CH, FORM>(v, acc, t, row, p.cols, nchunk, p.gamma, p.beta, p.eps, p.fq_out, p.y_idx, yr, red);
}

template <int IN, int FORM>
static int launch_ln_form(const LnArgs& a, const int ch, hipStream_t st) {
  const unsigned grid = (unsigned)(FORM == LN_WAVE ? (a.rows + 3) / 4 : a.rows);
  return dispatch_ln_ch<IN, FORM>(ch, [&](auto c) {
    hipLaunchKernelGGL((oeh_resid_ln_kernel<IN, decltype(c)::value, FORM>), dim3(grid), dim3(256), 0, st, a);
    return launch_status();
  });
}

int launch_resid_ln(const LnArgs& a, int in, LnPlan pl, hipStream_t st) {
  return dispatch_in(in, [&](auto t) {
    constexpr int IN = decltype(t)::value;
    switch (pl.form) {
      case LN_WAVE: return launch_ln_form<IN, LN_WAVE>(a, pl.ch, st);
      case LN_BLOCK: return launch_ln_form<IN, LN_BLOCK>(a, pl.ch, st);
      default: return launch_ln_form<IN, LN_SCALAR>(a, pl.ch, st);
    }
  });
}

}  // namespace oeh
