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
// Three launch forms (ln_plan, oeh_ln_row.h): one wave per row with four rows per workgroup (rows of up to 1024 elements), one workgroup per
// row (up to 8192), both with 16-byte accesses; and one workgroup per row with element accesses for whatever is not 16-byte aligned.
// In every form thread t owns the elements of its own chunks and has loaded all of them (x and r) before its first store, and no thread
// reads an element another one writes: sum_out may be r or x, and y may be x (same row stride).
#include "oeh_ln_row.h"  // the launch forms and the row arithmetic behind the loads, shared with oeh_embed.hip and oeh_ln_train.hip

#include <cstdio>

namespace oeh {

struct LnArgs {
  const void *x, *r;              // r may be null
  const float *gamma, *beta;      // beta may be null
  void *sum, *y;                  // sum may be null
  unsigned char *sum_idx, *y_idx; // tests; may be null
  long rows;
  int cols;
  long x_stride, r_stride, sum_stride, y_stride;
  float eps;
  FqP fq_sum, fq_out;
};

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
    if (ch < nchunk) load_chunk<IN, FORM>(xr, ch, v[c]);
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

namespace {

// oeh_resid_ln_quant / oeh_resid_ln_variant: the descriptor's own refusals (no pointers), then the launch form for `vec16`
int ln_check(const oeh_ln_desc* d, bool with_sum, bool with_sum_idx, bool with_y_idx) {
  if (d == nullptr || d->cols < 1 || d->rows < 0 || !dtype_ok(d->dtype) || !(d->eps >= 0.0f) || d->reserved != 0) return OEH_EINVAL;
  if (d->x_stride < 0 || d->r_stride < 0 || d->sum_stride < 0 || d->y_stride < 0) return OEH_EINVAL;
  if (d->rows > 1 && (d->y_stride < d->cols || (with_sum && d->sum_stride < d->cols))) return OEH_EINVAL;
  if (d->fq_sum.enable && !fq_grid_ok(d->fq_sum, false)) return OEH_EINVAL;
  if (d->fq_out.enable && !fq_grid_ok(d->fq_out, false)) return OEH_EINVAL;
  if ((with_sum_idx && !d->fq_sum.enable) || (with_y_idx && !d->fq_out.enable)) return OEH_EINVAL;
  if (d->cols > kLnMaxCols || d->rows >= ((int64_t)1 << 31)) return OEH_ENOTSUP;
  if ((with_sum_idx && d->fq_sum.qmax > 255.0f) || (with_y_idx && d->fq_out.qmax > 255.0f)) return OEH_ENOTSUP;
  return OEH_OK;
}
bool ln_strides_vec16(const oeh_ln_desc* d, bool with_r, bool with_sum) {
  return rows_vec16(d->dtype, d->cols, {d->x_stride, d->y_stride, with_r ? d->r_stride : 0, with_sum ? d->sum_stride : 0});
}

}  // namespace
}  // namespace oeh

using namespace oeh;

extern "C" {

int oeh_resid_ln_quant(const oeh_ln_desc* d, const void* x, const void* r, const float* gamma, const float* beta, void* sum_out, void* y,
                       uint8_t* sum_idx, uint8_t* y_idx, void* stream) {
  if (x == nullptr || gamma == nullptr || y == nullptr) return OEH_EINVAL;
  const int rc = ln_check(d, sum_out != nullptr, sum_idx != nullptr, y_idx != nullptr);
  if (rc != OEH_OK) return rc;
  if (d->rows == 0) return OEH_OK;
  const bool vec16 = ln_strides_vec16(d, r != nullptr, sum_out != nullptr) && all16(addr(x) | addr(r) | addr(gamma) | addr(beta) | addr(sum_out) | addr(y));
  LnArgs a = {};
  a.x = x; a.r = r; a.gamma = gamma; a.beta = beta; a.sum = sum_out; a.y = y; a.sum_idx = sum_idx; a.y_idx = y_idx;
  a.rows = d->rows; a.cols = d->cols;
  a.x_stride = d->x_stride; a.r_stride = d->r_stride; a.sum_stride = d->sum_stride; a.y_stride = d->y_stride;
  a.eps = d->eps;
  a.fq_sum = make_fq(&d->fq_sum); a.fq_out = make_fq(&d->fq_out);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return launch_ln_rows(d->dtype, ln_plan(d->cols, d->dtype, vec16), d->rows, [&](auto in, auto form, auto ch, unsigned grid) {
    hipLaunchKernelGGL((oeh_resid_ln_kernel<decltype(in)::value, decltype(ch)::value, decltype(form)::value>), dim3(grid), dim3(256), 0, st, a);
  });
}

const char* oeh_resid_ln_variant(const oeh_ln_desc* d) {
  static thread_local char name[48];
  if (ln_check(d, d != nullptr && d->sum_stride != 0, false, false) != OEH_OK) return nullptr;
  const LnPlan pl = ln_plan(d->cols, d->dtype, ln_strides_vec16(d, true, true));
  std::snprintf(name, sizeof name, "ln/%s/CH%d/%s", ln_form_name(pl.form), pl.ch, dtype_name(d->dtype));
  return name;
}

}  // extern "C"
