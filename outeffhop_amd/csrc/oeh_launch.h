// The host side that every unit with a launcher shares: the storage-type dispatcher, the status of a launch chain, and the launchers'
// prototypes - declared HERE and nowhere else, and included by the unit that defines each of them as well as by oeh_api.hip, which calls them:
// one text for both sides (a definition whose return type drifts no longer compiles; one whose parameters drift is an unresolved symbol of
// the library, not a silently different overload behind a hand-copied declaration).  No device code: a unit that wants none of the streaming helpers (oeh_stream.h)
// includes this header alone.  (The projection GEMM's launcher lives with its parameter block: oeh_gemm.h.)
#pragma once
#include "../../include/oeh.h"
#include "oeh_attn_params.h"

#include <type_traits>

namespace oeh {

// OEH_OK, or OEH_ELAUNCH if any launch of the chain since the last look failed
inline int launch_status() { return hipGetLastError() == hipSuccess ? OEH_OK : OEH_ELAUNCH; }

// f(std::integral_constant<int, IN>{}) for the storage type `in` (anything that is not IN_F16 / IN_BF16 is fp32, as in every launcher
// before this header): dispatch_in(in, [&](auto t) { constexpr int IN = decltype(t)::value; hipLaunchKernelGGL(k<IN>, ...); });
template <class F>
inline auto dispatch_in(const int in, F&& f) {
  switch (in) {
    case IN_F16: return f(std::integral_constant<int, IN_F16>{});
    case IN_BF16: return f(std::integral_constant<int, IN_BF16>{});
    default: return f(std::integral_constant<int, IN_F32>{});
  }
}

// The callers pass a descriptor's OEH_* storage type as `in`: the ABI's values and the kernels' template arguments are the same numbers
static_assert(IN_F16 == OEH_F16 && IN_BF16 == OEH_BF16 && IN_F32 == OEH_F32, "dispatch_in[16] take an oeh_attn_desc.dtype");

// The 16-bit sibling, for kernels without an fp32-storage form (training, decode: dispatch_in would instantiate one): IN_BF16 or (anything
// else) IN_F16.  With `flag`: a second compile-time switch, f(std::integral_constant<int, IN>{}, std::bool_constant<FLAG>{})
template <class F>
inline auto dispatch_in16(const int in, F&& f) {
  return in == IN_BF16 ? f(std::integral_constant<int, IN_BF16>{}) : f(std::integral_constant<int, IN_F16>{});
}
template <class F>
inline auto dispatch_in16(const int in, const bool flag, F&& f) {
  return dispatch_in16(in, [&](auto t) { return flag ? f(t, std::true_type{}) : f(t, std::false_type{}); });
}

// oeh_attn_mfma_d*.hip, oeh_attn_fast_d*.hip, oeh_attn_flash_d*.hip
int launch_attn_mfma_d32(const AttnParams& P, int in, bool fq, hipStream_t st);
int launch_attn_mfma_d64(const AttnParams& P, int in, bool fq, hipStream_t st);
int launch_attn_mfma_d128(const AttnParams& P, int in, bool fq, hipStream_t st);
int launch_attn_fast_d32(const AttnParams& P, int in, hipStream_t st);
int launch_attn_fast_d64(const AttnParams& P, int in, hipStream_t st);
int launch_attn_fast_d128(const AttnParams& P, int in, hipStream_t st);
int launch_attn_flash_d32(const AttnParams& P, const AttnHot* hot, int in, int mq, hipStream_t st);
int launch_attn_flash_d64(const AttnParams& P, const AttnHot* hot, int in, int mq, hipStream_t st);
int launch_attn_flash_d128(const AttnParams& P, const AttnHot* hot, int in, int mq, hipStream_t st);
// oeh_attn_generic.hip, oeh_attn_small.hip, oeh_attn_i8.hip
int launch_attn_generic(const AttnParams& P, int in, hipStream_t st);
int launch_attn_small(const AttnParams& P, int in, hipStream_t st);
int launch_attn_i8(const AttnParams& P, int out, hipStream_t st);
// oeh_rows.hip
int launch_softmax_rows(const void* x, void* y, long rows, int cols, int in, int base, int clip, float w, float g, hipStream_t st);
int launch_fake_quant(const void* x, void* y, unsigned char* idx, long n, int in, FqP f, hipStream_t st);
int launch_gate(const void* hidden, int in, int B, int T, int H, int d, long hs_b, long hs_t, const float* w1, const float* b1,
                const float* w2, const float* b2, int m_units, int pool, float scaling, float* out, hipStream_t st);
int launch_minmax(const void* x, long n, int in, float* out2, hipStream_t st);
// oeh_ln.hip: residual + sum quantiser + LayerNorm + output quantiser on rows (include/oeh.h: oeh_resid_ln_quant).  The kernel's argument
// block; which of the three launch forms a problem takes and with how many accesses per thread (CH) is decided HERE, for the launch and for
// oeh_resid_ln_variant alike.
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
enum { LN_WAVE = 0, LN_BLOCK = 1, LN_SCALAR = 2 };
constexpr int kLnWaveCols = 1024, kLnMaxCols = 8192;
struct LnPlan {
  int form, ch;
};
// vec16: every base pointer is 16-byte aligned and cols and every row stride are multiples of the 16-byte vector (4 fp32 / 8 16-bit elements)
inline LnPlan ln_plan(const int cols, const int in, const bool vec16) {
  const int nv = in == IN_F32 ? 4 : 8;
  auto pow2_at_least = [](int need, int lo) { while (lo < need) lo *= 2; return lo; };
  if (!vec16) {
    const int need = (cols + 255) / 256;
    return LnPlan{LN_SCALAR, need <= 1 ? 1 : need <= 4 ? 4 : need <= 16 ? 16 : 32};
  }
  const int chunks = cols / nv;
  if (cols <= kLnWaveCols) return LnPlan{LN_WAVE, pow2_at_least((chunks + 63) / 64, 1)};
  return LnPlan{LN_BLOCK, pow2_at_least((chunks + 255) / 256, 1)};
}
int launch_resid_ln(const LnArgs& a, int in, LnPlan pl, hipStream_t st);
// oeh_embed.hip: up to three gathered table rows -> sums with their quantisers -> (LayerNorm -> output quantiser) per (b, s) of an id grid
// (include/oeh.h: oeh_embed_sum_quant).  The launch forms are ln_plan's; vec16 there also covers every table's base and row stride.
enum { TAB_PLAIN = 0, TAB_GRID = 1, TAB_I8 = 2 };
struct EmbedTab {
  const void* w;       // the table: storage type (TAB_PLAIN, TAB_GRID) or int8 indices (TAB_I8)
  const void* ids;     // null: lookup 0 reads row (b * S + s) of w ("dense rows")
  long n_rows, row_stride, id_sb, id_ss;
  int form, id64;
  float scale, lo, hi;  // the weight grid of TAB_GRID / TAB_I8: fp32 scale (rounded to the storage type in the kernel), int_min, int_max
};
struct EmbedArgs {
  EmbedTab tab[3];
  FqP fq_sum[3];                  // [t]: behind the add of lookup t (t >= 1); [0] is never enabled
  const float *gamma, *beta;      // gamma null: no LayerNorm, y is the final sum
  void *sum, *y;                  // sum may be null
  unsigned char *sum_idx, *y_idx; // tests; may be null
  int* bad_rows;                  // may be null
  long rows;
  int S, cols;
  long sum_stride, y_stride;
  float eps;
  FqP fq_out;
};
int launch_embed(const EmbedArgs& a, int in, int n_tab, LnPlan pl, hipStream_t st);
// oeh_xent.hip: cross-entropy rows over (B, S, V) logits - forward + reduce, backward (include/oeh.h: oeh_xent_fwd, oeh_xent_bwd)
struct XentArgs {
  const void *x, *labels;
  float *lse, *row_loss;  // row_loss may be null (without label smoothing)
  double* out2;           // {sum, count}: written by the reduce launch, read by the backward with mean_reduction
  float* mean;            // may be null
  double* meter;          // may be null
  int* bad_rows;          // may be null
  const float* grad;      // backward only
  void* dx;               // backward only
  long x_sb, x_ss, l_sb, l_ss, dx_sb, dx_ss, grad_stride;  // elements
  long ignore_index, rows;
  int S, V, in, label64, mean_reduction;
  float eps_ls;           // label smoothing
};
int launch_xent_fwd(const XentArgs& a, hipStream_t st);
int launch_xent_bwd(const XentArgs& a, bool el, hipStream_t st);
// oeh_stats.hip, oeh_qmse.hip
long stats_chunks(long cols);
int launch_outlier_stats(const void* x, long rows, long cols, long row_stride, int in, double eps, float* stats, double* meter, int accumulate, void* work,
                         hipStream_t st);
long qmse_blocks(long n, long* nch_out, long* cpb_out);
int launch_quant_mse(const void* x, long n, int in, const float* cand, int K, double* loss, int accumulate, void* work, hipStream_t st);
// oeh_calib.hip
int launch_percentile_ema(const void* x, long n, int in, double q_lo, double q_hi, double momentum, int first, double* state, void* work,
                          hipStream_t st);
int launch_fake_quant_range(const void* x, void* y, long n, int in, const double* range, float qmax, double eps, hipStream_t st);
int launch_attn_calibrate(const AttnParams& P, int in, int which, const double* s_range, const double* p_range, float qmax, double eps, double q_lo,
                          double q_hi, double momentum, int first, double* state, void* work, hipStream_t st);
int launch_split_pairs(const float* x, void* out, long rows, int K, long x_sr, hipStream_t st);
int launch_split_triples(const float* x, void* out, long rows, int K, long x_sr, hipStream_t st);
int launch_quantize_heads_i8(const void* x, signed char* out, void* y, long B, int S, int H, long x_sb, long x_ss, long y_sb, long y_ss, int in,
                             FqP f, int transpose, float alpha, const float* bias, hipStream_t st);

}  // namespace oeh
