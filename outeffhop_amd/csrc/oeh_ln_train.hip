// The tail of a transformer block in TRAINING: dropout -> residual add -> LayerNorm, forward and backward (include/oeh.h:
// oeh_drop_resid_ln_fwd / oeh_drop_resid_ln_bwd) - dense -> dropout -> + input -> LayerNorm of BertSelfOutput / BertOutput (the fp32 shape of
// quantized_bert.py:541-606) and residual + dropout(h) with the next LayerNorm behind it of the OPT decoder layer (quantized_opt.py:277-384).
// Eager, that is about seven passes over a (tokens, hidden) tensor forward, the stored dropout mask included, and as many backward plus a
// column reduction; here a row is read twice and written twice forward (x, r -> sum, y), and backward read twice (s, dy; dsum where the sum
// has a gradient of its own) and written once or twice (dx, dr), with the mask regenerated from the seed as the attention backward does.
//
// Forward: the three launch forms and the CH selection of oeh_resid_ln_quant (ln_plan, LnForm, dispatch_ln_ch), and behind the sum the SAME
// program text (oeh_ln_row.h: ln_sum_stage, ln_norm_stage with both quantisers off): with p == 0 the two entry points give the same bits.
// Per element, every operation rounded on its own (-ffp-contract=off):
//   d = keep ? fp32(x) * inv : 0,  inv = 1 / (1 - p) formed once in fp32;  s = RN_storage(d + fp32(r))  - one rounding;  sum_out <- s
//   y from the stored s as oeh_resid_ln_quant defines it (its fp32 moments);  mean[i], rstd[i] <- the row's float64 statistics, rounded to fp32 once
// Keep bit of element (i, j): oeh_philox.h: row_dropout_words - counter (j >> 2, i lo, i hi, 1), word j & 3, kept iff word >= thr.
//
// Backward, two kernels, no atomics.  Row kernel: a bounded grid (kLnTrainMaxGroups workgroups: two per CU of the 256); each workgroup -
// in the wave form each of its four waves - walks a contiguous slab of rows_per_group rows and keeps sum(dy * xhat) and sum(dy) of its
// columns in registers, in float64, with xhat for these two sums from a mean and rstd formed again from the row in float64: each entry of
// dgamma and dbeta is rounded to fp32 once, at the end of the column kernel.  Per row, fp32, with the forward's mean and rstd:
//   xhat = (s - mean) * rstd;  g = dy * gamma;  c1 = sum(g) / cols;  c2 = sum(g * xhat) / cols;  ds = rstd * ((g - c1) - xhat * c2) [+ dsum]
//   dr <- RN_storage(ds);  dx <- RN_storage(keep ? ds * inv : 0)
// and at the end one (2, cols) float64 partial per workgroup into `work` (the wave form adds its four waves' in LDS first, in a fixed order).
// Column kernel: the partials of 32 columns per workgroup, 32 slices of the workgroup list each added in order and then combined by a
// pairwise tree ((0 + 1) + (2 + 3)) + ..., into dgamma and dbeta.
// In every form thread t owns the elements of its own chunks and has loaded all of them before its first store of a row: sum_out may be r,
// y may be x, dx may be dy, dr may be dsum (same row stride).
#include "../../include/oeh.h"
#include "oeh_desc.h"
#include "oeh_ln_row.h"
#include "oeh_philox.h"

#include <algorithm>
#include <cstdio>

namespace oeh {
namespace {

constexpr int kLnTrainMaxGroups = OEH_LN_TRAIN_MAX_GROUPS;  // workgroups of the backward's row kernel
constexpr int kLnTrainSlices = 32;                          // of the partial list, per column, in the column kernel

struct DropP {
  float inv;           // 1 / (1 - p)
  unsigned thr, k0, k1;
};

struct LnTrainArgs {
  const void *x, *r;          // r may be null
  const float *gamma, *beta;  // beta may be null
  void *sum, *y;
  float *mean, *rstd;
  long rows;
  int cols;
  long x_stride, r_stride, sum_stride, y_stride;
  float eps;
  DropP drop;
};

struct LnTrainBwdArgs {
  const void *dy, *dsum, *s;  // dsum may be null
  const float *gamma, *mean, *rstd;
  void *dx, *dr;              // dr may be null
  double* work;               // (workgroups, 2, cols): sum(dy * xhat), sum(dy)
  long rows, rows_per_group;
  int cols;
  long dx_stride, dr_stride, s_stride, dy_stride, dsum_stride;
  float eps;
  DropP drop;
};

// v <- keep ? v * inv : 0 for the NV elements from column j0 of row `row` (j0 % 4 == 0 in the 16-byte forms)
template <int NV>
__device__ __forceinline__ void drop_scale(float (&v)[NV], const int j0, const long row, const DropP& d) {
  if constexpr (NV == 1) {
    const Philox4 w = row_dropout_words((unsigned)j0 >> 2, (uint64_t)row, d.k0, d.k1);
    const int k = j0 & 3;
    const unsigned word = k == 0 ? w.x[0] : k == 1 ? w.x[1] : k == 2 ? w.x[2] : w.x[3];
    v[0] = word >= d.thr ? v[0] * d.inv : 0.0f;
  } else {
#pragma unroll
    for (int i = 0; i < NV; i += 4) {
      const Philox4 w = row_dropout_words((unsigned)(j0 + i) >> 2, (uint64_t)row, d.k0, d.k1);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[i + k] = w.x[k] >= d.thr ? v[i + k] * d.inv : 0.0f;
    }
  }
}

// (load_chunk, store_chunk, load_f32: oeh_ln_row.h)  NV float64 values from / to p (16-byte aligned unless NV == 1): the backward's column partials
typedef double d2 __attribute__((ext_vector_type(2)));
template <int NV>
__device__ __forceinline__ void load_f64(const double* p, double (&out)[NV]) {
  if constexpr (NV == 1) out[0] = p[0];
  else {
#pragma unroll
    for (int i = 0; i < NV; i += 2) {
      const d2 w = *reinterpret_cast<const d2*>(p + i);
      out[i] = w[0]; out[i + 1] = w[1];
    }
  }
}
template <int NV>
__device__ __forceinline__ void store_f64(double* p, const double (&v)[NV]) {
  if constexpr (NV == 1) p[0] = v[0];
  else {
#pragma unroll
    for (int i = 0; i < NV; i += 2) *reinterpret_cast<d2*>(p + i) = d2{v[i], v[i + 1]};
  }
}

// mean and rstd = 1 / sqrt(var + eps) of the row a workgroup (a wave in the wave form) holds in v, in float64: two reductions, in the
// workgroup forms each through four LDS slots of its own and one barrier (red_m, red_v: 4 doubles each).  Every thread gets both.
template <int CH, int FORM, int NV>
__device__ __forceinline__ void row_stats64(const float (&v)[CH][NV], const int t, const int nchunk, const int cols, const float eps, double* red_m,
                                            double* red_v, double& mean64, double& rstd64) {
  constexpr int T = FORM == LN_WAVE ? 64 : 256;
  const int wave = (int)(threadIdx.x >> 6);
  double sm = 0.0;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (t + T * c < nchunk) {
#pragma unroll
      for (int i = 0; i < NV; ++i) sm += (double)v[c][i];
    }
  }
  sm = wave_sum(sm);
  if constexpr (FORM != LN_WAVE) {
    if ((t & 63) == 0) red_m[wave] = sm;
    __syncthreads();
    sm = (red_m[0] + red_m[1]) + (red_m[2] + red_m[3]);
  }
  mean64 = sm / (double)cols;
  double sv = 0.0;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (t + T * c < nchunk) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const double d = (double)v[c][i] - mean64;
        sv += d * d;
      }
    }
  }
  sv = wave_sum(sv);
  if constexpr (FORM != LN_WAVE) {
    if ((t & 63) == 0) red_v[wave] = sv;
    __syncthreads();
    sv = (red_v[0] + red_v[1]) + (red_v[2] + red_v[3]);
  }
  rstd64 = 1.0 / __builtin_sqrt(sv / (double)cols + (double)eps);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
template <int IN, int CH, int FORM, bool DROP>
__global__ __launch_bounds__(256) void oeh_ln_train_fwd_kernel(const LnTrainArgs p) {
  typedef LnForm<IN, FORM> Fm;
  constexpr int NV = Fm::NV;
  constexpr int T = Fm::T;
  typedef typename In<IN>::elem E;
  __shared__ float red[8];
  __shared__ double red_m[4], red_v[4];
  const int t = Fm::thread();
  const long row = Fm::row();
  if (FORM == LN_WAVE && row >= p.rows) return;  // (wave-uniform; this form has no workgroup barrier)
  const int nchunk = p.cols / NV;
  const E* xr = reinterpret_cast<const E*>(p.x) + row * p.x_stride;
  const E* rr = p.r != nullptr ? reinterpret_cast<const E*>(p.r) + row * p.r_stride : nullptr;
  E* sr = reinterpret_cast<E*>(p.sum) + row * p.sum_stride;
  E* yr = reinterpret_cast<E*>(p.y) + row * p.y_stride;

  // ---- the row into registers: every load of this thread before its first store
  float v[CH][NV];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = t + T * c;
    if (ch < nchunk) load_chunk<IN, FORM>(xr, ch, v[c]);
  }
  if constexpr (DROP) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = t + T * c;
      if (ch < nchunk) drop_scale<NV>(v[c], ch * NV, row, p.drop);
    }
  }
  if (rr != nullptr) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = t + T * c;
      if (ch < nchunk) {
        float w[NV];
        load_chunk<IN, FORM>(rr, ch, w);
#pragma unroll
        for (int i = 0; i < NV; ++i) v[c][i] = round_storage<IN>(v[c][i] + w[i]);
      }
    }
  } else if constexpr (DROP && IN != IN_F32) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (t + T * c < nchunk) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[c][i] = round_storage<IN>(v[c][i]);
      }
    }
  }

  const FqP off = {};
  const float acc = ln_sum_stage<IN, CH, FORM>(v, t, row, p.cols, nchunk, off, nullptr, sr);
  // the statistics handed to the backward: float64's, rounded once - the fp32 numbers next to the true mean and rstd (y below is formed
  // with the fp32 moments of ln_norm_stage, as oeh_resid_ln_quant forms it)
  double mean64, rstd64;
  row_stats64<CH, FORM, NV>(v, t, nchunk, p.cols, p.eps, red_m, red_v, mean64, rstd64);
  if (t == 0) {
    p.mean[row] = (float)mean64;
    p.rstd[row] = (float)rstd64;
  }
  ln_norm_stage<IN, CH, FORM>(v, acc, t, row, p.cols, nchunk, p.gamma, p.beta, p.eps, off, nullptr, yr, red);
}

// ---- backward: rows -----------------------------------------------------------------------------------------------------------------
template <int IN, int CH, int FORM, bool DROP>
__global__ __launch_bounds__(256) void oeh_ln_train_bwd_kernel(const LnTrainBwdArgs p) {
  typedef LnForm<IN, FORM> Fm;
  constexpr int NV = Fm::NV;
  constexpr int T = Fm::T;
  typedef typename In<IN>::elem E;
  __shared__ float red[8];                                                    // the workgroup forms' three reductions of a row, each with
  __shared__ double red_m[4], red_v[4];                                       // slots of its own: a wave a row ahead overwrites nothing unread
  __shared__ double part[FORM == LN_WAVE ? 3 * 2 * kLnWaveCols : 1];          // waves 1..3 of the wave form
  const int t = Fm::thread();
  const int wave = (int)(threadIdx.x >> 6);
  const long grp = FORM == LN_WAVE ? (long)blockIdx.x * 4 + wave : (long)blockIdx.x;
  const long row0 = grp * p.rows_per_group;
  const long row1 = row0 + p.rows_per_group < p.rows ? row0 + p.rows_per_group : p.rows;  // (a wave past the last group: no rows)
  const int nchunk = p.cols / NV;
  const float n = (float)p.cols;

  double ag[CH][NV], ab[CH][NV];  // this thread's columns: sum(dy * xhat), sum(dy) over the slab
#pragma unroll
  for (int c = 0; c < CH; ++c) {
#pragma unroll
    for (int i = 0; i < NV; ++i) ag[c][i] = ab[c][i] = 0.0;
  }

  for (long row = row0; row < row1; ++row) {
    const E* sr = reinterpret_cast<const E*>(p.s) + row * p.s_stride;
    const E* dyr = reinterpret_cast<const E*>(p.dy) + row * p.dy_stride;
    // ---- the row into registers: every load of s and dy before the first store
    float xs[CH][NV], g[CH][NV];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = t + T * c;
      if (ch < nchunk) {
        load_chunk<IN, FORM>(sr, ch, xs[c]);
        load_chunk<IN, FORM>(dyr, ch, g[c]);
      }
    }
    // ---- the row's statistics once more, in float64, for the columns' sums alone: with an fp32 rstd an entry of dgamma that one row
    // dominates inherits that rstd's rounding, which alone can exceed four times what a CPU fp32 evaluation happens to be off by
    double mean64, rstd64;
    row_stats64<CH, FORM, NV>(xs, t, nchunk, p.cols, p.eps, red_m, red_v, mean64, rstd64);

    const float mean = p.mean[row], rstd = p.rstd[row];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = t + T * c;
      if (ch < nchunk) {
        float gm[NV];
        load_f32<NV>(p.gamma + (long)ch * NV, gm);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const float xh = (xs[c][i] - mean) * rstd;
          const float dy = g[c][i];
          ab[c][i] += (double)dy;
          ag[c][i] += (double)dy * (((double)xs[c][i] - mean64) * rstd64);
          const float gg = dy * gm[i];
          s1 += gg;
          s2 += gg * xh;
          xs[c][i] = xh;
          g[c][i] = gg;
        }
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if constexpr (FORM != LN_WAVE) {
      if ((t & 63) == 0) {
        red[wave] = s1;
        red[4 + wave] = s2;
      }
      __syncthreads();
      s1 = (red[0] + red[1]) + (red[2] + red[3]);
      s2 = (red[4] + red[5]) + (red[6] + red[7]);
    }
    const float c1 = s1 / n, c2 = s2 / n;

    const E* dsr = p.dsum != nullptr ? reinterpret_cast<const E*>(p.dsum) + row * p.dsum_stride : nullptr;
    E* drr = p.dr != nullptr ? reinterpret_cast<E*>(p.dr) + row * p.dr_stride : nullptr;
    E* dxr = reinterpret_cast<E*>(p.dx) + row * p.dx_stride;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = t + T * c;
      if (ch < nchunk) {
#pragma unroll
        for (int i = 0; i < NV; ++i) g[c][i] = rstd * ((g[c][i] - c1) - xs[c][i] * c2);
        if (dsr != nullptr) {
          float w[NV];
          load_chunk<IN, FORM>(dsr, ch, w);
#pragma unroll
          for (int i = 0; i < NV; ++i) g[c][i] = g[c][i] + w[i];
        }
        if (drr != nullptr) store_chunk<IN, FORM>(drr, ch, g[c]);
        if constexpr (DROP) drop_scale<NV>(g[c], ch * NV, row, p.drop);
        store_chunk<IN, FORM>(dxr, ch, g[c]);
      }
    }
  }

  // ---- one partial per workgroup
  double* wg = p.work + (long)blockIdx.x * 2 * p.cols;
  if constexpr (FORM == LN_WAVE) {
    if (wave > 0) {
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int ch = t + T * c;
        if (ch < nchunk) {
          store_f64<NV>(part + ((wave - 1) * 2) * kLnWaveCols + ch * NV, ag[c]);
          store_f64<NV>(part + ((wave - 1) * 2 + 1) * kLnWaveCols + ch * NV, ab[c]);
        }
      }
    }
    __syncthreads();
    if (wave == 0) {
      auto combine = [&](double(&a)[NV], const int k, const int ch) {  // (wave 0 + wave 1) + (wave 2 + wave 3)
        double w1[NV], w2[NV], w3[NV];
        load_f64<NV>(part + k * kLnWaveCols + ch * NV, w1);
        load_f64<NV>(part + (2 + k) * kLnWaveCols + ch * NV, w2);
        load_f64<NV>(part + (4 + k) * kLnWaveCols + ch * NV, w3);
#pragma unroll
        for (int i = 0; i < NV; ++i) a[i] = (a[i] + w1[i]) + (w2[i] + w3[i]);
        store_f64<NV>(wg + (long)k * p.cols + ch * NV, a);
      };
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int ch = t + T * c;
        if (ch < nchunk) {
          combine(ag[c], 0, ch);
          combine(ab[c], 1, ch);
        }
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = t + T * c;
      if (ch < nchunk) {
        store_f64<NV>(wg + ch * NV, ag[c]);
        store_f64<NV>(wg + p.cols + ch * NV, ab[c]);
      }
    }
  }
}

// ---- backward: columns --------------------------------------------------------------------------------------------------------------
// (1024 threads: 32 columns x 32 slices of the partial list - with 512 partials a thread adds 16 of them, its loads in flight four at a time)
__global__ __launch_bounds__(1024) void oeh_ln_train_cols_kernel(const double* __restrict__ work, const int groups, const int cols,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ double sh[2][kLnTrainSlices][32];
  const int lane = (int)(threadIdx.x & 31), slice = (int)(threadIdx.x >> 5);
  const int col = (int)blockIdx.x * 32 + lane;
  const int per = (groups + kLnTrainSlices - 1) / kLnTrainSlices;
  const int g0 = slice * per, g1 = g0 + per < groups ? g0 + per : groups;
  double a = 0.0, b = 0.0;
  if (col < cols) {
#pragma unroll 4
    for (int g = g0; g < g1; ++g) {
      a += work[(long)g * 2 * cols + col];
      b += work[((long)g * 2 + 1) * cols + col];
    }
  }
  sh[0][slice][lane] = a;
  sh[1][slice][lane] = b;
  __syncthreads();
  if (slice < 2 && col < cols && (slice == 0 || dbeta != nullptr)) {  // slice 0: dgamma, slice 1: dbeta; a pairwise tree over the slices
    double v[kLnTrainSlices];
#pragma unroll
    for (int k = 0; k < kLnTrainSlices; ++k) v[k] = sh[slice][k][lane];
#pragma unroll
    for (int w = 1; w < kLnTrainSlices; w *= 2) {
#pragma unroll
      for (int k = 0; k < kLnTrainSlices; k += 2 * w) v[k] = v[k] + v[k + w];
    }
    (slice == 0 ? dgamma : dbeta)[col] = (float)v[0];  // the one rounding to fp32
  }
}

// ---- the keep mask (tests) ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void oeh_ln_train_mask_kernel(unsigned char* keep, const long rows, const int cols, const DropP d) {
  const long quads = (cols + 3) / 4, total = rows * quads;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long row = idx / quads;
    const int c = (int)(idx - row * quads);
    const Philox4 w = row_dropout_words((unsigned)c, (uint64_t)row, d.k0, d.k1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (4 * c + k < cols) keep[row * cols + 4 * c + k] = w.x[k] >= d.thr ? 1 : 0;
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
DropP make_drop(const oeh_dropout& drop) {
  DropP d = {};
  d.inv = 1.0f / (1.0f - drop.p);
  d.thr = dropout_threshold(drop.p);  // (p == 0: threshold 0, every element kept)
  d.k0 = (unsigned)(drop.seed & 0xffffffffu);
  d.k1 = (unsigned)(drop.seed >> 32);
  return d;
}

// p in [0, 1), NaN refused: checked before anything else of an entry point (include/oeh.h: oeh_dropout)
bool drop_bad(const oeh_dropout& drop) { return !(drop.p >= 0.0f && drop.p < 1.0f) || drop.reserved != 0; }

// the descriptor's own refusals (no pointers).  out_a / out_b: which strides belong to outputs of this direction
int check_desc(const oeh_ln_train_desc* d, const int64_t out_a, const bool with_b, const int64_t out_b) {
  if (d == nullptr) return OEH_EINVAL;
  if (drop_bad(d->drop)) return OEH_EINVAL;  // first, as oeh_dropout documents
  if (d->cols < 1 || d->rows < 0 || !dtype_ok(d->dtype) || !(d->eps >= 0.0f) || d->reserved != 0) return OEH_EINVAL;
  if (d->x_stride < 0 || d->r_stride < 0 || d->sum_stride < 0 || d->y_stride < 0 || d->dsum_stride < 0) return OEH_EINVAL;
  if (d->rows > 1 && (out_a < d->cols || (with_b && out_b < d->cols))) return OEH_EINVAL;
  if (d->cols > kLnMaxCols || d->rows >= ((int64_t)1 << 31)) return OEH_ENOTSUP;
  return OEH_OK;
}
int check_fwd(const oeh_ln_train_desc* d) { return d == nullptr ? OEH_EINVAL : check_desc(d, d->sum_stride, true, d->y_stride); }
int check_bwd(const oeh_ln_train_desc* d, const bool with_dr) { return d == nullptr ? OEH_EINVAL : check_desc(d, d->x_stride, with_dr, d->r_stride); }

bool strides_vec16(const oeh_ln_train_desc* d, const bool with_r, const bool with_dsum) {
  return rows_vec16(d->dtype, d->cols, {d->x_stride, d->sum_stride, d->y_stride, with_r ? d->r_stride : 0, with_dsum ? d->dsum_stride : 0});
}

// the backward's slabs: workgroups of the row kernel (= partials in `work`) and rows per group (a workgroup; in the wave form a wave)
struct BwdPlan {
  LnPlan ln;
  long rows_per_group, workgroups;
};
BwdPlan bwd_plan(const long rows, const int cols, const int in, const bool vec16) {
  BwdPlan b;
  b.ln = ln_plan(cols, in, vec16);
  const long per_wg = b.ln.form == LN_WAVE ? 4 : 1;
  const long max_groups = kLnTrainMaxGroups * per_wg;
  b.rows_per_group = std::max<long>(1, (rows + max_groups - 1) / max_groups);
  const long groups = (rows + b.rows_per_group - 1) / b.rows_per_group;
  b.workgroups = (groups + per_wg - 1) / per_wg;
  return b;
}

}  // namespace
}  // namespace oeh

using namespace oeh;

extern "C" {

int oeh_drop_resid_ln_fwd(const oeh_ln_train_desc* d, const void* x, const void* r, const float* gamma, const float* beta, void* sum_out, void* y,
                          float* mean, float* rstd, void* stream) {
  if (d != nullptr && drop_bad(d->drop)) return OEH_EINVAL;
  if (x == nullptr || gamma == nullptr || sum_out == nullptr || y == nullptr || mean == nullptr || rstd == nullptr) return OEH_EINVAL;
  const int rc = check_fwd(d);
  if (rc != OEH_OK) return rc;
  if (d->rows == 0) return OEH_OK;
  const bool vec16 = strides_vec16(d, r != nullptr, false) && all16(addr(x) | addr(r) | addr(gamma) | addr(beta) | addr(sum_out) | addr(y));
  LnTrainArgs a = {};
  a.x = x; a.r = r; a.gamma = gamma; a.beta = beta; a.sum = sum_out; a.y = y; a.mean = mean; a.rstd = rstd;
  a.rows = d->rows; a.cols = d->cols;
  a.x_stride = d->x_stride; a.r_stride = d->r_stride; a.sum_stride = d->sum_stride; a.y_stride = d->y_stride;
  a.eps = d->eps;
  a.drop = make_drop(d->drop);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return launch_ln_rows(d->dtype, ln_plan(d->cols, d->dtype, vec16), d->rows, [&](auto in, auto form, auto ch, unsigned grid) {
    constexpr int IN = decltype(in)::value, CH = decltype(ch)::value, FORM = decltype(form)::value;
    if (d->drop.p > 0.0f) hipLaunchKernelGGL((oeh_ln_train_fwd_kernel<IN, CH, FORM, true>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((oeh_ln_train_fwd_kernel<IN, CH, FORM, false>), dim3(grid), dim3(256), 0, st, a);
  });
}

size_t oeh_drop_resid_ln_bwd_work_bytes(const oeh_ln_train_desc* d) {
  if (check_bwd(d, false) != OEH_OK) return 0;
  // (the element form's bound: one row per group, never fewer workgroups than a 16-byte form takes)
  const long wgs = std::min<long>(std::max<long>(d->rows, 1), kLnTrainMaxGroups);
  return (size_t)wgs * 2 * (size_t)d->cols * sizeof(double);
}

int oeh_drop_resid_ln_bwd(const oeh_ln_train_desc* d, const void* dy, const void* dsum, const void* s, const float* gamma, const float* mean,
                          const float* rstd, void* dx, void* dr, float* dgamma, float* dbeta, void* work, void* stream) {
  if (d != nullptr && drop_bad(d->drop)) return OEH_EINVAL;
  if (dy == nullptr || s == nullptr || gamma == nullptr || mean == nullptr || rstd == nullptr || dx == nullptr || dgamma == nullptr || work == nullptr)
    return OEH_EINVAL;
  const int rc = check_bwd(d, dr != nullptr);
  if (rc != OEH_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d->rows == 0) {  // no row, no launch: the parameters' gradients are sums over nothing
    bool ok = hipMemsetAsync(dgamma, 0, (size_t)d->cols * sizeof(float), st) == hipSuccess;
    if (dbeta != nullptr) ok = hipMemsetAsync(dbeta, 0, (size_t)d->cols * sizeof(float), st) == hipSuccess && ok;
    return ok ? OEH_OK : OEH_ELAUNCH;
  }
  const bool vec16 = strides_vec16(d, dr != nullptr, dsum != nullptr) && all16(addr(dy) | addr(dsum) | addr(s) | addr(gamma) | addr(dx) | addr(dr) | addr(work));
  LnTrainBwdArgs a = {};
  a.dy = dy; a.dsum = dsum; a.s = s; a.gamma = gamma; a.mean = mean; a.rstd = rstd; a.dx = dx; a.dr = dr; a.work = static_cast<double*>(work);
  a.rows = d->rows; a.cols = d->cols;
  a.dx_stride = d->x_stride; a.dr_stride = d->r_stride; a.s_stride = d->sum_stride; a.dy_stride = d->y_stride; a.dsum_stride = d->dsum_stride;
  a.eps = d->eps;
  a.drop = make_drop(d->drop);
  const BwdPlan pl = bwd_plan(d->rows, d->cols, d->dtype, vec16);
  a.rows_per_group = pl.rows_per_group;
  const dim3 grid((unsigned)pl.workgroups);  // (the slabs' own grid, not a workgroup per row)
  const int rc2 = launch_ln_rows(d->dtype, pl.ln, d->rows, [&](auto in, auto form, auto ch, unsigned) {
    constexpr int IN = decltype(in)::value, CH = decltype(ch)::value, FORM = decltype(form)::value;
    if (d->drop.p > 0.0f) hipLaunchKernelGGL((oeh_ln_train_bwd_kernel<IN, CH, FORM, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((oeh_ln_train_bwd_kernel<IN, CH, FORM, false>), grid, dim3(256), 0, st, a);
  });
  if (rc2 != OEH_OK) return rc2;
  hipLaunchKernelGGL(oeh_ln_train_cols_kernel, dim3((unsigned)((d->cols + 31) / 32)), dim3(1024), 0, st, a.work, (int)pl.workgroups, d->cols, dgamma, dbeta);
  return launch_status();
}

int oeh_drop_resid_ln_mask(const oeh_ln_train_desc* d, uint8_t* keep, void* stream) {
  if (d != nullptr && drop_bad(d->drop)) return OEH_EINVAL;
  if (keep == nullptr) return OEH_EINVAL;
  if (d == nullptr || d->cols < 1 || d->rows < 0 || d->reserved != 0) return OEH_EINVAL;
  if (d->cols > kLnMaxCols || d->rows >= ((int64_t)1 << 31)) return OEH_ENOTSUP;
  if (d->rows == 0) return OEH_OK;
  const long total = d->rows * ((d->cols + 3) / 4);
  const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 16384);
  hipLaunchKernelGGL(oeh_ln_train_mask_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), keep, (long)d->rows, d->cols,
                     make_drop(d->drop));
  return launch_status();
}

const char* oeh_drop_resid_ln_variant(const oeh_ln_train_desc* d, int backward) {
  static thread_local char name[64];
  if ((backward ? check_bwd(d, true) : check_fwd(d)) != OEH_OK) return nullptr;
  // (every optional tensor taken as given and 16-byte aligned, as oeh_resid_ln_variant does)
  const bool vec16 = strides_vec16(d, true, backward != 0);
  const char* drop = d->drop.p > 0.0f ? "/drop" : "";
  if (!backward) {
    const LnPlan pl = ln_plan(d->cols, d->dtype, vec16);
    std::snprintf(name, sizeof name, "ln_train/fwd/%s/CH%d/%s%s", ln_form_name(pl.form), pl.ch, dtype_name(d->dtype), drop);
  } else {
    const BwdPlan pl = bwd_plan(std::max<long>(d->rows, 1), d->cols, d->dtype, vec16);
    std::snprintf(name, sizeof name, "ln_train/bwd/%s/CH%d/%s%s/G%ldx%ld", ln_form_name(pl.ln.form), pl.ln.ch, dtype_name(d->dtype), drop, pl.workgroups,
                  pl.rows_per_group);
  }
  return name;
}

}  // extern "C"
