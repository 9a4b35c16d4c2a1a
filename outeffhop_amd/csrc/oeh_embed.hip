// The front of a quantised transformer in one pass over its rows: up to three embedding lookups -> their sums, each behind its activation
// quantiser -> LayerNorm -> output quantiser (quantized_bert.py:146-218 QuantizedBertEmbeddings; quantized_opt.py:27-51, 549-569: embed_tokens
// + QuantizedOPTLearnedPositionalEmbedding -> embed_sum_act_quantizer, no LayerNorm; QuantEmbedding of autoquant_utils.py:75-95).  The
// reference runs it as a chain of eager ops over (B * S, E) tensors, on tables it fake-quantises as whole tensors; here a row costs its
// gathered table rows in and one row out (two with the sum).  HBM-bound; the block-tail kernel's sibling (oeh_ln.hip): the launch forms are
// ln_plan's and everything behind the last add is oeh_ln_row.h, so the two give the same bits for the same summed row.
//
// A table row arrives in one of three forms (include/oeh.h: oeh_embed_sum_quant has the order of the roundings):
//   TAB_PLAIN  storage type, taken as it is
//   TAB_GRID   storage type, the per-tensor symmetric weight grid applied to the gathered row: sc = RN(scale), e = RN(sc * clamp(rint(RN(w / sc))))
//   TAB_I8     int8 indices: e = RN(sc * idx) - a quarter of the gather traffic of an fp32 table, the same bits as TAB_GRID
// Ids are data: one outside [0, n_rows) reads nothing from its table; the row's outputs become NaN and bad_rows counts it.
// Every load of a thread (ids, table rows) is issued before its first store.
#include "oeh_ln_row.h"

#include <cmath>
#include <cstdio>

namespace oeh {

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

// thread t's chunks of row `id` of table tb, as fp32 values of the storage type IN
template <int IN, int CH, int FORM, int NV = LnForm<IN, FORM>::NV>
__device__ __forceinline__ void load_tab(const EmbedTab& tb, const long id, const int t, const int nchunk, float (&out)[CH][NV]) {
  constexpr int T = LnForm<IN, FORM>::T;
  typedef typename In<IN>::elem E;
  const float sc = round_storage<IN>(tb.scale);
  if (tb.form == TAB_I8) {
    const signed char* wr = reinterpret_cast<const signed char*>(tb.w) + id * tb.row_stride;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = t + T * c;
      if (ch < nchunk) {
        if constexpr (FORM == LN_SCALAR) {
          out[c][0] = round_storage<IN>(sc * (float)wr[ch]);
        } else {
          unsigned w[NV / 4];
          if constexpr (NV == 4) {
            w[0] = *reinterpret_cast<const unsigned*>(wr + (long)ch * NV);
          } else {
            const u2 ww = *reinterpret_cast<const u2*>(wr + (long)ch * NV);
            w[0] = ww[0]; w[1] = ww[1];
          }
#pragma unroll
          for (int i = 0; i < NV; ++i) out[c][i] = round_storage<IN>(sc * (float)((int)(w[i / 4] << (24 - 8 * (i % 4))) >> 24));
        }
      }
    }
    return;
  }
  const E* wr = reinterpret_cast<const E*>(tb.w) + id * tb.row_stride;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = t + T * c;
    if (ch < nchunk) {
      if constexpr (FORM == LN_SCALAR) out[c][0] = In<IN>::to_f32(wr[ch]);
      else Vec16<IN>::load(wr + (long)ch * NV, out[c]);
    }
  }
  if (tb.form == TAB_GRID) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (t + T * c < nchunk) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          // (a true division, as the reference's; + 0: an index is never -0, so that this form and TAB_I8 agree on the sign of a zero)
          const float q = round_storage<IN>(out[c][i] / sc);
          const float idx = __builtin_fminf(__builtin_fmaxf(__builtin_rintf(q), tb.lo), tb.hi) + 0.0f;
          out[c][i] = round_storage<IN>(sc * idx);
        }
      }
    }
  }
}

template <int IN, int CH, int FORM, int NV = LnForm<IN, FORM>::NV>
__device__ __forceinline__ void store_row(typename In<IN>::elem* dst, const float (&v)[CH][NV], const int t, const int nchunk) {
  constexpr int T = LnForm<IN, FORM>::T;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = t + T * c;
    if (ch < nchunk) {
      if constexpr (FORM == LN_SCALAR) dst[ch] = In<IN>::from_f32(v[c][0]);
      else Vec16<IN>::store(dst + (long)ch * NV, v[c]);
    }
  }
}

template <int IN, int CH, int FORM, int NT>
__global__ __launch_bounds__(256) void oeh_embed_kernel(const EmbedArgs p) {
  typedef LnForm<IN, FORM> Fm;
  constexpr int NV = Fm::NV;
  typedef typename In<IN>::elem E;
  __shared__ float red[8];
  const int t = Fm::thread();
  const long row = Fm::row();
  if (FORM == LN_WAVE && row >= p.rows) return;  // (wave-uniform; this form has no workgroup barrier)
  const int nchunk = p.cols / NV;
  const unsigned b = (unsigned)row / (unsigned)p.S, s = (unsigned)row - b * (unsigned)p.S;  // (rows < 2^31: embed_check)
  E* sr = p.sum != nullptr ? reinterpret_cast<E*>(p.sum) + row * p.sum_stride : nullptr;
  E* yr = reinterpret_cast<E*>(p.y) + row * p.y_stride;

  // ---- the row's ids: one value per lookup, the same for every thread of the row
  long id[NT];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const EmbedTab& tb = p.tab[k];
    if (tb.ids == nullptr) {
      id[k] = row;  // dense rows (lookup 0 only)
    } else {
      const long off = (long)b * tb.id_sb + (long)s * tb.id_ss;
      id[k] = tb.id64 ? reinterpret_cast<const long*>(tb.ids)[off] : (long)reinterpret_cast<const int*>(tb.ids)[off];
      bad = bad || id[k] < 0 || id[k] >= tb.n_rows;
    }
  }
  float v[CH][NV];
  if (bad) {  // (uniform over the row's threads) nothing is read from any table; the row's outputs say so
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[c][i] = __builtin_nanf("");
    }
    if (sr != nullptr) store_row<IN, CH, FORM>(sr, v, t, nchunk);
    store_row<IN, CH, FORM>(yr, v, t, nchunk);
    if (t == 0 && p.bad_rows != nullptr) atomicAdd(p.bad_rows, 1);
    return;
  }

  // ---- the gathered rows into registers, then the sums in lookup order, each add rounded to the storage type, each behind its quantiser
  float e[NT > 1 ? NT - 1 : 1][CH][NV];
  load_tab<IN, CH, FORM>(p.tab[0], id[0], t, nchunk, v);
#pragma unroll
  for (int k = 1; k < NT; ++k) load_tab<IN, CH, FORM>(p.tab[k], id[k], t, nchunk, e[k - 1]);
#pragma unroll
  for (int k = 1; k < NT; ++k) {
    const bool mid = k < NT - 1 && p.fq_sum[k].en;  // (the last sum's quantiser is ln_sum_stage's, with its index dump)
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (t + Fm::T * c < nchunk) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          float x = round_storage<IN>(v[c][i] + e[k - 1][c][i]);
          if (mid) x = round_storage<IN>(p.fq_sum[k].scale * fq_rel_sat(x, p.fq_sum[k]));
          v[c][i] = x;
        }
      }
    }
  }

  const float acc = ln_sum_stage<IN, CH, FORM>(v, t, row, p.cols, nchunk, p.fq_sum[NT - 1], p.sum_idx, sr);
  if (p.gamma == nullptr) {  // (uniform) OPT: no LayerNorm, y is the final sum
    store_row<IN, CH, FORM>(yr, v, t, nchunk);
    return;
  }
  ln_norm_stage<IN, CH, FORM>(v, acc, t, row, p.cols, nchunk, p.gamma, p.beta, p.eps, p.fq_out, p.y_idx, yr, red);
}

namespace {

template <int NT>
int launch_embed_nt(const EmbedArgs& a, const int in, const LnPlan pl, hipStream_t st) {
  return launch_ln_rows(in, pl, a.rows, [&](auto t, auto form, auto ch, unsigned grid) {
    hipLaunchKernelGGL((oeh_embed_kernel<decltype(t)::value, decltype(ch)::value, decltype(form)::value, NT>), dim3(grid), dim3(256), 0, st, a);
  });
}

// oeh_embed_sum_quant / oeh_embed_sum_variant: every refusal in the order OEH_EINVAL -> OEH_ENOTSUP -> OEH_EALIGN, then whether the 16-byte forms apply
int embed_check(const oeh_embed_desc* d, const float* gamma, const float* beta, const void* sum_out, const void* y, bool with_sum_idx,
                bool with_y_idx, bool* vec16) {
  if (d == nullptr || y == nullptr || d->n_tab < 1 || d->n_tab > 3 || d->cols < 1 || d->B < 0 || d->S < 0 || !dtype_ok(d->dtype)) return OEH_EINVAL;
  if (d->reserved != 0 || d->reserved2 != 0 || d->sum_stride < 0 || d->y_stride < 0) return OEH_EINVAL;
  const int64_t rows = (int64_t)d->B * d->S;
  if (rows > 1 && (d->y_stride < d->cols || (sum_out != nullptr && d->sum_stride < d->cols))) return OEH_EINVAL;
  for (int t = 0; t < d->n_tab; ++t) {
    const oeh_embed_lookup& l = d->tab[t];
    if (l.table == nullptr || (t >= 1 && l.ids == nullptr) || l.reserved != 0) return OEH_EINVAL;
    if (l.ids == nullptr && l.n_rows < rows) return OEH_EINVAL;  // dense rows: one per (b, s)
    if (l.n_rows < 0 || l.row_stride < 0 || l.id_stride_b < 0 || l.id_stride_s < 0) return OEH_EINVAL;
    if ((l.id_dtype != OEH_ID_I32 && l.id_dtype != OEH_ID_I64) || l.form < OEH_TAB_PLAIN || l.form > OEH_TAB_I8) return OEH_EINVAL;
    if (l.form != OEH_TAB_PLAIN && (!(l.scale > 0.0f) || !std::isfinite(l.scale) || !(l.int_min < l.int_max))) return OEH_EINVAL;
  }
  for (int t = 0; t < 3; ++t) {
    if (d->fq_sum[t].enable && (t == 0 || t >= d->n_tab || !fq_grid_ok(d->fq_sum[t], false))) return OEH_EINVAL;
  }
  if (d->fq_out.enable && !fq_grid_ok(d->fq_out, false)) return OEH_EINVAL;
  if (gamma == nullptr && (beta != nullptr || d->fq_out.enable || with_y_idx)) return OEH_EINVAL;
  if ((with_sum_idx && !d->fq_sum[d->n_tab - 1].enable) || (with_y_idx && !d->fq_out.enable)) return OEH_EINVAL;
  if (gamma != nullptr && !(d->eps >= 0.0f)) return OEH_EINVAL;
  if (d->cols > kLnMaxCols || rows >= ((int64_t)1 << 31)) return OEH_ENOTSUP;
  for (int t = 0; t < d->n_tab; ++t) {
    if (d->tab[t].form == OEH_TAB_I8 && (d->tab[t].int_min < -128.0f || d->tab[t].int_max > 127.0f)) return OEH_ENOTSUP;
  }
  if ((with_sum_idx && d->fq_sum[d->n_tab - 1].qmax > 255.0f) || (with_y_idx && d->fq_out.qmax > 255.0f)) return OEH_ENOTSUP;
  const int eb = elem_bytes(d->dtype), nv = vec16_elems(d->dtype);
  bool v16 = rows_vec16(d->dtype, d->cols, {d->y_stride, sum_out != nullptr ? d->sum_stride : 0}) && all16(addr(gamma) | addr(beta) | addr(sum_out) | addr(y));
  for (int t = 0; t < d->n_tab; ++t) {
    const oeh_embed_lookup& l = d->tab[t];
    if (l.ids != nullptr && addr(l.ids) % (l.id_dtype == OEH_ID_I64 ? 8 : 4) != 0) return OEH_EALIGN;
    if (addr(l.table) % (l.form == OEH_TAB_I8 ? 4 : eb) != 0) return OEH_EALIGN;
    // (an int8 row is read nv BYTES at a time; a float row nv elements = 16 bytes)
    v16 = v16 && rows_vec16(d->dtype, d->cols, {l.row_stride}) && (l.form == OEH_TAB_I8 ? addr(l.table) % nv == 0 : all16(addr(l.table)));
  }
  if (addr(y) % eb != 0 || addr(sum_out) % eb != 0 || addr(gamma) % 4 != 0 || addr(beta) % 4 != 0) return OEH_EALIGN;
  *vec16 = v16;
  return OEH_OK;
}

}  // namespace
}  // namespace oeh

using namespace oeh;

extern "C" {

int oeh_embed_sum_quant(const oeh_embed_desc* d, const float* gamma, const float* beta, void* sum_out, void* y, uint8_t* sum_idx, uint8_t* y_idx,
                        int32_t* bad_rows, void* stream) {
  bool vec16 = false;
  const int rc = embed_check(d, gamma, beta, sum_out, y, sum_idx != nullptr, y_idx != nullptr, &vec16);
  if (rc != OEH_OK) return rc;
  if (addr(bad_rows) % 4 != 0) return OEH_EALIGN;
  if ((int64_t)d->B * d->S == 0) return OEH_OK;
  EmbedArgs a = {};
  for (int t = 0; t < d->n_tab; ++t) {
    const oeh_embed_lookup& l = d->tab[t];
    a.tab[t] = EmbedTab{l.table, l.ids, l.n_rows, l.row_stride, l.id_stride_b, l.id_stride_s, l.form, l.id_dtype == OEH_ID_I64, l.scale, l.int_min, l.int_max};
    a.fq_sum[t] = make_fq(&d->fq_sum[t]);
  }
  a.gamma = gamma; a.beta = beta; a.sum = sum_out; a.y = y; a.sum_idx = sum_idx; a.y_idx = y_idx; a.bad_rows = bad_rows;
  a.rows = (long)d->B * d->S; a.S = d->S; a.cols = d->cols;
  a.sum_stride = d->sum_stride; a.y_stride = d->y_stride;
  a.eps = d->eps;
  a.fq_out = make_fq(&d->fq_out);
  const LnPlan pl = ln_plan(d->cols, d->dtype, vec16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (d->n_tab) {
    case 1: return launch_embed_nt<1>(a, d->dtype, pl, st);
    case 2: return launch_embed_nt<2>(a, d->dtype, pl, st);
    default: return launch_embed_nt<3>(a, d->dtype, pl, st);
  }
}

const char* oeh_embed_sum_variant(const oeh_embed_desc* d) {
  static thread_local char name[48];
  bool vec16 = false;
  // (the outputs and gamma / beta are taken as given with every part and 16-byte aligned, as oeh_resid_ln_variant does)
  const void* const aligned = reinterpret_cast<const void*>((uintptr_t)4096);
  if (embed_check(d, static_cast<const float*>(aligned), nullptr, d != nullptr && d->sum_stride != 0 ? aligned : nullptr, aligned, false, false, &vec16) != OEH_OK)
    return nullptr;
  const LnPlan pl = ln_plan(d->cols, d->dtype, vec16);
  std::snprintf(name, sizeof name, "embed/%s/CH%d/T%d/%s", ln_form_name(pl.form), pl.ch, d->n_tab, dtype_name(d->dtype));
  return name;
}

}  // extern "C"
