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

namespace oeh {

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
  const unsigned b = (unsigned)row / (unsigned)p.S, s = (unsigned)row - b * (unsigned)p.S;  // (rows < 2^31: oeh_api.hip)
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

template <int IN, int FORM, int NT>
static int launch_embed_form(const EmbedArgs& a, const int ch, hipStream_t st) {
  const unsigned grid = (unsigned)(FORM == LN_WAVE ? (a.rows + 3) / 4 : a.rows);
  return dispatch_ln_ch<IN, FORM>(ch, [&](auto c) {
    hipLaunchKernelGGL((oeh_embed_kernel<IN, decltype(c)::value, FORM, NT>), dim3(grid), dim3(256), 0, st, a);
    return launch_status();
  });
}

template <int IN, int NT>
static int launch_embed_nt(const EmbedArgs& a, LnPlan pl, hipStream_t st) {
  switch (pl.form) {
    case LN_WAVE: return launch_embed_form<IN, LN_WAVE, NT>(a, pl.ch, st);
    case LN_BLOCK: return launch_embed_form<IN, LN_BLOCK, NT>(a, pl.ch, st);
    default: return launch_embed_form<IN, LN_SCALAR, NT>(a, pl.ch, st);
  }
}

int launch_embed(const EmbedArgs& a, int in, int n_tab, LnPlan pl, hipStream_t st) {
  return dispatch_in(in, [&](auto t) {
    constexpr int IN = decltype(t)::value;
    switch (n_tab) {
      case 1: return launch_embed_nt<IN, 1>(a, pl, st);
      case 2: return launch_embed_nt<IN, 2>(a, pl, st);
      default: return launch_embed_nt<IN, 3>(a, pl, st);
    }
  });
}

}  // namespace oeh
