// What the LayerNorm-row family - the block-tail kernel (oeh_ln.hip), the embedding front (oeh_embed.hip) and the training tail
// (oeh_ln_train.hip) - shares.  Host: the launch forms (ln_plan), the one launcher over IN x FORM x CH (launch_ln_rows), the "rows are vector
// multiples" predicate and the form's name.  Device: a thread's chunk loads and stores, and the row arithmetic from the point where a thread
// holds its chunks of the summed row in registers: sum quantiser -> sum output -> first moment, then second moment -> rstd -> affine -> output
// quantiser -> store (include/oeh.h: oeh_resid_ln_quant has the formulas and their order).  One text: the kernels give the same bits for the
// same row in the same launch form, because there is no second copy of a summation order to drift.
#pragma once
#include "oeh_stream.h"
#include "oeh_launch.h"
#include "oeh_desc.h"

#include <initializer_list>

namespace oeh {

// ---- host: which of the three launch forms a problem takes and with how many accesses per thread (CH), for the launches and the
// *_variant names alike
enum { LN_WAVE = 0, LN_BLOCK = 1, LN_SCALAR = 2 };
constexpr int kLnWaveCols = 1024, kLnMaxCols = 8192;
struct LnPlan {
  int form, ch;
};
// vec16: every base pointer is 16-byte aligned and cols and every row stride are multiples of the 16-byte vector (4 fp32 / 8 16-bit elements)
inline LnPlan ln_plan(const int cols, const int in, const bool vec16) {
  const int nv = vec16_elems(in);
  auto pow2_at_least = [](int need, int lo) { while (lo < need) lo *= 2; return lo; };
  if (!vec16) {
    const int need = (cols + 255) / 256;
    return LnPlan{LN_SCALAR, need <= 1 ? 1 : need <= 4 ? 4 : need <= 16 ? 16 : 32};
  }
  const int chunks = cols / nv;
  if (cols <= kLnWaveCols) return LnPlan{LN_WAVE, pow2_at_least((chunks + 63) / 64, 1)};
  return LnPlan{LN_BLOCK, pow2_at_least((chunks + 255) / 256, 1)};
}
inline const char* ln_form_name(const int form) { return form == LN_WAVE ? "wave" : form == LN_BLOCK ? "block" : "scalar"; }
// the stride half of vec16: cols and every row stride that is in use (the caller passes 0 for one that is not) are vector multiples
inline bool rows_vec16(const int dtype, const long cols, std::initializer_list<int64_t> strides) {
  const int nv = vec16_elems(dtype);
  bool ok = cols % nv == 0;
  for (const int64_t s : strides) ok = ok && s % nv == 0;
  return ok;
}

// what a value becomes when it is stored in the storage type and read back
template <int IN>
__device__ __forceinline__ float round_storage(float f) {
  if constexpr (IN == IN_F32) return f;
  else return In<IN>::to_f32(In<IN>::from_f32(f));
}

// The geometry of a launch form: elements per access, threads per row, and which thread / row this one is
template <int IN, int FORM>
struct LnForm {
  static constexpr int NV = FORM == LN_SCALAR ? 1 : Vec16<IN>::N;
  static constexpr int T = FORM == LN_WAVE ? 64 : 256;
  static __device__ __forceinline__ int thread() { return FORM == LN_WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x; }
  static __device__ __forceinline__ long row() { return FORM == LN_WAVE ? (long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long)blockIdx.x; }
};

// chunk ch of a row of the storage type <-> NV fp32 values: one element in the scalar form, one 16-byte access otherwise.  (oeh_stream.h's rule:
// the sites below and in oeh_ln.hip / oeh_embed.hip that still spell this pair out change their kernels' instruction streams on the helper -
// profiles/entry_points.txt lists them.)
template <int IN, int FORM, int NV>
__device__ __forceinline__ void load_chunk(const typename In<IN>::elem* rowp, const int ch, float (&out)[NV]) {
  if constexpr (FORM == LN_SCALAR) out[0] = In<IN>::to_f32(rowp[ch]);
  else Vec16<IN>::load(rowp + (long)ch * NV, out);
}
template <int IN, int FORM, int NV>
__device__ __forceinline__ void store_chunk(typename In<IN>::elem* rowp, const int ch, const float (&v)[NV]) {
  if constexpr (FORM == LN_SCALAR) rowp[ch] = In<IN>::from_f32(v[0]);
  else Vec16<IN>::store(rowp + (long)ch * NV, v);
}
// NV fp32 values from p (16-byte aligned unless NV == 1)
template <int NV>
__device__ __forceinline__ void load_f32(const float* p, float (&out)[NV]) {
  if constexpr (NV == 1) out[0] = p[0];
  else {
#pragma unroll
    for (int i = 0; i < NV; i += 4) {
      const f4 w = *reinterpret_cast<const f4*>(p + i);
      out[i] = w[0]; out[i + 1] = w[1]; out[i + 2] = w[2]; out[i + 3] = w[3];
    }
  }
}

// ---- sum quantiser, sum output, first moment: returns this thread's share of sum(s); v becomes the quantised, storage-rounded sum
template <int IN, int CH, int FORM, int NV = LnForm<IN, FORM>::NV>
__device__ __forceinline__ float ln_sum_stage(float (&v)[CH][NV], const int t, const long row, const int cols, const int nchunk,
                                              const FqP& fq_sum, unsigned char* sum_idx, typename In<IN>::elem* sr) {
  constexpr int T = LnForm<IN, FORM>::T;
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = t + T * c;
    if (ch < nchunk) {
      if (fq_sum.en) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const float rel = fq_rel_sat(v[c][i], fq_sum);
          if (sum_idx != nullptr) sum_idx[row * cols + (long)ch * NV + i] = (unsigned char)(rel + fq_sum.zp);
          v[c][i] = round_storage<IN>(fq_sum.scale * rel);
        }
      }
      if (sr != nullptr) {
        if constexpr (FORM == LN_SCALAR) sr[ch] = In<IN>::from_f32(v[c][0]);
        else Vec16<IN>::store(sr + (long)ch * NV, v[c]);
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) acc += v[c][i];
    }
  }
  return acc;
}

// ---- both moments' reductions, rstd, affine, output quantiser, store.  red: 8 floats of LDS (unused by the wave form)
template <int IN, int CH, int FORM, int NV = LnForm<IN, FORM>::NV>
__device__ __forceinline__ void ln_norm_stage(float (&v)[CH][NV], float acc, const int t, const long row, const int cols, const int nchunk,
                                              const float* gamma, const float* beta, const float eps, const FqP& fq_out, unsigned char* y_idx,
                                              typename In<IN>::elem* yr, float* red) {
  constexpr int T = LnForm<IN, FORM>::T;
  acc = wave_sum(acc);
  if constexpr (FORM != LN_WAVE) {
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    acc = (red[0] + red[1]) + (red[2] + red[3]);
  }
  const float n = (float)cols;
  const float mean = acc / n;

  // ---- second moment about the mean
  float sq = 0.0f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (t + T * c < nchunk) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const float d = v[c][i] - mean;
        sq += d * d;
      }
    }
  }
  sq = wave_sum(sq);
  if constexpr (FORM != LN_WAVE) {
    if ((t & 63) == 0) red[4 + (t >> 6)] = sq;
    __syncthreads();
    sq = (red[4] + red[5]) + (red[6] + red[7]);
  }
  const float var = sq / n;
  const float rstd = 1.0f / __builtin_sqrtf(var + eps);

  // ---- affine, output quantiser, store
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = t + T * c;
    if (ch < nchunk) {
      // (loaded here, after the reductions: with gamma and beta fetched next to the row the two model shapes with the sum output measured
      // 11-12 % slower - the registers they hold cost more than the wave's second wait for memory)
      float g[NV], b[NV] = {};
      if constexpr (FORM == LN_SCALAR) {
        g[0] = gamma[ch];
        if (beta != nullptr) b[0] = beta[ch];
      } else {
#pragma unroll
        for (int i = 0; i < NV; i += 4) {
          const f4 gv = *reinterpret_cast<const f4*>(gamma + (long)ch * NV + i);
          g[i] = gv[0]; g[i + 1] = gv[1]; g[i + 2] = gv[2]; g[i + 3] = gv[3];
          if (beta != nullptr) {
            const f4 bv = *reinterpret_cast<const f4*>(beta + (long)ch * NV + i);
            b[i] = bv[0]; b[i + 1] = bv[1]; b[i + 2] = bv[2]; b[i + 3] = bv[3];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        float y = ((v[c][i] - mean) * rstd) * g[i];
        if (beta != nullptr) y = y + b[i];
        if (fq_out.en) {
          const float rel = fq_rel_sat(y, fq_out);
          if (y_idx != nullptr) y_idx[row * cols + (long)ch * NV + i] = (unsigned char)(rel + fq_out.zp);
          y = fq_out.scale * rel;
        }
        v[c][i] = y;
      }
      if constexpr (FORM == LN_SCALAR) yr[ch] = In<IN>::from_f32(v[c][0]);
      else Vec16<IN>::store(yr + (long)ch * NV, v[c]);
    }
  }
}

// ---- which CH instantiation of a form a plan's `ch` selects: f(std::integral_constant<int, CH>{}) (ln_plan gives powers of two)
template <int IN, int FORM, class F>
inline int dispatch_ln_ch(const int ch, F&& f) {
#define OEH_CH(N_) return f(std::integral_constant<int, N_>{})
  if constexpr (FORM == LN_SCALAR) {
    switch (ch) {
      case 1: OEH_CH(1);
      case 4: OEH_CH(4);
      case 16: OEH_CH(16);
      default: OEH_CH(32);
    }
  } else if constexpr (IN == IN_F32 && FORM == LN_BLOCK) {
    switch (ch) {
      case 2: OEH_CH(2);
      case 4: OEH_CH(4);
      default: OEH_CH(8);
    }
  } else if constexpr (IN != IN_F32 && FORM == LN_WAVE) {
    switch (ch) {
      case 1: OEH_CH(1);
      default: OEH_CH(2);
    }
  } else {  // fp32 rows over a wave, 16-bit rows over a workgroup
    switch (ch) {
      case 1: OEH_CH(1);
      case 2: OEH_CH(2);
      default: OEH_CH(4);
    }
  }
#undef OEH_CH
}

// ---- the launch of a plan: f(IN, FORM, CH as std::integral_constants, grid) launches the kernel instantiation; grid is a workgroup per row,
// in the wave form one per four rows (a kernel with a grid of its own ignores it)
template <class F>
inline int launch_ln_rows(const int in, const LnPlan pl, const long rows, F&& f) {
  return dispatch_in(in, [&](auto t) {
    auto go = [&](auto form) {
      constexpr int FORM = decltype(form)::value;
      const unsigned grid = (unsigned)(FORM == LN_WAVE ? (rows + 3) / 4 : rows);
      return dispatch_ln_ch<decltype(t)::value, FORM>(pl.ch, [&](auto c) {
        f(t, form, c, grid);
        return launch_status();
      });
    };
    switch (pl.form) {
      case LN_WAVE: return go(std::integral_constant<int, LN_WAVE>{});
      case LN_BLOCK: return go(std::integral_constant<int, LN_BLOCK>{});
      default: return go(std::integral_constant<int, LN_SCALAR>{});
    }
  });
}

}  // namespace oeh
