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
#include "oeh_stream.h"
#include "oeh_launch.h"

namespace oeh {

// what a value becomes when it is stored in the storage type and read back
template <int IN>
__device__ __forceinline__ float round_storage(float f) {
  if constexpr (IN == IN_F32) return f;
  else return In<IN>::to_f32(In<IN>::from_f32(f));
}

template <int IN, int CH, int FORM>
__global__ __launch_bounds__(256) void oeh_resid_ln_kernel(const LnArgs p) {
  constexpr int NV = FORM == LN_SCALAR ? 1 : Vec16<IN>::N;  // elements per access
  constexpr int T = FORM == LN_WAVE ? 64 : 256;             // threads per row
  typedef typename In<IN>::elem E;
  __shared__ float red[8];
  const int t = FORM == LN_WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const long row = FORM == LN_WAVE ? (long)blockIdx.x * 4 + (threadIdx.x >> 6) : (long)blockIdx.x;
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

  // ---- sum quantiser, sum output, first moment
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = t + T * c;
    if (ch < nchunk) {
      if (p.fq_sum.en) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const float rel = fq_rel_sat(v[c][i], p.fq_sum);
          if (p.sum_idx != nullptr) p.sum_idx[row * p.cols + (long)ch * NV + i] = (unsigned char)(rel + p.fq_sum.zp);
          v[c][i] = round_storage<IN>(p.fq_sum.scale * rel);
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
  acc = wave_sum(acc);
  if constexpr (FORM != LN_WAVE) {
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    acc = (red[0] + red[1]) + (red[2] + red[3]);
  }
  const float n = (float)p.cols;
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
  const float rstd = 1.0f / __builtin_sqrtf(var + p.eps);

  // ---- affine, output quantiser, store
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = t + T * c;
    if (ch < nchunk) {
      // (loaded here, after the reductions: with gamma and beta fetched next to the row the two model shapes with the sum output measured
      // 11-12 % slower - the registers they hold cost more than the wave's second wait for memory)
      float g[NV], b[NV] = {};
      if constexpr (FORM == LN_SCALAR) {
        g[0] = p.gamma[ch];
        if (p.beta != nullptr) b[0] = p.beta[ch];
      } else {
#pragma unroll
        for (int i = 0; i < NV; i += 4) {
          const f4 gv = *reinterpret_cast<const f4*>(p.gamma + (long)ch * NV + i);
          g[i] = gv[0]; g[i + 1] = gv[1]; g[i + 2] = gv[2]; g[i + 3] = gv[3];
          if (p.beta != nullptr) {
            const f4 bv = *reinterpret_cast<const f4*>(p.beta + (long)ch * NV + i);
            b[i] = bv[0]; b[i + 1] = bv[1]; b[i + 2] = bv[2]; b[i + 3] = bv[3];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        float y = ((v[c][i] - mean) * rstd) * g[i];
        if (p.beta != nullptr) y = y + b[i];
        if (p.fq_out.en) {
          const float rel = fq_rel_sat(y, p.fq_out);
          if (p.y_idx != nullptr) p.y_idx[row * p.cols + (long)ch * NV + i] = (unsigned char)(rel + p.fq_out.zp);
          y = p.fq_out.scale * rel;
        }
        v[c][i] = y;
      }
      if constexpr (FORM == LN_SCALAR) yr[ch] = In<IN>::from_f32(v[c][0]);
      else Vec16<IN>::store(yr + (long)ch * NV, v[c]);
    }
  }
}

template <int IN, int FORM>
static int launch_ln_form(const LnArgs& a, const int ch, hipStream_t st) {
  const unsigned grid = (unsigned)(FORM == LN_WAVE ? (a.rows + 3) / 4 : a.rows);
#define OEH_LN(CH_) hipLaunchKernelGGL((oeh_resid_ln_kernel<IN, CH_, FORM>), dim3(grid), dim3(256), 0, st, a); return launch_status()
  if constexpr (FORM == LN_SCALAR) {
    switch (ch) {
      case 1: OEH_LN(1);
      case 4: OEH_LN(4);
      case 16: OEH_LN(16);
      default: OEH_LN(32);
    }
  } else if constexpr (IN == IN_F32 && FORM == LN_BLOCK) {
    switch (ch) {
      case 2: OEH_LN(2);
      case 4: OEH_LN(4);
      default: OEH_LN(8);
    }
  } else if constexpr (IN != IN_F32 && FORM == LN_WAVE) {
    switch (ch) {
      case 1: OEH_LN(1);
      default: OEH_LN(2);
    }
  } else {  // fp32 rows over a wave, 16-bit rows over a workgroup
    switch (ch) {
      case 1: OEH_LN(1);
      case 2: OEH_LN(2);
      default: OEH_LN(4);
    }
  }
#undef OEH_LN
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
