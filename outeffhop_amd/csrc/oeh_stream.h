// Device helpers of the streaming (non-attention) kernels - oeh_rows.hip, oeh_calib.hip, oeh_stats.hip, oeh_qmse.hip - and of whoever else
// reduces over a wave: 16 bytes of storage <-> fp32, the wave butterflies with the fixed four-wave step behind them, and the pieces of
// reading an array in chunks cut at its own 16-byte boundaries.  One copy each: a new storage type, or the next compiler workaround of the
// kind of oeh_common.h's f32_bits, is one edit.  Host-side launch helpers are in oeh_launch.h.  A site moves onto a helper only if every
// kernel it is compiled into keeps its instruction stream (tools/device_asm_diff.py); the sites that do not are listed, with what changes,
// in profiles/stream_helpers.txt.
#pragma once
#include "oeh_common.h"

namespace oeh {

// ---- 16 bytes of storage <-> fp32: 4 fp32 or 8 x 16-bit elements ---------------------------------------------------------------------
template <int IN>
__device__ __forceinline__ void unpack16(const u4 w, float* out) {
  if constexpr (IN == IN_F32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = bits_f32(w[i]);
  } else if constexpr (IN == IN_BF16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned u = w[i];
      out[2 * i] = bits_f32(u << 16);
      out[2 * i + 1] = bits_f32(u & 0xffff0000u);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned u = w[i];
      const h2 p = __builtin_bit_cast(h2, u);
      out[2 * i] = (float)p[0];
      out[2 * i + 1] = (float)p[1];
    }
  }
}
// (round to nearest even, one v_cvt_pk per pair)
template <int IN>
__device__ __forceinline__ u4 pack16(const float* v) {
  if constexpr (IN == IN_F32) return u4{f32_bits(v[0]), f32_bits(v[1]), f32_bits(v[2]), f32_bits(v[3])};
  else if constexpr (IN == IN_BF16) return u4{pack2_bf16(v[0], v[1]), pack2_bf16(v[2], v[3]), pack2_bf16(v[4], v[5]), pack2_bf16(v[6], v[7])};
  else return u4{pack2_f16(v[0], v[1]), pack2_f16(v[2], v[3]), pack2_f16(v[4], v[5]), pack2_f16(v[6], v[7])};
}
// one 16-byte access: N elements
template <int IN>
struct Vec16 {
  static constexpr int N = 16 / In<IN>::bytes;
  static __device__ __forceinline__ void load(const void* p, float* out) { unpack16<IN>(*reinterpret_cast<const u4*>(p), out); }
  static __device__ __forceinline__ void store(void* p, const float* v) { *reinterpret_cast<u4*>(p) = pack16<IN>(v); }
};

// ---- reductions over the 64 lanes of a wave: xor butterflies from 32 down to 1, every lane gets the result ----------------------------
// (a sum's order is part of the result: the kernels' bitwise reproducibility rests on this one)
template <class T>  // float, double, unsigned
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, m));
  return v;
}
__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, m));
  return v;
}

// The step behind them in a 256-thread workgroup: each wave's lane 0 has left its value in s[wave] of an LDS array, a barrier has passed,
// and every thread combines the four in the fixed order (0, 1), (2, 3).
__device__ __forceinline__ float block4_max(const float* s) { return __builtin_fmaxf(__builtin_fmaxf(s[0], s[1]), __builtin_fmaxf(s[2], s[3])); }
__device__ __forceinline__ float block4_min(const float* s) { return __builtin_fminf(__builtin_fminf(s[0], s[1]), __builtin_fminf(s[2], s[3])); }
__device__ __forceinline__ unsigned block4_max(const unsigned* s) { return max(max(s[0], s[1]), max(s[2], s[3])); }
__device__ __forceinline__ unsigned block4_min(const unsigned* s) { return min(min(s[0], s[1]), min(s[2], s[3])); }

// ---- an array of n elements that may start at ANY element, read in chunks of C elements cut at 16-byte boundaries of its address ---------
// The 16-byte boundary at or below `addr`; a = the elements between it and the array's first one (at most 7: chunks_for).  Chunk ch then
// starts ch * C elements behind that boundary and covers the array's elements [a, a + n) clamped to its own C (the clamp itself is
// written out in the two chunk kernels, oeh_stats.hip and oeh_qmse.hip).
__device__ __forceinline__ const char* aligned_base(const void* addr, const int elem_bytes, int& a) {
  const char* p = reinterpret_cast<const char*>(addr);
  const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 15);
  a = mis / elem_bytes;
  return p - mis;
}
// how many chunks of C elements that takes (7: the most elements an array can start after a 16-byte boundary)
inline __host__ __device__ long chunks_for(const long n, const long C) { return (n + 7 + C - 1) / C; }

// A full chunk of THREADS * K 16-byte slots into the registers of thread t: slot k * THREADS + t is the lane's k-th.  Every load is issued
// before the first value is used (unpack16 per slot afterwards: xs[k * V, (k + 1) * V) are the lane's elements of slot k).
template <int IN, int THREADS, int K>
__device__ __forceinline__ void load_chunk_full(const char* __restrict__ p, const int t, u4 (&raw)[K]) {
  constexpr int V = 16 / In<IN>::bytes;
#pragma unroll
  for (int k = 0; k < K; ++k) raw[k] = *reinterpret_cast<const u4*>(p + (size_t)((k * THREADS + t) * V) * In<IN>::bytes);
}

}  // namespace oeh
