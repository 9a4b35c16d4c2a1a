// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC 2011) with the Random123 / cuRAND
// constants: the counter-based generator of the fused attention dropout (oeh_attn_bwd.hip, include/oeh.h: oeh_dropout).  Host and
// device share this one definition, so a CPU restatement (tests/test_attn_dropout_cpu.py) reproduces the device's bits.
//
// Attention dropout stream: key (seed & 0xffffffff, seed >> 32); the counter of element (b, h, i, j) - query row i, key column j of
// the logical problem - is (j >> 2, i, b * H + h, 0) and output word j & 3 belongs to it.  Keep iff word >= thr, thr =
// floor(p * 2^32) (dropout_threshold); kept elements are scaled by 1 / (1 - p) in fp32.  The mask does not depend on any tiling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oeh {

struct Philox4 {
  uint32_t x[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// thr = floor(p * 2^32) for 0 <= p < 1 (the caller validates p): a word keeps its element iff word >= thr
__host__ __device__ __forceinline__ uint32_t dropout_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }

// the four words of key columns 4 c .. 4 c + 3 of query row i in head bh = b * H + h
// (device, wave-uniform key: the opaque statement keeps the compiler from hoisting the 20 round keys out of the kernels' tile loops
// into SGPRs - they spilled - so each call forms them again with scalar adds, which issue beside the vector work)
__host__ __device__ __forceinline__ Philox4 dropout_words(uint32_t c, uint32_t i, uint32_t bh, uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(k0), "+s"(k1));
#endif
  return philox4x32_10(c, i, bh, 0u, k0, k1);
}

// Row dropout stream (oeh_ln_train.hip, include/oeh.h: oeh_drop_resid_ln_fwd): the same key; the counter of element (i, j) of a
// (rows, cols) array is (j >> 2, i & 0xffffffff, i >> 32, 1) and output word j & 3 belongs to it - the fourth counter word keeps the
// stream apart from attention dropout's under one seed.  The four words of columns 4 c .. 4 c + 3 of row i:
__host__ __device__ __forceinline__ Philox4 row_dropout_words(uint32_t c, uint64_t i, uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(k0), "+s"(k1));  // (as dropout_words: the round keys are formed again per call, not kept in SGPRs across the row loop)
#endif
  return philox4x32_10(c, (uint32_t)(i & 0xffffffffu), (uint32_t)(i >> 32), 1u, k0, k1);
}

}  // namespace oeh
