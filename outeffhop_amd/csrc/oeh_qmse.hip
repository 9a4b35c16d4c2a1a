// Quantisation-error search: the squared error of K candidate quantiser grids on one array, every candidate from one read of the
// data (include/oeh.h: oeh_quant_mse).
//
// The reference's MSE range estimator (quantization/range_estimators.py:109-395) calls loss_fx once per candidate range: fake-quantise,
// subtract, square, sum, .cpu() - six eager passes over the tensor and a host synchronisation, 100 times per tensor and batch in the
// 1-D search, 100 * 64 * 2 times in the 2-D search.  Here:
//
//   * The flat array is cut into chunks of kQmseC elements at 16-byte boundaries of its own address (it may start at any element).  A
//     workgroup keeps a chunk in registers as fp32 - kQmseLane floats per lane, loaded as 16-byte vectors, all of them in flight at
//     once - and loops over the candidates of the launch's slice.  A candidate's parameters are wave-uniform: one scalar 16-byte load.
//   * Per element and candidate, in separately rounded fp32 operations (the unit is built with -ffp-contract=off), exactly what the
//     reference's eager ops compute (uniform_quantizers.py:114-115,146, range_estimators.py:134-136):
//         q = RN(x / scale)    (fq_quot_sat: the correctly rounded quotient in three instructions, finite first product)
//         r = clamp(rint(q), lo, hi);  y = scale * r;  d = x - y;  term = d * d
//     ten vector instructions.  RN(1 / scale) is formed per candidate by a true division.
//   * A lane adds its kQmseLane = 32 terms pairwise in fp32 (five levels); from there on every sum is float64 (calls of at most
//     OEH_QMSE_F64_K candidates - the steps of a sequential search, whose result moves with the noise of its loss, and whose pass is
//     bound by the read rather than the arithmetic - add in float64 from the first term): a butterfly over the wave,
//     one float64 slot per (wave, candidate) in LDS that the wave's lane 0 adds to chunk after chunk, the four waves in fixed order, one
//     record of doubles per workgroup in `work`, and a merge launch - one wave per candidate, lane l over workgroups l, l + 64, ... in
//     ascending order, then a butterfly - that stores, or adds to, loss[k].
//   * K is cut into slices of kQmseSlice candidates: a pass over the data and a merge per slice, chained on one stream (`work` is
//     reused from slice to slice).  The kernel is bound by its vector arithmetic, not by the re-read.
//
// Plain launches in a linear chain: no atomics, no allocation, no host synchronisation; the geometry is a function of (n, K) only and
// every sum has a fixed order, so results are bitwise reproducible.
#include "oeh_stream.h"
#include "oeh_launch.h"
#include "oeh_desc.h"

namespace oeh {

namespace {

constexpr int kQmseLane = 32;                 // floats a lane keeps of a chunk: the most terms ever added in fp32
constexpr int kQmseC = 256 * kQmseLane;       // elements per chunk (OEH_QMSE_CHUNK)
constexpr int kQmseSlice = 256;               // candidates per launch (OEH_QMSE_SLICE): one float64 LDS slot per wave and candidate
constexpr int kQmseMaxBlocks = 1024;          // workgroups per launch (OEH_QMSE_MAX_BLOCKS): beyond that a workgroup takes several chunks
static_assert(kQmseC == OEH_QMSE_CHUNK && kQmseSlice == OEH_QMSE_SLICE && kQmseMaxBlocks == OEH_QMSE_MAX_BLOCKS, "include/oeh.h names the same constants");

struct QmseCand {  // include/oeh.h: one candidate grid, 16 bytes
  float scale, lo, hi, reserved;
};
static_assert(sizeof(QmseCand) == OEH_QMSE_CAND_BYTES, "candidate record");

// One chunk into thread t's registers: slot s of the chunk's 16-byte slots (s * 256 + t) holds the lane's elements [s * V, (s + 1) * V).
// The whole chunk is covered by the array: 16-byte loads, all in flight before the first is used.
template <int IN>
__device__ __forceinline__ void qmse_load_full(const char* __restrict__ p, const int t, float (&xs)[kQmseLane]) {
  constexpr int V = 16 / In<IN>::bytes, S = kQmseLane / V;
  u4 raw[S];
  load_chunk_full<IN, 256, S>(p, t, raw);
#pragma unroll
  for (int s = 0; s < S; ++s) unpack16<IN>(raw[s], &xs[s * V]);
}
// The array's first or last chunk, covered in [lo_c, hi_c) only (indices relative to `p`, the chunk's 16-byte aligned base): the same
// placement by element loads of the covered elements - nothing outside the array is touched.  An element outside is 0 and its bit in
// the returned mask is clear.
template <int IN>
__device__ __forceinline__ unsigned qmse_load_part(const char* __restrict__ p, const int lo_c, const int hi_c, const int t, float (&xs)[kQmseLane]) {
  constexpr int V = 16 / In<IN>::bytes;
  typedef typename In<IN>::elem elem;
  unsigned valid = 0u;
#pragma unroll
  for (int i = 0; i < kQmseLane; ++i) {
    const int o = ((i / V) * 256 + t) * V + i % V;
    xs[i] = 0.0f;
    if (o >= lo_c && o < hi_c) {
      xs[i] = In<IN>::to_f32(reinterpret_cast<const elem*>(p)[o]);
      valid |= 1u << i;
    }
  }
  return valid;
}

// One candidate over the lane's 32 elements: the fp32 terms, added pairwise in fp32 (five levels) - or, F64, each widened and added in
// float64 - as a double.
template <bool FULL, bool F64>
__device__ __forceinline__ double qmse_lane(const float (&xs)[kQmseLane], const unsigned valid, const FqP& f) {
  float tm[kQmseLane];
#pragma unroll
  for (int i = 0; i < kQmseLane; ++i) {
    const float r = __builtin_amdgcn_fmed3f(__builtin_rintf(fq_quot_sat(xs[i], f)), f.lo, f.hi);
    const float y = f.scale * r;
    const float d = xs[i] - y;
    tm[i] = d * d;
    if (!FULL && ((valid >> i) & 1u) == 0u) tm[i] = 0.0f;
  }
  if constexpr (F64) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < kQmseLane; ++i) a[i & 3] += (double)tm[i];
    return (a[0] + a[1]) + (a[2] + a[3]);
  } else {
#pragma unroll
    for (int w = kQmseLane / 2; w >= 1; w >>= 1)
#pragma unroll
      for (int i = 0; i < w; ++i) tm[i] = tm[2 * i] + tm[2 * i + 1];
    return (double)tm[0];
  }
}

template <bool FULL, bool F64>
__device__ __forceinline__ void qmse_candidates(const float (&xs)[kQmseLane], const unsigned valid, const QmseCand* __restrict__ cand, const int ks,
                                                const int t, double (*acc)[kQmseSlice]) {
  for (int k = 0; k < ks; ++k) {
    const QmseCand c = cand[k];  // wave-uniform: scalar loads
    FqP f;
    f.scale = c.scale;
    f.rscale = 1.0f / c.scale;   // a true (correctly rounded) division, once per candidate
    f.lo = c.lo;
    f.hi = c.hi;
    const double s = wave_sum(qmse_lane<FULL, F64>(xs, valid, f));
    if ((t & 63) == 0) acc[t >> 6][k] += s;  // (this wave's own slot: nobody else touches it before the barrier at the end)
  }
}

// Workgroup b takes the chunks [b * cpb, (b + 1) * cpb) and writes work[b * ks + k] for the ks candidates of this slice.
template <int IN, bool F64>
__global__ __launch_bounds__(256, 4) void oeh_qmse_chunk_kernel(const void* __restrict__ x, const long n, const long nch, const long cpb,
                                                             const QmseCand* __restrict__ cand, const int ks, double* __restrict__ work) {
  __shared__ double acc[4][kQmseSlice];
  const int t = threadIdx.x;
#pragma unroll
  for (int w = 0; w < 4; ++w) acc[w][t] = 0.0;
  __syncthreads();
  int a;
  const char* base = aligned_base(x, In<IN>::bytes, a);
  const long c0 = (long)blockIdx.x * cpb;
  for (long j = 0; j < cpb; ++j) {
    const long ch = c0 + j;
    if (ch >= nch) break;
    const long cbase = ch * kQmseC;
    const long lo_l = (long)a - cbase, hi_l = (long)a + n - cbase;
    const int lo_c = (int)(lo_l < 0 ? 0 : (lo_l > kQmseC ? kQmseC : lo_l));
    int hi_c = (int)(hi_l < 0 ? 0 : (hi_l > kQmseC ? kQmseC : hi_l));
    if (hi_c < lo_c) hi_c = lo_c;
    const char* p = base + (size_t)cbase * In<IN>::bytes;
    float xs[kQmseLane];
    if (lo_c == 0 && hi_c == kQmseC) {
      qmse_load_full<IN>(p, t, xs);
      qmse_candidates<true, F64>(xs, 0xffffffffu, cand, ks, t, acc);
    } else if (hi_c > lo_c) {
      const unsigned valid = qmse_load_part<IN>(p, lo_c, hi_c, t, xs);
      qmse_candidates<false, F64>(xs, valid, cand, ks, t, acc);
    }
  }
  __syncthreads();
  if (t < ks) work[(size_t)blockIdx.x * ks + t] = (acc[0][t] + acc[1][t]) + (acc[2][t] + acc[3][t]);
}

// One wave per candidate: lane l adds the workgroups l, l + 64, ... in ascending order, a butterfly adds the lanes.
__global__ __launch_bounds__(256) void oeh_qmse_merge_kernel(const double* __restrict__ work, const int blocks, const int ks, double* __restrict__ loss,
                                                             const int accumulate) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= ks) return;  // (whole waves; no barrier here)
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  for (int b = lane; b < blocks; b += 64) s += work[(size_t)b * ks + k];
  s = wave_sum(s);
  if (lane == 0) loss[k] = accumulate ? loss[k] + s : s;
}

// workgroups of a pass (= records in `work`), with the chunks and the chunks per workgroup behind that number
long qmse_blocks(long n, long* nch_out, long* cpb_out) {
  const long nch = chunks_for(n, kQmseC);
  const long cpb = (nch + kQmseMaxBlocks - 1) / kQmseMaxBlocks;
  if (nch_out) *nch_out = nch;
  if (cpb_out) *cpb_out = cpb;
  return (nch + cpb - 1) / cpb;
}

}  // namespace
}  // namespace oeh

using namespace oeh;

extern "C" {

size_t oeh_quant_mse_work_bytes(int64_t n, int32_t K) {
  if (n < 1 || K < 1) return 0;
  return (size_t)qmse_blocks(n, nullptr, nullptr) * (size_t)(K < OEH_QMSE_SLICE ? K : OEH_QMSE_SLICE) * sizeof(double);
}

int oeh_quant_mse(const void* x, int64_t n, int32_t dtype, const float* cand, int32_t K, double* loss, int32_t accumulate, void* work,
                  void* stream) {
  if (x == nullptr || cand == nullptr || loss == nullptr || work == nullptr || n < 1 || K < 1 || !dtype_ok(dtype)) return OEH_EINVAL;
  if ((addr(cand) & 15) != 0 || (addr(loss) & 7) != 0 || (addr(work) & 7) != 0 || (addr(x) & (uintptr_t)(elem_bytes(dtype) - 1)) != 0) return OEH_EALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  long nch, cpb;
  const long blocks = qmse_blocks(n, &nch, &cpb);
  const QmseCand* c = reinterpret_cast<const QmseCand*>(cand);
  double* w = reinterpret_cast<double*>(work);
  const bool f64 = K <= OEH_QMSE_F64_K;
  for (int k0 = 0; k0 < K; k0 += kQmseSlice) {
    const int ks = K - k0 < kQmseSlice ? K - k0 : kQmseSlice;
    dispatch_in(dtype, [&](auto t) {
      constexpr int IN = decltype(t)::value;
      if (f64) hipLaunchKernelGGL((oeh_qmse_chunk_kernel<IN, true>), dim3((unsigned)blocks), dim3(256), 0, st, x, n, nch, cpb, c + k0, ks, w);
      else hipLaunchKernelGGL((oeh_qmse_chunk_kernel<IN, false>), dim3((unsigned)blocks), dim3(256), 0, st, x, n, nch, cpb, c + k0, ks, w);
    });
    hipLaunchKernelGGL(oeh_qmse_merge_kernel, dim3((unsigned)((ks + 3) / 4)), dim3(256), 0, st, w, (int)blocks, ks, loss + k0, accumulate != 0);
  }
  return launch_status();
}

}  // extern "C"
