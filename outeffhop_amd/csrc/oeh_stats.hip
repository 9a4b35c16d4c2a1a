// Outlier statistics: per-row infinity norm, kurtosis, mean and unbiased std in one pass over HBM (include/oeh.h: oeh_outlier_stats).
//
// The reference measures its results with an eager chain per hooked tensor and batch (validate_clm.py:565-621, validate_mlm.py:497-533,
// transformers_language/utils.py:9-20): x.norm(p=inf), mean, std, (x - mu) ** 4, mean - six or more passes over a (B, S * E) activation and
// one .item() per sample and statistic.  Here every element is read from HBM once:
//
//   * A row is cut into chunks of kStatsC elements at 16-byte boundaries of its own address (a row may start at any element: base pointers
//     one element off, odd row strides).  A chunk's elements stay in registers - kStatsLane floats per lane, loaded as 16-byte vectors, all
//     of them in flight at once - for two sweeps:
//       sweep 1: sum of x, max of |x| and min / max of the bit patterns (integer operations: a NaN compares above infinity, so it is
//                neither dropped as fmaxf would drop it nor in need of a flag of its own; min == max tells a constant chunk);
//       sweep 2: sums of d, d^2, d^3, d^4 for d = x - c in fp32, c = fl32(sum / n) (or the element itself in a constant chunk, so that
//                d = 0 exactly), four independent accumulators per lane and sum, then a shuffle butterfly over the wave and a fixed-order
//                sum over the workgroup's four waves through LDS: a summation tree of depth 8 + 2 + 6 + 2.
//     No raw power sums anywhere: at mean 1000 and std 1 they hold nothing but the mean.
//   * The chunk's (n, mean, M2, M3, M4) follows in float64 from (c, sum d^k) by the shift delta = sum d / n, which removes the rounding
//     of c:  mean = c + delta, M2 = S2 - n delta^2, M3 = S3 - 3 delta S2 + 2 n delta^3, M4 = S4 - 4 delta S3 + 6 delta^2 S2 - 3 n delta^4.
//   * Chunks are merged in float64 with the pairwise update of central moments (Chan et al. 1979; Pebay 2008), in a fixed tree.
//
// Two forms, chosen on the host: rows of at most kStatsW elements take one wave per row, four rows per workgroup, one launch and no work
// buffer; longer rows take one workgroup per (row, chunk), which writes a 48-byte record to `work`, and a second small launch with one
// wave per row that merges the records and writes `stats`.  The optional running meter is added by a one-wave launch at the end of the
// same chain, rows in ascending order in float64.  Plain launches on one stream: no atomics, no allocation, no host synchronisation.
#include "oeh_stream.h"
#include "oeh_launch.h"
#include "oeh_desc.h"

namespace oeh {

namespace {

constexpr int kStatsLane = 32;                      // floats a lane keeps of a chunk
constexpr int kStatsC = 256 * kStatsLane;           // elements per chunk of the long-row form (OEH_STATS_CHUNK)
constexpr int kStatsW = 64 * kStatsLane - 8;        // longest row of the one-wave form (OEH_STATS_WAVE_COLS): any misalignment (< 8 elements) still fits
static_assert(kStatsC == OEH_STATS_CHUNK && kStatsW == OEH_STATS_WAVE_COLS, "include/oeh.h names the same constants");

struct StatsRec {  // one chunk, or a merged run of chunks (48 bytes in `work`)
  double n, mean, m2, m3, m4;
  unsigned amax;   // bit pattern of max |x| (above 0x7f800000: a NaN was seen)
  unsigned pad;
};
static_assert(sizeof(StatsRec) == OEH_STATS_RECORD_BYTES, "work buffer record");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The statistics of the elements [lo_c, hi_c) of one chunk (element indices relative to `p`, the chunk's 16-byte aligned base) by a
// group of WAVES waves, thread t of it.  FULL: lo_c == 0 and hi_c == the chunk's capacity, no element is tested.  Every thread returns
// the same record.  lds: WAVES > 1 only, [8][WAVES] words.
template <int IN, int WAVES, bool FULL>
__device__ __forceinline__ StatsRec chunk_pass(const char* __restrict__ p, const int lo_c, const int hi_c, const int t, unsigned (*lds)[4]) {
  constexpr int V = 16 / In<IN>::bytes, K = kStatsLane / V, T = 64 * WAVES;
  typedef typename In<IN>::elem elem;
  float xs[K][V];
  u4 raw[K];
  // every 16-byte load of the chunk is issued before the first value is used
  if constexpr (FULL) {
    load_chunk_full<IN, T, K>(p, t, raw);
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int o = (k * T + t) * V;
      raw[k] = u4{0u, 0u, 0u, 0u};
      if (o >= lo_c && o + V <= hi_c) raw[k] = *reinterpret_cast<const u4*>(p + (size_t)o * In<IN>::bytes);
    }
  }
  float s = 0.0f;
  unsigned amax = 0u, maxb = 0u, minb = 0xffffffffu;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int o = (k * T + t) * V;
    const int lo = FULL ? 0 : clampi(lo_c - o, 0, V), hi = FULL ? V : clampi(hi_c - o, 0, V);
    if (lo == 0 && hi == V) {
      unpack16<IN>(raw[k], xs[k]);
      float ps[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const unsigned b = f32_bits(xs[k][e]);
        amax = max(amax, b & 0x7fffffffu);
        maxb = max(maxb, b);
        minb = min(minb, b);
        ps[e] = xs[k][e];
      }
#pragma unroll
      for (int w = V / 2; w >= 1; w >>= 1)
#pragma unroll
        for (int e = 0; e < w; ++e) ps[e] += ps[e + w];
      s += ps[0];
    } else {
      // a slot that the row covers in part (its first or last one), or not at all: element loads of the covered ones only
#pragma unroll
      for (int e = 0; e < V; ++e) {
        xs[k][e] = 0.0f;
        if (e >= lo && e < hi) {
          const float x = In<IN>::to_f32(reinterpret_cast<const elem*>(p)[o + e]);
          const unsigned b = f32_bits(x);
          xs[k][e] = x;
          amax = max(amax, b & 0x7fffffffu);
          maxb = max(maxb, b);
          minb = min(minb, b);
          s += x;
        }
      }
    }
  }
  s = wave_sum(s);
  amax = wave_max(amax);
  maxb = wave_max(maxb);
  minb = wave_min(minb);
  if constexpr (WAVES > 1) {
    static_assert(WAVES == 4, "the fixed order below is written for four waves");
    if ((t & 63) == 0) {
      lds[0][t >> 6] = f32_bits(s);
      lds[1][t >> 6] = amax;
      lds[2][t >> 6] = maxb;
      lds[3][t >> 6] = minb;
    }
    __syncthreads();
    // (the float sums in block4's order, written out: behind a helper the compiler pairs them differently - profiles/stream_helpers.txt)
    s = (bits_f32(lds[0][0]) + bits_f32(lds[0][1])) + (bits_f32(lds[0][2]) + bits_f32(lds[0][3]));
    amax = block4_max(lds[1]);
    maxb = block4_max(lds[2]);
    minb = block4_min(lds[3]);
  }
  const int n = hi_c - lo_c;
  // the centre: any value near the mean serves (its distance from the mean is taken out below); a constant chunk is centred on its value
  const float c = minb == maxb ? bits_f32(minb) : s / (float)n;

  float s1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s2[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s3[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int o = (k * T + t) * V;
    const int lo = FULL ? 0 : clampi(lo_c - o, 0, V), hi = FULL ? V : clampi(hi_c - o, 0, V);
    if (hi > lo) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        float d = xs[k][e] - c;
        if (!FULL && (e < lo || e >= hi)) d = 0.0f;
        const float d2 = d * d;
        s1[e & 3] += d;
        s2[e & 3] = __builtin_fmaf(d, d, s2[e & 3]);
        s3[e & 3] = __builtin_fmaf(d2, d, s3[e & 3]);
        s4[e & 3] = __builtin_fmaf(d2, d2, s4[e & 3]);
      }
    }
  }
  float r1 = wave_sum((s1[0] + s1[1]) + (s1[2] + s1[3]));
  float r2 = wave_sum((s2[0] + s2[1]) + (s2[2] + s2[3]));
  float r3 = wave_sum((s3[0] + s3[1]) + (s3[2] + s3[3]));
  float r4 = wave_sum((s4[0] + s4[1]) + (s4[2] + s4[3]));
  if constexpr (WAVES > 1) {
    if ((t & 63) == 0) {
      lds[4][t >> 6] = f32_bits(r1);
      lds[5][t >> 6] = f32_bits(r2);
      lds[6][t >> 6] = f32_bits(r3);
      lds[7][t >> 6] = f32_bits(r4);
    }
    __syncthreads();
    r1 = (bits_f32(lds[4][0]) + bits_f32(lds[4][1])) + (bits_f32(lds[4][2]) + bits_f32(lds[4][3]));
    r2 = (bits_f32(lds[5][0]) + bits_f32(lds[5][1])) + (bits_f32(lds[5][2]) + bits_f32(lds[5][3]));
    r3 = (bits_f32(lds[6][0]) + bits_f32(lds[6][1])) + (bits_f32(lds[6][2]) + bits_f32(lds[6][3]));
    r4 = (bits_f32(lds[7][0]) + bits_f32(lds[7][1])) + (bits_f32(lds[7][2]) + bits_f32(lds[7][3]));
  }
  StatsRec r;
  r.amax = amax;
  r.pad = 0u;
  if (n <= 0) {
    r.n = r.mean = r.m2 = r.m3 = r.m4 = 0.0;
    r.amax = 0u;
    return r;
  }
  const double dn = (double)n, S1 = (double)r1, S2 = (double)r2, S3 = (double)r3, S4 = (double)r4;
  const double dl = S1 / dn, dl2 = dl * dl;
  r.n = dn;
  r.mean = (double)c + dl;
  r.m2 = fmax(S2 - dn * dl2, 0.0);
  r.m3 = S3 - 3.0 * dl * S2 + 2.0 * dn * dl2 * dl;
  r.m4 = fmax(S4 - 4.0 * dl * S3 + 6.0 * dl2 * S2 - 3.0 * dn * dl2 * dl2, 0.0);
  return r;
}

// a followed by b (Pebay 2008, eq. 3.1): the moments of the union about its own mean
__device__ __forceinline__ StatsRec stats_merge(const StatsRec& a, const StatsRec& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  StatsRec r;
  const double n = a.n + b.n, rn = 1.0 / n;
  const double dl = b.mean - a.mean, dn = dl * rn, dn2 = dn * dn;
  r.n = n;
  r.mean = a.mean + b.n * dn;
  r.m2 = a.m2 + b.m2 + dl * dn * a.n * b.n;
  r.m3 = a.m3 + b.m3 + dl * dn2 * a.n * b.n * (a.n - b.n) + 3.0 * dn * (a.n * b.m2 - b.n * a.m2);
  r.m4 = a.m4 + b.m4 + dl * dn2 * dn * a.n * b.n * (a.n * a.n - a.n * b.n + b.n * b.n) + 6.0 * dn2 * (a.n * a.n * b.m2 + b.n * b.n * a.m2) +
         4.0 * dn * (a.n * b.m3 - b.n * a.m3);
  r.amax = max(a.amax, b.amax);
  r.pad = 0u;
  return r;
}

// (inf_norm, kurtosis, mean, std) of a finished row, one 16-byte store
__device__ __forceinline__ void stats_store(const StatsRec& r, const double eps, float* __restrict__ out) {
  const float qnan = bits_f32(0x7fc00000u);
  const bool has_nan = r.amax > 0x7f800000u, finite = r.amax < 0x7f800000u;
  const double var = r.m2 / (r.n - 1.0);  // cols = 1: 0 / 0
  const double kurt = (r.m4 / r.n) / (var * var + eps);
  f4 o;
  o[0] = has_nan ? qnan : bits_f32(r.amax);
  o[1] = finite ? (float)kurt : qnan;
  o[2] = finite ? (float)r.mean : qnan;
  o[3] = finite ? (float)sqrt(var) : qnan;
  *reinterpret_cast<f4*>(out) = o;
}

template <int IN>
__global__ __launch_bounds__(256) void oeh_stats_wave_kernel(const void* __restrict__ x, const long rows, const int cols, const long row_stride_bytes,
                                                             const double eps, float* __restrict__ stats) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // (whole waves; this form has no barrier)
  int a;
  const char* p = aligned_base(reinterpret_cast<const char*>(x) + row * row_stride_bytes, In<IN>::bytes, a);
  const StatsRec r = chunk_pass<IN, 1, false>(p, a, a + cols, threadIdx.x & 63, nullptr);
  if ((threadIdx.x & 63) == 0) stats_store(r, eps, stats + row * 4);
}

template <int IN>
__global__ __launch_bounds__(256) void oeh_stats_chunk_kernel(const void* __restrict__ x, const long cols, const long row_stride_bytes, const int nch,
                                                              StatsRec* __restrict__ work) {
  __shared__ unsigned lds[8][4];
  const unsigned row = blockIdx.x / (unsigned)nch, ch = blockIdx.x - row * (unsigned)nch;
  int a;
  const char* p = aligned_base(reinterpret_cast<const char*>(x) + (long)row * row_stride_bytes, In<IN>::bytes, a);
  const long cbase = (long)ch * kStatsC;
  const long lo_l = (long)a - cbase, hi_l = (long)a + cols - cbase;
  const int lo_c = (int)(lo_l < 0 ? 0 : (lo_l > kStatsC ? kStatsC : lo_l)), hi_c = (int)(hi_l < 0 ? 0 : (hi_l > kStatsC ? kStatsC : hi_l));
  p += cbase * In<IN>::bytes;
  StatsRec r;
  if (lo_c == 0 && hi_c == kStatsC) r = chunk_pass<IN, 4, true>(p, lo_c, hi_c, threadIdx.x, lds);
  else r = chunk_pass<IN, 4, false>(p, lo_c, hi_c < lo_c ? lo_c : hi_c, threadIdx.x, lds);
  if (threadIdx.x == 0) work[blockIdx.x] = r;
}

// One round of the running meter: the values of up to 64 rows, one per lane, are added in lane order - the float64 sums that
// AverageMeter.update(v.item()) forms row by row.  m (wave-uniform): rows in this round.  Every lane computes the same sums.
__device__ __forceinline__ void meter_round(const float vi, const float vk, const int m, double& si, double& sk) {
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    if (i < m) {
      si += (double)bits_f32(__builtin_amdgcn_readlane(f32_bits(vi), i));
      sk += (double)bits_f32(__builtin_amdgcn_readlane(f32_bits(vk), i));
    }
  }
}
__device__ __forceinline__ void meter_store(double* __restrict__ meter, const int accumulate, const double si, const double sk, const long rows) {
  if (accumulate & 1) {
    meter[0] = si;
    meter[1] += (double)rows;
  }
  if (accumulate & 2) {
    meter[2] = sk;
    meter[3] += (double)rows;
  }
}

__global__ __launch_bounds__(256) void oeh_stats_merge_kernel(const StatsRec* __restrict__ work, const long rows, const int nch, const double eps,
                                                              float* __restrict__ stats) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  StatsRec r;
  r.n = r.mean = r.m2 = r.m3 = r.m4 = 0.0;
  r.amax = r.pad = 0u;
  for (int i = lane; i < nch; i += 64) r = stats_merge(r, work[row * nch + i]);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {  // lane l takes in lane l + off: chunks stay in ascending order inside every merge
    StatsRec b;
    b.n = __shfl_down(r.n, off);
    b.mean = __shfl_down(r.mean, off);
    b.m2 = __shfl_down(r.m2, off);
    b.m3 = __shfl_down(r.m3, off);
    b.m4 = __shfl_down(r.m4, off);
    b.amax = (unsigned)__shfl_down((int)r.amax, off);
    b.pad = 0u;
    if (lane + off < 64) r = stats_merge(r, b);
  }
  if (lane == 0) stats_store(r, eps, stats + row * 4);
}

// the running meter: a one-wave launch at the end of the chain (a folded form - the merge launch as ONE workgroup that also adds the
// meter - measured slower: 17.9 against 13.3 us at 16 rows of 393216 fp16, the serial merges cost more than the launch saves)
__global__ __launch_bounds__(64) void oeh_stats_meter_kernel(const float* __restrict__ stats, const long rows, double* __restrict__ meter, const int accumulate) {
  const int lane = threadIdx.x;
  double si = meter[0], sk = meter[2];
  for (long base = 0; base < rows; base += 64) {
    float vi = 0.0f, vk = 0.0f;
    if (base + lane < rows) {
      const f4 v = *reinterpret_cast<const f4*>(stats + (base + lane) * 4);
      vi = v[0];
      vk = v[1];
    }
    meter_round(vi, vk, (int)(rows - base < 64 ? rows - base : 64), si, sk);
  }
  if (lane == 0) meter_store(meter, accumulate, si, sk, rows);
}

// records per row in `work`: 0 in the one-wave form
long stats_chunks(long cols) { return cols <= kStatsW ? 0 : chunks_for(cols, kStatsC); }

}  // namespace
}  // namespace oeh

using namespace oeh;

extern "C" {

size_t oeh_outlier_stats_work_bytes(int64_t rows, int64_t cols) {
  if (rows < 1 || cols < 1) return 0;
  return (size_t)rows * (size_t)stats_chunks(cols) * OEH_STATS_RECORD_BYTES;
}

int oeh_outlier_stats(const void* x, int64_t rows, int64_t cols, int64_t row_stride, int32_t dtype, double eps, float* stats, double* meter,
                      int32_t accumulate, void* work, void* stream) {
  if (x == nullptr || stats == nullptr || rows < 1 || cols < 1 || row_stride < cols || !dtype_ok(dtype) || !(eps >= 0.0)) return OEH_EINVAL;
  if (accumulate < 0 || accumulate > 3 || (accumulate != 0 && meter == nullptr)) return OEH_EINVAL;
  const long nch = stats_chunks(cols);
  if (nch > 0 && work == nullptr) return OEH_EINVAL;
  const int eb = elem_bytes(dtype);
  if ((addr(stats) & 15) != 0 || (addr(meter) & 7) != 0 || (nch > 0 && (addr(work) & 7) != 0) || (addr(x) & (uintptr_t)(eb - 1)) != 0) return OEH_EALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long blocks4 = (rows + 3) / 4;
  if (blocks4 >= ((long)1 << 31) || rows * (nch > 0 ? nch : 1) >= ((long)1 << 31)) return OEH_ENOTSUP;
  if (nch == 0) {
    dispatch_in(dtype, [&](auto t) {
      constexpr int IN = decltype(t)::value;
      hipLaunchKernelGGL(oeh_stats_wave_kernel<IN>, dim3((unsigned)blocks4), dim3(256), 0, st, x, rows, (int)cols, row_stride * eb, eps, stats);
    });
  } else {
    StatsRec* w = reinterpret_cast<StatsRec*>(work);
    const unsigned grid = (unsigned)(rows * nch);
    dispatch_in(dtype, [&](auto t) {
      constexpr int IN = decltype(t)::value;
      hipLaunchKernelGGL(oeh_stats_chunk_kernel<IN>, dim3(grid), dim3(256), 0, st, x, cols, row_stride * eb, (int)nch, w);
    });
    hipLaunchKernelGGL(oeh_stats_merge_kernel, dim3((unsigned)blocks4), dim3(256), 0, st, w, rows, (int)nch, eps, stats);
  }
  if (accumulate != 0) hipLaunchKernelGGL(oeh_stats_meter_kernel, dim3(1), dim3(64), 0, st, stats, rows, meter, accumulate);
  return launch_status();
}

}  // extern "C"
