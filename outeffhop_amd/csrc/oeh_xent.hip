// Cross-entropy over a vocabulary: per-row loss, its mean and the logit gradient, each from ONE pass over the logits (include/oeh.h:
// oeh_xent_fwd / oeh_xent_bwd).
//
// The reference ends both of its language models in CrossEntropyLoss over the whole vocabulary (quantized_opt.py:868-877 on the shifted
// .contiguous() copy of the logits; quantized_bert.py:910-915 with -100 labels; validate_clm.py:556-594 takes exp(mean of the batch
// losses)): a copy, an fp32 upcast under autocast, log_softmax read and write and nll_loss - five or more passes over a (B * S, V) tensor,
// and as many again backward.  Here the forward reads every logit once and the backward reads it once and writes its gradient once.
//
//   * The logits are a (B, S, V) VIEW, V contiguous: the reference's shift is two pointer offsets on the host.  A row may start at any
//     element (V = 30522 in fp16: rows of 61044 bytes); it is read with 16-byte loads on its OWN 16-byte boundaries (aligned_base), in
//     steps of T = 256 * kXentK slots.  The first and the last slot of a row may reach outside it - inside the enclosing 16-byte slot, never
//     further - and their outside elements are set to -inf in registers; a slot wholly outside is not loaded.  All kXentK loads of a
//     thread are issued before the first value is used: 16 KiB in flight per workgroup and step.
//   * Forward, per thread an online (m, l): m the running maximum, l = sum exp(x - m) in fp32, rescaled once per step.  exp(d) is
//     exp2(RN(RN(x - m) * log2e)) (v_exp_f32).  The threads' pairs are merged at the row maximum M by wave_max / wave_sum and the fixed
//     four-wave step; lse = M + log(L).  One lane loads x[label]: loss = lse - x[label], one fp32 subtraction.  With label smoothing the
//     pass also forms sum(x): a step's sum in fp32 (a fixed tree), the steps and the threads in float64.
//   * Labels are data.  A row whose label is ignore_index reads no logit: loss 0, lse 0, not counted.  A label outside [0, V) is found
//     before any address is formed from it: NaN loss and lse, counted, and *bad_rows counts it.
//   * Reduce: a second launch of one workgroup of 1024 threads adds the fp32 row losses of the counted rows and their number in float64 -
//     thread t the rows t, t + 1024, ... in ascending order, then the butterflies, then the 16 waves in order - and writes {sum, count}, the fp32 mean, the
//     running meter and the bad-label count.  No atomics anywhere; the chain is bitwise reproducible.
//   * Backward, per element  d = RN_dtype((exp(x - lse) - (1 - eps)[j == y] - eps / V) * g), every operation rounded on its own in this
//     order (the last term only with smoothing).  A thread reads the slots of a step before it writes them: dlogits may BE logits.
//     Stores are 16 bytes wide where every dlogits row sits as far from a 16-byte boundary as its logits row (the host decides; the edge
//     slots take element stores), per element otherwise.
#include "oeh_stream.h"
#include "oeh_launch.h"
#include "oeh_desc.h"

#include <cstdio>

namespace oeh {

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

namespace {

constexpr int kXentK = OEH_XENT_SLOTS;  // 16-byte slots a thread has in flight per step
constexpr int kReduceU = 8;             // rows a thread of the reduce launch has in flight

__device__ __forceinline__ float neg_inf() { return bits_f32(0xff800000u); }
__device__ __forceinline__ float qnan() { return bits_f32(0x7fc00000u); }
// the reference point of exp(x - m): the maximum, or 0 while that is still -inf (nothing but -inf seen: every term is exp(-inf) = 0)
__device__ __forceinline__ float mref(const float m) { return m == neg_inf() ? 0.0f : m; }

__device__ __forceinline__ long xent_label(const XentArgs& p, const unsigned row, unsigned& b, unsigned& s) {
  b = row / (unsigned)p.S;  // (rows < 2^31: xent_check)
  s = row - b * (unsigned)p.S;
  const long off = (long)b * p.l_sb + (long)s * p.l_ss;
  return p.label64 ? reinterpret_cast<const long*>(p.labels)[off] : (long)reinterpret_cast<const int*>(p.labels)[off];
}

// The slots of thread t in the step that starts `o0` elements behind the row's aligned base `pc0`: v[k] = the NV elements of slot
// k * 256 + t as fp32.  The row covers the elements [a, end) counted from that base.  FULL: the step lies inside the row, nothing is tested.
// Otherwise a slot the row touches is loaded whole and a slot it does not touch is not loaded; MASK: elements outside the row become -inf.
// (No __restrict__ on this or the backward's pointers: dlogits may be logits.)
template <int IN, bool FULL, bool MASK>
__device__ __forceinline__ void xent_load(const char* pc, const long o0, const long a, const long end, const int t,
                                          float (&v)[kXentK][Vec16<IN>::N]) {
  constexpr int NV = Vec16<IN>::N, K = kXentK;
  u4 raw[K];
  if constexpr (FULL) {
    load_chunk_full<IN, 256, K>(pc, t, raw);
#pragma unroll
    for (int k = 0; k < K; ++k) unpack16<IN>(raw[k], v[k]);
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const long o = o0 + (long)((k * 256 + t) * NV);
      raw[k] = u4{0u, 0u, 0u, 0u};
      if (o + NV > a && o < end) raw[k] = *reinterpret_cast<const u4*>(pc + (size_t)((k * 256 + t) * NV) * In<IN>::bytes);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const long o = o0 + (long)((k * 256 + t) * NV);
      unpack16<IN>(raw[k], v[k]);
      if (MASK && !(o >= a && o + NV <= end)) {  // an edge slot, or one outside the row
#pragma unroll
        for (int e = 0; e < NV; ++e)
          if (o + e < a || o + e >= end) v[k][e] = neg_inf();
      }
    }
  }
}

// one step of the online statistics
template <int IN, bool LS, bool FULL>
__device__ __forceinline__ void xent_step(const char* __restrict__ pc, const long o0, const long a, const long end, const int t, float& m, float& l,
                                          double& sx) {
  constexpr int NV = Vec16<IN>::N, K = kXentK;
  float v[K][NV];
  xent_load<IN, FULL, true>(pc, o0, a, end, t, v);
  float mk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    mk[k] = v[k][0];
#pragma unroll
    for (int e = 1; e < NV; ++e) mk[k] = __builtin_fmaxf(mk[k], v[k][e]);
  }
  float ms = mk[0];
#pragma unroll
  for (int k = 1; k < K; ++k) ms = __builtin_fmaxf(ms, mk[k]);
  const float mn = __builtin_fmaxf(m, ms), r = mref(mn);
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    acc[k] = 0.0f;
#pragma unroll
    for (int e = 0; e < NV; ++e) acc[k] += exp_fast(v[k][e] - r);
  }
  static_assert(K == 4, "the fixed order below is written for four slots");
  const float step = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  // (a thread that has seen nothing but -inf has l = 0 and keeps it: its factor exp(0 - r) may overflow)
  l = (m == neg_inf() ? 0.0f : l * exp_fast(m - r)) + step;
  m = mn;
  if constexpr (LS) {
    float sk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float ps[NV];
      const long o = o0 + (long)((k * 256 + t) * NV);
#pragma unroll
      for (int e = 0; e < NV; ++e) ps[e] = (FULL || (o + e >= a && o + e < end)) ? v[k][e] : 0.0f;
#pragma unroll
      for (int w = NV / 2; w >= 1; w >>= 1)
#pragma unroll
        for (int e = 0; e < w; ++e) ps[e] += ps[e + w];
      sk[k] = ps[0];
    }
    sx += (double)((sk[0] + sk[1]) + (sk[2] + sk[3]));
  }
}

template <int IN, bool LS>
__global__ __launch_bounds__(256) void oeh_xent_fwd_kernel(const XentArgs p) {
  constexpr int NV = Vec16<IN>::N, T = 256 * kXentK * NV;
  typedef typename In<IN>::elem E;
  __shared__ float red_m[4], red_l[4];
  __shared__ double red_s[4];
  const int t = threadIdx.x;
  const unsigned row = blockIdx.x;
  unsigned b, s;
  const long y = xent_label(p, row, b, s);
  if (y == p.ignore_index || y < 0 || y >= p.V) {  // (uniform over the row's threads) no logit is read
    if (t == 0) {
      const float w = y == p.ignore_index ? 0.0f : qnan();
      p.lse[row] = w;
      if (p.row_loss != nullptr) p.row_loss[row] = w;
    }
    return;
  }
  const E* xr = reinterpret_cast<const E*>(p.x) + ((long)b * p.x_sb + (long)s * p.x_ss);
  int a0;
  const char* base = aligned_base(xr, In<IN>::bytes, a0);
  const long a = a0, end = a + p.V;
  float m = neg_inf(), l = 0.0f, xy = 0.0f;
  double sx = 0.0;
  if (t == 0) xy = In<IN>::to_f32(xr[y]);  // (issued with the first step's loads, not behind the last reduction)
  const long nsteps = chunks_for(p.V, T);
  for (long i = 0; i < nsteps; ++i) {
    const long o0 = i * T;
    const char* pc = base + (size_t)o0 * In<IN>::bytes;
    if (o0 >= a && o0 + T <= end) xent_step<IN, LS, true>(pc, o0, a, end, t, m, l, sx);
    else xent_step<IN, LS, false>(pc, o0, a, end, t, m, l, sx);
  }
  // ---- the threads' (m, l) at the row maximum
  const float wm = wave_max(m);
  if ((t & 63) == 0) red_m[t >> 6] = wm;
  __syncthreads();
  const float M = block4_max(red_m), r = mref(M);
  const float wl = wave_sum(m == neg_inf() ? 0.0f : l * exp_fast(m - r));
  if ((t & 63) == 0) red_l[t >> 6] = wl;
  if constexpr (LS) {
    const double ws = wave_sum(sx);
    if ((t & 63) == 0) red_s[t >> 6] = ws;
  }
  __syncthreads();
  if (t == 0) {
    const float L = (red_l[0] + red_l[1]) + (red_l[2] + red_l[3]);
    const float lse = M + logf(L);
    float loss = lse - xy;
    if constexpr (LS) {
      const double SX = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
      const float smooth = lse - (float)(SX / (double)p.V);
      loss = (1.0f - p.eps_ls) * loss + p.eps_ls * smooth;
    }
    p.lse[row] = lse;
    if (p.row_loss != nullptr) p.row_loss[row] = loss;
  }
}

// x[y] of a row as fp32, for the reduce launch without stored row losses
__device__ __forceinline__ float xent_gather(const XentArgs& p, const unsigned b, const unsigned s, const long y) {
  const long off = (long)b * p.x_sb + (long)s * p.x_ss + y;
  if (p.in == IN_F32) return reinterpret_cast<const float*>(p.x)[off];
  const unsigned short u = reinterpret_cast<const unsigned short*>(p.x)[off];
  return p.in == IN_BF16 ? In<IN_BF16>::to_f32(u) : In<IN_F16>::to_f32(u);
}

constexpr int kReduceT = 1024;  // threads of the reduce launch: 16 waves, added in wave order
__global__ __launch_bounds__(kReduceT) void oeh_xent_reduce_kernel(const XentArgs p) {
  constexpr int W = kReduceT / 64;
  __shared__ double red_s[W], red_c[W];
  __shared__ unsigned red_b[W];
  const int t = threadIdx.x;
  double sum = 0.0, cnt = 0.0;
  unsigned nbad = 0u;
  // (kReduceU rows of a thread at a time, their loads in flight together; added in ascending row order all the same)
  for (long base = t; base < p.rows; base += kReduceT * kReduceU) {
    long y[kReduceU];
    float li[kReduceU];
    unsigned b[kReduceU], s[kReduceU];
#pragma unroll
    for (int u = 0; u < kReduceU; ++u) {
      const long row = base + kReduceT * u;
      y[u] = row < p.rows ? xent_label(p, (unsigned)row, b[u], s[u]) : p.ignore_index;
      li[u] = qnan();
      if (row < p.rows && p.row_loss != nullptr) li[u] = p.row_loss[row];  // (read for an ignored row too - it is 0 there - and not used)
    }
    if (p.row_loss == nullptr) {
#pragma unroll
      for (int u = 0; u < kReduceU; ++u) {
        const long row = base + kReduceT * u;
        if (y[u] != p.ignore_index && y[u] >= 0 && y[u] < p.V)
          li[u] = p.lse[row] - xent_gather(p, b[u], s[u], y[u]);  // (the forward's own subtraction: the same bits)
      }
    }
#pragma unroll
    for (int u = 0; u < kReduceU; ++u) {
      if (y[u] == p.ignore_index) continue;
      sum += (double)li[u];
      cnt += 1.0;
      nbad += (y[u] < 0 || y[u] >= p.V) ? 1u : 0u;
    }
  }
  sum = wave_sum(sum);
  cnt = wave_sum(cnt);
  nbad = wave_sum(nbad);
  if ((t & 63) == 0) {
    red_s[t >> 6] = sum;
    red_c[t >> 6] = cnt;
    red_b[t >> 6] = nbad;
  }
  __syncthreads();
  if (t == 0) {
    double S = 0.0, N = 0.0;
    unsigned nb = 0u;
    for (int w = 0; w < W; ++w) {
      S += red_s[w];
      N += red_c[w];
      nb += red_b[w];
    }
    const double mean = S / N;  // 0 / 0: NaN, as torch's mean over no row
    p.out2[0] = S;
    p.out2[1] = N;
    if (p.mean != nullptr) *p.mean = (float)mean;
    if (p.meter != nullptr) {
      p.meter[0] += mean;
      p.meter[1] += 1.0;
    }
    if (p.bad_rows != nullptr) *p.bad_rows += (int)nb;
  }
}

// thread t's slots of a step to the gradient row: dr = the row's first element; a, end, o0 as in xent_load (the logits row's geometry).
// !EL: dr is as far behind a 16-byte boundary as the logits row, so the slots inside the row are whole 16-byte stores.
template <int IN, bool EL, bool FULL>
__device__ __forceinline__ void xent_store(typename In<IN>::elem* dr, const long o0, const long a, const long end, const int t,
                                           const float (&v)[kXentK][Vec16<IN>::N]) {
  constexpr int NV = Vec16<IN>::N, K = kXentK;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const long o = o0 + (long)((k * 256 + t) * NV);
    if (!EL && (FULL || (o >= a && o + NV <= end))) {
      Vec16<IN>::store(dr + (o - a), v[k]);
    } else {
      // (the 16-byte form's own conversion, then single elements of it: written as from_f32(v) the compiler folds the product in front
      // of it into one v_fma_mixlo_f16 - ONE rounding where the contract and the 16-byte form have two)
      const u4 w = pack16<IN>(v[k]);
#pragma unroll
      for (int e = 0; e < NV; ++e) {
        if (FULL || (o + e >= a && o + e < end)) {
          if constexpr (IN == IN_F32) dr[o + e - a] = bits_f32(w[e]);
          else dr[o + e - a] = (unsigned short)(w[e / 2] >> (16 * (e & 1)));
        }
      }
    }
  }
}

template <int IN, bool LS, bool EL, bool FULL>
__device__ __forceinline__ void xent_bwd_step(const char* pc, typename In<IN>::elem* dr, const long o0, const long a,
                                              const long end, const int t, const float lse, const float g, const long y, const float keep,
                                              const float ev) {
  constexpr int NV = Vec16<IN>::N, K = kXentK;
  float v[K][NV];
  xent_load<IN, FULL, false>(pc, o0, a, end, t, v);  // (every load of the step before its first store)
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const long j0 = o0 + (long)((k * 256 + t) * NV) - a;  // the slot's first element as a column of the row
#pragma unroll
    for (int e = 0; e < NV; ++e) {
      float d = exp_fast(v[k][e] - lse);
      if (j0 + e == y) d = d - keep;
      if constexpr (LS) d = d - ev;
      v[k][e] = d * g;
    }
  }
  xent_store<IN, EL, FULL>(dr, o0, a, end, t, v);
}

template <int IN, bool LS, bool EL>
__global__ __launch_bounds__(256) void oeh_xent_bwd_kernel(const XentArgs p) {
  constexpr int NV = Vec16<IN>::N, K = kXentK, T = 256 * K * NV;
  typedef typename In<IN>::elem E;
  const int t = threadIdx.x;
  const unsigned row = blockIdx.x;
  unsigned b, s;
  const long y = xent_label(p, row, b, s);
  const E* xr = reinterpret_cast<const E*>(p.x) + ((long)b * p.x_sb + (long)s * p.x_ss);
  E* dr = reinterpret_cast<E*>(p.dx) + ((long)b * p.dx_sb + (long)s * p.dx_ss);
  int a0;
  const char* base = aligned_base(xr, In<IN>::bytes, a0);  // (an address only: nothing is read through it in an ignored or bad row)
  const long a = a0, end = a + p.V;
  const long nsteps = chunks_for(p.V, T);
  if (y == p.ignore_index || y < 0 || y >= p.V) {  // (uniform) a row of zeros, or of NaN for a label that is none
    float w[K][NV];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int e = 0; e < NV; ++e) w[k][e] = y == p.ignore_index ? 0.0f : qnan();
    for (long i = 0; i < nsteps; ++i) xent_store<IN, EL, false>(dr, i * T, a, end, t, w);
    return;
  }
  float g = p.grad[(long)row * p.grad_stride];
  if (p.mean_reduction) g = (float)((double)g / p.out2[1]);
  const float lse = p.lse[row], keep = 1.0f - p.eps_ls, ev = p.eps_ls / (float)p.V;
  for (long i = 0; i < nsteps; ++i) {
    const long o0 = i * T;
    const char* pc = base + (size_t)o0 * In<IN>::bytes;
    if (o0 >= a && o0 + T <= end) xent_bwd_step<IN, LS, EL, true>(pc, dr, o0, a, end, t, lse, g, y, keep, ev);
    else xent_bwd_step<IN, LS, EL, false>(pc, dr, o0, a, end, t, lse, g, y, keep, ev);
  }
}

// oeh_xent_fwd / oeh_xent_bwd / oeh_xent_variant: every refusal in the order OEH_EINVAL -> OEH_ENOTSUP -> OEH_EALIGN.  bwd: dx_stride is looked at.
int xent_check(const oeh_xent_desc* d, const void* logits, const void* labels, bool bwd) {
  if (d == nullptr || logits == nullptr || labels == nullptr || d->V < 1 || d->B < 0 || d->S < 0 || !dtype_ok(d->dtype)) return OEH_EINVAL;
  if (d->label_dtype != OEH_ID_I32 && d->label_dtype != OEH_ID_I64) return OEH_EINVAL;
  for (int i = 0; i < 2; ++i) {
    if (d->x_stride[i] < 0 || d->label_stride[i] < 0 || (bwd && d->dx_stride[i] < 0)) return OEH_EINVAL;
  }
  if (bwd && ((d->S > 1 && d->dx_stride[1] < d->V) || (d->B > 1 && d->dx_stride[0] < d->V))) return OEH_EINVAL;
  if (!(d->label_smoothing >= 0.0f && d->label_smoothing < 1.0f) || d->reserved != 0) return OEH_EINVAL;
  if ((int64_t)d->B * d->S >= ((int64_t)1 << 31)) return OEH_ENOTSUP;
  if (addr(logits) % elem_bytes(d->dtype) != 0 || addr(labels) % (d->label_dtype == OEH_ID_I64 ? 8 : 4) != 0) return OEH_EALIGN;
  return OEH_OK;
}
XentArgs xent_args(const oeh_xent_desc* d, const void* logits, const void* labels) {
  XentArgs a = {};
  a.x = logits; a.labels = labels;
  a.x_sb = d->x_stride[0]; a.x_ss = d->x_stride[1]; a.l_sb = d->label_stride[0]; a.l_ss = d->label_stride[1];
  a.dx_sb = d->dx_stride[0]; a.dx_ss = d->dx_stride[1];
  a.ignore_index = d->ignore_index; a.rows = (long)d->B * d->S;
  a.S = d->S; a.V = d->V; a.in = d->dtype; a.label64 = d->label_dtype == OEH_ID_I64; a.mean_reduction = d->mean_reduction != 0;
  a.eps_ls = d->label_smoothing;
  return a;
}
// whether the gradient rows take element stores: a dlogits row that is not as far from a 16-byte boundary as its logits row
bool xent_el(const oeh_xent_desc* d, const void* logits, const void* dlogits) {
  const int64_t eb = elem_bytes(d->dtype);
  bool same = (addr(logits) - addr(dlogits)) % 16 == 0;
  if (d->B > 1) same = same && ((d->x_stride[0] - d->dx_stride[0]) * eb) % 16 == 0;
  if (d->S > 1) same = same && ((d->x_stride[1] - d->dx_stride[1]) * eb) % 16 == 0;
  return !same;
}

}  // namespace
}  // namespace oeh

using namespace oeh;

extern "C" {

int oeh_xent_fwd(const oeh_xent_desc* d, const void* logits, const void* labels, float* lse, float* row_loss, double* out2, float* mean,
                 double* meter, int32_t* bad_rows, void* stream) {
  if (lse == nullptr || out2 == nullptr) return OEH_EINVAL;
  if (d != nullptr && row_loss == nullptr && d->label_smoothing > 0.0f) return OEH_EINVAL;
  const int rc = xent_check(d, logits, labels, false);
  if (rc != OEH_OK) return rc;
  if ((addr(lse) | addr(row_loss) | addr(mean) | addr(bad_rows)) % 4 != 0 || (addr(out2) | addr(meter)) % 8 != 0) return OEH_EALIGN;
  XentArgs a = xent_args(d, logits, labels);
  a.lse = lse; a.row_loss = row_loss; a.out2 = out2; a.mean = mean; a.meter = meter; a.bad_rows = bad_rows;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (a.rows > 0) {
    dispatch_in(a.in, [&](auto t) {
      constexpr int IN = decltype(t)::value;
      if (a.eps_ls > 0.0f) hipLaunchKernelGGL((oeh_xent_fwd_kernel<IN, true>), dim3((unsigned)a.rows), dim3(256), 0, st, a);
      else hipLaunchKernelGGL((oeh_xent_fwd_kernel<IN, false>), dim3((unsigned)a.rows), dim3(256), 0, st, a);
    });
  }
  hipLaunchKernelGGL(oeh_xent_reduce_kernel, dim3(1), dim3(kReduceT), 0, st, a);
  return launch_status();
}

int oeh_xent_bwd(const oeh_xent_desc* d, const void* logits, const void* labels, const float* lse, const double* out2, const float* grad,
                 int64_t grad_stride, void* dlogits, void* stream) {
  if (lse == nullptr || out2 == nullptr || grad == nullptr || dlogits == nullptr || grad_stride < 0) return OEH_EINVAL;
  const int rc = xent_check(d, logits, labels, true);
  if (rc != OEH_OK) return rc;
  if ((addr(lse) | addr(grad)) % 4 != 0 || addr(out2) % 8 != 0 || addr(dlogits) % elem_bytes(d->dtype) != 0) return OEH_EALIGN;
  XentArgs a = xent_args(d, logits, labels);
  a.lse = const_cast<float*>(lse); a.out2 = const_cast<double*>(out2); a.grad = grad; a.grad_stride = grad_stride; a.dx = dlogits;
  if (a.rows == 0) return OEH_OK;
  const bool el = xent_el(d, logits, dlogits);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)a.rows);
  dispatch_in(a.in, [&](auto t) {
    constexpr int IN = decltype(t)::value;
    const bool ls = a.eps_ls > 0.0f;
    if (ls && el) hipLaunchKernelGGL((oeh_xent_bwd_kernel<IN, true, true>), grid, dim3(256), 0, st, a);
    else if (ls) hipLaunchKernelGGL((oeh_xent_bwd_kernel<IN, true, false>), grid, dim3(256), 0, st, a);
    else if (el) hipLaunchKernelGGL((oeh_xent_bwd_kernel<IN, false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((oeh_xent_bwd_kernel<IN, false, false>), grid, dim3(256), 0, st, a);
  });
  return launch_status();
}

const char* oeh_xent_variant(const oeh_xent_desc* d, const void* logits, const void* dlogits) {
  static thread_local char name[48];
  const void* const aligned = reinterpret_cast<const void*>((uintptr_t)4096);  // (the labels are taken as given and aligned)
  if (xent_check(d, logits, aligned, dlogits != nullptr) != OEH_OK) return nullptr;
  if (dlogits != nullptr && addr(dlogits) % elem_bytes(d->dtype) != 0) return nullptr;
  std::snprintf(name, sizeof name, "xent/block/CH%d/%s%s%s", OEH_XENT_SLOTS, dtype_name(d->dtype), d->label_smoothing > 0.0f ? "/ls" : "",
                dlogits != nullptr && xent_el(d, logits, dlogits) ? "/el" : "");
  return name;
}

}  // extern "C"
