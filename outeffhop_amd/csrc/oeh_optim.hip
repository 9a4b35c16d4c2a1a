// The optimizer phase of a training step over ALL parameter tensors of a model at once (include/oeh.h: oeh_mt_plan, oeh_grad_norm,
// oeh_grad_scale, oeh_adamw_step): what the reference's loops do after backward() - accelerator.clip_grad_norm_ and then the step of a
// torch.optim.AdamW over a decay and a no-decay group (run_clm.py:440-462, 589-601; run_mlm.py the same).  Eager, that is a norm per tensor,
// a stack, a norm of norms, a multiply over every gradient and the foreach chain of the update: a dozen passes over parameter-sized tensors
// in several hundred launches.  Here the gradients are read once for the norm, and one launch reads g, p, m, v and writes p, m, v:
// 32 bytes per parameter with fp32 gradients.
//
//   * The plan (host): a 16-byte entry per workgroup {tensor, count, offset} - a chunk of at most OEH_MT_CHUNK = 4096 elements of ONE tensor -
//     followed by a 56-byte record per tensor.  blockIdx.x is the entry: both reads are scalar loads.  Offsets are 64-bit.
//   * A workgroup of 256 threads holds its whole chunk in registers: 16 elements per thread and tensor, every load issued before the first
//     value is used (64 KiB in flight per workgroup in the step kernel) and every load of a thread before its first store.
//   * Two access forms per tensor, decided by the plan.  vec16: thread t owns the elements [4 (k * 256 + t), + 4), k = 0..3 - one 16-byte
//     access of p, m, v and one of 16 (fp32) or 8 (16-bit) bytes of g; in a tensor's last chunk a group of four that reaches past the end is
//     done element by element.  elem (a pointer that does not allow it): thread t owns the elements k * 256 + t, k = 0..15, one each.
//   * Norm: per chunk sum (double)g * (double)g - every product exact - a thread's 16 in index order, the wave butterflies, the four waves as
//     (0 + 1) + (2 + 3); the second launch adds the chunk partials in a fixed order too.  No atomics: the same bits on every call.
//   * Step: fp32, every operation rounded on its own (-ffp-contract=off), plain `/` and sqrt (correctly rounded, denormals kept); the
//     per-group constants are formed in double by the host and rounded once.  The clip coefficient is read from the device.
//   * Under fp16 loss scaling (oeh_grad_norm_amp, oeh_adamw_step_amp, oeh_loss_scale_update): the norm's finalize divides the scale out of
//     norm and coefficient and raises the flag when the sum is not finite; the step is the same body behind one uniform early return on
//     that flag, with the two constants that depend on the step number formed on the device from fp32 counters kept there (a launch of one
//     thread per tensor); the scale's update is one thread.  Nothing is read back and the gradients get no pass of their own.
#include "../../include/oeh.h"
#include "oeh_desc.h"
#include "oeh_launch.h"
#include "oeh_stream.h"

#include <cmath>
#include <cstring>

namespace oeh {
namespace {

constexpr int kChunk = OEH_MT_CHUNK;  // elements of a chunk
constexpr int kPer = kChunk / 256;    // elements per thread: 16
constexpr int kMaxGroups = OEH_MT_MAX_GROUPS;
static_assert(kChunk == 4096 && kPer == 16, "a thread's share of a chunk is four 16-byte accesses of fp32");

struct MtEntry {
  int tensor, count;
  long off;
};
struct MtRec {
  void* p;
  const void* g;
  void* m;
  void* v;
  long n;
  int g_dtype, group, vec16, zero;
};
static_assert(sizeof(MtEntry) == OEH_MT_ENTRY_BYTES && sizeof(MtRec) == OEH_MT_RECORD_BYTES, "the plan's layout is part of include/oeh.h");

// a launch's view of the plan
struct MtArgs {
  const MtEntry* entries;
  const MtRec* recs;
};
// the step's constants per group (RN32 of include/oeh.h)
struct AdamwArgs {
  MtArgs mt;
  const double* clip;  // may be null
  int n_groups;
  float decay[kMaxGroups], omb1[kMaxGroups], b2[kMaxGroups], omb2[kMaxGroups], bc2[kMaxGroups], eps[kMaxGroups], ss[kMaxGroups];
};
struct GroupK {
  float decay, omb1, b2, omb2, bc2, eps, ss;
};

enum { MT_VEC_FULL = 0, MT_VEC_PART = 1, MT_ELEM = 2 };

__device__ __forceinline__ const MtRec& chunk_of(const MtArgs& a, long& off, int& cnt) {
  const MtEntry e = a.entries[blockIdx.x];
  off = e.off;
  cnt = e.count;
  return a.recs[e.tensor];
}

// four elements of storage type IN from two (16-bit) or four (fp32) words
template <int IN>
__device__ __forceinline__ void unpack4(const u4 w, float* out) {
  if constexpr (IN == IN_F32) {
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = bits_f32(w[i]);
  } else if constexpr (IN == IN_BF16) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      out[2 * i] = bits_f32(w[i] << 16);
      out[2 * i + 1] = bits_f32(w[i] & 0xffff0000u);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const h2 p = __builtin_bit_cast(h2, (unsigned)w[i]);
      out[2 * i] = (float)p[0];
      out[2 * i + 1] = (float)p[1];
    }
  }
}
// The tensors' addresses come out of the plan, not out of the kernel's arguments: said to be global memory here, or every access is a flat one
// that counts against the LDS counter as well.
template <class T>
__device__ __forceinline__ T gload(const void* p) {
  return *(const __attribute__((address_space(1))) T*)p;
}
template <class T>
__device__ __forceinline__ void gstore(void* p, const T v) {
  *(__attribute__((address_space(1))) T*)p = v;
}
template <int IN>
__device__ __forceinline__ u4 load4(const void* p) {
  if constexpr (IN == IN_F32) {
    return gload<u4>(p);
  } else {
    const u2 w = gload<u2>(p);
    return u4{w[0], w[1], 0u, 0u};
  }
}
// (the 16-bit conversion is the packed one in BOTH forms: written as a scalar conversion behind the product the compiler may fold the two
// into one mixed-precision fma - ONE rounding where the contract has two; oeh_xent.hip: xent_store)
template <int IN>
__device__ __forceinline__ u4 pack4(const float* x) {
  if constexpr (IN == IN_F32) return u4{f32_bits(x[0]), f32_bits(x[1]), f32_bits(x[2]), f32_bits(x[3])};
  else return u4{pack2<IN>(x[0], x[1]), pack2<IN>(x[2], x[3]), 0u, 0u};
}
template <int IN>
__device__ __forceinline__ void store4(void* p, const u4 w) {
  if constexpr (IN == IN_F32) gstore<u4>(p, w);
  else gstore<u2>(p, u2{w[0], w[1]});
}
template <int IN>
__device__ __forceinline__ void store1(typename In<IN>::elem* p, const u4 w, const int e) {
  if constexpr (IN == IN_F32) gstore<float>(p, bits_f32(w[e]));
  else gstore<unsigned short>(p, (unsigned short)(w[e >> 1] >> (16 * (e & 1))));
}

// Thread t's 16 elements of the chunk [off, off + cnt) of `base` as fp32; elements past cnt are 0.
// MT_VEC_*: x[4 k + e] = element 4 (k * 256 + t) + e;  MT_ELEM: x[k] = element k * 256 + t.
template <int IN, int MODE>
__device__ __forceinline__ void mt_load(const void* base, const long off, const int cnt, const int t, float (&x)[kPer]) {
  typedef typename In<IN>::elem E;
  const E* b = reinterpret_cast<const E*>(base) + off;
  if constexpr (MODE == MT_VEC_FULL) {
    u4 raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) raw[k] = load4<IN>(b + (k * 256 + t) * 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) unpack4<IN>(raw[k], &x[4 * k]);
  } else if constexpr (MODE == MT_VEC_PART) {
    u4 raw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = (k * 256 + t) * 4;
      raw[k] = u4{0u, 0u, 0u, 0u};
      if (o + 4 <= cnt) raw[k] = load4<IN>(b + o);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) unpack4<IN>(raw[k], &x[4 * k]);
    // (the one group of four that the end of the tensor cuts: one thread's, element by element)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = (k * 256 + t) * 4;
      if (o < cnt && o + 4 > cnt) {
#pragma unroll
        for (int e = 0; e < 3; ++e)
          if (o + e < cnt) x[4 * k + e] = In<IN>::to_f32(gload<E>(b + o + e));
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int o = k * 256 + t;
      x[k] = o < cnt ? In<IN>::to_f32(gload<E>(b + o)) : 0.0f;
    }
  }
}
template <int IN, int MODE>
__device__ __forceinline__ void mt_store(void* base, const long off, const int cnt, const int t, const float (&x)[kPer]) {
  typedef typename In<IN>::elem E;
  E* b = reinterpret_cast<E*>(base) + off;
  if constexpr (MODE == MT_ELEM) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u4 w = pack4<IN>(&x[4 * k]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int o = (4 * k + e) * 256 + t;
        if (o < cnt) store1<IN>(b + o, w, e);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = (k * 256 + t) * 4;
      const u4 w = pack4<IN>(&x[4 * k]);
      if (MODE == MT_VEC_FULL || o + 4 <= cnt) {
        store4<IN>(b + o, w);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (o + e < cnt) store1<IN>(b + o + e, w, e);
      }
    }
  }
}

// f(storage type of g, access mode) for the chunk's tensor - every condition is uniform over the workgroup
template <class F>
__device__ __forceinline__ void dispatch_chunk(const int g_dtype, const int vec16, const int cnt, F&& f) {
  auto modes = [&](auto in) {
    if (!vec16) f(in, std::integral_constant<int, MT_ELEM>{});
    else if (cnt == kChunk) f(in, std::integral_constant<int, MT_VEC_FULL>{});
    else f(in, std::integral_constant<int, MT_VEC_PART>{});
  };
  if (g_dtype == IN_F32) modes(std::integral_constant<int, IN_F32>{});
  else if (g_dtype == IN_BF16) modes(std::integral_constant<int, IN_BF16>{});
  else modes(std::integral_constant<int, IN_F16>{});
}

// ---- the norm: one float64 partial per chunk, then one workgroup over the partials
__global__ __launch_bounds__(256) void oeh_mt_sumsq_kernel(const MtArgs a, double* __restrict__ partial) {
  __shared__ double red[4];
  const int t = threadIdx.x;
  long off;
  int cnt;
  const MtRec& r = chunk_of(a, off, cnt);
  const void* g = r.g;
  double acc = 0.0;
  dispatch_chunk(r.g_dtype, r.vec16, cnt, [&](auto in, auto mode) {
    float x[kPer];
    mt_load<decltype(in)::value, decltype(mode)::value>(g, off, cnt, t, x);
#pragma unroll
    for (int i = 0; i < kPer; ++i) acc += (double)x[i] * (double)x[i];
  });
  acc = wave_sum(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

constexpr int kNormT = 1024, kNormU = 8;  // threads of the second launch; partials a thread has in flight
// the sum of the chunk partials in the fixed order of include/oeh.h; thread 0 has it
__device__ __forceinline__ double norm_sumsq(const double* __restrict__ partial, const long n) {
  constexpr int W = kNormT / 64;
  __shared__ double red[W];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (long base = t; base < n; base += (long)kNormT * kNormU) {
    double v[kNormU];
#pragma unroll
    for (int u = 0; u < kNormU; ++u) {
      const long i = base + (long)kNormT * u;
      v[u] = i < n ? partial[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kNormU; ++u) acc += v[u];  // (ascending)
  }
  acc = wave_sum(acc);
  if ((t & 63) == 0) red[t >> 6] = acc;
  __syncthreads();
  double s[W];
  if (t == 0) {
#pragma unroll
    for (int w = 0; w < W; ++w) s[w] = red[w];
#pragma unroll
    for (int w = W / 2; w >= 1; w >>= 1)
#pragma unroll
      for (int i = 0; i < w; ++i) s[i] = s[2 * i] + s[2 * i + 1];
  } else {
    s[0] = 0.0;
  }
  return s[0];
}
// oeh_grad_norm's coefficient from a norm: 1 when max_norm <= 0, NaN or +inf
__device__ __forceinline__ double clip_coef(const double norm, const double max_norm) {
  double coef = 1.0;
  if (max_norm > 0.0 && max_norm < __builtin_inf()) {
    const double c = max_norm / (norm + 1e-6);
    coef = c > 1.0 ? 1.0 : c;  // (NaN stays NaN, as torch's clamp)
  }
  return coef;
}

// the finalize under loss scaling (include/oeh.h: oeh_grad_norm_amp): the same sum, the scale divided out of norm and coefficient, the flag
__global__ __launch_bounds__(kNormT) void oeh_mt_norm_amp_kernel(const double* __restrict__ partial, const long n, const double max_norm,
                                                                 const float* __restrict__ grad_scale, const float* __restrict__ found_in,
                                                                 float* __restrict__ found_acc, double* __restrict__ out4) {
  const double sumsq = norm_sumsq(partial, n);
  if (threadIdx.x == 0) {
    const double s = grad_scale != nullptr ? (double)*grad_scale : 1.0;
    const bool s_ok = s > 0.0 && s < __builtin_inf();
    const bool finite = __builtin_fabs(sumsq) < __builtin_inf();  // (false for NaN)
    const bool found = !finite || (found_in != nullptr && *found_in != 0.0f) || !s_ok;
    const double norm = __builtin_sqrt(sumsq) / s;
    out4[0] = sumsq;
    out4[1] = norm;
    out4[2] = clip_coef(norm, max_norm) / s;
    out4[3] = found ? 1.0 : 0.0;
    if (found && found_acc != nullptr) *found_acc = 1.0f;
  }
}

__global__ __launch_bounds__(kNormT) void oeh_mt_norm_kernel(const double* __restrict__ partial, const long n, const double max_norm,
                                                             double* __restrict__ out4) {
  const double sumsq = norm_sumsq(partial, n);
  if (threadIdx.x == 0) {
    const double norm = __builtin_sqrt(sumsq);
    out4[0] = sumsq;
    out4[1] = norm;
    out4[2] = clip_coef(norm, max_norm);
    out4[3] = 0.0;
  }
}

// ---- the stand-alone clip
__global__ __launch_bounds__(256) void oeh_mt_scale_kernel(const MtArgs a, const double* __restrict__ clip) {
  const int t = threadIdx.x;
  long off;
  int cnt;
  const MtRec& r = chunk_of(a, off, cnt);
  void* g = const_cast<void*>(r.g);
  const float c = (float)clip[2];
  dispatch_chunk(r.g_dtype, r.vec16, cnt, [&](auto in, auto mode) {
    constexpr int IN = decltype(in)::value, MODE = decltype(mode)::value;
    float x[kPer];
    mt_load<IN, MODE>(g, off, cnt, t, x);
#pragma unroll
    for (int i = 0; i < kPer; ++i) x[i] = x[i] * c;
    mt_store<IN, MODE>(g, off, cnt, t, x);
  });
}

// ---- the step
// the loss-scaling form's arguments: bc2 and ss per plan record from the advance launch, the other five constants per group from the host
struct AdamwAmpArgs {
  MtArgs mt;
  const double* clip;  // required: clip[2] the coefficient, clip[3] != 0 skips the step
  const float* work;   // {bc2, ss} per record
  int n_groups;
  float decay[kMaxGroups], omb1[kMaxGroups], b2[kMaxGroups], omb2[kMaxGroups], eps[kMaxGroups];
};
struct AdvanceArgs {
  const MtRec* recs;
  const double* clip;
  float* steps;
  const int* slot;
  float* work;
  int n_tensors, n_groups;
  float lr[kMaxGroups], b1[kMaxGroups], b2[kMaxGroups];
};

// One body for both kernels: AMP = false is oeh_adamw_step's launch, AMP = true the step under loss scaling - the skip in front, bc2 and
// ss from the device; the arithmetic per element is the same text.
template <bool AMP, class Args>
__device__ __forceinline__ void adamw_body(const Args& a) {
  if constexpr (AMP) {
    if (a.clip[3] != 0.0) return;  // (uniform) an overflow was found: p, m and v are neither read nor written
  }
  const int t = threadIdx.x;
  const MtEntry e = a.mt.entries[blockIdx.x];
  const long off = e.off;
  const int cnt = e.count;
  const MtRec& r = a.mt.recs[e.tensor];
  const void* gp = r.g;
  void *pp = r.p, *mp = r.m, *vp = r.v;
  const int grp = r.group;
  if (grp < 0 || grp >= a.n_groups) return;  // (uniform) a tensor of a group the descriptor does not have is left as it is
  GroupK k;
  float c;
  if constexpr (AMP) {
    k = GroupK{a.decay[grp], a.omb1[grp], a.b2[grp], a.omb2[grp], a.work[2 * e.tensor], a.eps[grp], a.work[2 * e.tensor + 1]};
    c = (float)a.clip[2];
  } else {
    k = GroupK{a.decay[grp], a.omb1[grp], a.b2[grp], a.omb2[grp], a.bc2[grp], a.eps[grp], a.ss[grp]};
    c = a.clip != nullptr ? (float)a.clip[2] : 1.0f;
  }
  dispatch_chunk(r.g_dtype, r.vec16, cnt, [&](auto in, auto mode) {
    constexpr int IN = decltype(in)::value, MODE = decltype(mode)::value;
    float g[kPer], p[kPer], m[kPer], v[kPer];
    mt_load<IN, MODE>(gp, off, cnt, t, g);
    mt_load<IN_F32, MODE>(pp, off, cnt, t, p);
    mt_load<IN_F32, MODE>(mp, off, cnt, t, m);
    mt_load<IN_F32, MODE>(vp, off, cnt, t, v);
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const float gc = g[i] * c;
      const float p1 = p[i] * k.decay;
      const float mn = m[i] + (gc - m[i]) * k.omb1;
      const float vn = v[i] * k.b2 + (gc * gc) * k.omb2;
      const float den = __builtin_sqrtf(vn) / k.bc2 + k.eps;
      p[i] = p1 - k.ss * (mn / den);
      m[i] = mn;
      v[i] = vn;
    }
    mt_store<IN_F32, MODE>(pp, off, cnt, t, p);
    mt_store<IN_F32, MODE>(mp, off, cnt, t, m);
    mt_store<IN_F32, MODE>(vp, off, cnt, t, v);
  });
}
__global__ __launch_bounds__(256) void oeh_adamw_kernel(const AdamwArgs a) { adamw_body<false>(a); }
__global__ __launch_bounds__(256) void oeh_adamw_amp_kernel(const AdamwAmpArgs a) { adamw_body<true>(a); }

// beta^n by binary exponentiation (include/oeh.h): IEEE multiplications only, so that numpy gives the same bits
__device__ __forceinline__ double pw(const double beta, long n) {
  double r = 1.0, base = beta;
  while (n) {
    if (n & 1) r *= base;
    n >>= 1;
    if (n) base *= base;
  }
  return r;
}
// the counters: one thread per plan record
__global__ __launch_bounds__(256) void oeh_adamw_advance_kernel(const AdvanceArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_tensors) return;
  const int grp = a.recs[i].group;
  if (grp < 0 || grp >= a.n_groups) return;
  const bool found = a.clip[3] != 0.0;
  const int j = a.slot[i];
  const float t = a.steps[j] + (found ? 0.0f : 1.0f);
  if (!found) a.steps[j] = t;
  float bc2 = 0.0f, ss = 0.0f;
  if (t >= 1.0f) {
    const long n = (long)t;
    bc2 = (float)__builtin_sqrt(1.0 - pw((double)a.b2[grp], n));
    ss = (float)((double)a.lr[grp] / (1.0 - pw((double)a.b1[grp], n)));
  }
  a.work[2 * i] = bc2;
  a.work[2 * i + 1] = ss;
}

// the loss scale (include/oeh.h: oeh_loss_scale_update): one thread
__global__ void oeh_loss_scale_kernel(float* __restrict__ st, const float growth, const float backoff, const float interval) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float scale = st[0], tracker = st[1], skipped = st[3];
  if (st[2] != 0.0f) {
    scale = scale * backoff;
    tracker = 0.0f;
    skipped = skipped + 1.0f;
  } else if (tracker + 1.0f == interval) {
    const float ns = scale * growth;
    if (__builtin_fabsf(ns) < __builtin_inff()) scale = ns;
    tracker = 0.0f;
  } else {
    tracker = tracker + 1.0f;
  }
  st[0] = scale;
  st[1] = tracker;
  st[2] = 0.0f;
  st[3] = skipped;
}

// ---- host
int elem_size(const int dtype) { return dtype == OEH_F32 ? 4 : 2; }

int tensor_check(const oeh_mt_tensor& t) {
  if (t.n < 0 || t.p == nullptr || t.g == nullptr || t.m == nullptr || t.v == nullptr) return OEH_EINVAL;
  if (t.group < 0 || t.group >= kMaxGroups || !dtype_ok(t.g_dtype)) return OEH_EINVAL;
  if ((addr(t.p) | addr(t.m) | addr(t.v)) % 4 != 0 || addr(t.g) % elem_size(t.g_dtype) != 0) return OEH_EALIGN;
  return OEH_OK;
}
bool tensor_vec16(const oeh_mt_tensor& t) {
  return all16(addr(t.p) | addr(t.m) | addr(t.v)) && addr(t.g) % (4 * elem_size(t.g_dtype)) == 0;
}
int plan_count(const oeh_mt_tensor* t, const int32_t n_tensors, int64_t& chunks) {
  chunks = 0;
  if (n_tensors < 0 || (t == nullptr && n_tensors > 0)) return OEH_EINVAL;
  for (int32_t i = 0; i < n_tensors; ++i) {
    const int rc = tensor_check(t[i]);
    if (rc != OEH_OK) return rc;
    chunks += t[i].n / kChunk + (t[i].n % kChunk != 0);
  }
  return chunks >= ((int64_t)1 << 31) ? OEH_ENOTSUP : OEH_OK;
}
MtArgs plan_view(const void* plan_dev, const int64_t n_chunks) {
  const char* b = static_cast<const char*>(plan_dev);
  return MtArgs{reinterpret_cast<const MtEntry*>(b), reinterpret_cast<const MtRec*>(b + n_chunks * (int64_t)sizeof(MtEntry))};
}
int plan_args_check(const void* plan_dev, const int64_t n_chunks) {
  if (n_chunks < 0 || (plan_dev == nullptr && n_chunks > 0)) return OEH_EINVAL;
  return n_chunks >= ((int64_t)1 << 31) ? OEH_ENOTSUP : OEH_OK;
}

bool hyper_ok(const oeh_adamw_desc& d, const int i) {
  if (!(d.lr[i] >= 0.0f) || !(d.eps[i] >= 0.0f) || !(d.weight_decay[i] >= 0.0f)) return false;
  return d.beta1[i] >= 0.0f && d.beta1[i] < 1.0f && d.beta2[i] >= 0.0f && d.beta2[i] < 1.0f;
}

}  // namespace
}  // namespace oeh

using namespace oeh;

extern "C" {

int64_t oeh_mt_plan_bytes(const oeh_mt_tensor* t, int32_t n_tensors) {
  int64_t chunks;
  if (plan_count(t, n_tensors, chunks) != OEH_OK) return -1;
  return chunks * (int64_t)sizeof(MtEntry) + (int64_t)n_tensors * (int64_t)sizeof(MtRec);
}

int oeh_mt_plan(const oeh_mt_tensor* t, int32_t n_tensors, void* plan_host, int64_t* n_chunks) {
  if (n_chunks == nullptr) return OEH_EINVAL;
  int64_t chunks;
  const int rc = plan_count(t, n_tensors, chunks);
  if (rc != OEH_OK) return rc;
  if (addr(plan_host) % 8 != 0) return OEH_EALIGN;
  *n_chunks = chunks;
  if (plan_host == nullptr) return OEH_OK;
  MtEntry* e = static_cast<MtEntry*>(plan_host);
  MtRec* recs = reinterpret_cast<MtRec*>(e + chunks);
  for (int32_t i = 0; i < n_tensors; ++i) {
    for (int64_t off = 0; off < t[i].n; off += kChunk) *e++ = MtEntry{i, (int)(t[i].n - off < kChunk ? t[i].n - off : kChunk), (long)off};
    recs[i] = MtRec{t[i].p, t[i].g, t[i].m, t[i].v, (long)t[i].n, t[i].g_dtype, t[i].group, tensor_vec16(t[i]) ? 1 : 0, 0};
  }
  return OEH_OK;
}

const char* oeh_mt_variant(const oeh_mt_tensor* t) {
  if (t == nullptr || tensor_check(*t) != OEH_OK) return nullptr;
  return tensor_vec16(*t) ? "vec16" : "elem";
}

int64_t oeh_grad_norm_work_bytes(int64_t n_chunks) { return n_chunks < 0 ? 0 : n_chunks * (int64_t)sizeof(double); }

int oeh_grad_norm(const void* plan_dev, int64_t n_chunks, double max_norm, void* work, double* out4, void* stream) {
  if (out4 == nullptr || (work == nullptr && n_chunks > 0)) return OEH_EINVAL;
  const int rc = plan_args_check(plan_dev, n_chunks);
  if (rc != OEH_OK) return rc;
  if ((addr(work) | addr(out4)) % 8 != 0) return OEH_EALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n_chunks > 0) hipLaunchKernelGGL(oeh_mt_sumsq_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, plan_view(plan_dev, n_chunks), static_cast<double*>(work));
  hipLaunchKernelGGL(oeh_mt_norm_kernel, dim3(1), dim3(kNormT), 0, st, static_cast<const double*>(work), (long)n_chunks, max_norm, out4);
  return launch_status();
}

int oeh_grad_scale(const void* plan_dev, int64_t n_chunks, const double* clip4, void* stream) {
  if (clip4 == nullptr) return OEH_EINVAL;
  const int rc = plan_args_check(plan_dev, n_chunks);
  if (rc != OEH_OK) return rc;
  if (addr(clip4) % 8 != 0) return OEH_EALIGN;
  if (n_chunks == 0) return OEH_OK;
  hipLaunchKernelGGL(oeh_mt_scale_kernel, dim3((unsigned)n_chunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), plan_view(plan_dev, n_chunks), clip4);
  return launch_status();
}

int oeh_adamw_step(const void* plan_dev, int64_t n_chunks, const oeh_adamw_desc* d, const double* clip4, void* stream) {
  if (d == nullptr || d->n_groups < 1 || d->n_groups > kMaxGroups || d->reserved != 0) return OEH_EINVAL;
  AdamwArgs a;
  std::memset(&a, 0, sizeof a);
  for (int i = 0; i < d->n_groups; ++i) {
    if (d->step[i] < 1 || !hyper_ok(*d, i)) return OEH_EINVAL;
    const double lr = d->lr[i], b1 = d->beta1[i], b2 = d->beta2[i], wd = d->weight_decay[i], t = (double)d->step[i];
    a.decay[i] = (float)(1.0 - lr * wd);
    a.omb1[i] = (float)(1.0 - b1);
    a.b2[i] = d->beta2[i];
    a.omb2[i] = (float)(1.0 - b2);
    a.bc2[i] = (float)std::sqrt(1.0 - std::pow(b2, t));
    a.eps[i] = d->eps[i];
    a.ss[i] = (float)(lr / (1.0 - std::pow(b1, t)));
  }
  const int rc = plan_args_check(plan_dev, n_chunks);
  if (rc != OEH_OK) return rc;
  if (addr(clip4) % 8 != 0) return OEH_EALIGN;
  if (n_chunks == 0) return OEH_OK;
  a.mt = plan_view(plan_dev, n_chunks);
  a.clip = clip4;
  a.n_groups = d->n_groups;
  hipLaunchKernelGGL(oeh_adamw_kernel, dim3((unsigned)n_chunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return launch_status();
}

int oeh_grad_norm_amp(const void* plan_dev, int64_t n_chunks, double max_norm, const float* grad_scale, const float* found_in, float* found_acc,
                      void* work, double* out4, void* stream) {
  if (out4 == nullptr || (work == nullptr && n_chunks > 0)) return OEH_EINVAL;
  const int rc = plan_args_check(plan_dev, n_chunks);
  if (rc != OEH_OK) return rc;
  if ((addr(work) | addr(out4)) % 8 != 0 || (addr(grad_scale) | addr(found_in) | addr(found_acc)) % 4 != 0) return OEH_EALIGN;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n_chunks > 0) hipLaunchKernelGGL(oeh_mt_sumsq_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, plan_view(plan_dev, n_chunks), static_cast<double*>(work));
  hipLaunchKernelGGL(oeh_mt_norm_amp_kernel, dim3(1), dim3(kNormT), 0, st, static_cast<const double*>(work), (long)n_chunks, max_norm, grad_scale, found_in,
                     found_acc, out4);
  return launch_status();
}

int64_t oeh_adamw_amp_work_bytes(int32_t n_tensors) { return n_tensors < 0 ? 0 : (int64_t)n_tensors * 8; }

int oeh_adamw_step_amp(const void* plan_dev, int64_t n_chunks, int32_t n_tensors, const oeh_adamw_desc* d, const double* clip4, float* steps,
                       const int32_t* slot, void* work, void* stream) {
  if (d == nullptr || d->n_groups < 1 || d->n_groups > kMaxGroups || d->reserved != 0 || n_tensors < 0) return OEH_EINVAL;
  AdamwAmpArgs a;
  AdvanceArgs adv;
  std::memset(&a, 0, sizeof a);
  std::memset(&adv, 0, sizeof adv);
  for (int i = 0; i < d->n_groups; ++i) {
    if (!hyper_ok(*d, i)) return OEH_EINVAL;
    const double lr = d->lr[i], b1 = d->beta1[i], b2 = d->beta2[i], wd = d->weight_decay[i];
    a.decay[i] = (float)(1.0 - lr * wd);
    a.omb1[i] = (float)(1.0 - b1);
    a.b2[i] = d->beta2[i];
    a.omb2[i] = (float)(1.0 - b2);
    a.eps[i] = d->eps[i];
    adv.lr[i] = d->lr[i];
    adv.b1[i] = d->beta1[i];
    adv.b2[i] = d->beta2[i];
  }
  const int rc = plan_args_check(plan_dev, n_chunks);
  if (rc != OEH_OK) return rc;
  if (n_chunks > 0 && (clip4 == nullptr || steps == nullptr || slot == nullptr || work == nullptr)) return OEH_EINVAL;
  if (addr(clip4) % 8 != 0 || (addr(steps) | addr(slot) | addr(work)) % 4 != 0) return OEH_EALIGN;
  if (n_chunks == 0) return OEH_OK;
  a.mt = plan_view(plan_dev, n_chunks);
  a.clip = clip4;
  a.work = static_cast<const float*>(work);
  a.n_groups = d->n_groups;
  adv.recs = a.mt.recs;
  adv.clip = clip4;
  adv.steps = steps;
  adv.slot = slot;
  adv.work = static_cast<float*>(work);
  adv.n_tensors = n_tensors;
  adv.n_groups = d->n_groups;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (n_tensors > 0) hipLaunchKernelGGL(oeh_adamw_advance_kernel, dim3((unsigned)((n_tensors + 255) / 256)), dim3(256), 0, st, adv);
  hipLaunchKernelGGL(oeh_adamw_amp_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, a);
  return launch_status();
}

int oeh_loss_scale_update(float* state4, double growth_factor, double backoff_factor, int32_t growth_interval, void* stream) {
  if (state4 == nullptr || growth_interval < 1) return OEH_EINVAL;
  if (!(growth_factor > 0.0 && std::isfinite(growth_factor)) || !(backoff_factor > 0.0 && std::isfinite(backoff_factor))) return OEH_EINVAL;
  if (addr(state4) % 4 != 0) return OEH_EALIGN;
  hipLaunchKernelGGL(oeh_loss_scale_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), state4, (float)growth_factor, (float)backoff_factor,
                     (float)growth_interval);
  return launch_status();
}

}  // extern "C"
