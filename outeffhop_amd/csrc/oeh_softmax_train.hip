// The softmax rows of the unfused attention path in TRAINING (include/oeh.h: oeh_softmax_train_fwd / oeh_softmax_train_bwd): scale ->
// additive mask -> clamp -> softmax / softmax_1 -> clip -> dropout in one pass over the (B,H,Sq,Sk) scores, and a backward that recomputes
// the probabilities from the scores and two fp32 numbers per row (the row's max m and denominator den).  Eager, the chain is twelve passes
// and keeps most of its intermediates (attention.unfused_core with softmax.softmax_autograd).
//
// Per row in fp32, every operation rounded on its own (-ffp-contract=off):
//   z = x * scale | x / scale_div;  z += mask;  z = max(z, clamp_min);  m = max z;  e = exp(z - m);  den = sum e [+ exp(-m)];  p = e / den
//   y = RN(clamp(p (eta - gamma) + gamma, 0, 1));  u = RN(keep ? y * inv : 0)
// with oeh_softmax_rows' arithmetic AND summation order per launch form (oeh_rows.hip), so the plain case gives its bits:
//   lanes     the row's elements dealt over G lanes of a wave (G a power of two), VEC contiguous elements per lane and chunk, chunk c of lane
//             g at element (g + G c) VEC; a lane adds its own elements in order, then xor butterflies from G / 2 down to 1.  G = 64, VEC =
//             one 16-byte vector: oeh_softmax_rows_wave_kernel.  G < 64: 64 / G rows per wave - rows of up to 32 16-byte vectors (the
//             same tree as the wave kernel, whose other lanes add zeros), or Sk <= 64 with VEC = 1 where the vector form does not apply (the
//             tree of the staged kernel below, whose other lanes and waves add zeros)
//   block     a 256-thread workgroup per row, thread t the elements t, t + 256, ...: oeh_softmax_rows_kernel<STAGED>
// Backward: g = dy + (keep ? du * inv : 0);  clip: g = (eta - gamma) g inside the closed interval, else 0;  delta = sum p g (the form's
// order);  dz = p (g - delta);  the clamp's gate 1 / 0.5 / 0;  dx = RN(dz * scale | dz / scale_div).
// A row with a NaN (or +inf) z has m = den = NaN and is NaN throughout; a row with den = inf has p = 0 and dx = 0.
#include "oeh_stream.h"
#include "oeh_launch.h"
#include "oeh_desc.h"
#include "oeh_philox.h"

#include <cstdio>

namespace oeh {
namespace {

constexpr int kMaxCols = OEH_SOFTMAX_TRAIN_MAX_COLS;

struct SmtArgs {
  const void *x, *mask;  // mask may be null
  void *y, *u;           // forward: either may be null
  float* stats;          // (rows, 2): m, den
  const void *dy, *du;   // backward: either may be null
  void* dx;
  long rows;
  int H, Sq, Sk;
  int gshift;            // lanes form: log2 of the lanes per row
  long xs[3], ys[3], us[3], ms[3], dys[3], dus[3], dxs[3];
  int ydt, mdt, base, clip, clamp, drop;
  float clip_w, clip_g, scale, scale_div, clamp_min, inv;
  unsigned thr, k0, k1;
};

// ---- N contiguous elements of storage type DT <-> fp32 (N == 1, or N elements aligned to min(16, N * bytes)) -------------------------------
template <int DT, int N>
__device__ __forceinline__ void load_t(const void* p, float* out) {
  if constexpr (N == 1) {
    out[0] = In<DT>::to_f32(*reinterpret_cast<const typename In<DT>::elem*>(p));
  } else if constexpr (DT == IN_F32) {
#pragma unroll
    for (int i = 0; i < N; i += 4) unpack16<IN_F32>(*reinterpret_cast<const u4*>(reinterpret_cast<const char*>(p) + 4 * i), out + i);
  } else if constexpr (N == 8) {
    unpack16<DT>(*reinterpret_cast<const u4*>(p), out);
  } else {
    const u2 w = *reinterpret_cast<const u2*>(p);
    float t[8];
    unpack16<DT>(u4{w[0], w[1], 0u, 0u}, t);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = t[i];
  }
}
template <int DT, int N>
__device__ __forceinline__ void store_t(void* p, const float* v) {
  if constexpr (N == 1) {
    *reinterpret_cast<typename In<DT>::elem*>(p) = In<DT>::from_f32(v[0]);
  } else if constexpr (DT == IN_F32) {
#pragma unroll
    for (int i = 0; i < N; i += 4) *reinterpret_cast<u4*>(reinterpret_cast<char*>(p) + 4 * i) = pack16<IN_F32>(v + i);
  } else if constexpr (N == 8) {
    *reinterpret_cast<u4*>(p) = pack16<DT>(v);
  } else {
    const float t[8] = {v[0], v[1], v[2], v[3], 0.0f, 0.0f, 0.0f, 0.0f};
    const u4 w = pack16<DT>(t);
    *reinterpret_cast<u2*>(p) = u2{w[0], w[1]};
  }
}
// the same with the storage type a (wave-uniform) run-time value: element j0 .. j0 + N - 1 of the row at `row`
template <int N>
__device__ __forceinline__ void load_rt(const int dt, const void* row, const int j0, float* out) {
  if (dt == IN_F32) load_t<IN_F32, N>(reinterpret_cast<const char*>(row) + (long)j0 * 4, out);
  else if (dt == IN_BF16) load_t<IN_BF16, N>(reinterpret_cast<const char*>(row) + (long)j0 * 2, out);
  else load_t<IN_F16, N>(reinterpret_cast<const char*>(row) + (long)j0 * 2, out);
}
template <int N>
__device__ __forceinline__ void store_rt(const int dt, void* row, const int j0, const float* v) {
  if (dt == IN_F32) store_t<IN_F32, N>(reinterpret_cast<char*>(row) + (long)j0 * 4, v);
  else if (dt == IN_BF16) store_t<IN_BF16, N>(reinterpret_cast<char*>(row) + (long)j0 * 2, v);
  else store_t<IN_F16, N>(reinterpret_cast<char*>(row) + (long)j0 * 2, v);
}
// what a value reads back as after its one rounding to the storage type
__device__ __forceinline__ float round_rt(const int dt, const float v) {
  if (dt == IN_F32) return v;
  if (dt == IN_BF16) return In<IN_BF16>::to_f32(In<IN_BF16>::from_f32(v));
  return In<IN_F16>::to_f32(In<IN_F16>::from_f32(v));
}
__device__ __forceinline__ const char* row_at(const void* base, const long* st, const int dt, const long b, const long h, const long i) {
  return reinterpret_cast<const char*>(base) + (b * st[0] + h * st[1] + i * st[2]) * (dt == IN_F32 ? 4 : 2);
}

// ---- the element steps, shared by every form and by both directions ---------------------------------------------------------------------
// z before the clamp; the clamp itself keeps a NaN (torch.max does)
__device__ __forceinline__ float z_pre(const SmtArgs& a, const float xv, const float mv) {
  float z = a.scale_div > 0.0f ? xv / a.scale_div : xv * a.scale;
  if (a.mask != nullptr) z = z + mv;
  return z;
}
__device__ __forceinline__ float z_clamp(const SmtArgs& a, const float z) { return (a.clamp && z < a.clamp_min) ? a.clamp_min : z; }
// for the row maximum: a NaN counts as +inf, and a row whose maximum is +inf is a NaN row
__device__ __forceinline__ float z_key(const float z) { return z != z ? __builtin_inff() : z; }
// den of the row from the sum of its exponentials, NaN for a NaN row
__device__ __forceinline__ float row_den(const SmtArgs& a, const float m, const float sum) {
  float den = sum;
  if (a.base != 0) den = sum + exp_acc(m * -1.0f);
  if (!(m < __builtin_inff())) den = __builtin_nanf("");
  return den;
}
// e / den: the correctly rounded quotient of oeh_softmax_rows_wave_kernel (rden = RN(1 / den)); den = inf: 0
__device__ __forceinline__ float quot(const float e, const float den, const float rden) {
  const float q0 = e * rden;
  float p = __builtin_fmaf(__builtin_fmaf(-q0, den, e), rden, q0);
  if (!(den < 3.0e38f)) p = e / den;
  return p;
}
__device__ __forceinline__ float clip_t(const SmtArgs& a, float p) {
  p = p * a.clip_w;
  return p + a.clip_g;
}
// the clip of the forward (a NaN stays, as under torch.clip)
__device__ __forceinline__ float clip_y(const SmtArgs& a, const float p) {
  if (!a.clip) return p;
  const float t = clip_t(a, p);
  return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
}
__device__ __forceinline__ unsigned word_of(const Philox4& w, const int k) { return k == 0 ? w.x[0] : k == 1 ? w.x[1] : k == 2 ? w.x[2] : w.x[3]; }
// keep bits of the N elements from column j0 of query row i in head bh (N == 1, or j0 % 4 == 0): the attention dropout stream
template <int N>
__device__ __forceinline__ void keep_bits(const SmtArgs& a, const int j0, const unsigned i, const unsigned bh, bool* keep) {
  if constexpr (N == 1) {
    keep[0] = word_of(dropout_words((unsigned)j0 >> 2, i, bh, a.k0, a.k1), j0 & 3) >= a.thr;
  } else {
#pragma unroll
    for (int t = 0; t < N; t += 4) {
      const Philox4 w = dropout_words((unsigned)(j0 + t) >> 2, i, bh, a.k0, a.k1);
#pragma unroll
      for (int k = 0; k < 4; ++k) keep[t + k] = w.x[k] >= a.thr;
    }
  }
}
// the gradient that reaches p: dy + dropout's share of du, then the clip's gate
__device__ __forceinline__ float grad_p(const SmtArgs& a, const float p, const float dyv, const float duv, const bool keep) {
  float g = 0.0f;
  if (a.dy != nullptr) g = dyv;
  if (a.du != nullptr) {
    const float d = keep ? duv * a.inv : 0.0f;
    g = a.dy != nullptr ? g + d : d;
  }
  if (a.clip) {
    const float t = clip_t(a, p);
    g = (t >= 0.0f && t <= 1.0f) ? a.clip_w * g : 0.0f;
  }
  return g;
}
__device__ __forceinline__ float grad_x(const SmtArgs& a, float dz, const float gate) {
  if (a.clamp) dz = dz * gate;
  return a.scale_div > 0.0f ? dz / a.scale_div : dz * a.scale;
}

__device__ __forceinline__ float group_sum(float v, const int G) {
  for (int o = G >> 1; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float group_max(float v, const int G) {
  for (int o = G >> 1; o >= 1; o >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ---- lanes form: the row in the registers of G = 1 << gshift lanes, 64 / G rows per wave, four waves per workgroup ---------------------------
template <int IN, int VEC, int CH, bool BWD>
__global__ __launch_bounds__(256) void oeh_softmax_train_lanes_kernel(const SmtArgs a) {
  const int lane = threadIdx.x & 63;
  const int G = 1 << a.gshift;
  const int g = lane & (G - 1);
  const long row = (((long)blockIdx.x * 4 + (threadIdx.x >> 6)) << (6 - a.gshift)) + (lane >> a.gshift);
  if (row >= a.rows) return;  // (a group's lanes share their row: nobody reads a lane that has left)
  const unsigned bh = (unsigned)(row / a.Sq);
  const unsigned i = (unsigned)(row - (long)bh * a.Sq);
  const long b = bh / (unsigned)a.H, h = bh - (unsigned)b * (unsigned)a.H;
  const int nchunk = a.Sk / VEC;
  const char* xr = row_at(a.x, a.xs, IN, b, h, i);
  const char* mr = a.mask != nullptr ? row_at(a.mask, a.ms, a.mdt, b, h, i) : nullptr;
  float v[CH][VEC];
  unsigned long long lt = 0, eq = 0;  // backward: elements below / at the clamp's floor
  float m = -__builtin_inff();
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = g + G * c;
    if (ch < nchunk) {
      float mv[VEC];
      load_t<IN, VEC>(xr + (long)ch * VEC * In<IN>::bytes, v[c]);
      if (mr != nullptr) load_rt<VEC>(a.mdt, mr, ch * VEC, mv);
#pragma unroll
      for (int t = 0; t < VEC; ++t) {
        const float z = z_pre(a, v[c][t], mr != nullptr ? mv[t] : 0.0f);
        if (BWD && a.clamp) {
          if (z < a.clamp_min) lt |= 1ull << (c * VEC + t);
          if (z == a.clamp_min) eq |= 1ull << (c * VEC + t);
        }
        v[c][t] = z_clamp(a, z);
        if (!BWD) m = __builtin_fmaxf(m, z_key(v[c][t]));
      }
    }
  }
  float den;
  if constexpr (!BWD) {
    m = group_max(m, G);
    float sum = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (g + G * c < nchunk) {
#pragma unroll
        for (int t = 0; t < VEC; ++t) {
          v[c][t] = exp_acc(v[c][t] - m);
          sum += v[c][t];
        }
      }
    }
    sum = group_sum(sum, G);
    den = row_den(a, m, sum);
    if (g == 0) {
      a.stats[2 * row] = den != den ? den : m;
      a.stats[2 * row + 1] = den;
    }
  } else {
    m = a.stats[2 * row];
    den = a.stats[2 * row + 1];
  }
  const float rden = 1.0f / den;
  if constexpr (!BWD) {
    char* yr = a.y != nullptr ? const_cast<char*>(row_at(a.y, a.ys, a.ydt, b, h, i)) : nullptr;
    char* ur = a.u != nullptr ? const_cast<char*>(row_at(a.u, a.us, a.ydt, b, h, i)) : nullptr;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = g + G * c;
      if (ch < nchunk) {
#pragma unroll
        for (int t = 0; t < VEC; ++t) v[c][t] = clip_y(a, quot(v[c][t], den, rden));
        if (yr != nullptr) store_rt<VEC>(a.ydt, yr, ch * VEC, v[c]);
        if (ur != nullptr) {
          bool keep[VEC];
          keep_bits<VEC>(a, ch * VEC, i, bh, keep);
#pragma unroll
          for (int t = 0; t < VEC; ++t) v[c][t] = keep[t] ? round_rt(a.ydt, v[c][t]) * a.inv : 0.0f;
          store_rt<VEC>(a.ydt, ur, ch * VEC, v[c]);
        }
      }
    }
  } else {
    const char* dyr = a.dy != nullptr ? row_at(a.dy, a.dys, a.ydt, b, h, i) : nullptr;
    const char* dur = a.du != nullptr ? row_at(a.du, a.dus, a.ydt, b, h, i) : nullptr;
    char* dxr = const_cast<char*>(row_at(a.dx, a.dxs, IN, b, h, i));
    float gr[CH][VEC];
    float delta = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = g + G * c;
      if (ch < nchunk) {
        float dyv[VEC], duv[VEC];
        bool keep[VEC];
        if (dyr != nullptr) load_rt<VEC>(a.ydt, dyr, ch * VEC, dyv);
        if (dur != nullptr) {
          load_rt<VEC>(a.ydt, dur, ch * VEC, duv);
          keep_bits<VEC>(a, ch * VEC, i, bh, keep);
        }
#pragma unroll
        for (int t = 0; t < VEC; ++t) {
          v[c][t] = quot(exp_acc(v[c][t] - m), den, rden);
          gr[c][t] = grad_p(a, v[c][t], dyr != nullptr ? dyv[t] : 0.0f, dur != nullptr ? duv[t] : 0.0f, dur != nullptr ? keep[t] : false);
          delta += v[c][t] * gr[c][t];
        }
      }
    }
    delta = group_sum(delta, G);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = g + G * c;
      if (ch < nchunk) {
#pragma unroll
        for (int t = 0; t < VEC; ++t) {
          const int bit = c * VEC + t;
          const float gate = ((lt >> bit) & 1) ? 0.0f : ((eq >> bit) & 1) ? 0.5f : 1.0f;
          v[c][t] = grad_x(a, v[c][t] * (gr[c][t] - delta), gate);
        }
        store_t<IN, VEC>(dxr + (long)ch * VEC * In<IN>::bytes, v[c]);
      }
    }
  }
}

// ---- block form: a 256-thread workgroup per row, the row's fp32 values staged in LDS (each thread reads back only what it wrote) ----------------
template <int IN, bool BWD>
__global__ __launch_bounds__(256) void oeh_softmax_train_block_kernel(const SmtArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rowbuf[];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int cols = a.Sk;
  for (long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const unsigned bh = (unsigned)(row / a.Sq);
    const unsigned i = (unsigned)(row - (long)bh * a.Sq);
    const long b = bh / (unsigned)a.H, h = bh - (unsigned)b * (unsigned)a.H;
    const char* xr = row_at(a.x, a.xs, IN, b, h, i);
    const char* mr = a.mask != nullptr ? row_at(a.mask, a.ms, a.mdt, b, h, i) : nullptr;
    auto z_at = [&](const int j, float& gate) {
      float xv, mv = 0.0f;
      load_t<IN, 1>(xr + (long)j * In<IN>::bytes, &xv);
      if (mr != nullptr) load_rt<1>(a.mdt, mr, j, &mv);
      const float z = z_pre(a, xv, mv);
      gate = z < a.clamp_min ? 0.0f : (z == a.clamp_min ? 0.5f : 1.0f);
      return z_clamp(a, z);
    };
    if constexpr (!BWD) {
      float lmax = -__builtin_inff(), gate;
      for (int j = tid; j < cols; j += 256) {
        const float z = z_at(j, gate);
        rowbuf[j] = z;
        lmax = __builtin_fmaxf(lmax, z_key(z));
      }
      lmax = wave_max(lmax);
      __syncthreads();
      if ((tid & 63) == 0) red[tid >> 6] = lmax;
      __syncthreads();
      const float m = block4_max(red);
      float lsum = 0.0f;
      for (int j = tid; j < cols; j += 256) {
        const float e = exp_acc(rowbuf[j] - m);
        rowbuf[j] = e;
        lsum += e;
      }
      lsum = wave_sum(lsum);
      __syncthreads();
      if ((tid & 63) == 0) red[tid >> 6] = lsum;
      __syncthreads();
      const float sum = ((red[0] + red[1]) + red[2]) + red[3];  // (wave order, as oeh_softmax_rows_kernel)
      const float den = row_den(a, m, sum);
      const float rden = 1.0f / den;
      if (tid == 0) {
        a.stats[2 * row] = den != den ? den : m;
        a.stats[2 * row + 1] = den;
      }
      char* yr = a.y != nullptr ? const_cast<char*>(row_at(a.y, a.ys, a.ydt, b, h, i)) : nullptr;
      char* ur = a.u != nullptr ? const_cast<char*>(row_at(a.u, a.us, a.ydt, b, h, i)) : nullptr;
      for (int j = tid; j < cols; j += 256) {
        float yv = clip_y(a, quot(rowbuf[j], den, rden));
        if (yr != nullptr) store_rt<1>(a.ydt, yr, j, &yv);
        if (ur != nullptr) {
          bool keep;
          keep_bits<1>(a, j, i, bh, &keep);
          float uv = keep ? round_rt(a.ydt, yv) * a.inv : 0.0f;
          store_rt<1>(a.ydt, ur, j, &uv);
        }
      }
    } else {
      const float m = a.stats[2 * row], den = a.stats[2 * row + 1];
      const float rden = 1.0f / den;
      const char* dyr = a.dy != nullptr ? row_at(a.dy, a.dys, a.ydt, b, h, i) : nullptr;
      const char* dur = a.du != nullptr ? row_at(a.du, a.dus, a.ydt, b, h, i) : nullptr;
      char* dxr = const_cast<char*>(row_at(a.dx, a.dxs, IN, b, h, i));
      auto g_at = [&](const int j, const float p) {
        float dyv = 0.0f, duv = 0.0f;
        bool keep = false;
        if (dyr != nullptr) load_rt<1>(a.ydt, dyr, j, &dyv);
        if (dur != nullptr) {
          load_rt<1>(a.ydt, dur, j, &duv);
          keep_bits<1>(a, j, i, bh, &keep);
        }
        return grad_p(a, p, dyv, duv, keep);
      };
      float acc = 0.0f, gate;
      for (int j = tid; j < cols; j += 256) {
        const float p = quot(exp_acc(z_at(j, gate) - m), den, rden);
        rowbuf[j] = p;
        acc += p * g_at(j, p);
      }
      acc = wave_sum(acc);
      __syncthreads();
      if ((tid & 63) == 0) red[tid >> 6] = acc;
      __syncthreads();
      const float delta = ((red[0] + red[1]) + red[2]) + red[3];
      for (int j = tid; j < cols; j += 256) {
        const float p = rowbuf[j];
        gate = 1.0f;
        if (a.clamp) (void)z_at(j, gate);
        float dxv = grad_x(a, p * (g_at(j, p) - delta), gate);
        store_t<IN, 1>(dxr + (long)j * In<IN>::bytes, &dxv);
      }
    }
    __syncthreads();
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
bool drop_bad(const oeh_dropout& drop) { return !(drop.p >= 0.0f && drop.p < 1.0f) || drop.reserved != 0; }

bool strides_neg(const int64_t* s) { return s[0] < 0 || s[1] < 0 || s[2] < 0; }
bool out_stride_short(const oeh_softmax_train_desc* d, const int64_t* s) {
  return (d->B > 1 && s[0] < d->Sk) || (d->H > 1 && s[1] < d->Sk) || (d->Sq > 1 && s[2] < d->Sk);
}

// the descriptor's refusals behind the dropout and pointer checks, in the order include/oeh.h lists them
int check_desc(const oeh_softmax_train_desc* d, const bool with_mask, const bool with_y, const bool with_u, const bool backward, const bool with_dy,
               const bool with_du) {
  if (!dtype_ok(d->x_dtype) || !dtype_ok(d->y_dtype) || (with_mask && !dtype_ok(d->mask_dtype))) return OEH_EINVAL;
  if (d->y_dtype != d->x_dtype && d->y_dtype != OEH_F32) return OEH_EINVAL;
  if (d->Sk < 1 || d->B < 0 || d->H < 0 || d->Sq < 0) return OEH_EINVAL;
  if (strides_neg(d->x_stride) || strides_neg(d->y_stride) || strides_neg(d->u_stride) || strides_neg(d->mask_stride) || strides_neg(d->dy_stride) ||
      strides_neg(d->du_stride) || strides_neg(d->dx_stride))
    return OEH_EINVAL;
  if (!backward && ((with_y && out_stride_short(d, d->y_stride)) || (with_u && out_stride_short(d, d->u_stride)))) return OEH_EINVAL;
  if (backward && out_stride_short(d, d->dx_stride)) return OEH_EINVAL;
  if (!softmax_base_ok(d->softmax_base)) return OEH_EINVAL;
  if (d->clip && !(d->eta > d->gamma)) return OEH_EINVAL;
  if (!(d->scale_div >= 0.0f)) return OEH_EINVAL;
  if (d->scale != d->scale || d->gamma != d->gamma || d->eta != d->eta) return OEH_EINVAL;
  if (d->Sk > kMaxCols || (int64_t)d->B * d->H * d->Sq >= ((int64_t)1 << 31)) return OEH_ENOTSUP;
  return OEH_OK;
}

enum { FORM_LANES = 0, FORM_WAVE = 1, FORM_BLOCK = 2 };
struct Plan {
  int form, vec, ch, gshift;
};
int ceil_log2(int n) {
  int s = 0;
  while ((1 << s) < n) ++s;
  return s;
}
// vec16: Sk is a multiple of x's 16-byte vector and every row of every given tensor starts on a 16-byte boundary
Plan plan_of(const int Sk, const int x_dtype, const bool vec16) {
  const int N = vec16_elems(x_dtype);
  if (vec16) {
    const int nchunk = Sk / N;
    // (up to 32 vectors: as many lanes as the row has vectors, rounded up to a power of two - the short rows, and the rows of a few hundred
    // elements that would leave most of a wave idle)
    if (nchunk <= 32) return Plan{FORM_LANES, N, 1, ceil_log2(nchunk)};
    if (nchunk <= 512) return Plan{FORM_WAVE, N, nchunk <= 64 ? 1 : nchunk <= 128 ? 2 : nchunk <= 256 ? 4 : 8, 6};
    return Plan{FORM_BLOCK, 1, 1, 0};
  }
  if (Sk <= 64) return Plan{FORM_LANES, 1, 1, ceil_log2(Sk)};
  return Plan{FORM_BLOCK, 1, 1, 0};
}
bool rows16(const void* p, const int64_t* st, const int dt) { return p == nullptr || aligned16(p, st, elem_bytes(dt)); }

void fill(SmtArgs& a, const oeh_softmax_train_desc* d) {
  a.rows = (long)d->B * d->H * d->Sq;
  a.H = d->H; a.Sq = d->Sq; a.Sk = d->Sk;
  for (int k = 0; k < 3; ++k) {
    a.xs[k] = d->x_stride[k]; a.ys[k] = d->y_stride[k]; a.us[k] = d->u_stride[k]; a.ms[k] = d->mask_stride[k];
    a.dys[k] = d->dy_stride[k]; a.dus[k] = d->du_stride[k]; a.dxs[k] = d->dx_stride[k];
  }
  a.ydt = d->y_dtype; a.mdt = d->mask_dtype; a.base = d->softmax_base; a.clip = d->clip ? 1 : 0; a.clamp = d->clamp ? 1 : 0;
  a.clip_w = (float)((double)d->eta - (double)d->gamma);  // (as fill_problem: formed in double, rounded once)
  a.clip_g = d->gamma;
  a.scale = d->scale; a.scale_div = d->scale_div; a.clamp_min = d->clamp_min;
  a.drop = d->drop.p > 0.0f ? 1 : 0;
  a.inv = 1.0f / (1.0f - d->drop.p);
  a.thr = dropout_threshold(d->drop.p);
  a.k0 = (unsigned)(d->drop.seed & 0xffffffffu);
  a.k1 = (unsigned)(d->drop.seed >> 32);
}

template <bool BWD>
int launch(const oeh_softmax_train_desc* d, SmtArgs& a, const Plan pl, hipStream_t st) {
  a.gshift = pl.gshift;
  if (pl.form == FORM_BLOCK) {
    const unsigned grid = (unsigned)(a.rows < 65536 ? a.rows : 65536);
    dispatch_in(d->x_dtype, [&](auto t) {
      hipLaunchKernelGGL((oeh_softmax_train_block_kernel<decltype(t)::value, BWD>), dim3(grid), dim3(256), (size_t)a.Sk * 4, st, a);
    });
    return launch_status();
  }
  const long rows_per_wg = 4L << (6 - pl.gshift);
  const unsigned grid = (unsigned)((a.rows + rows_per_wg - 1) / rows_per_wg);
  dispatch_in(d->x_dtype, [&](auto t) {
    constexpr int IN = decltype(t)::value;
    constexpr int N = Vec16<IN>::N;
#define OEH_SMT(VEC_, CH_) hipLaunchKernelGGL((oeh_softmax_train_lanes_kernel<IN, VEC_, CH_, BWD>), dim3(grid), dim3(256), 0, st, a)
    if (pl.vec == 1) OEH_SMT(1, 1);
    else if (pl.ch == 1) OEH_SMT(N, 1);
    else if (pl.ch == 2) OEH_SMT(N, 2);
    else if (pl.ch == 4) OEH_SMT(N, 4);
    else OEH_SMT(N, 8);
#undef OEH_SMT
  });
  return launch_status();
}

}  // namespace
}  // namespace oeh

using namespace oeh;

extern "C" {

int oeh_softmax_train_fwd(const oeh_softmax_train_desc* d, const void* x, const void* mask, void* y, void* u, float* stats, void* stream) {
  if (d != nullptr && (drop_bad(d->drop) || d->reserved != 0)) return OEH_EINVAL;
  if (d == nullptr || x == nullptr || stats == nullptr) return OEH_EINVAL;
  if ((y == nullptr && u == nullptr) || (u != nullptr && !(d->drop.p > 0.0f))) return OEH_EINVAL;
  const int rc = check_desc(d, mask != nullptr, y != nullptr, u != nullptr, false, false, false);
  if (rc != OEH_OK) return rc;
  if ((int64_t)d->B * d->H * d->Sq == 0) return OEH_OK;
  const bool vec16 = d->Sk % vec16_elems(d->x_dtype) == 0 && rows16(x, d->x_stride, d->x_dtype) && rows16(mask, d->mask_stride, d->mask_dtype) &&
                     rows16(y, d->y_stride, d->y_dtype) && rows16(u, d->u_stride, d->y_dtype);
  SmtArgs a = {};
  a.x = x; a.mask = mask; a.y = y; a.u = u; a.stats = stats;
  fill(a, d);
  return launch<false>(d, a, plan_of(d->Sk, d->x_dtype, vec16), reinterpret_cast<hipStream_t>(stream));
}

int oeh_softmax_train_bwd(const oeh_softmax_train_desc* d, const void* x, const void* mask, const float* stats, const void* dy, const void* du, void* dx,
                          void* stream) {
  if (d != nullptr && (drop_bad(d->drop) || d->reserved != 0)) return OEH_EINVAL;
  if (d == nullptr || x == nullptr || stats == nullptr || dx == nullptr) return OEH_EINVAL;
  if (du != nullptr && !(d->drop.p > 0.0f)) return OEH_EINVAL;
  if (dy == nullptr && du == nullptr) return OEH_EINVAL;
  const int rc = check_desc(d, mask != nullptr, false, false, true, dy != nullptr, du != nullptr);
  if (rc != OEH_OK) return rc;
  if ((int64_t)d->B * d->H * d->Sq == 0) return OEH_OK;
  const bool vec16 = d->Sk % vec16_elems(d->x_dtype) == 0 && rows16(x, d->x_stride, d->x_dtype) && rows16(mask, d->mask_stride, d->mask_dtype) &&
                     rows16(dy, d->dy_stride, d->y_dtype) && rows16(du, d->du_stride, d->y_dtype) && rows16(dx, d->dx_stride, d->x_dtype);
  SmtArgs a = {};
  a.x = x; a.mask = mask; a.stats = const_cast<float*>(stats); a.dy = dy; a.du = du; a.dx = dx;
  fill(a, d);
  return launch<true>(d, a, plan_of(d->Sk, d->x_dtype, vec16), reinterpret_cast<hipStream_t>(stream));
}

const char* oeh_softmax_train_variant(const oeh_softmax_train_desc* d, int backward) {
  static thread_local char name[128];
  if (d == nullptr || drop_bad(d->drop) || d->reserved != 0) return nullptr;
  // (a mask where mask_dtype names a storage type, y / dy always, u / du with dropout; every tensor taken as 16-byte aligned where its
  // strides are)
  const bool with_mask = dtype_ok(d->mask_dtype);
  const bool drop = d->drop.p > 0.0f;
  if (check_desc(d, with_mask, true, drop, backward != 0, true, drop) != OEH_OK) return nullptr;
  auto st16 = [](const int64_t* s, int dt) { return aligned16(nullptr, s, elem_bytes(dt)); };
  bool vec16 = d->Sk % vec16_elems(d->x_dtype) == 0 && st16(d->x_stride, d->x_dtype) && (!with_mask || st16(d->mask_stride, d->mask_dtype));
  if (!backward) vec16 = vec16 && st16(d->y_stride, d->y_dtype) && (!drop || st16(d->u_stride, d->y_dtype));
  else vec16 = vec16 && st16(d->dy_stride, d->y_dtype) && (!drop || st16(d->du_stride, d->y_dtype)) && st16(d->dx_stride, d->x_dtype);
  const Plan pl = plan_of(d->Sk, d->x_dtype, vec16);
  char form[32];
  if (pl.form == FORM_BLOCK) std::snprintf(form, sizeof form, "block");
  else if (pl.form == FORM_WAVE) std::snprintf(form, sizeof form, "wave/CH%d", pl.ch);
  else std::snprintf(form, sizeof form, "lanes/G%dx%d", 1 << pl.gshift, pl.vec);
  char ydt[16] = "";
  if (d->y_dtype != d->x_dtype) std::snprintf(ydt, sizeof ydt, ">%s", dtype_name(d->y_dtype));
  std::snprintf(name, sizeof name, "softmax_train/%s/%s/%s%s/%s%s%s%s%s", backward ? "bwd" : "fwd", form, dtype_name(d->x_dtype), ydt,
                d->softmax_base == OEH_SOFTMAX_ONE ? "softmax1" : "softmax", d->clip ? "/clip" : "", with_mask ? "/mask" : "", d->clamp ? "/clamp" : "",
                drop ? "/drop" : "");
  return name;
}

}  // extern "C"
