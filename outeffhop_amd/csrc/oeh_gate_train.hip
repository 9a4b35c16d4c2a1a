// The conditional per-token gate in TRAINING (include/oeh.h: oeh_gate_apply_fwd / oeh_gate_apply_bwd): per-head predictor -> sigmoid ->
// context * gate, forward and backward - what attention.gate_autograd and attention.gated_merge do as torch ops (H small Linear or
// Linear-ReLU-Linear modules on strided slices, stack, sigmoid, multiply: about 40 launches forward and well over a hundred backward for
// 12 heads with an MLP predictor).
//
// Forward, two launches: the gate probabilities by oeh_gate_fwd's own launch (scaling 1: gate_out has its bits), then the product kernel -
// a thread per 16 bytes of a (token, head) row: out[b, t, h d + j] = RN(fp32(ctx[b, h, t, j]) * (gate_out[b, h, t] * scaling)).
//
// Backward, two launches, no atomics.  Row kernel: a workgroup is ONE wave and takes tiles of 64 consecutive tokens of one head, lane =
// token.  Per token (phase A): dctx in fp32; then, in float64 (what feeds a sum over tokens: include/oeh.h says why), the row's dot product
// sum_j dout_j ctx_j, the logit once more - the token's d inputs in registers, the hidden units one after the other with the weights as
// scalar loads (the unit index is wave-uniform, as in oeh_gate_logit_fast_kernel) -, the ReLU's decisions as a bit mask, pi and dz; and in
// fp32 dhidden += da_j * W1[j] over the units.  x, r_j, dz and the mask of the tile go to LDS (rows padded to an odd length: the column
// writes of phase A and the row reads of phase B are conflict-free).  Phase B turns the tile round: lane = input feature k, and for every
// token in ascending order the lane adds dz * x_k to the accumulator of every unit whose bit is set (the bit is wave-uniform here), lane j
// also [u_j > 0] dz and dz r_j - float64 registers that live across the tiles the workgroup walks; w2_j multiplies once at the end.  Then
// ONE record per (workgroup, head) in `work`, laid out as the outputs one after the other.  Reduce kernel: per output element 16 slices of
// the workgroup list, each added in ascending order, then a pairwise tree over the slices, one rounding to fp32.
#include "../../include/oeh.h"
#include "oeh_desc.h"
#include "oeh_launch.h"
#include "oeh_stream.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace oeh {
namespace {

constexpr int kTile = 64;                                // tokens of a tile: the lanes of the wave
constexpr int kMaxGroups = OEH_GATE_TRAIN_MAX_GROUPS;    // workgroups of the backward's row kernel, over all heads
constexpr int kSlices = 16;                              // of the workgroup list, per output element, in the reduce kernel
constexpr int kMaxUnits = 64;
constexpr int kMaxHeads = 65535;                         // the head is the grids' y

struct GateFwdArgs {
  const void* ctx;
  const float* gate;
  void* out;
  long nth;  // B * T * H
  int T, H;
  long cs_b, cs_h, cs_t, os_b, os_t;
  float scaling;
};

struct GateBwdArgs {
  const void *dout, *ctx, *hidden;
  const float *gate, *w1, *b1, *w2, *b2;
  void *dctx, *dhidden;  // dhidden may be null
  double* work;
  long ntok, ntiles;
  int T, H, m, tiles_per_wg;
  long rec;  // doubles of a record
  long hs_b, hs_t, cs_b, cs_h, cs_t, os_b, os_t, dcs_b, dcs_h, dcs_t, dhs_b, dhs_t;
  float scaling;
};

// ---- forward: context * gate ---------------------------------------------------------------------------------------------------------
template <int IN, int D>
__global__ __launch_bounds__(256) void oeh_gate_apply_fwd_kernel(const GateFwdArgs p) {
  typedef typename In<IN>::elem E;
  constexpr int NV = Vec16<IN>::N, CPR = D / NV;  // 16-byte chunks of a (token, head) row
  const long total = p.nth * CPR;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long th = idx / CPR;
    const int c = (int)(idx - th * CPR);
    const long bt = th / p.H;
    const int h = (int)(th - bt * p.H);
    const long b = bt / p.T;
    const int t = (int)(bt - b * p.T);
    const float g = p.gate[(b * p.H + h) * p.T + t] * p.scaling;
    float v[NV];
    Vec16<IN>::load(reinterpret_cast<const E*>(p.ctx) + b * p.cs_b + (long)h * p.cs_h + (long)t * p.cs_t + c * NV, v);
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = v[i] * g;
    Vec16<IN>::store(reinterpret_cast<E*>(p.out) + b * p.os_b + (long)t * p.os_t + (long)h * D + c * NV, v);
  }
}

// ---- backward: rows ------------------------------------------------------------------------------------------------------------------
// MP: 0 - Linear(d, 1); else the hidden units the registers and LDS rows are laid out for (16, 32, 64 >= m)
template <int IN, int D, int MP>
__global__ __launch_bounds__(64) void oeh_gate_train_bwd_kernel(const GateBwdArgs p) {
  typedef typename In<IN>::elem E;
  constexpr int NV = Vec16<IN>::N;
  constexpr int MR = MP == 0 ? 1 : MP;
  constexpr int XS = D + 1, AS = MR + 1;  // odd row lengths
  __shared__ float xs[kTile * XS];                         // x[token][k]
  __shared__ double rs[MP == 0 ? 1 : kTile * AS];          // r_j[token][j], float64
  __shared__ double dzs[kTile];                            // dz[token], float64
  __shared__ unsigned long long act[kTile];                // bit j: u_j[token] > 0
  const int lane = (int)threadIdx.x;
  const int h = (int)blockIdx.y;
  const int m = MP == 0 ? 1 : p.m;  // rows of w1 of a head (wave-uniform)
  const float* wh = p.w1 + (long)h * m * D;
  const float* b1h = p.b1 + (long)h * m;
  const float* w2h = MP == 0 ? nullptr : p.w2 + (long)h * m;

  double aw[MR];  // sum over tokens of [u_j > 0] dz x[lane]: dW1[j][lane] / w2_j
#pragma unroll
  for (int j = 0; j < MR; ++j) aw[j] = 0.0;
  double ab1 = 0.0, aw2 = 0.0, ab2 = 0.0;  // lane j: sum [u_j > 0] dz (db1_j / w2_j), sum dz r_j (dw2_j); sum dz
  const int kx = lane & (D - 1);           // (d = 32: the upper half of the wave repeats the lower and writes nothing)
  const int jl = lane < MR ? lane : 0;

  const long tile0 = (long)blockIdx.x * p.tiles_per_wg;
  const long tile1 = tile0 + p.tiles_per_wg < p.ntiles ? tile0 + p.tiles_per_wg : p.ntiles;
  for (long tile = tile0; tile < tile1; ++tile) {
    // ---- phase A: lane = token
    long tok = tile * kTile + lane;
    const bool live = tok < p.ntok;
    if (!live) tok = p.ntok - 1;
    const long b = tok / p.T;
    const int t = (int)(tok - b * p.T);
    const float g = p.gate[(b * p.H + h) * p.T + t] * p.scaling;
    const E* dor = reinterpret_cast<const E*>(p.dout) + b * p.os_b + (long)t * p.os_t + (long)h * D;
    const E* cr = reinterpret_cast<const E*>(p.ctx) + b * p.cs_b + (long)h * p.cs_h + (long)t * p.cs_t;
    E* dcr = reinterpret_cast<E*>(p.dctx) + b * p.dcs_b + (long)h * p.dcs_h + (long)t * p.dcs_t;
    double dot = 0.0;  // sum_j dout_j ctx_j, j ascending (the products are exact in float64)
#pragma unroll
    for (int k = 0; k < D; k += NV) {
      float a[NV], c[NV], o[NV];
      Vec16<IN>::load(dor + k, a);
      Vec16<IN>::load(cr + k, c);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        o[i] = a[i] * g;
        dot = __builtin_fma((double)a[i], (double)c[i], dot);
      }
      if (live) Vec16<IN>::store(dcr + k, o);
    }

    float x[D];
    const E* xr = reinterpret_cast<const E*>(p.hidden) + b * p.hs_b + (long)t * p.hs_t + (long)h * D;
#pragma unroll
    for (int k = 0; k < D; k += NV) Vec16<IN>::load(xr + k, &x[k]);
#pragma unroll
    for (int k = 0; k < D; ++k) xs[lane * XS + k] = live ? x[k] : 0.0f;

    // the logit once more, in float64 (k ascending per unit, the units ascending), with the ReLU's decisions as a bit mask
    double z = 0.0;
    unsigned long long mk = 0;
    if constexpr (MP == 0) {
#pragma unroll
      for (int k = 0; k < D; ++k) z = __builtin_fma((double)x[k], (double)wh[k], z);
      z = z + (double)b1h[0];
    } else {
      for (int j = 0; j < m; ++j) {
        const float* wr = wh + (long)j * D;  // wave-uniform: scalar loads
        double u = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) u = __builtin_fma((double)x[k], (double)wr[k], u);
        u = u + (double)b1h[j];
        const bool on = u > 0.0;  // the ReLU passes nothing at 0
        const double r = on ? u : 0.0;
        if (on) mk |= 1ull << j;
        rs[lane * AS + j] = r;
        z = __builtin_fma(r, (double)w2h[j], z);
      }
      for (int j = m; j < MP; ++j) rs[lane * AS + j] = 0.0;  // (the units the layout has and the predictor has not)
      z = z + (double)p.b2[h];
    }
    const double pi = 1.0 / (1.0 + exp(-z));
    const double dz = live ? (((double)p.scaling * dot) * pi) * (1.0 - pi) : 0.0;
    dzs[lane] = dz;
    act[lane] = live ? mk : 0ull;

    if (p.dhidden != nullptr) {  // dhidden_h = sum_j da_j W1[j] in fp32, j ascending, da_j = [u_j > 0] RN(dz) * w2_j
      const float dz32 = (float)dz;
      float dh[D];
      if constexpr (MP == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) dh[k] = dz32 * wh[k];
      } else {
#pragma unroll
        for (int k = 0; k < D; ++k) dh[k] = 0.0f;
        for (int j = 0; j < m; ++j) {
          const float* wr = wh + (long)j * D;
          const float da = ((mk >> j) & 1ull) ? dz32 * w2h[j] : 0.0f;
#pragma unroll
          for (int k = 0; k < D; ++k) dh[k] = dh[k] + da * wr[k];
        }
      }
      if (live) {
        E* dhr = reinterpret_cast<E*>(p.dhidden) + b * p.dhs_b + (long)t * p.dhs_t + (long)h * D;
#pragma unroll
        for (int k = 0; k < D; k += NV) Vec16<IN>::store(dhr + k, &dh[k]);
      }
    }
    __syncthreads();

    // ---- phase B: lane = input feature; the tile's tokens in ascending order
    const long left = p.ntok - tile * kTile;
    const int nlive = left < kTile ? (int)left : kTile;
    for (int tk = 0; tk < nlive; ++tk) {
      const double dzv = dzs[tk];
      const double dzx = dzv * (double)xs[tk * XS + kx];
      if constexpr (MP == 0) {
        aw[0] += dzx;
      } else {
        const unsigned long long mv = act[tk];  // (one address for the wave: the unit's decision is wave-uniform here)
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)mv), hi = __builtin_amdgcn_readfirstlane((unsigned)(mv >> 32));
#pragma unroll
        for (int j = 0; j < MR; ++j) aw[j] += (((j < 32 ? lo >> (j & 31) : hi >> (j & 31)) & 1u) ? dzx : 0.0);
        const double rv = rs[tk * AS + jl];
        aw2 = __builtin_fma(dzv, rv, aw2);
        ab1 += rv > 0.0 ? dzv : 0.0;
      }
      ab2 += dzv;
    }
    __syncthreads();  // (the next tile writes the arrays again)
  }

  // ---- one record per (workgroup, head): [dw1 | db1] or [dw1 | db1 | dw2 | db2]
  double* rec = p.work + ((long)blockIdx.x * p.H + h) * p.rec;
  if constexpr (MP == 0) {
    if (lane < D) rec[lane] = aw[0];
    if (lane == 0) rec[D] = ab2;
  } else {
#pragma unroll
    for (int j = 0; j < MR; ++j) {
      if (j < m && lane < D) rec[j * D + lane] = aw[j] * (double)w2h[j];
    }
    if (lane < m) {
      rec[m * D + lane] = ab1 * (double)w2h[lane];
      rec[m * D + m + lane] = aw2;
    }
    if (lane == 0) rec[m * D + 2 * m] = ab2;
  }
}

// ---- backward: the records over the workgroups -----------------------------------------------------------------------------------------
// 256 threads: 16 output elements x 16 slices of the workgroup list; units == 0: m = 0
__global__ __launch_bounds__(256) void oeh_gate_train_reduce_kernel(const double* __restrict__ work, const int groups, const int H, const int D, const int m,
                                                                    const long rec, float* __restrict__ dw1, float* __restrict__ db1,
                                                                    float* __restrict__ dw2, float* __restrict__ db2) {
  __shared__ double sh[kSlices][16];
  const int el = (int)(threadIdx.x & 15), slice = (int)(threadIdx.x >> 4);
  const long e = (long)blockIdx.x * 16 + el;
  const int h = (int)blockIdx.y;
  const int per = (groups + kSlices - 1) / kSlices;
  const int g0 = slice * per, g1 = g0 + per < groups ? g0 + per : groups;
  double a = 0.0;
  if (e < rec) {
#pragma unroll 4
    for (int g = g0; g < g1; ++g) a += work[((long)g * H + h) * rec + e];
  }
  sh[slice][el] = a;
  __syncthreads();
  if (slice == 0 && e < rec) {
    double v[kSlices];
#pragma unroll
    for (int k = 0; k < kSlices; ++k) v[k] = sh[k][el];
#pragma unroll
    for (int w = 1; w < kSlices; w *= 2) {
#pragma unroll
      for (int k = 0; k < kSlices; k += 2 * w) v[k] = v[k] + v[k + w];
    }
    const float r = (float)v[0];  // the one rounding to fp32
    if (m == 0) {
      if (e < D) dw1[(long)h * D + e] = r;
      else db1[h] = r;
    } else {
      const long md = (long)m * D;
      if (e < md) dw1[(long)h * md + e] = r;
      else if (e < md + m) db1[(long)h * m + (e - md)] = r;
      else if (e < md + 2 * m) dw2[(long)h * m + (e - md - m)] = r;
      else db2[h] = r;
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
bool strides_nonneg(const int64_t* st, const int n) {
  for (int i = 0; i < n; ++i)
    if (st[i] < 0) return false;
  return true;
}

// the descriptor's own refusals (no pointers)
int check_inval(const oeh_gate_train_desc* d, const bool backward) {
  if (d->B < 1 || d->T < 1 || d->H < 1 || d->d < 1 || d->units < 0 || !dtype_ok(d->dtype) || d->reserved != 0) return OEH_EINVAL;
  if (!strides_nonneg(d->hidden_stride, 2) || !strides_nonneg(d->ctx_stride, 3) || !strides_nonneg(d->out_stride, 2)) return OEH_EINVAL;
  if (backward && (!strides_nonneg(d->dctx_stride, 3) || !strides_nonneg(d->dhidden_stride, 2))) return OEH_EINVAL;
  if (!std::isfinite(d->scaling)) return OEH_EINVAL;
  return OEH_OK;
}
int check_scope(const int B, const int T, const int H, const int d, const int units) {
  if ((d != 32 && d != 64) || units > kMaxUnits || H > kMaxHeads || (int64_t)B * T * H >= ((int64_t)1 << 31)) return OEH_ENOTSUP;
  return OEH_OK;
}
bool rows16(const void* p, const int64_t* st, const int n, const int eb) {
  uintptr_t o = addr(p);
  for (int i = 0; i < n; ++i) o |= (uintptr_t)(st[i] * eb);
  return all16(o);
}
int check_align(const oeh_gate_train_desc* d, const void* hidden, const void* ctx, const void* out, const bool backward, const void* dctx,
                const void* dhidden, const void* work) {
  const int eb = elem_bytes(d->dtype);
  if (!rows16(hidden, d->hidden_stride, 2, eb) || !rows16(ctx, d->ctx_stride, 3, eb) || !rows16(out, d->out_stride, 2, eb)) return OEH_EALIGN;
  if (backward) {
    if (!rows16(dctx, d->dctx_stride, 3, eb)) return OEH_EALIGN;
    if (dhidden != nullptr && !rows16(dhidden, d->dhidden_stride, 2, eb)) return OEH_EALIGN;
    if ((addr(work) & 7) != 0) return OEH_EALIGN;
  }
  return OEH_OK;
}

// the backward's slabs: workgroups per head (= records per head in `work`) and tiles per workgroup
struct BwdPlan {
  long ntok, ntiles, groups, rec;
  int tiles_per_wg, mp;
};
BwdPlan bwd_plan(const int B, const int T, const int H, const int d, const int units) {
  BwdPlan pl;
  pl.ntok = (long)B * T;
  pl.ntiles = (pl.ntok + kTile - 1) / kTile;
  const long max_groups = std::max<long>(1, kMaxGroups / H);
  pl.tiles_per_wg = (int)((pl.ntiles + max_groups - 1) / max_groups);
  pl.groups = (pl.ntiles + pl.tiles_per_wg - 1) / pl.tiles_per_wg;
  pl.rec = units > 0 ? (long)units * d + 2 * units + 1 : d + 1;
  pl.mp = units == 0 ? 0 : units <= 16 ? 16 : units <= 32 ? 32 : 64;
  return pl;
}

template <class F>
int dispatch_d(const int d, F&& f) {
  if (d == 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}
template <class F>
int dispatch_mp(const int mp, F&& f) {
  switch (mp) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    default: return f(std::integral_constant<int, 64>{});
  }
}

}  // namespace
}  // namespace oeh

using namespace oeh;

extern "C" {

int oeh_gate_apply_fwd(const oeh_gate_train_desc* d, const void* hidden, const float* w1, const float* b1, const float* w2, const float* b2,
                       const void* ctx, float* gate_out, void* out, void* stream) {
  if (d == nullptr || hidden == nullptr || w1 == nullptr || b1 == nullptr || ctx == nullptr || gate_out == nullptr || out == nullptr) return OEH_EINVAL;
  int rc = check_inval(d, false);
  if (rc != OEH_OK) return rc;
  if (d->units > 0 && (w2 == nullptr || b2 == nullptr)) return OEH_EINVAL;
  if ((rc = check_scope(d->B, d->T, d->H, d->d, d->units)) != OEH_OK) return rc;
  if ((rc = check_align(d, hidden, ctx, out, false, nullptr, nullptr, nullptr)) != OEH_OK) return rc;
  rc = oeh_gate_fwd(hidden, d->dtype, d->B, d->T, d->H, d->d, d->hidden_stride[0], d->hidden_stride[1], w1, b1, w2, b2, d->units, 0, 1.0f, gate_out,
                    stream);
  if (rc != OEH_OK) return rc;
  GateFwdArgs a = {};
  a.ctx = ctx; a.gate = gate_out; a.out = out;
  a.nth = (long)d->B * d->T * d->H;
  a.T = d->T; a.H = d->H;
  a.cs_b = d->ctx_stride[0]; a.cs_h = d->ctx_stride[1]; a.cs_t = d->ctx_stride[2];
  a.os_b = d->out_stride[0]; a.os_t = d->out_stride[1];
  a.scaling = d->scaling;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long chunks = a.nth * (d->d / vec16_elems(d->dtype));
  const unsigned grid = (unsigned)std::min<long>((chunks + 255) / 256, 8192);
  dispatch_in(d->dtype, [&](auto in) {
    constexpr int IN = decltype(in)::value;
    return dispatch_d(d->d, [&](auto dd) {
      hipLaunchKernelGGL((oeh_gate_apply_fwd_kernel<IN, decltype(dd)::value>), dim3(grid), dim3(256), 0, st, a);
      return 0;
    });
  });
  return launch_status();
}

int64_t oeh_gate_apply_bwd_work_bytes(int32_t B, int32_t T, int32_t H, int32_t d, int32_t units) {
  if (B < 1 || T < 1 || H < 1 || d < 1 || units < 0) return OEH_EINVAL;
  const int rc = check_scope(B, T, H, d, units);
  if (rc != OEH_OK) return rc;
  const BwdPlan pl = bwd_plan(B, T, H, d, units);
  return (int64_t)pl.groups * H * pl.rec * (int64_t)sizeof(double);
}

int oeh_gate_apply_bwd(const oeh_gate_train_desc* d, const void* dout, const void* ctx, const void* hidden, const float* gate_out, const float* w1,
                       const float* b1, const float* w2, const float* b2, void* dctx, void* dhidden, float* dw1, float* db1, float* dw2, float* db2,
                       void* work, void* stream) {
  if (d == nullptr || dout == nullptr || ctx == nullptr || hidden == nullptr || gate_out == nullptr || w1 == nullptr || b1 == nullptr ||
      dctx == nullptr || dw1 == nullptr || db1 == nullptr || work == nullptr)
    return OEH_EINVAL;
  int rc = check_inval(d, true);
  if (rc != OEH_OK) return rc;
  if (d->units > 0 && (w2 == nullptr || b2 == nullptr || dw2 == nullptr || db2 == nullptr)) return OEH_EINVAL;
  if ((rc = check_scope(d->B, d->T, d->H, d->d, d->units)) != OEH_OK) return rc;
  if ((rc = check_align(d, hidden, ctx, dout, true, dctx, dhidden, work)) != OEH_OK) return rc;
  const BwdPlan pl = bwd_plan(d->B, d->T, d->H, d->d, d->units);
  GateBwdArgs a = {};
  a.dout = dout; a.ctx = ctx; a.hidden = hidden; a.gate = gate_out; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.dctx = dctx; a.dhidden = dhidden; a.work = static_cast<double*>(work);
  a.ntok = pl.ntok; a.ntiles = pl.ntiles; a.T = d->T; a.H = d->H; a.m = d->units; a.tiles_per_wg = pl.tiles_per_wg; a.rec = pl.rec;
  a.hs_b = d->hidden_stride[0]; a.hs_t = d->hidden_stride[1];
  a.cs_b = d->ctx_stride[0]; a.cs_h = d->ctx_stride[1]; a.cs_t = d->ctx_stride[2];
  a.os_b = d->out_stride[0]; a.os_t = d->out_stride[1];
  a.dcs_b = d->dctx_stride[0]; a.dcs_h = d->dctx_stride[1]; a.dcs_t = d->dctx_stride[2];
  a.dhs_b = d->dhidden_stride[0]; a.dhs_t = d->dhidden_stride[1];
  a.scaling = d->scaling;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)pl.groups, (unsigned)d->H);
  dispatch_in(d->dtype, [&](auto in) {
    constexpr int IN = decltype(in)::value;
    return dispatch_d(d->d, [&](auto dd) {
      constexpr int D = decltype(dd)::value;
      return dispatch_mp(pl.mp, [&](auto mp) {
        hipLaunchKernelGGL((oeh_gate_train_bwd_kernel<IN, D, decltype(mp)::value>), grid, dim3(64), 0, st, a);
        return 0;
      });
    });
  });
  if ((rc = launch_status()) != OEH_OK) return rc;
  hipLaunchKernelGGL(oeh_gate_train_reduce_kernel, dim3((unsigned)((pl.rec + 15) / 16), (unsigned)d->H), dim3(256), 0, st, a.work, (int)pl.groups, d->H,
                     d->d, d->units, pl.rec, dw1, db1, dw2, db2);
  return launch_status();
}

const char* oeh_gate_apply_variant(const oeh_gate_train_desc* d, int backward) {
  static thread_local char name[64];
  if (d == nullptr || check_inval(d, backward != 0) != OEH_OK || check_scope(d->B, d->T, d->H, d->d, d->units) != OEH_OK) return nullptr;
  const int eb = elem_bytes(d->dtype);  // (every pointer taken as given and aligned: the strides alone)
  const void* z = nullptr;
  if (!rows16(z, d->hidden_stride, 2, eb) || !rows16(z, d->ctx_stride, 3, eb) || !rows16(z, d->out_stride, 2, eb)) return nullptr;
  if (backward && (!rows16(z, d->dctx_stride, 3, eb) || !rows16(z, d->dhidden_stride, 2, eb))) return nullptr;
  if (!backward) {
    std::snprintf(name, sizeof name, "gate_train/fwd/D%d/M%d/%s", d->d, d->units, dtype_name(d->dtype));
  } else {
    const BwdPlan pl = bwd_plan(d->B, d->T, d->H, d->d, d->units);
    std::snprintf(name, sizeof name, "gate_train/bwd/D%d/M%d/%s/G%ldx%d", d->d, d->units, dtype_name(d->dtype), pl.groups, pl.tiles_per_wg);
  }
  return name;
}

}  // extern "C"
