// Attention core for TRAINING on gfx950 (MI355X): a forward that also writes the row statistic lse, and a FlashAttention-style
// backward that recomputes the probabilities from it - nothing of size Sq x Sk reaches memory (include/oeh.h: oeh_attn_fwd_train,
// oeh_attn_bwd).  Head dim 64, fp16 / bf16 storage, fp32 accumulation; softmax / softmax_1, each plain or clipped
// (models/softmax.py:10-19, vutils/softmax_1.py:11-21), the additive masks and clamp of the inference kernels.
//
// Row statistic.  lse = m' + log(sum_k e^(x_k - m') + [softmax_1] e^(-m')), m' = max(m, 0) for softmax_1 (the implicit zero logit)
// and m for softmax, so that p_k = e^(x_k - lse) for either base.  A fully masked softmax_1 row (every x at the mask floor) has
// lse = 0 and p = 0; a fully masked vanilla row (every x at mask_min after the clamp) is uniform.
//
// Gradients.  With dY = dO V^T, y = clip((eta - gamma) p + gamma, 0, 1) and g = (eta - gamma) dY [0 <= (eta-gamma)p+gamma <= 1] (torch.clamp
// passes the gradient on the closed interval) - g = dY without the clip -, dX = p (g - delta) with delta = sum_k p_k g_k.  Without the
// clip delta = rowsum(dO o O) (O = P V; the zero logit of softmax_1 has no value row, so nothing changes for it); with the clip it is a
// sweep over the keys.  dV = y^T dO, dQ = scale dX K, dK = scale dX^T Q.
//
// Kernels (one workgroup = 4 waves of 16 rows, 64-row tiles, v_mfma_f32_16x16x32_{f16,bf16}):
//   fwd   per (b, h, 64 queries): S^T = K Q^T, online row statistics, O^T = V^T P^T (clip: a statistics pass, then the exact p)
//   dq    per (b, h, 64 queries): delta (rowsum(dO o O), or the clip's key sweep) -> work, then dQ^T += K^T dX^T over the key tiles
//   dkdv  per (b, h, 64 keys):    S = Q K^T and dY = dO V^T per query tile, dV^T += dO^T y, dK^T += Q^T dX
// Every gradient element is summed by ONE wave in a fixed order: no atomics, bitwise-reproducible.  Causal problems skip the
// tiles that are fully hidden when that cannot change the result (the forward's skip rule, oeh_desc.h: causal_skip_ok), and the block order puts
// the heaviest tiles first.  In the C/D layout of a 16x16 MFMA lane l holds column l & 15, rows 4 (l >> 4) + i; a 16x16 tile of
// probabilities therefore is, for the next product, the lane's own k-slots: slot j of lane group g is row 16 t0 + 4 g + j (j < 4)
// or 16 t1 + 4 g + j - 4, and the other operand is read from a TRANSPOSED LDS image in that order (two ds_read_b64).
#include "../../include/oeh.h"
#include "oeh_desc.h"
#include "oeh_launch.h"
#include "oeh_philox.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace oeh {
namespace bwd {

constexpr int D = 64;
constexpr int T = 64;     // rows per tile
constexpr int LD = 72;    // LDS row pitch in elements (144 B: 16-byte reads of 16 consecutive rows spread over the banks)

struct Params {
  const void *q, *k, *v, *o, *dout;
  void *dq, *dk, *dv, *out;
  float* lse;
  float* delta;
  float* rowc;                // log of the number of keys at the row maximum where lse could not hold it (saturated rows), else 0
  int B, H, Sq, Sk;
  long qs_b, qs_h, qs_s, ks_b, ks_h, ks_s, vs_b, vs_h, vs_s, os_b, os_h, os_s, ds_b, ds_h, ds_s;
  long dqs_b, dqs_h, dqs_s, dks_b, dks_h, dks_s, dvs_b, dvs_h, dvs_s;
  float scale;                // multiplier of q.k (1 / scale_div when the descriptor divides)
  int base, clip;
  float clip_w, clip_g;       // fl32(eta - gamma), gamma
  const void* pad;
  int pad_f16;
  long pad_sb;
  const void* full;
  int full_f16;
  long full_sb, full_sq;
  int causal, clamp_min;
  float mask_min;
  int skip_ok;
  int nQT, nKT;
  unsigned drop_k0, drop_k1, drop_thr;  // dropout (the DROP instantiations): Philox key, keep threshold (oeh_philox.h),
  float drop_scale;                     // and 1 / (1 - p)
};

__device__ __forceinline__ u4 ldg16(const void* base, long off, bool ok) {
  if (!ok) return u4{0u, 0u, 0u, 0u};
  return *reinterpret_cast<const u4*>(reinterpret_cast<const unsigned short*>(base) + off);
}

// 64 x 64 tile of a (rows, 64) view -> LDS, row-major (pitch LD) and/or transposed (col-major, pitch LD); rows >= nrows are zeros
template <bool ROW, bool TR>
__device__ __forceinline__ void tile_to_lds(const void* g, long s_row, int row0, int nrows, unsigned short* row_img, unsigned short* tr_img) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int row = (tid >> 3) + 32 * r, c = (tid & 7) * 8;
    const u4 w = ldg16(g, (long)(row0 + row) * s_row + c, row0 + row < nrows);
    if constexpr (ROW) *reinterpret_cast<u4*>(row_img + row * LD + c) = w;
    if constexpr (TR) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        tr_img[(c + 2 * j) * LD + row] = (unsigned short)(w[j] & 0xffffu);
        tr_img[(c + 2 * j + 1) * LD + row] = (unsigned short)(w[j] >> 16);
      }
    }
  }
}

// A operand from a row-major image: row (lane & 15) of the 16-row block at r0, k-slots 32 kc + 8 g .. + 7
__device__ __forceinline__ u4 a_rows(const unsigned short* img, int r0, int kc, int lane) {
  return *reinterpret_cast<const u4*>(img + (r0 + (lane & 15)) * LD + 32 * kc + 8 * (lane >> 4));
}
// A operand from a transposed image in the probability-tile slot order: row d = d0 + (lane & 15), slots rows 16 t0 + 4 g .. and 16 t1 + 4 g ..
__device__ __forceinline__ u4 a_tr(const unsigned short* img, int d0, int t0, int t1, int lane) {
  const unsigned short* p = img + (d0 + (lane & 15)) * LD + 4 * (lane >> 4);
  const u2 lo = *reinterpret_cast<const u2*>(p + 16 * t0);
  const u2 hi = *reinterpret_cast<const u2*>(p + 16 * t1);
  return u4{lo[0], lo[1], hi[0], hi[1]};
}

// the reference's score chain after the product: * scale, + key padding, + (B,1,Sq,Sk) mask, + causal mask_min, clamp; -inf for
// keys past Sk (not part of the row)
__device__ __forceinline__ float score(const Params& P, float dot, int b, int qi, int ki, float padv) {
  if (ki >= P.Sk) return -INFINITY;
  float x = dot * P.scale;
  if (P.pad) x = x + padv;
  if (P.full) x = x + load_mask(P.full, P.full_f16, (long)b * P.full_sb + (long)min(qi, P.Sq - 1) * P.full_sq + ki);
  if (P.causal && ki > qi + (P.Sk - P.Sq)) x = x + P.mask_min;
  if (P.clamp_min) x = __builtin_fmaxf(x, P.mask_min);
  return x;
}
// the clamp's gradient gate: torch.max(x, floor) passes nothing where x was below the floor, and half where x equals it (autograd
// splits the gradient of a tie between the two arguments; with bf16 storage x + finfo.min is the floor itself in fp32 and in float64)
__device__ __forceinline__ float clamp_pass(const Params& P, float dot, int b, int qi, int ki, float padv) {
  if (!P.clamp_min) return 1.0f;
  float x = dot * P.scale;
  if (P.pad) x = x + padv;
  if (P.full) x = x + load_mask(P.full, P.full_f16, (long)b * P.full_sb + (long)min(qi, P.Sq - 1) * P.full_sq + ki);
  if (P.causal && ki > qi + (P.Sk - P.Sq)) x = x + P.mask_min;
  return x < P.mask_min ? 0.0f : (x == P.mask_min ? 0.5f : 1.0f);
}

__device__ __forceinline__ float pad_of(const Params& P, int b, int ki) {
  return (P.pad && ki < P.Sk) ? load_mask(P.pad, P.pad_f16, (long)b * P.pad_sb + ki) : 0.0f;
}

// dX element from p and dY (the clip's y and gradient gate included); y returned for dV
__device__ __forceinline__ float dx_of(const Params& P, float p, float dy, float delta, float& y) {
  float g = dy;
  y = p;
  if (P.clip) {
    const float u = p * P.clip_w + P.clip_g;
    y = __builtin_fminf(__builtin_fmaxf(u, 0.0f), 1.0f);
    g = (u >= 0.0f && u <= 1.0f) ? P.clip_w * dy : 0.0f;
  }
  return p * (g - delta);
}

// number of 64-key tiles a causal 64-query tile qt needs (the tiles past it are fully hidden)
__device__ __forceinline__ int key_tiles_for(const Params& P, int qt) {
  if (!P.skip_ok) return P.nKT;
  const int last_q = min(qt * T + T - 1, P.Sq - 1);
  return min(P.nKT, (last_q + (P.Sk - P.Sq)) / T + 1);
}
__device__ __forceinline__ int first_query_tile(const Params& P, int kt) {
  if (!P.skip_ok) return 0;
  const int first_visible_q = kt * T - (P.Sk - P.Sq);
  return first_visible_q <= 0 ? 0 : first_visible_q / T;
}

// dropout factors keep / (1 - p) (0 where dropped) of keys key0 .. key0 + 3 (key0 % 4 == 0) of query qi: the fwd / dq layout, where a
// lane holds 4 consecutive keys of one query - one Philox block
__device__ __forceinline__ f4 drop4(const Params& P, int bh, int qi, int key0) {
  const Philox4 r = dropout_words((unsigned)key0 >> 2, (unsigned)qi, (unsigned)bh, P.drop_k0, P.drop_k1);
  return f4{r.x[0] >= P.drop_thr ? P.drop_scale : 0.0f, r.x[1] >= P.drop_thr ? P.drop_scale : 0.0f, r.x[2] >= P.drop_thr ? P.drop_scale : 0.0f,
            r.x[3] >= P.drop_thr ? P.drop_scale : 0.0f};
}

// the dkdv layout: a lane holds ONE key ki and queries q0 + 16 t + 4 g + i (t, i < 4), and the 4 keys of a Philox block sit in the 4
// lanes of a DPP quad (lane & 3 == ki & 3, same g).  Lane r of the quad draws the blocks of queries q0 + 16 t + 4 g + r and turns each
// into a keep nibble (bit m: key 4 (ki >> 2) + m); two quad_perm xor exchanges give every lane all 16 nibbles - 4 Philox calls per
// lane per tile instead of 16.  Returned shifted by r: keep(t, i) of the lane's own key is bit 16 (t & 1) + 4 i of word t >> 1.
__device__ __forceinline__ u2 drop_bits_quad(const Params& P, int bh, int q0, int g, int ki) {
  const int r = ki & 3;
  unsigned thr = P.drop_thr;
  asm volatile("" : "+v"(thr));  // (held in a vector register: the kernel is at the scalar register limit)
  unsigned x[2] = {0u, 0u};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const Philox4 w = dropout_words((unsigned)ki >> 2, (unsigned)(q0 + 16 * t + 4 * g + r), (unsigned)bh, P.drop_k0, P.drop_k1);
    const unsigned nib = (unsigned)(w.x[0] >= thr) | ((unsigned)(w.x[1] >= thr) << 1) | ((unsigned)(w.x[2] >= thr) << 2) | ((unsigned)(w.x[3] >= thr) << 3);
    x[t >> 1] |= nib << (16 * (t & 1) + 4 * r);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    x[j] |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x[j], 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
    x[j] |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x[j], 0x4E, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
  }
  return u2{x[0] >> r, x[1] >> r};
}

// ---------------------------------------------------------------- forward (training): O and lse
template <int IN, bool DROP>
__global__ __launch_bounds__(256) void fwd_kernel(const Params P) {
  __shared__ __attribute__((aligned(16))) unsigned short Ks[T * LD];
  __shared__ __attribute__((aligned(16))) unsigned short Vt[D * LD];
  __shared__ float padS[T];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4;
  const int nBH = P.B * P.H;
  const int bid = blockIdx.x;
  const int qt = P.nQT - 1 - bid / nBH, bh = bid % nBH;  // heaviest causal q tiles first
  const int b = bh / P.H, h = bh - b * P.H;
  const unsigned short* q = reinterpret_cast<const unsigned short*>(P.q) + (long)b * P.qs_b + (long)h * P.qs_h;
  const unsigned short* k = reinterpret_cast<const unsigned short*>(P.k) + (long)b * P.ks_b + (long)h * P.ks_h;
  const unsigned short* v = reinterpret_cast<const unsigned short*>(P.v) + (long)b * P.vs_b + (long)h * P.vs_h;
  const int qi = qt * T + 16 * w + (lane & 15);
  const bool qok = qi < P.Sq;
  u4 qf[2];
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) qf[kc] = ldg16(q, (long)qi * P.qs_s + 32 * kc + 8 * g, qok);
  const int nkt = key_tiles_for(P, qt);
  const float m_init = P.base == 1 ? 0.0f : -INFINITY;
  float m = m_init, l = 0.0f;  // running max (>= 0 for softmax_1: m' = max(m, 0)), lane-partial sum
  f4 acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = f4{0.f, 0.f, 0.f, 0.f};
  float lse_row = 0.0f, c_row = 0.0f;  // c_row: log(den) of a saturated row (lse_row + 64 == lse_row: the sum is lost in it), else 0
  // pass 0: statistics only (clip: p must be final before the clip), pass 1: P V with the final p; no clip: one online pass
  const int npass = P.clip ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    const bool stats = !P.clip || pass == 0;
    const bool pv = !P.clip || pass == 1;
    for (int kt = 0; kt < nkt; ++kt) {
      __syncthreads();
      tile_to_lds<true, false>(k, P.ks_s, kt * T, P.Sk, Ks, nullptr);
      if (pv) tile_to_lds<false, true>(v, P.vs_s, kt * T, P.Sk, nullptr, Vt);
      if (threadIdx.x < T) padS[threadIdx.x] = pad_of(P, b, kt * T + threadIdx.x);
      __syncthreads();
      f4 x[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f4 s = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) s = mfma16<IN>(a_rows(Ks, 16 * t, kc, lane), qf[kc], s);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int kl = 16 * t + 4 * g + i;
          x[t][i] = score(P, s[i], b, qi, kt * T + kl, padS[kl]);
        }
      }
      float alpha = 1.0f, mu;
      if (stats) {
        float mt = m;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) mt = __builtin_fmaxf(mt, x[t][i]);
        mt = row4_max(mt);
        mu = mt == -INFINITY ? 0.0f : mt;  // (nothing visible yet: keep the exponents finite)
        alpha = expf((m == -INFINITY ? 0.0f : m) - mu);
        if (m == -INFINITY) alpha = 0.0f;
        m = mt;
      } else {
        mu = 0.0f;
      }
      f4 p[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float e;
          if (P.clip && pass == 1) {
            const float pp = expf((x[t][i] - lse_row) - c_row);
            const float u = pp * P.clip_w + P.clip_g;
            e = __builtin_fminf(__builtin_fmaxf(u, 0.0f), 1.0f);
          } else {
            e = expf(x[t][i] - mu);
          }
          p[t][i] = e;
        }
      if (stats) {
        float ls = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) ls += (p[t][0] + p[t][1]) + (p[t][2] + p[t][3]);
        l = l * alpha + ls;
      }
      if constexpr (DROP) {  // z = keep y / (1 - p) into the product only: the row statistics stay those of the undropped row
        if (pv) {
#pragma unroll
          for (int t = 0; t < 4; ++t) p[t] = p[t] * drop4(P, bh, qi, kt * T + 16 * t + 4 * g);
        }
      }
      if (pv) {
        if (!P.clip) {
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) acc[dt] = acc[dt] * alpha;
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const u4 bp = pack8<IN>(p[2 * c], p[2 * c + 1]);
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) acc[dt] = mfma16<IN>(a_tr(Vt, 16 * dt, 2 * c, 2 * c + 1, lane), bp, acc[dt]);
        }
      }
    }
    if (stats) {
      const float lt = row4_sum(l);
      const float mm = m == -INFINITY ? 0.0f : m;
      const float den = P.base == 1 ? lt + expf(-mm) : lt;
      lse_row = den > 0.0f ? mm + logf(den) : INFINITY;  // (INFINITY: a vanilla row with no finite score - p = 0)
      if (lse_row < 0.0f && lse_row + 64.0f == lse_row) c_row = logf(den);  // (the dq kernel counts the same den: see there)
      if (!P.clip) {
        const float r = den > 0.0f ? 1.0f / den : 0.0f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) acc[dt] = acc[dt] * r;
      }
    }
  }
  (void)m_init;
  if (qok) {
    if (g == 0) P.lse[(long)bh * P.Sq + qi] = lse_row;
    unsigned short* o = reinterpret_cast<unsigned short*>(P.out) + (long)b * P.os_b + (long)h * P.os_h + (long)qi * P.os_s;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      *reinterpret_cast<u2*>(o + 16 * dt + 4 * g) = u2{pack2<IN>(acc[dt][0], acc[dt][1]), pack2<IN>(acc[dt][2], acc[dt][3])};
  }
}

// ---------------------------------------------------------------- dQ (and the row term delta)
template <int IN, bool DROP>
__global__ __launch_bounds__(256) void dq_kernel(const Params P) {
  __shared__ __attribute__((aligned(16))) unsigned short Ks[T * LD];
  __shared__ __attribute__((aligned(16))) unsigned short Vs[T * LD];
  __shared__ __attribute__((aligned(16))) unsigned short Kt[D * LD];
  __shared__ float padS[T];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4;
  const int nBH = P.B * P.H;
  const int bid = blockIdx.x;
  const int qt = P.nQT - 1 - bid / nBH, bh = bid % nBH;
  const int b = bh / P.H, h = bh - b * P.H;
  const unsigned short* q = reinterpret_cast<const unsigned short*>(P.q) + (long)b * P.qs_b + (long)h * P.qs_h;
  const unsigned short* k = reinterpret_cast<const unsigned short*>(P.k) + (long)b * P.ks_b + (long)h * P.ks_h;
  const unsigned short* v = reinterpret_cast<const unsigned short*>(P.v) + (long)b * P.vs_b + (long)h * P.vs_h;
  const unsigned short* o = reinterpret_cast<const unsigned short*>(P.o) + (long)b * P.os_b + (long)h * P.os_h;
  const unsigned short* dO = reinterpret_cast<const unsigned short*>(P.dout) + (long)b * P.ds_b + (long)h * P.ds_h;
  const int qi = qt * T + 16 * w + (lane & 15);
  const bool qok = qi < P.Sq;
  u4 qf[2], df[2];
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    qf[kc] = ldg16(q, (long)qi * P.qs_s + 32 * kc + 8 * g, qok);
    df[kc] = ldg16(dO, (long)qi * P.ds_s + 32 * kc + 8 * g, qok);
  }
  const float L = qok ? P.lse[(long)bh * P.Sq + qi] : INFINITY;
  const int nkt = key_tiles_for(P, qt);
  // A saturated row: its maximum m is so large in magnitude (a vanilla row masked by finfo.min of bf16 / fp32) that fp32 lse = m +
  // log(den) IS m - e^(x - lse) would be 1 on every key at the maximum instead of 1 / den.  There every x is either m itself or far
  // enough below it to give p = 0, so den is the number of keys with x == lse: counted here, and p = e^((x - lse) - c) with c = log(den)
  // (c = 0 on every other row: the same bits as e^(x - lse)).
  const bool sat = qok && L < 0.0f && L + 64.0f == L;
  float c = 0.0f;
  if (__syncthreads_or(sat)) {
    float cnt = 0.0f;
    for (int kt = 0; kt < nkt; ++kt) {
      __syncthreads();
      tile_to_lds<true, false>(k, P.ks_s, kt * T, P.Sk, Ks, nullptr);
      if (threadIdx.x < T) padS[threadIdx.x] = pad_of(P, b, kt * T + threadIdx.x);
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f4 s = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) s = mfma16<IN>(a_rows(Ks, 16 * t, kc, lane), qf[kc], s);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int kl = 16 * t + 4 * g + i;
          cnt += score(P, s[i], b, qi, kt * T + kl, padS[kl]) == L ? 1.0f : 0.0f;
        }
      }
    }
    cnt = row4_sum(cnt);
    if (sat && cnt > 1.0f) c = logf(cnt);
  }
  if (qok && g == 0) P.rowc[(long)bh * P.Sq + qi] = c;
  float delta = 0.0f;
  if (!P.clip) {  // rowsum(dO o O): the lane's 16 of the row's 64 products, then the 4 lanes of the row
    float part = 0.0f;
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      const u4 of = ldg16(o, (long)qi * P.os_s + 32 * kc + 8 * g, qok);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        part += In<IN>::to_f32((unsigned short)(df[kc][j] & 0xffffu)) * In<IN>::to_f32((unsigned short)(of[j] & 0xffffu));
        part += In<IN>::to_f32((unsigned short)(df[kc][j] >> 16)) * In<IN>::to_f32((unsigned short)(of[j] >> 16));
      }
    }
    delta = row4_sum(part);
  }
  f4 acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = f4{0.f, 0.f, 0.f, 0.f};
  // clip: pass 0 sums delta = sum_k p g over the keys; pass 1 (the only pass without the clip) accumulates dQ
  const int npass = P.clip ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    const bool sweep = P.clip && pass == 0;
    float dpart = 0.0f;
    for (int kt = 0; kt < nkt; ++kt) {
      __syncthreads();
      if (sweep) tile_to_lds<true, false>(k, P.ks_s, kt * T, P.Sk, Ks, nullptr);
      else tile_to_lds<true, true>(k, P.ks_s, kt * T, P.Sk, Ks, Kt);
      tile_to_lds<true, false>(v, P.vs_s, kt * T, P.Sk, Vs, nullptr);
      if (threadIdx.x < T) padS[threadIdx.x] = pad_of(P, b, kt * T + threadIdx.x);
      __syncthreads();
      f4 dx[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        f4 s = f4{0.f, 0.f, 0.f, 0.f}, dy = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
          s = mfma16<IN>(a_rows(Ks, 16 * t, kc, lane), qf[kc], s);
          dy = mfma16<IN>(a_rows(Vs, 16 * t, kc, lane), df[kc], dy);
        }
        if constexpr (DROP) dy = dy * drop4(P, bh, qi, kt * T + 16 * t + 4 * g);  // dY = keep / (1 - p) dZ
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int kl = 16 * t + 4 * g + i, ki = kt * T + kl;
          const float x = score(P, s[i], b, qi, ki, padS[kl]);
          const float p = (qok && ki < P.Sk) ? expf((x - L) - c) : 0.0f;
          if (sweep) {
            float y;
            dpart += dx_of(P, p, dy[i], 0.0f, y);
            dx[t][i] = 0.0f;
          } else {
            float y;
            dx[t][i] = dx_of(P, p, dy[i], delta, y) * clamp_pass(P, s[i], b, qi, ki, padS[kl]);
          }
        }
      }
      if (!sweep) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const u4 bx = pack8<IN>(dx[2 * c], dx[2 * c + 1]);
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) acc[dt] = mfma16<IN>(a_tr(Kt, 16 * dt, 2 * c, 2 * c + 1, lane), bx, acc[dt]);
        }
      }
    }
    if (sweep) delta = row4_sum(dpart);
  }
  if (qok) {
    if (g == 0) P.delta[(long)bh * P.Sq + qi] = delta;
    unsigned short* dq = reinterpret_cast<unsigned short*>(P.dq) + (long)b * P.dqs_b + (long)h * P.dqs_h + (long)qi * P.dqs_s;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const f4 r = acc[dt] * P.scale;
      *reinterpret_cast<u2*>(dq + 16 * dt + 4 * g) = u2{pack2<IN>(r[0], r[1]), pack2<IN>(r[2], r[3])};
    }
  }
}

// ---------------------------------------------------------------- dK and dV
template <int IN, bool DROP>
__global__ __launch_bounds__(256) void dkdv_kernel(const Params P) {
  __shared__ __attribute__((aligned(16))) unsigned short Qs[T * LD];
  __shared__ __attribute__((aligned(16))) unsigned short Qt[D * LD];
  __shared__ __attribute__((aligned(16))) unsigned short Ds[T * LD];
  __shared__ __attribute__((aligned(16))) unsigned short Dt[D * LD];
  __shared__ float lseS[T], deltaS[T], cS[T];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4;
  const int nBH = P.B * P.H;
  const int bid = blockIdx.x;
  const int kt = bid / nBH, bh = bid % nBH;  // causal: the first key tiles see the most query tiles
  const int b = bh / P.H, h = bh - b * P.H;
  const unsigned short* q = reinterpret_cast<const unsigned short*>(P.q) + (long)b * P.qs_b + (long)h * P.qs_h;
  const unsigned short* k = reinterpret_cast<const unsigned short*>(P.k) + (long)b * P.ks_b + (long)h * P.ks_h;
  const unsigned short* v = reinterpret_cast<const unsigned short*>(P.v) + (long)b * P.vs_b + (long)h * P.vs_h;
  const unsigned short* dO = reinterpret_cast<const unsigned short*>(P.dout) + (long)b * P.ds_b + (long)h * P.ds_h;
  const int ki = kt * T + 16 * w + (lane & 15);
  const bool kok = ki < P.Sk;
  u4 kf[2], vf[2];
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    kf[kc] = ldg16(k, (long)ki * P.ks_s + 32 * kc + 8 * g, kok);
    vf[kc] = ldg16(v, (long)ki * P.vs_s + 32 * kc + 8 * g, kok);
  }
  const float padv = pad_of(P, b, ki);
  f4 dkacc[4], dvacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dkacc[dt] = dvacc[dt] = f4{0.f, 0.f, 0.f, 0.f};
  for (int qt = first_query_tile(P, kt); qt < P.nQT; ++qt) {
    __syncthreads();
    tile_to_lds<true, true>(q, P.qs_s, qt * T, P.Sq, Qs, Qt);
    tile_to_lds<true, true>(dO, P.ds_s, qt * T, P.Sq, Ds, Dt);
    if (threadIdx.x < T) {
      const int qq = qt * T + threadIdx.x;
      lseS[threadIdx.x] = qq < P.Sq ? P.lse[(long)bh * P.Sq + qq] : INFINITY;
      deltaS[threadIdx.x] = qq < P.Sq ? P.delta[(long)bh * P.Sq + qq] : 0.0f;
      cS[threadIdx.x] = qq < P.Sq ? P.rowc[(long)bh * P.Sq + qq] : 0.0f;
    }
    __syncthreads();
    u2 kb = u2{0u, 0u};
    if constexpr (DROP) kb = drop_bits_quad(P, bh, qt * T, g, ki);
    f4 y[4], dx[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f4 s = f4{0.f, 0.f, 0.f, 0.f}, dy = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        s = mfma16<IN>(a_rows(Qs, 16 * t, kc, lane), kf[kc], s);
        dy = mfma16<IN>(a_rows(Ds, 16 * t, kc, lane), vf[kc], dy);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ql = 16 * t + 4 * g + i, qi = qt * T + ql;
        const bool ok = kok && qi < P.Sq;
        const float x = score(P, s[i], b, qi, ki, padv);
        const float p = ok ? expf((x - lseS[ql]) - cS[ql]) : 0.0f;
        float yy;
        if constexpr (DROP) {  // dV takes z = keep y / (1 - p), dX takes dY = keep / (1 - p) dZ
          const float f = ((kb[t >> 1] >> (16 * (t & 1) + 4 * i)) & 1u) ? P.drop_scale : 0.0f;
          const float d = dx_of(P, p, dy[i] * f, deltaS[ql], yy);
          y[t][i] = ok ? yy * f : 0.0f;
          dx[t][i] = ok ? d * clamp_pass(P, s[i], b, qi, ki, padv) : 0.0f;
          continue;
        }
        const float d = dx_of(P, p, dy[i], deltaS[ql], yy);
        y[t][i] = ok ? yy : 0.0f;
        dx[t][i] = ok ? d * clamp_pass(P, s[i], b, qi, ki, padv) : 0.0f;
      }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const u4 by = pack8<IN>(y[2 * c], y[2 * c + 1]);
      const u4 bx = pack8<IN>(dx[2 * c], dx[2 * c + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        dvacc[dt] = mfma16<IN>(a_tr(Dt, 16 * dt, 2 * c, 2 * c + 1, lane), by, dvacc[dt]);
        dkacc[dt] = mfma16<IN>(a_tr(Qt, 16 * dt, 2 * c, 2 * c + 1, lane), bx, dkacc[dt]);
      }
    }
  }
  if (kok) {
    unsigned short* dk = reinterpret_cast<unsigned short*>(P.dk) + (long)b * P.dks_b + (long)h * P.dks_h + (long)ki * P.dks_s;
    unsigned short* dv = reinterpret_cast<unsigned short*>(P.dv) + (long)b * P.dvs_b + (long)h * P.dvs_h + (long)ki * P.dvs_s;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const f4 r = dkacc[dt] * P.scale;
      *reinterpret_cast<u2*>(dk + 16 * dt + 4 * g) = u2{pack2<IN>(r[0], r[1]), pack2<IN>(r[2], r[3])};
      *reinterpret_cast<u2*>(dv + 16 * dt + 4 * g) = u2{pack2<IN>(dvacc[dt][0], dvacc[dt][1]), pack2<IN>(dvacc[dt][2], dvacc[dt][3])};
    }
  }
}

// ---------------------------------------------------------------- host side
bool aligned_rows(const void* p, const int64_t st[3]) { return aligned16(p, st, 2); }

// what both entry points accept (include/oeh.h): the pointer checks come after, per entry point
int check_desc(const oeh_attn_desc* d) {
  if (!desc_sane(d, true, true) || !softmax_base_ok(d->softmax_base) || !key_pad_ok(d) || !full_mask_ok(d)) return OEH_EINVAL;
  if (d->dtype == OEH_F32 || d->dtype == OEH_I8) return OEH_ENOTSUP;   // fp16 / bf16 storage only
  if (d->D != 64) return OEH_ENOTSUP;
  if (d->gate != nullptr || d->gate_hidden != nullptr) return OEH_ENOTSUP;  // the gate stays outside the differentiable core
  if (d->o_dtype == OEH_F32) return OEH_ENOTSUP;                       // (the inference kernels' fp32-accumulator output)
  if (d->scale_div != 0.0f ? !(std::isfinite(d->scale_div) && d->scale_div != 0.0f) : !std::isfinite(d->scale)) return OEH_EINVAL;
  if (!desc_strides_in_range(d)) return OEH_ENOTSUP;
  if ((int64_t)d->B * d->H * (d->Sq > d->Sk ? d->Sq : d->Sk) >= ((int64_t)1 << 31)) return OEH_ENOTSUP;
  return OEH_OK;
}

void fill(Params& P, const oeh_attn_desc* d) {
  std::memset(&P, 0, sizeof(P));
  fill_problem(P, d);
  P.scale = d->scale_div != 0.0f ? (float)(1.0 / (double)d->scale_div) : d->scale;
  P.skip_ok = causal_skip_ok(d, false) ? 1 : 0;  // (the inference forward's rule; the training kernels have no index dumps)
  P.nQT = (d->Sq + T - 1) / T;
  P.nKT = (d->Sk + T - 1) / T;
}

// the dropout descriptor (include/oeh.h: oeh_dropout): p in [0, 1), NaN refused; checked before anything else of an entry point
int check_drop(const oeh_dropout* drop) {
  if (drop == nullptr) return OEH_EINVAL;
  if (!(drop->p >= 0.0f && drop->p < 1.0f)) return OEH_EINVAL;
  return OEH_OK;
}
void fill_drop(Params& P, const oeh_dropout* drop) {
  P.drop_k0 = (unsigned)(drop->seed & 0xffffffffu);
  P.drop_k1 = (unsigned)(drop->seed >> 32);
  P.drop_thr = dropout_threshold(drop->p);
  P.drop_scale = 1.0f / (1.0f - drop->p);
}

// the (B,H,Sq,Sk) keep mask, one Philox block (4 keys of one query) per thread, grid-stride
__global__ __launch_bounds__(256) void dropout_mask_kernel(unsigned char* keep, int BH, int Sq, int Sk, unsigned k0, unsigned k1, unsigned thr) {
  const int nc = (Sk + 3) >> 2;
  const long n = (long)BH * Sq * nc;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) {
    const long row = e / nc;
    const int c = (int)(e - row * nc);
    const int qi = (int)(row % Sq), bh = (int)(row / Sq);
    const Philox4 w = dropout_words((unsigned)c, (unsigned)qi, (unsigned)bh, k0, k1);
    unsigned char* o = keep + row * Sk + 4 * c;
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (4 * c + m < Sk) o[m] = w.x[m] >= thr ? 1 : 0;
  }
}

// the entry points' bodies; drop == nullptr (or p == 0): the DROP = false kernels
int fwd_train(const oeh_attn_desc* desc, const oeh_dropout* drop, const void* q, const void* k, const void* v, void* o, float* lse, void* stream) {
  int rc = check_desc(desc);
  if (rc != OEH_OK) return rc;
  if (q == nullptr || k == nullptr || v == nullptr || o == nullptr || lse == nullptr) return OEH_EINVAL;
  if (!aligned_rows(q, desc->q_stride) || !aligned_rows(k, desc->k_stride) || !aligned_rows(v, desc->v_stride) || !aligned_rows(o, desc->o_stride) ||
      (reinterpret_cast<uintptr_t>(lse) & 3) != 0)
    return OEH_EALIGN;
  Params P;
  fill(P, desc);
  P.q = q; P.k = k; P.v = v; P.out = o; P.lse = lse;
  const bool dr = drop != nullptr && drop->p > 0.0f;
  if (dr) fill_drop(P, drop);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(P.nQT * P.B * P.H));
  dispatch_in16(desc->dtype, dr, [&](auto t, auto drop_on) {
    hipLaunchKernelGGL((fwd_kernel<decltype(t)::value, decltype(drop_on)::value>), grid, dim3(256), 0, st, P);
  });
  return oeh::launch_status();
}

int bwd_run(const oeh_attn_desc* desc, const oeh_dropout* drop, const void* q, const void* k, const void* v, const void* o, const void* do_,
            const int64_t do_stride[3], const float* lse, void* dq, const int64_t dq_stride[3], void* dk, const int64_t dk_stride[3], void* dv,
            const int64_t dv_stride[3], void* work, void* stream) {
  int rc = check_desc(desc);
  if (rc != OEH_OK) return rc;
  if (q == nullptr || k == nullptr || v == nullptr || o == nullptr || do_ == nullptr || lse == nullptr || dq == nullptr || dk == nullptr ||
      dv == nullptr || work == nullptr || do_stride == nullptr || dq_stride == nullptr || dk_stride == nullptr || dv_stride == nullptr)
    return OEH_EINVAL;
  if (!strides_in_range(do_stride) || !strides_in_range(dq_stride) || !strides_in_range(dk_stride) || !strides_in_range(dv_stride)) return OEH_ENOTSUP;
  if (!aligned_rows(q, desc->q_stride) || !aligned_rows(k, desc->k_stride) || !aligned_rows(v, desc->v_stride) || !aligned_rows(o, desc->o_stride) ||
      !aligned_rows(do_, do_stride) || !aligned_rows(dq, dq_stride) || !aligned_rows(dk, dk_stride) || !aligned_rows(dv, dv_stride) ||
      ((reinterpret_cast<uintptr_t>(lse) | reinterpret_cast<uintptr_t>(work)) & 3) != 0)
    return OEH_EALIGN;
  Params P;
  fill(P, desc);
  P.q = q; P.k = k; P.v = v; P.o = o; P.dout = do_; P.lse = const_cast<float*>(lse); P.delta = reinterpret_cast<float*>(work);
  P.rowc = P.delta + (long)desc->B * desc->H * desc->Sq;
  P.dq = dq; P.dk = dk; P.dv = dv;
  P.ds_b = do_stride[0]; P.ds_h = do_stride[1]; P.ds_s = do_stride[2];
  P.dqs_b = dq_stride[0]; P.dqs_h = dq_stride[1]; P.dqs_s = dq_stride[2];
  P.dks_b = dk_stride[0]; P.dks_h = dk_stride[1]; P.dks_s = dk_stride[2];
  P.dvs_b = dv_stride[0]; P.dvs_h = dv_stride[1]; P.dvs_s = dv_stride[2];
  const bool dr = drop != nullptr && drop->p > 0.0f;
  if (dr) fill_drop(P, drop);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 gq((unsigned)(P.nQT * P.B * P.H)), gk((unsigned)(P.nKT * P.B * P.H));
  // dq first: it writes delta, which dkdv reads (stream order)
  dispatch_in16(desc->dtype, dr, [&](auto t, auto drop_on) {
    hipLaunchKernelGGL((dq_kernel<decltype(t)::value, decltype(drop_on)::value>), gq, dim3(256), 0, st, P);
    hipLaunchKernelGGL((dkdv_kernel<decltype(t)::value, decltype(drop_on)::value>), gk, dim3(256), 0, st, P);
  });
  return oeh::launch_status();
}

}  // namespace bwd
}  // namespace oeh

using namespace oeh;
using namespace oeh::bwd;

extern "C" {

int oeh_attn_fwd_train(const oeh_attn_desc* desc, const void* q, const void* k, const void* v, void* o, float* lse, void* stream) {
  return fwd_train(desc, nullptr, q, k, v, o, lse, stream);
}

int oeh_attn_fwd_train_dropout(const oeh_attn_desc* desc, const oeh_dropout* drop, const void* q, const void* k, const void* v, void* o, float* lse,
                               void* stream) {
  const int rc = check_drop(drop);
  if (rc != OEH_OK) return rc;
  return fwd_train(desc, drop, q, k, v, o, lse, stream);
}

int64_t oeh_attn_bwd_work_bytes(const oeh_attn_desc* desc) {
  const int rc = check_desc(desc);
  if (rc != OEH_OK) return rc;
  return 2 * (int64_t)desc->B * desc->H * desc->Sq * (int64_t)sizeof(float);  // delta and rowc per query row
}

int oeh_attn_bwd(const oeh_attn_desc* desc, const void* q, const void* k, const void* v, const void* o, const void* do_,
                 const int64_t do_stride[3], const float* lse, void* dq, const int64_t dq_stride[3], void* dk, const int64_t dk_stride[3],
                 void* dv, const int64_t dv_stride[3], void* work, void* stream) {
  return bwd_run(desc, nullptr, q, k, v, o, do_, do_stride, lse, dq, dq_stride, dk, dk_stride, dv, dv_stride, work, stream);
}

int oeh_attn_bwd_dropout(const oeh_attn_desc* desc, const oeh_dropout* drop, const void* q, const void* k, const void* v, const void* o,
                         const void* do_, const int64_t do_stride[3], const float* lse, void* dq, const int64_t dq_stride[3], void* dk,
                         const int64_t dk_stride[3], void* dv, const int64_t dv_stride[3], void* work, void* stream) {
  const int rc = check_drop(drop);
  if (rc != OEH_OK) return rc;
  return bwd_run(desc, drop, q, k, v, o, do_, do_stride, lse, dq, dq_stride, dk, dk_stride, dv, dv_stride, work, stream);
}

int oeh_attn_dropout_mask(const oeh_attn_desc* desc, const oeh_dropout* drop, uint8_t* keep, void* stream) {
  int rc = check_drop(drop);
  if (rc != OEH_OK) return rc;
  if (keep == nullptr || !desc_sizes_ok(desc, false)) return OEH_EINVAL;  // (the mask has no storage type and no head dim)
  if ((int64_t)desc->B * desc->H >= ((int64_t)1 << 31)) return OEH_ENOTSUP;
  Params P;
  std::memset(&P, 0, sizeof(P));
  if (drop->p > 0.0f) fill_drop(P, drop);  // (p == 0: threshold 0, every element kept)
  const int64_t n = (int64_t)desc->B * desc->H * desc->Sq * ((desc->Sk + 3) / 4);
  const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 16384);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), keep, desc->B * desc->H, desc->Sq,
                     desc->Sk, P.drop_k0, P.drop_k1, P.drop_thr);
  return oeh::launch_status();
}

}  // extern "C"
