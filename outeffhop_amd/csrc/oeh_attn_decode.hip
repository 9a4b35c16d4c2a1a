// Split-key decode attention (include/oeh.h: oeh_attn_decode): a generation step - 1 .. 16 query rows against a long key / value
// cache, head dim 64, 16-bit storage.  The one-pass kernel gives such a problem ONE workgroup per (batch, head) that walks the whole
// cache serially (OPT-125m at batch 1: 12 workgroups on 256 CUs); here the KEYS of a head are split over `n` workgroups and the partial
// results are combined by a second, tiny launch.  Plain launches only: no atomics, no arrival counters, a fixed summation order - the
// result is bitwise reproducible and the chain is graph-capture safe.
//
//  * partial pass: one 4-wave workgroup per (batch, head, split).  Chunk = `chunk` keys (a multiple of 64); wave w takes the chunk's
//    32-key units w, w + 4, ...  Swapped products as everywhere (oeh_attn_mfma.inl): S^T = K Q^T with the K rows read from global memory
//    straight into the A operand (lane (c, g): key c of the tile, d = 32 ks + 8 g ..) and the 16 x 64 query block (rows beyond Sq zero)
//    as the B operand, held in registers for the whole kernel; O^T = V^T P^T with P^T the lane's own score registers and V^T fetched
//    from a per-wave 4-KB LDS image with ds_read_b64_tr_b16 (same row swizzle as the other kernels).  Each wave keeps an online
//    (m, l, acc); the four waves merge through LDS and the workgroup writes one (m, l) pair per real query row and its 64 fp32
//    accumulators.
//  * combine pass: M = max_s m_s (softmax_1: max(., 0)), den = sum_s l_s e^(m_s - M) (+ e^(-M)), o = sum_s acc_s e^(m_s - M) / den, gate, store.
//    (M, den) stay TWO numbers: a vanilla row without a visible key sits at finfo.min, where M + log(den) rounds back to M.
//  * clipped softmax needs the row's denominator before the clip: a statistics pass (scores only), a product pass that forms (M, den) of
//    its rows from the n statistic pairs and accumulates y = clip((eta - gamma) e^(x - M) / den + gamma, 0, 1) times V, and a plain sum.
//  * the mask arithmetic is literal (fp32 add, then the clamp) and no chunk is skipped: under the vanilla softmax a row without a visible
//    key is uniform over ALL keys, those of fully padded chunks included.
//  * the fused INT8 chain (oeh_attn_decode_fq; FQ = true instantiations, the forms above compile as before): the scores quantiser sits right
//    after the scaling, in front of the literal mask arithmetic, in EVERY pass that forms scores (the same operations: the same bits); the
//    probability quantiser needs the row's denominator before the grid, so with it (as with the clip) the three-launch form runs - statistics,
//    a product pass that forms p = e^(x - M) / den, [clip], rel = idx - zp and feeds the INTEGERS rel to the second product (exact in f16 and
//    bf16), a plain sum that applies the probability scale in fp32; the context quantiser and the gate, in either order, sit in the last launch.
//    Exponentials that feed a quantiser are the ~1 ulp exp_acc_nonpos, as in the other fake-quant kernels.
#include "../../include/oeh.h"
#include "oeh_desc.h"
#include "oeh_launch.h"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace oeh {

struct DecodeParams {
  AttnParams A;
  int n;        // effective number of splits
  int chunk;    // keys per split (multiple of 64)
  float* ml;    // (B*H, n, Sq, 2): m, l
  float* acc;   // (B*H, n, Sq, 64)
  int out;      // the combine pass's output type: IN_F16 | IN_BF16 | IN_F32
};

namespace {

constexpr float kNegInf = -__builtin_huge_valf();

enum { DEC_PLAIN = 0, DEC_STATS = 1, DEC_CLIP = 2 };

// e^(a - b) for a <= b or a = -inf; b finite
__device__ __forceinline__ float exp_diff(float a, float b) { return __builtin_amdgcn_exp2f((a - b) * kLog2e); }

// the same, ACC: to ~1 ulp (the fake-quant forms: the value feeds a quantiser)
template <bool ACC>
__device__ __forceinline__ float exp_d(float a, float b) {
  if constexpr (ACC) return exp_acc_nonpos(a - b);
  else return exp_diff(a, b);
}

// (M, den) of one query row from its n statistic pairs, in split order.  A row whose every score is -inf keeps M finite (0): all weights 0.
template <bool ACC = false>
__device__ __forceinline__ void row_stats(const float* ml, const int n, const long stride, const int base, float& M, float& den) {
  float mx = kNegInf;
  for (int s = 0; s < n; ++s) mx = __builtin_fmaxf(mx, ml[s * stride]);
  if (base != 0) mx = __builtin_fmaxf(mx, 0.0f);
  if (mx == kNegInf) mx = 0.0f;
  float d = 0.0f;
  for (int s = 0; s < n; ++s) d = d + ml[s * stride + 1] * exp_d<ACC>(ml[s * stride], mx);
  if (base != 0) d = d + exp_d<ACC>(-mx, 0.0f);
  M = mx;
  den = d;
}

// FQ: the forms with the scores / probability quantisers (each under a wave-uniform test of its enable flag; FQ = false: none of that code).
// The fake-quant plain / product forms ask the register allocator for four waves per SIMD (the non-quantised product form's occupancy): left
// alone they come out at 122 / 114 VGPRs + 16 AGPRs, three waves; with the request 112 / 113 VGPRs, no AGPRs, no scratch.  (1: no request.)
template <int IN, int MODE, bool FQ = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FQ && MODE != DEC_STATS ? 4 : 1))) void oeh_attn_decode_partial(const DecodeParams DP) {
  const AttnParams& P = DP.A;
  constexpr int ROWB = 128;  // bytes of a 64-element 16-bit row
  // per wave: the 32-key V image of the loop, then (the same 4 KB, after the wave's last transposed read) its 16 x 64 fp32 accumulators
  __shared__ __attribute__((aligned(16))) unsigned char lds_v[MODE == DEC_STATS ? 1 : 4][MODE == DEC_STATS ? 16 : 32 * ROWB];
  __shared__ float lds_ml[4][16][2];

  const int bid = blockIdx.x;
  const int bh = bid / DP.n, split = bid - bh * DP.n;
  const int b = bh / P.H, h = bh - b * P.H;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int off = P.Sk - P.Sq;
  const bool qvalid = c < P.Sq;

  // Q^T operand: the lane's query row, 8 consecutive d per k-step (rows beyond Sq: zero)
  u4 qf[2] = {u4{0, 0, 0, 0}, u4{0, 0, 0, 0}};
  if (qvalid) {
    const long qoff = bh_offset(b, P.qs_b, h, P.qs_h) + (long)c * P.qs_s;
    qf[0] = load8_as16<IN>(P.q, qoff + 8 * g);
    qf[1] = load8_as16<IN>(P.q, qoff + 32 + 8 * g);
  }
  const long kbase = bh_offset(b, P.ks_b, h, P.ks_h);
  const long vbase = bh_offset(b, P.vs_b, h, P.vs_h);

  float M = 0.0f, inv_den = 1.0f;  // DEC_CLIP: the whole row's statistics
  if constexpr (MODE == DEC_CLIP) {
    if (qvalid) {
      float den;
      row_stats<FQ>(DP.ml + ((long)bh * DP.n * P.Sq + c) * 2, DP.n, (long)P.Sq * 2, P.base, M, den);
      inv_den = 1.0f / den;
    }
  }

  float m = kNegInf, l = 0.0f;
  f4 acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = f4{0.f, 0.f, 0.f, 0.f};

  const int kchunk0 = split * DP.chunk;
  const int kchunk1 = min(P.Sk, kchunk0 + DP.chunk);
  unsigned char* vt = lds_v[MODE == DEC_STATS ? 0 : wave];

  // loads of one 32-key unit: K rows into the A operand, V rows on their way to LDS
  auto load_unit = [&](const int key0, u4 (&kk)[2][2], u4 (&vv)[4]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = key0 + 16 * t + c;
      kk[t][0] = kk[t][1] = u4{0, 0, 0, 0};
      if (key < P.Sk) {
        const long ko = kbase + (long)key * P.ks_s;
        kk[t][0] = load8_as16<IN>(P.k, ko + 8 * g);
        kk[t][1] = load8_as16<IN>(P.k, ko + 32 + 8 * g);
      }
    }
    if constexpr (MODE != DEC_STATS) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int id = lane + 64 * i, row = id >> 3, ch = id & 7;
        vv[i] = u4{0, 0, 0, 0};  // (keys beyond Sk: zero rows - their probabilities are 0, and 0 x garbage could be NaN)
        if (key0 + row < P.Sk) vv[i] = load8_as16<IN>(P.v, vbase + (long)(key0 + row) * P.vs_s + 8 * ch);
      }
    }
  };
  u4 kn[2][2], vn[4];  // the NEXT unit's rows: requested one unit ahead, so that their latency runs under this unit's arithmetic
  if (kchunk0 + 32 * wave < kchunk1) load_unit(kchunk0 + 32 * wave, kn, vn);

  for (int key0 = kchunk0 + 32 * wave; key0 < kchunk1; key0 += 128) {
    u4 kf[2][2], vr[4];
#pragma unroll
    for (int t = 0; t < 2; ++t) { kf[t][0] = kn[t][0]; kf[t][1] = kn[t][1]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) vr[i] = vn[i];
    if (key0 + 128 < kchunk1) load_unit(key0 + 128, kn, vn);
    // ---- scores: lane (c, g) holds query c, keys key0 + 16 t + 4 g + r
    f4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = mfma16<IN>(kf[t][0], qf[0], f4{0.f, 0.f, 0.f, 0.f});
      s[t] = mfma16<IN>(kf[t][1], qf[1], s[t]);
    }
    float mx = kNegInf;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + 16 * t + 4 * g + r;
        float x;
        if constexpr (FQ) {
          // the reference's order: scale (BERT: a true division), quantise, then the masks.  The statistics and the product pass run these
          // very operations on the same MFMA chain: the same quantised scores, bit for bit.
          x = P.scale_div != 0.0f ? s[t][r] / P.scale_div : s[t][r] * P.scale;
          if (P.fq_s.en) {
            const float rel = fq_rel(x, P.fq_s);
            if constexpr (MODE != DEC_STATS) {
              if (P.fq_s.dump != nullptr && qvalid && key < P.Sk) P.fq_s.dump[((long)bh * P.Sq + c) * P.Sk + key] = (unsigned char)(rel + P.fq_s.zp);
            }
            x = P.fq_s.scale * rel;
          }
        } else {
          x = s[t][r] * P.scale;
        }
        if (key < P.Sk) {
          if (P.pad != nullptr) x = x + load_mask(P.pad, P.pad_f16, (long)b * P.pad_sb + key);
          if (P.causal && key > c + off) x = x + P.mask_min;
          if (P.clamp_min) x = __builtin_fmaxf(x, P.mask_min);
        } else {
          x = kNegInf;
        }
        s[t][r] = x;
        mx = __builtin_fmaxf(mx, x);
      }
    }
    if constexpr (MODE == DEC_CLIP) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float p = exp_d<FQ>(s[t][r], M) * inv_den;
          if (!FQ || P.clip) {
            p = p * P.clip_w;
            p = p + P.clip_g;
            p = __builtin_fminf(__builtin_fmaxf(p, 0.0f), 1.0f);  // (a key beyond Sk: clip(gamma) = 0, gamma <= 0)
          }
          if constexpr (FQ) {
            if (P.fq_p.en) {  // the integer idx - zp (|.| <= 255: exact in f16 and bf16) is the P operand; the scale follows the product in fp32
              const int key = key0 + 16 * t + 4 * g + r;
              p = fq_rel(p, P.fq_p);  // (a masked key or one beyond Sk: p = 0, rel = 0)
              if (P.fq_p.dump != nullptr && qvalid && key < P.Sk) P.fq_p.dump[((long)bh * P.Sq + c) * P.Sk + key] = (unsigned char)(p + P.fq_p.zp);
            }
          }
          s[t][r] = p;
        }
      }
    } else {
      mx = row4_max(mx);
      const float m_new = __builtin_fmaxf(m, mx);
      const float m_ref = m_new == kNegInf ? 0.0f : m_new;  // (every score so far -inf: all terms 0, no inf - inf)
      const float alpha = exp_d<FQ>(m, m_ref);
      float sum = 0.0f;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[t][r] = exp_d<FQ>(s[t][r], m_ref);
          sum = sum + s[t][r];
        }
      }
      l = l * alpha + sum;
      m = m_new;
      if constexpr (MODE == DEC_PLAIN) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[dt][r] = acc[dt][r] * alpha;
      }
    }
    if constexpr (MODE != DEC_STATS) {
      // ---- V rows -> the wave's LDS image (swizzled 32-byte groups), then O^T += V^T P^T
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the previous unit's transposed reads are done
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int id = lane + 64 * i, row = id >> 3, ch = id & 7;
        *reinterpret_cast<u4*>(vt + row * ROWB + (((ch >> 1) ^ ((row >> 1) & 3)) << 5) + ((ch & 1) << 4)) = vr[i];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (a wave's LDS operations complete in order; the image is private to the wave)
      u4 pb;
      if constexpr (IN == IN_BF16) pb = u4{pack2_bf16(s[0][0], s[0][1]), pack2_bf16(s[0][2], s[0][3]), pack2_bf16(s[1][0], s[1][1]), pack2_bf16(s[1][2], s[1][3])};
      else pb = u4{pack2_f16(s[0][0], s[0][1]), pack2_f16(s[0][2], s[0][3]), pack2_f16(s[1][0], s[1][1]), pack2_f16(s[1][2], s[1][3])};
      // The two-launch fake-quant form (no probability quantiser: the weights e^(x - m) are no integers): what the 16-bit rounding of a weight
      // drops goes through the product as a second operand, so that the context - it may feed the context quantiser - carries the weights to
      // ~2^-17 instead of bf16's 2^-9 / fp16's 2^-11 (a context grid has 255 steps: 2^-9 of a value is a sizeable share of one).
      u4 pb2 = u4{0, 0, 0, 0};
      if constexpr (FQ && MODE == DEC_PLAIN) {
        float lo[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const unsigned w = pb[2 * t + (r >> 1)];
            float hi;
            if constexpr (IN == IN_BF16) hi = __builtin_bit_cast(float, (r & 1) ? (w & 0xffff0000u) : (w << 16));
            else hi = (float)__builtin_bit_cast(_Float16, (unsigned short)((r & 1) ? (w >> 16) : (w & 0xffffu)));
            lo[t][r] = s[t][r] - hi;
          }
        if constexpr (IN == IN_BF16) pb2 = u4{pack2_bf16(lo[0][0], lo[0][1]), pack2_bf16(lo[0][2], lo[0][3]), pack2_bf16(lo[1][0], lo[1][1]), pack2_bf16(lo[1][2], lo[1][3])};
        else pb2 = u4{pack2_f16(lo[0][0], lo[0][1]), pack2_f16(lo[0][2], lo[0][3]), pack2_f16(lo[1][0], lo[1][1]), pack2_f16(lo[1][2], lo[1][3])};
      }
      const int row = 4 * g + (c >> 2);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const unsigned char* a0 = vt + row * ROWB + ((dt ^ ((row >> 1) & 3)) << 5) + ((c & 3) << 3);
        const s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(a0));
        const s4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(a0 + 16 * ROWB));
        const u2 l2 = __builtin_bit_cast(u2, lo), h2 = __builtin_bit_cast(u2, hi);
        if constexpr (FQ && MODE == DEC_PLAIN) acc[dt] = mfma16<IN>(u4{l2.x, l2.y, h2.x, h2.y}, pb2, acc[dt]);  // (the small part first)
        acc[dt] = mfma16<IN>(u4{l2.x, l2.y, h2.x, h2.y}, pb, acc[dt]);
      }
    }
  }

  // ---- the four waves' partial results -> one per workgroup.  Lane (c, g) holds O[c][16 dt + 4 g + r].
  if constexpr (MODE != DEC_CLIP) {
    l = row4_sum(l);
    if (g == 0) {
      lds_ml[wave][c][0] = m;
      lds_ml[wave][c][1] = l;
    }
  }
  // (16-byte slot j of accumulator row c sits at j ^ c: the 16 rows of a store no longer share their banks)
  auto acc_slot = [&](const int w, const int r, const int j) { return reinterpret_cast<f4*>(lds_v[MODE == DEC_STATS ? 0 : w]) + r * 16 + (j ^ r); };
  if constexpr (MODE != DEC_STATS) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own last transposed reads of this region are done
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *acc_slot(wave, c, 4 * dt + g) = acc[dt];
  }
  __syncthreads();
  const int row = tid >> 4, quad = tid & 15;
  if (row >= P.Sq) return;
  const long slot = ((long)bh * DP.n + split) * P.Sq + row;
  f4 a = f4{0.f, 0.f, 0.f, 0.f};
  if constexpr (MODE == DEC_CLIP) {
#pragma unroll
    for (int w = 0; w < 4; ++w) a = a + *acc_slot(w, row, quad);
  } else {
    float mw = kNegInf;
#pragma unroll
    for (int w = 0; w < 4; ++w) mw = __builtin_fmaxf(mw, lds_ml[w][row][0]);
    const float m_ref = mw == kNegInf ? 0.0f : mw;
    float lw = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float e = exp_d<FQ>(lds_ml[w][row][0], m_ref);
      lw = lw + lds_ml[w][row][1] * e;
      if constexpr (MODE == DEC_PLAIN) a = a + *acc_slot(w, row, quad) * e;
    }
    if (quad == 0) *reinterpret_cast<f2*>(DP.ml + slot * 2) = f2{mw, lw};
  }
  if constexpr (MODE != DEC_STATS) *reinterpret_cast<f4*>(DP.acc + slot * 64 + 4 * quad) = a;
}

// One thread per (batch, head, query row, 4 output columns): the splits in their fixed order, the gate, the store.
// SUM: the three-launch forms - the slabs are sums of y v already (with the probability quantiser: of (idx - zp) v, its scale applied here).
// FQ: the context quantiser before or after the gate (oeh_common.h: ctx_chain), its index dump.
template <bool SUM, bool FQ = false>
__global__ __launch_bounds__(256) void oeh_attn_decode_combine(const DecodeParams DP) {
  const AttnParams& P = DP.A;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long rows = (long)P.nBH * P.Sq;
  if (idx >= rows * 16) return;
  const int quad = (int)(idx & 15);
  const long r = idx >> 4;
  const int bh = (int)(r / P.Sq), row = (int)(r - (long)bh * P.Sq);
  const int b = bh / P.H, h = bh - b * P.H;
  const long stride = (long)P.Sq * 64;
  const float* ap = DP.acc + ((long)bh * DP.n * P.Sq + row) * 64 + 4 * quad;
  f4 o = f4{0.f, 0.f, 0.f, 0.f};
  if constexpr (SUM) {
    for (int s = 0; s < DP.n; ++s) o = o + *reinterpret_cast<const f4*>(ap + s * stride);
    if constexpr (FQ) {
      if (P.fq_p.en) o = o * P.fq_p.scale;
    }
  } else {
    const float* ml = DP.ml + ((long)bh * DP.n * P.Sq + row) * 2;
    float M, den;
    row_stats<FQ>(ml, DP.n, (long)P.Sq * 2, P.base, M, den);
    for (int s = 0; s < DP.n; ++s) o = o + *reinterpret_cast<const f4*>(ap + s * stride) * exp_d<FQ>(ml[s * (long)P.Sq * 2], M);
    const float inv = 1.0f / den;
    o = o * inv;
  }
  if constexpr (FQ) {
    const bool gated = P.gate != nullptr;
    const float gatev = gated ? P.gate[(long)b * P.gs_b + (long)h * P.gs_h + (long)row * P.gs_s] : 1.0f;
    float x[4] = {o[0], o[1], o[2], o[3]}, rel[4] = {0.f, 0.f, 0.f, 0.f};
    ctx_chain<4, true>(x, P.fq_c, P.ctx_before_gate, gated, gatev, rel);
    if (P.fq_c.en && P.fq_c.dump != nullptr) *reinterpret_cast<unsigned int*>(P.fq_c.dump + r * 64 + 4 * quad) = fq_dump_word(f4{rel[0], rel[1], rel[2], rel[3]}, P.fq_c);
    o = f4{x[0], x[1], x[2], x[3]};
  } else {
    if (P.gate != nullptr) o = o * P.gate[(long)b * P.gs_b + (long)h * P.gs_h + (long)row * P.gs_s];
  }
  const long ooff = bh_offset(b, P.os_b, h, P.os_h) + (long)row * P.os_s + 4 * quad;
  if (DP.out == IN_F32) *reinterpret_cast<f4*>(reinterpret_cast<float*>(P.o) + ooff) = o;
  else if (DP.out == IN_BF16) *reinterpret_cast<u2*>(reinterpret_cast<unsigned short*>(P.o) + ooff) = u2{pack2_bf16(o[0], o[1]), pack2_bf16(o[2], o[3])};
  else *reinterpret_cast<u2*>(reinterpret_cast<unsigned short*>(P.o) + ooff) = u2{pack2_f16(o[0], o[1]), pack2_f16(o[2], o[3])};
}

template <int IN>
int launch_decode_in(const DecodeParams& DP, hipStream_t st, const bool fq) {
  const dim3 grid((unsigned)((long)DP.A.nBH * DP.n)), block(256);
  const dim3 cgrid((unsigned)(((long)DP.A.nBH * DP.A.Sq * 16 + 255) / 256));
  if (fq) {
    if (DP.A.clip || DP.A.fq_p.en) {
      hipLaunchKernelGGL((oeh_attn_decode_partial<IN, DEC_STATS, true>), grid, block, 0, st, DP);
      hipLaunchKernelGGL((oeh_attn_decode_partial<IN, DEC_CLIP, true>), grid, block, 0, st, DP);
      hipLaunchKernelGGL((oeh_attn_decode_combine<true, true>), cgrid, block, 0, st, DP);
    } else {
      hipLaunchKernelGGL((oeh_attn_decode_partial<IN, DEC_PLAIN, true>), grid, block, 0, st, DP);
      hipLaunchKernelGGL((oeh_attn_decode_combine<false, true>), cgrid, block, 0, st, DP);
    }
  } else if (DP.A.clip) {
    hipLaunchKernelGGL((oeh_attn_decode_partial<IN, DEC_STATS>), grid, block, 0, st, DP);
    hipLaunchKernelGGL((oeh_attn_decode_partial<IN, DEC_CLIP>), grid, block, 0, st, DP);
    hipLaunchKernelGGL((oeh_attn_decode_combine<true>), cgrid, block, 0, st, DP);
  } else {
    hipLaunchKernelGGL((oeh_attn_decode_partial<IN, DEC_PLAIN>), grid, block, 0, st, DP);
    hipLaunchKernelGGL((oeh_attn_decode_combine<false>), cgrid, block, 0, st, DP);
  }
  return launch_status();
}

}  // namespace

namespace {

// ---- host side: validation in the order the ABI promises, the split rule, the launches

// The default split count (splits == 0): chunks of at least 256 keys and about three workgroups per CU (B H n ~ 768), n <= 64; one split up to
// 128 keys (in fact below 512) and once the heads fill the chip by themselves (B H >= 512).
// Measured (one MI355X, H = 12, Sq = 1, fp16, causal; event times of graph replays over a ring of K / V buffer sets, tools/decode_bench.py
// --sweep, profiles/decode_bench.txt; us per call, softmax1 / clippedsoftmax1) - the issue's starting rule (B H n ~ 512, chunks >= 128) split too fine:
//   B = 1,  Sk = 2048: SP1 22.0 / 41.0  SP2 14.5 / 24.9  SP4 11.1 / 17.8  SP8 10.7 / 15.5  SP16 13.0 / 17.0  SP32 20.2 / 24.6   -> 8 (chunks of 256)
//   B = 1,  Sk = 512:  SP1 9.0 / 14.7   SP2 7.5 / 11.5   SP4 7.3 / 10.4   SP8 8.6 / 11.6                                       -> 2 (within 3 % / 10 % of 4)
//   B = 16, Sk = 2048: SP1 27.4 / 48.6  SP2 24.1 / 36.8  SP4 24.6 / 34.1  SP8 25.6 / 37.8  SP16 30.9 / 47.2  SP32 45.7 / 89.3   -> 4
//   B = 16, Sk = 512:  SP1 10.9 / 17.6  SP2 10.8 / 15.5  SP4 11.5 / 15.3  SP8 15.0 / 20.8                                       -> 2
int default_splits(const oeh_attn_desc* d) {
  const long bh = (long)d->B * d->H;
  if (d->Sk <= 128 || bh >= 512) return 1;
  long n = (768 + bh - 1) / bh;
  const long by_len = d->Sk / 256;
  if (n > by_len) n = by_len;
  if (n > OEH_DECODE_MAX_SPLITS) n = OEH_DECODE_MAX_SPLITS;
  return n < 1 ? 1 : (int)n;
}

struct DecodePlan {
  int rc;
  int n, chunk;
};

// host_only (work_bytes / variant): no pointers to judge
DecodePlan plan_decode(const oeh_attn_desc* d, int splits, bool host_only, const void* q, const void* k, const void* v, const void* o, const void* work) {
  DecodePlan pl = {OEH_OK, 0, 0};
  // 1. invalid arguments
  if (!host_only && (q == nullptr || k == nullptr || v == nullptr || o == nullptr || work == nullptr)) { pl.rc = OEH_EINVAL; return pl; }
  if (!desc_sane(d, true, true) || splits < 0 || splits > OEH_DECODE_MAX_SPLITS || !softmax_base_ok(d->softmax_base) || !key_pad_ok(d)) { pl.rc = OEH_EINVAL; return pl; }
  // 2. outside the scope
  if (d->full_mask != nullptr || d->gate_hidden != nullptr || (d->dtype != OEH_F16 && d->dtype != OEH_BF16) || d->D != 64 || d->Sq > 16 ||
      (d->clip && d->gamma > 0.0f) || (d->causal && d->Sq > d->Sk)) { pl.rc = OEH_ENOTSUP; return pl; }
  if (d->scale_div != 0.0f ? !(d->scale_div > 0.0f && std::isfinite(d->scale_div)) : !std::isfinite(d->scale)) { pl.rc = OEH_ENOTSUP; return pl; }
  if ((int64_t)d->B * d->H * OEH_DECODE_MAX_SPLITS >= ((int64_t)1 << 31)) { pl.rc = OEH_ENOTSUP; return pl; }
  if (!host_only && !desc_strides_in_range(d)) { pl.rc = OEH_ENOTSUP; return pl; }  // (the host-only calls do not judge strides)
  // 3. alignment
  if (!host_only) {
    const int ob = d->o_dtype == OEH_F32 ? 4 : 2;
    if (!aligned16(q, d->q_stride, 2) || !aligned16(k, d->k_stride, 2) || !aligned16(v, d->v_stride, 2) || !aligned16(o, d->o_stride, ob) || !all16(addr(work))) {
      pl.rc = OEH_EALIGN;
      return pl;
    }
  }
  const int want = splits == 0 ? default_splits(d) : splits;
  const int per = (d->Sk + want - 1) / want;
  pl.chunk = (per + 63) & ~63;
  pl.n = (d->Sk + pl.chunk - 1) / pl.chunk;
  return pl;
}

int64_t ml_bytes(const oeh_attn_desc* d, int n) { return (((int64_t)d->B * d->H * n * d->Sq * 2 * 4) + 15) & ~(int64_t)15; }

// oeh_attn_decode_fq's own refusals, after those of the plan: OEH_EINVAL (a grid that is none), then OEH_ENOTSUP
int check_fq(const oeh_fq_desc* fq) {
  const oeh_fq* fs[3] = {&fq->scores, &fq->probs, &fq->ctx};
  for (const oeh_fq* f : fs)
    if (f->enable && !fq_grid_ok(*f, true)) return OEH_EINVAL;
  if (fq->ctx_emit_index) return OEH_ENOTSUP;
  for (const oeh_fq* f : fs)
    if (f->enable && !fq_dump_fits(*f)) return OEH_ENOTSUP;
  return OEH_OK;
}

// fq: null or with at least one quantiser enabled and judged by check_fq
int run_decode(const oeh_attn_desc* desc, const oeh_fq_desc* fq, const DecodePlan& pl, const void* q, const void* k, const void* v, void* o, void* work, void* stream) {
  DecodeParams DP;
  std::memset(&DP, 0, sizeof(DP));
  AttnParams& P = DP.A;
  fill_problem(P, desc);  // (no (B,1,Sq,Sk) mask: the plan has refused it; nothing of the inference kernels' launch geometry)
  P.q = q; P.k = k; P.v = v; P.o = o;
  P.D = desc->D;
  P.scale = desc->scale_div != 0.0f ? 1.0f / desc->scale_div : desc->scale;  // (a divisor: one more rounding of 6e-8 relative, as in the other 16-bit kernels)
  P.gate = desc->gate; P.gs_b = desc->gate_stride[0]; P.gs_h = desc->gate_stride[1]; P.gs_s = desc->gate_stride[2];
  P.nBH = desc->B * desc->H;
  if (fq != nullptr) {
    P.scale_div = desc->scale_div;  // (the fake-quant forms divide: the quotient feeds the scores quantiser)
    P.fq_s = make_fq(&fq->scores); P.fq_p = make_fq(&fq->probs); P.fq_c = make_fq(&fq->ctx);
    P.ctx_before_gate = fq->ctx_quant_before_gate ? 1 : 0;
  }
  DP.n = pl.n;
  DP.chunk = pl.chunk;
  DP.ml = static_cast<float*>(work);
  DP.acc = reinterpret_cast<float*>(static_cast<unsigned char*>(work) + ml_bytes(desc, pl.n));
  DP.out = desc->o_dtype == OEH_F32 ? IN_F32 : (desc->dtype == OEH_BF16 ? IN_BF16 : IN_F16);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return dispatch_in16(desc->dtype, [&](auto t) { return launch_decode_in<decltype(t)::value>(DP, st, fq != nullptr); });
}

}  // namespace
}  // namespace oeh

extern "C" {

int64_t oeh_attn_decode_work_bytes(const oeh_attn_desc* desc, int32_t splits) {
  const oeh::DecodePlan pl = oeh::plan_decode(desc, splits, true, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (pl.rc != OEH_OK) return pl.rc;
  return oeh::ml_bytes(desc, pl.n) + (int64_t)desc->B * desc->H * pl.n * desc->Sq * 64 * 4;
}

const char* oeh_attn_decode_variant(const oeh_attn_desc* desc, int32_t splits) {
  static thread_local char buf[64];
  const oeh::DecodePlan pl = oeh::plan_decode(desc, splits, true, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (pl.rc != OEH_OK) return nullptr;
  std::snprintf(buf, sizeof(buf), "decode16/SP%d/D64/%s%s", pl.n, desc->dtype == OEH_BF16 ? "bf16" : "f16", desc->clip ? "/clip" : "");
  return buf;
}

int oeh_attn_decode(const oeh_attn_desc* desc, int32_t splits, const void* q, const void* k, const void* v, void* o, void* work, void* stream) {
  const oeh::DecodePlan pl = oeh::plan_decode(desc, splits, false, q, k, v, o, work);
  if (pl.rc != OEH_OK) return pl.rc;
  return oeh::run_decode(desc, nullptr, pl, q, k, v, o, work, stream);
}

const char* oeh_attn_decode_fq_variant(const oeh_attn_desc* desc, const oeh_fq_desc* fq, int32_t splits) {
  static thread_local char buf[64];
  const char* name = oeh_attn_decode_variant(desc, splits);
  if (name == nullptr || !oeh::any_fq(fq)) return name;
  if (oeh::check_fq(fq) != OEH_OK) return nullptr;
  std::snprintf(buf, sizeof(buf), "%s/fq", name);
  return buf;
}

int oeh_attn_decode_fq(const oeh_attn_desc* desc, const oeh_fq_desc* fq, int32_t splits, const void* q, const void* k, const void* v, void* o, void* work,
                       void* stream) {
  const oeh::DecodePlan pl = oeh::plan_decode(desc, splits, false, q, k, v, o, work);
  if (pl.rc != OEH_OK) return pl.rc;
  if (!oeh::any_fq(fq)) return oeh::run_decode(desc, nullptr, pl, q, k, v, o, work, stream);
  const int rc = oeh::check_fq(fq);
  if (rc != OEH_OK) return rc;
  return oeh::run_decode(desc, fq, pl, q, k, v, o, work, stream);
}

}  // extern "C"
