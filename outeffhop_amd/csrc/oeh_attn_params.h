// Kernel-argument block shared by the fused attention kernels (the host fills it: the problem fields in oeh_desc.h fill_problem, the rest in oeh_api.hip fill_params).
#pragma once
#include "oeh_common.h"

namespace oeh {

struct AttnParams {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  int B, H, Sq, Sk, D;
  long qs_b, qs_h, qs_s;
  long ks_b, ks_h, ks_s;
  long vs_b, vs_h, vs_s;
  long os_b, os_h, os_s;
  float scale, scale_div;     // scale_div != 0: divide (BERT), else multiply
  int base;                   // 0 vanilla, 1 softmax_1
  int clip;
  float clip_w, clip_g;       // fl32(eta - gamma), fl32(gamma)
  const void* pad;            // (B,Sk) additive or null
  int pad_f16;
  long pad_sb;
  const void* full;           // (B,1,Sq,Sk) additive or null
  int full_f16;
  long full_sb, full_sq;
  int causal, clamp_min;
  float mask_min;
  const float* gate;          // null = none
  long gs_b, gs_h, gs_s;
  // fused gate predictor (null gh = none): layer input rows, per-head weights, optional copy of the gate (include/oeh.h)
  const void* gh;
  long ghs_b, ghs_t;
  const float *gw1, *gb1, *gw2, *gb2;
  int g_units;
  float g_scaling;
  float* g_out;
  FqP fq_s, fq_p, fq_c;
  int ctx_before_gate;
  int src32;                  // fp32 q / k / v read directly by the kernel and fp32 output (SRC32 variants); 2: the same with the probability
                              // operand as an fp16 pair (PV2 variants, include/oeh.h: oeh_attn_opts.pv_pairs) - host side only, a launch choice
  int out32;                  // 16-bit q / k / v, fp32 output straight from the accumulators (o_dtype = OEH_F32; one-pass and full-row kernels)
  // INT8 storage (oeh_attn_i8.hip): 128 - zero point of q, k, v and of the probabilities; RN(s_q s_k scale / s_scores), RN(s_p s_v)
  int i8_cq, i8_ck, i8_cv, i8_cp;
  float i8_k1, i8_so;
  // launch geometry
  int nQT;                    // q tiles (64 rows) per (b,h)
  int nBH, nBHpad;            // B*H and B*H rounded up to a multiple of 8 (XCD affinity of a head's q tiles)
  unsigned magic_nbh, magic_h;  // floor(2^32 / nBHpad), floor(2^32 / H): block id -> (q tile, batch, head) without integer divisions (oeh_common.h: div_magic)
  int skip_ok;                // causal tiles above the diagonal may be skipped (oeh_desc.h: causal_skip_ok)
  int pad_bool;   // key_pad_boolean (include/oeh.h): mask entries are 0 or <= -1e4
  int head_major;             // fp32-storage kernels: block order in groups of this many heads (0 = all heads' heaviest q tiles first;
                              // oeh_common.h: block_to_tile)
  int snake;                  // one-pass kernel: every second row of 256 block ids walked backwards (snake_block_id, oeh_common.h)
  unsigned long long* stamps; // diagnostic builds only: per-wave s_memtime stamps (null in production)
};

// The hot argument prefix of the one-pass kernel's plain 16-bit forms (oeh_attn_flash.inl: oeh_attn_flash_hot_kernel): what the block-id
// decode and the Q / K / V requests read, as LEADING SCALAR kernel arguments in front of the AttnParams block.  gfx950 delivers leading
// scalar arguments in user SGPRs at wave launch (kernarg preload: 16 user SGPRs less the 2 of the segment pointer = 14 dwords; a by-value
// struct is never preloaded), so a wave needs no memory round trip before its first request.  Exactly 14 dwords: nBHpad is the kernel's
// (nBH + 7) & ~7, Sq and Sk share a dword, q / k / v share one set of strides (the host launches this form only then: oeh_api.hip,
// fill_hot).  The kernel's parameter list spells the same fields in the same order (OEH_HOT_PARAMS / OEH_HOT_ARGS).
struct AttnHot {
  const void *q, *k, *v;
  int nBH;
  unsigned magic_nbh, magic_h;
  unsigned geom;              // H [15:0] | nQT [27:16] | causal [30] | snake [31]
  unsigned sqsk;              // Sq [15:0] | Sk [31:16]
  unsigned s_b, s_h, s_s;     // (batch, head, row) strides in elements, the same for q, k and v
};
#define OEH_HOT_PARAMS const void *hq, const void *hk, const void *hv, int h_nbh, unsigned h_mnbh, unsigned h_mh, unsigned h_geom, unsigned h_sqsk, unsigned h_sb, unsigned h_sh, unsigned h_ss
#define OEH_HOT_ARGS(X) (X).q, (X).k, (X).v, (X).nBH, (X).magic_nbh, (X).magic_h, (X).geom, (X).sqsk, (X).s_b, (X).s_h, (X).s_s
constexpr int kHotMaxH = 0xffff, kHotMaxNQT = 0xfff, kHotMaxS = 0xffff;

// The kernels' view of one quantiser from the ABI's oeh_fq (include/oeh.h; a template only so that this header does not need it): host side,
// shared by every entry point that takes an oeh_fq_desc.
template <class OehFq>
inline FqP make_fq(const OehFq* f) {
  FqP r = {};
  if (f != nullptr && f->enable) {
    r.en = 1;
    r.scale = f->scale;
    r.rscale = 1.0f / f->scale;
    r.zp = f->zero_point;
    r.qmax = f->qmax;
    r.lo = -f->zero_point;
    r.hi = f->qmax - f->zero_point;
    r.dump = f->dump_idx;
    r.c2 = (float)((double)f->scale * 1.4426950408889634074);  // RN(scale * log2(e)), the product formed in double
    r.oscale = f->scale;
  }
  return r;
}

}  // namespace oeh
