// The attention forward dispatcher of liboeh_hip.so - oeh_attn_fwd[_ex], oeh_attn_variant[_ex] and oeh_attn_calibrate: descriptor validation,
// kernel variant selection and the launch across the attention units (oeh_launch.h) - plus what belongs to the whole library: the debug
// hooks, oeh_abi_version, oeh_build_info, oeh_strerror.  Every other extern "C" entry point of include/oeh.h lives in the unit that owns its
// kernels.  No allocation, no synchronisation: safe under hipGraph capture.
#include "../../include/oeh.h"
#include "../../include/oeh_debug.h"
#include "oeh_desc.h"
#include "oeh_launch.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using oeh::AttnParams;
using oeh::FqP;
// the descriptor predicates and the descriptor -> kernel block fill (oeh_desc.h)
using oeh::addr; using oeh::aligned16; using oeh::all16; using oeh::any_fq; using oeh::desc_sane; using oeh::dtype_ok; using oeh::elem_bytes; using oeh::softmax_base_ok;

namespace {

using oeh::make_fq;  // (oeh_attn_params.h)

enum Variant { V_NONE = 0, V_FLASH, V_FAST, V_MFMA, V_GENERIC, V_SMALL, V_I8 };

// Diagnostic hooks (include/oeh_debug.h; oeh_debug_set_variant / oeh_debug_set_stamps below): the bits of off_mask by name.  Bit
// (1 << Variant) switches a variant off; bits 6 / 7 are no Variant values.
enum Hook {
  HOOK_NO_FLASH_F32 = 1 << 6,   // the fp32-storage form of the one-pass kernel off
  HOOK_NO_FAST_F32 = 1 << 7,    // the fp32-storage form of the full-row kernel off
  HOOK_FORCE_FLASH = 1 << 8,    // tools/microbench.py only: the one-pass kernel also where the full-row kernel measured faster
  HOOK_PLAIN_ORDER = 1 << 9,    // tools/microbench.py only: plain block order in the one-pass kernel (no snake placement)
  HOOK_FORCE_SMALL = 1 << 10,   // tests: the small-shape kernel wherever it can run (no size heuristic)
  HOOK_NO_D128_RULE = 1 << 11,  // tests: the full-row kernel also for head dim 128 with clip / INT8 (the comparison against the general kernel)
  HOOK_NO_HOT_ARGS = 1 << 13,   // tests / A-B: the one-pass kernel's plain forms from the AttnParams block alone (no hot argument prefix)
  HOOK_ALL = 0x2fff             // (bit 12, bit 14 and up: reserved, ignored)
};
struct Hooks {
  int off;                      // off_mask & HOOK_ALL
  int flash_mq;                 // tools/microbench.py only: force query blocks per wave
  int head_group;               // tools/microbench.py only (OEH_HEAD_GROUP): block order of the fp32-storage kernels in groups of heads
  unsigned long long* stamps;   // tools/timeline.py only
  long hot_launches;            // one-pass launches that took the hot argument prefix (oeh_debug_hot_launches)
} g_hooks = {};

int validate(const oeh_attn_desc* d, const void* q, const void* k, const void* v, void* o, const oeh_fq_desc* fq) {
  if (q == nullptr || k == nullptr || v == nullptr || o == nullptr || !desc_sane(d, true, true)) return OEH_EINVAL;
  if (d->dtype == OEH_I8) {
    if (!dtype_ok(d->o_dtype) && d->o_dtype != OEH_I8) return OEH_EINVAL;
    // (an int8 output is the context quantiser's centred indices: only with ctx_emit_index on a full 8-bit grid with a whole zero point)
    if (d->o_dtype == OEH_I8 && (fq == nullptr || !fq->ctx_emit_index || !fq->ctx.enable || fq->ctx.qmax != 255.0f || fq->ctx.zero_point != std::nearbyint(fq->ctx.zero_point)))
      return OEH_EINVAL;
    const float zs[3] = {d->q_grid.zero_point, d->k_grid.zero_point, d->v_grid.zero_point};
    const float ss[3] = {d->q_grid.scale, d->k_grid.scale, d->v_grid.scale};
    for (int i = 0; i < 3; ++i)
      if (!(ss[i] > 0.0f) || !(zs[i] >= 0.0f && zs[i] <= 255.0f) || zs[i] != std::nearbyint(zs[i])) return OEH_EINVAL;
  }
  if (!softmax_base_ok(d->softmax_base)) return OEH_EINVAL;
  if (!oeh::desc_strides_in_range(d)) return OEH_ENOTSUP;
  if (fq != nullptr && fq->ctx_emit_index) {  // the integers idx - zp instead of values: only where the context quantiser is the last op
    const bool gated = d->gate != nullptr || d->gate_hidden != nullptr;
    if (!fq->ctx.enable || (gated && fq->ctx_quant_before_gate)) return OEH_EINVAL;
  }
  if (!oeh::key_pad_ok(d) || !oeh::full_mask_ok(d)) return OEH_EINVAL;
  if (d->gate == nullptr && d->gate_hidden != nullptr) {
    if (d->gate_w1 == nullptr || d->gate_b1 == nullptr || d->gate_units < 0) return OEH_EINVAL;
    if (d->gate_units > 0 && (d->gate_w2 == nullptr || d->gate_b2 == nullptr)) return OEH_EINVAL;
  }
  if (fq != nullptr) {
    const oeh_fq* fs[3] = {&fq->scores, &fq->probs, &fq->ctx};
    for (const oeh_fq* f : fs) {
      if (!f->enable) continue;
      if (!oeh::fq_grid_ok(*f, false)) return OEH_EINVAL;
      if (!oeh::fq_dump_fits(*f)) return OEH_ENOTSUP;
    }
  }
  return OEH_OK;
}

// the per-token gate predictor evaluated in the kernel (gate values given: they win)
bool gate_in_kernel(const oeh_attn_desc* d) { return d->gate == nullptr && d->gate_hidden != nullptr; }

bool is_pow2(float x) {
  int e = 0;
  return x > 0.0f && std::isfinite(x) && std::frexp(x, &e) == 0.5f;
}

// ---- What each kernel family CAN run.  Where another family's kernel reuses these conditions it says so in the arguments: as16 - fp32
// storage counts as 16-bit (the SRC32 forms read it directly: tiles staged through registers, fp16 operands, fp32 output); no_full - the
// caller's kernel reads the (B,1,Sq,Sk) mask itself.

// The fast kernel (oeh_attn_fast.inl) covers 16-bit storage, masks in {none, key padding, causal} and a positive
// multiplicative scale (a power-of-two divisor is the same multiply, exactly); fake-quant is its FQ variant.
bool fast_can(const oeh_attn_desc* d, const oeh_fq_desc* fq, bool as16 = false, bool no_full = false) {
  if ((d->dtype == OEH_F32 && !as16) || (d->full_mask != nullptr && !no_full)) return false;
  // the LDS-DMA streams address a tile as scalar base + 32-bit lane byte offsets (up to 64 rows of the sequence stride)
  if (d->q_stride[2] >= (1 << 24) || d->k_stride[2] >= (1 << 24) || d->v_stride[2] >= (1 << 24) || d->q_stride[2] < 0 || d->k_stride[2] < 0 || d->v_stride[2] < 0) return false;
  if (any_fq(fq)) {  // the FQ variant: scores and probabilities both quantised (the reference's configuration), no in-kernel predictor
    if (!(fq->scores.enable && fq->probs.enable) || gate_in_kernel(d)) return false;
    if (fq->scores.dump_idx != nullptr || fq->probs.dump_idx != nullptr || fq->ctx.dump_idx != nullptr) return false;  // test-only dumps: general kernel
  }
  // a divisor (BERT order, bert_attention.py:265): a power of two is the same multiply exactly; any other positive divisor
  // becomes a multiply by RN(1/div) - one more rounding of 6e-8 relative, far inside the accuracy of the 16-bit paths -
  // except under fake-quant, where the index must come from the reference's own rounding (general kernel: true division)
  if (d->scale_div != 0.0f ? !(is_pow2(d->scale_div) || (!any_fq(fq) && d->scale_div > 0.0f && std::isfinite(d->scale_div)))
                           : !(d->scale > 0.0f && std::isfinite(d->scale))) return false;
  if (d->clip && d->gamma > 0.0f) return false;
  if (d->causal && d->Sq > d->Sk) return false;
  if ((d->causal || d->key_pad_mask != nullptr) && !(d->mask_min < -1.0e4f)) return false;
  return true;
}

// The one-pass kernel (oeh_attn_flash.inl) additionally needs the plain softmax_n (no clip).  No Sk limit.
// fp32 storage (as16): the same conditions on the problem; the in-kernel gate predictor reads a 16-bit layer input and is not available
bool flash_can(const oeh_attn_desc* d, const oeh_fq_desc* fq, bool as16) {
  if (d->clip || any_fq(fq) || (as16 && gate_in_kernel(d))) return false;
  // a (B,1,Sq,Sk) mask: only where the general kernel does not reach (rows of more than 512 keys); PAD variant
  if (d->full_mask != nullptr) return d->Sk > 512 && fast_can(d, fq, as16, true) && (d->mask_min < -1.0e4f);
  // (key padding under the vanilla softmax: a row without a visible key is uniform over ALL keys in the reference - the PAD variant's
  // epilogue gives such rows the mean of V, oeh_attn_flash.inl)
  return fast_can(d, fq, as16);
}

// The one-pass kernel's two-pass forms, in 16-bit and (SRC32, operand pairs) fp32 storage alike, no in-kernel gate predictor:
//  - the fused INT8 chain (TP = 2).  What the full-row kernel's FQ == 1 takes: scores and probabilities both quantised, no clip, no key
//    padding, no test dumps;
//  - clipped softmax (CLIP: statistics, then the product; oeh_attn_flash.inl).
bool flash_two_pass_can(const oeh_attn_desc* d, const oeh_fq_desc* fq) {
  if (gate_in_kernel(d)) return false;
  if (any_fq(fq)) {
    if (!fast_can(d, fq, true)) return false;  // (fast_can: both quantisers, no dumps, scale, masks, gamma <= 0 when clipped)
    // key padding: on the grid only as a vector of 0 / <= -1e4 entries (key_pad_boolean), and with softmax_1 (trailing padded tiles are not streamed)
    if (d->key_pad_mask != nullptr && !(d->key_pad_boolean && d->softmax_base == OEH_SOFTMAX_ONE)) return false;
    return !(fq->probs.qmax > (d->dtype == OEH_BF16 ? 255.0f : 2047.0f));  // the integer-valued P operand must be exact
  }
  // round 4: a (B,1,Sq,Sk) mask on rows of more than 512 keys too (the PAD variants read it per block, as the plain one-pass form does)
  const bool long_full = d->full_mask != nullptr && d->Sk > 512 && (d->mask_min < -1.0e4f);
  // (key padding / a full mask under the VANILLA softmax since round 4: a row without a visible key - uniform over all Sk keys in the
  // reference - gets clip(w / Sk + gamma) times the sum of V in the epilogue, oeh_attn_flash.inl)
  return d->clip && fast_can(d, fq, true, long_full);  // (fast_can: gamma <= 0, masks, scale)
}

// The small-shape kernel (oeh_attn_small.hip: one wave per (batch, head), K and V in registers, fp32 matrix-core products):
// many tiny problems - STanHop's Association (L, S ~ 28, H = 4, E in {16, 32, 64}, batch * data_dim problems).  No masks,
// no fake-quant, no in-kernel gate predictor; rows of 4 elements must be 4-element aligned (16 B in fp32, 8 B in 16-bit).
bool small_can(const oeh_attn_desc* d, const void* q, const void* k, const void* v, const void* o, const oeh_fq_desc* fq) {
  if (any_fq(fq) || d->key_pad_mask != nullptr || d->full_mask != nullptr || d->causal) return false;
  if (gate_in_kernel(d)) return false;
  if (!(d->D == 16 || d->D == 32 || d->D == 64) || d->Sk > 64 || d->Sq > 64) return false;
  const int ab = 4 * elem_bytes(d->dtype);
  const int64_t* sts[4] = {d->q_stride, d->k_stride, d->v_stride, d->o_stride};
  const void* ps[4] = {q, k, v, o};
  for (int t = 0; t < 4; ++t) {
    if (q != nullptr && (reinterpret_cast<uintptr_t>(ps[t]) % ab) != 0) return false;
    for (int i = 0; i < 3; ++i)
      if ((sts[t][i] & 3) != 0) return false;
  }
  return true;
}

// INT8 storage (oeh_attn_i8.hip): see include/oeh.h, oeh_attn_desc.q_grid
bool i8_eligible(const oeh_attn_desc* d, const void* q, const void* k, const void* v, const void* o, const oeh_fq_desc* fq) {
  if (d->dtype != OEH_I8 || d->D != 64 || d->Sk > 512 || (d->Sk & 15) != 0) return false;
  if (fq == nullptr || !fq->scores.enable || !fq->probs.enable || fq->probs.qmax != 255.0f) return false;
  // the kernel forms the probabilities' indices with the float zero point and centres them with the integer one; the score
  // index is rounded in the integer domain: both zero points must be whole numbers (they are: uniform_quantizers.py:79 rounds)
  if (fq->probs.zero_point != std::nearbyint(fq->probs.zero_point) || fq->scores.zero_point != std::nearbyint(fq->scores.zero_point)) return false;
  const bool dumps = fq->scores.dump_idx != nullptr || fq->probs.dump_idx != nullptr || fq->ctx.dump_idx != nullptr;
  if (dumps && d->o_dtype != OEH_F32) return false;  // the index dumps (tests) exist in the fp32-output form
  if ((d->clip && d->gamma > 0.0f) || d->full_mask != nullptr || gate_in_kernel(d)) return false;
  if (d->key_pad_mask != nullptr && !(d->mask_min < -1.0e4f)) return false;  // (a key-padding vector of 0 / <= -1e4 entries: include/oeh.h)
  if (d->scale_div != 0.0f ? !(d->scale_div > 0.0f && std::isfinite(d->scale_div)) : !(d->scale > 0.0f && std::isfinite(d->scale))) return false;
  if (d->causal && (d->Sq > d->Sk || !(d->mask_min < -1.0e4f))) return false;
  if (d->k_stride[2] <= 0 || d->k_stride[2] >= (1 << 24) || d->v_stride[2] <= 0 || d->v_stride[2] >= (1 << 24)) return false;  // 32-bit lane offsets inside a tile
  if (q != nullptr) {
    const int ob = elem_bytes(d->o_dtype);
    if (!aligned16(q, d->q_stride, 1) || !aligned16(k, d->k_stride, 1) || !aligned16(v, d->v_stride, 1) || !aligned16(o, d->o_stride, ob)) return false;
  }
  return true;
}

// ---- What MEASURED faster, among the kernels that can run a problem (16-bit and fp32 storage share every rule; HOOK_FORCE_FLASH
// lifts the ones on the one-pass kernel)

// The plain one-pass form against the full-row kernel on rows of <= 128 keys (never with a (B,1,Sq,Sk) mask: those rows have > 512 keys).
bool prefer_full_row_short(const oeh_attn_desc* d) {
  // short rows (<= 128 keys) fit the full-row kernel's registers in one pass, which measures faster there (BERT-base B=32 S=128:
  // 7.7 vs 9.7 us per launch) - until the batch is large enough for the one-pass kernel's 128-row workgroups to fill the chip by
  // themselves (>= 768 of them): then its halved K / V streaming wins (H=12 S=128, round 3: B=48 12.3 vs 13.0 us, B=64 15.5 vs 14.5,
  // B=96 23.0 vs 20.3, B=128 31.5 vs 24.2)
  // fp32 storage, rows of <= 128 keys: the full-row kernel's fp32 form where it applies, at every batch size measured (round 3, H=12 S=128: B=32 16.5
  // vs 20.0 us, B=64 29.8 vs 30.6, B=128 54.6 vs 57.7); what it does not take stays here (16.7 us in the general kernel)
  // (with >= 768 of its 128-row workgroups the one-pass form is ahead again: B=64 25.8 vs 30.5 us; with a padding vector 30.5 vs 31.5 -
  // round 4: one rule for both, profiles/r04_dispatch_ab.txt)
  if (d->full_mask != nullptr || d->Sk > 128 || (g_hooks.off & HOOK_FORCE_FLASH)) return false;
  const long wgs = (long)d->B * d->H * ((d->Sq + 127) / 128);
  // (one threshold for every head dim since round 4: at d = 32 and 768 workgroups the one-pass kernel measured 10.0 vs 11.0 us, at
  // 1536 16.7 vs 21.8 - the separate d <= 32 threshold of 1536 was the wrong way round on the re-measurement)
  return !(d->Sk > 64 && d->Sq >= 112 && wgs >= 768);
}

// ... and on causal rows whose count leaves the last 128-row workgroup at most half full, up to 384 keys
bool prefer_full_row_causal_tail(const oeh_attn_desc* d) {
  // causal rows whose count leaves the last 128-row workgroup at most half full (S = 192, 320, 448): the full-row kernel's 64-row
  // workgroups waste nothing there (16.9 vs 18.3, 15.7 vs 17.1, 18.7 vs 19.4 us); without the causal mask the one-pass kernel keeps its lead
  // (round 4, profiles/r04_dispatch_ab.txt - both sides of every rule in one process: S = 192 4.8 %, S = 320 3.1 % for the full-row kernel,
  // S = 448 a tie (18.3 vs 18.2 us): the rule ends at 384 keys, like its fp32 twin below)
  // fp32 storage: causal rows that leave the last 128-row workgroup at most half full, up to 320 rows (S = 192: 33.1 vs 40.3 us, S = 320: 38.4 vs
  // 39.0; S = 448: 42.9 vs 42.2 - the one-pass kernel again)
  if (d->full_mask != nullptr || (g_hooks.off & HOOK_FORCE_FLASH)) return false;
  return d->causal && d->Sk <= 384 && d->Sq > 128 && ((d->Sq - 1) % 128) < 64;
}

// The two-pass forms of the one-pass kernel on rows of MORE than 512 keys.  Up to 512 keys the full-row kernel computes the scores once
// and is the faster one - except the clipped softmax at head dim 128 from 384 keys.
bool prefer_two_pass(const oeh_attn_desc* d, const oeh_fq_desc* fq) {
  const bool forced = (g_hooks.off & HOOK_FORCE_FLASH) != 0;
  if (any_fq(fq)) return d->Sk > 512 || forced;
  return d->Sk > 512 || (d->D == 128 && d->Sk >= 384 && d->full_mask == nullptr) || (forced && d->full_mask == nullptr);  // (d = 128, S = 512: 47.4 vs 58.2 us in the full-row kernel, causal 38.1 vs 41.2)
}

// head dim 128: the full-row kernel fits ONE workgroup per CU (16-KB tiles), and with the clip or the INT8 chain on top the general
// kernel - smaller workgroups of its own - measures faster (round 3, B=16 H=8 S=512 causal: INT8 44.6 vs 39.8 us, clipped 41.2 vs 39.7;
// S=256 clipped 30.3 vs 25.0); the plain softmax stays on the one-pass / full-row kernels
bool prefer_general_d128(const oeh_attn_desc* d, const oeh_fq_desc* fq) {
  return !(g_hooks.off & HOOK_NO_D128_RULE) && d->D == 128 && d->dtype != OEH_F32 && (any_fq(fq) || d->clip) && d->key_pad_mask == nullptr && !gate_in_kernel(d);
}

// A wave per problem only pays when there are enough problems to fill the chip, on fp32 data - where it also is the EXACT path (fp32
// matrix-core products: 3e-6 of the reference; the operand-pair kernels round the probability operand to fp16) - and on rows of at
// most 32 keys: measured, round 3 (d = 64, against the full-row kernel's fp32 form): B*H = 896 S = 28 9.4 vs 8.9 us (kept here: STanHop's
// shape, the exact path), B*H = 1536 S = 32 13.3 vs 13.7, but S = 48 29.8 vs 20.2 and S = 64 37.0 vs 22.7; 16-bit data: S = 28 8.3 vs 8.05
// in the full-row kernel, S = 48 18.6 vs 6.6, S = 64 19.9 vs 7.1 - or when no matrix-core kernel takes the shape (d = 16)
bool prefer_small(const oeh_attn_desc* d) {
  return (g_hooks.off & HOOK_FORCE_SMALL) || d->D == 16 || !(d->dtype != OEH_F32 || d->Sk > 32 || d->Sq > 32 || (long)d->B * d->H < 256);
}

// query blocks (16 rows) per wave of the one-pass kernel: 2 (128-row workgroups) once that still gives every CU two
// workgroups, else 1
int flash_mq(const oeh_attn_desc* d, bool pv2) {
  // the probability pairs with key padding / a (B,1,Sq,Sk) mask at head dim 64: one block per wave (two spill - the fp32 forms with padding are
  // at the register file's edge already; oeh_attn_flash.inl instantiates only this one)
  if (pv2 && d->D == 64 && (d->key_pad_mask != nullptr || d->full_mask != nullptr)) return 1;
  if (g_hooks.flash_mq != 0 && !(d->D == 128 && d->dtype == OEH_F32)) return g_hooks.flash_mq;
  if (d->D == 128 && d->dtype == OEH_F32) return 1;  // two blocks of fp32 operand pairs at d = 128 do not fit the register file (130 spills)
  const long wg2 = (long)((d->Sq + 127) / 128) * d->B * d->H;
  return (d->Sq > 64 && wg2 >= 416) ? 2 : 1;  // (H=12 S=512 causal: B=8 - 384 workgroups - 10.8 vs 12.4 us with one block per wave, B=9 - 432 - 13.3 vs 12.8, B=10 14.5 vs 12.7, B=12 16.2 vs 13.5)
}

// The any-shape kernel (oeh_attn_generic.hip): the query row and the score row in LDS as fp32
bool generic_can(const oeh_attn_desc* d) { return (size_t)(d->D + d->Sk) * 4 <= 64 * 1024; }

Variant pick_variant(const oeh_attn_desc* d, const void* q, const void* k, const void* v, const void* o, const oeh_fq_desc* fq, bool out32) {
  if (d->dtype == OEH_I8) return i8_eligible(d, q, k, v, o, fq) ? V_I8 : V_NONE;
  const int eb = elem_bytes(d->dtype);
  const bool f32 = d->dtype == OEH_F32;
  const bool d_ok = d->D == 32 || d->D == 64 || d->D == 128;
  const bool shape_ok = d_ok && d->Sk <= 512;
  // integer-valued (idx - zp) must be exact in the 16-bit P operand: |.| <= 2048 (f16) / 256 (bf16)
  bool p_exact = true;
  if (fq != nullptr && fq->probs.enable) p_exact = fq->probs.qmax <= (d->dtype == OEH_BF16 ? 255.0f : 2047.0f);
  const bool al = (q == nullptr) || (aligned16(q, d->q_stride, eb) && aligned16(k, d->k_stride, eb) &&
                                     aligned16(v, d->v_stride, eb) && aligned16(o, d->o_stride, out32 ? 4 : eb));
  const int off = g_hooks.off;
  if (small_can(d, q, k, v, o, fq) && prefer_small(d) && !(off & (1 << V_SMALL))) return V_SMALL;
  if (d_ok && al && !(off & ((1 << V_FLASH) | (f32 ? HOOK_NO_FLASH_F32 : 0)))) {
    if (flash_can(d, fq, f32) && !prefer_full_row_short(d) && !prefer_full_row_causal_tail(d)) return V_FLASH;
    if (flash_two_pass_can(d, fq) && prefer_two_pass(d, fq)) return V_FLASH;
  }
  // fp32 storage on the full-row kernel: clipped softmax, the INT8 chain, vanilla softmax with key padding (the in-kernel gate predictor: on
  // operand pairs here - fast_can refuses it together with fake-quant)
  if (shape_ok && p_exact && al && fast_can(d, fq, f32) && !prefer_general_d128(d, fq) && !(off & ((1 << V_FAST) | (f32 ? HOOK_NO_FAST_F32 : 0)))) return V_FAST;
  if (shape_ok && p_exact && al && !(off & (1 << V_MFMA))) return V_MFMA;
  if (generic_can(d) && !(off & (1 << V_GENERIC))) return V_GENERIC;
  return V_NONE;
}

void fill_params(AttnParams& P, const oeh_attn_desc* d, const void* q, const void* k, const void* v, void* o, const oeh_fq_desc* fq) {
  std::memset(&P, 0, sizeof(P));
  oeh::fill_problem(P, d);
  P.q = q; P.k = k; P.v = v; P.o = o;
  P.D = d->D;
  P.scale = d->scale; P.scale_div = d->scale_div;  // (both: oeh_attn_fwd_ex folds the divisor for the one-pass and full-row kernels only)
  P.pad_bool = (d->key_pad_mask != nullptr && d->key_pad_boolean && d->mask_min < -1.0e4f) ? 1 : 0;
  P.gate = d->gate; P.gs_b = d->gate_stride[0]; P.gs_h = d->gate_stride[1]; P.gs_s = d->gate_stride[2];
  if (gate_in_kernel(d)) {
    P.gh = d->gate_hidden; P.ghs_b = d->gate_hidden_stride[0]; P.ghs_t = d->gate_hidden_stride[1];
    P.gw1 = d->gate_w1; P.gb1 = d->gate_b1; P.gw2 = d->gate_w2; P.gb2 = d->gate_b2;
    P.g_units = d->gate_units; P.g_scaling = d->gate_scaling; P.g_out = d->gate_out;
  }
  if (fq != nullptr) {
    P.fq_s = make_fq(&fq->scores); P.fq_p = make_fq(&fq->probs); P.fq_c = make_fq(&fq->ctx);
    P.ctx_before_gate = fq->ctx_quant_before_gate ? 1 : 0;
    if (fq->ctx_emit_index) P.fq_c.oscale = 1.0f;  // (validate(): the context quantiser is the last op)
  }
  P.stamps = g_hooks.stamps;
  P.snake = (g_hooks.off & HOOK_PLAIN_ORDER) ? 0 : 1;
  P.head_major = g_hooks.head_group;
  P.nQT = (d->Sq + 63) / 64;
  P.nBH = d->B * d->H;
  P.nBHpad = (P.nBH + 7) & ~7;
  P.magic_nbh = (unsigned)(0x100000000ULL / (unsigned long long)P.nBHpad > 0xffffffffULL ? 0xffffffffULL : 0x100000000ULL / (unsigned long long)P.nBHpad);
  P.magic_h = (unsigned)(0x100000000ULL / (unsigned long long)P.H > 0xffffffffULL ? 0xffffffffULL : 0x100000000ULL / (unsigned long long)P.H);
  P.skip_ok = oeh::causal_skip_ok(d, P.fq_s.dump != nullptr || P.fq_p.dump != nullptr) ? 1 : 0;
}

// The hot argument prefix of the one-pass kernel (oeh_attn_params.h: AttnHot; P as the V_FLASH case has completed it).  True = the launch may
// take the prefix form: the plain 16-bit kernel (no key padding / (B,1,Sq,Sk) mask, no in-kernel gate predictor, no clip / INT8 chain, no fp32
// storage or output), q, k and v with the same three strides, and every packed field inside its bits.  Everything else keeps the AttnParams-only
// launch.
bool fill_hot(oeh::AttnHot& hot, const AttnParams& P) {
  if (g_hooks.off & HOOK_NO_HOT_ARGS) return false;
  if (P.pad != nullptr || P.full != nullptr || P.gh != nullptr || P.clip || P.fq_s.en || P.src32 || P.out32) return false;
  if (P.qs_b != P.ks_b || P.qs_b != P.vs_b || P.qs_h != P.ks_h || P.qs_h != P.vs_h || P.qs_s != P.ks_s || P.qs_s != P.vs_s) return false;
  // (strides: in [0, 2^32), oeh_desc.h: strides_in_range)
  if (P.H > oeh::kHotMaxH || P.nQT > oeh::kHotMaxNQT || P.Sq > oeh::kHotMaxS || P.Sk > oeh::kHotMaxS || P.nBHpad != ((P.nBH + 7) & ~7)) return false;
  hot.q = P.q; hot.k = P.k; hot.v = P.v;
  hot.nBH = P.nBH; hot.magic_nbh = P.magic_nbh; hot.magic_h = P.magic_h;
  hot.geom = (unsigned)P.H | ((unsigned)P.nQT << 16) | (P.causal ? 1u << 30 : 0u) | (P.snake ? 1u << 31 : 0u);
  hot.sqsk = (unsigned)P.Sq | ((unsigned)P.Sk << 16);
  hot.s_b = (unsigned)P.qs_b; hot.s_h = (unsigned)P.qs_h; hot.s_s = (unsigned)P.qs_s;
  return true;
}

// Everything oeh_attn_fwd[_ex] decides before it launches, and what oeh_attn_variant[_ex] print
struct AttnPlan {
  int rc;       // OEH_OK, or the refusal (OEH_EINVAL / OEH_ENOTSUP / OEH_EALIGN)
  Variant var;
  int mq;       // one-pass kernel: query blocks per wave (AttnParams.nQT follows; the launch ladder's MQ)
  int src32;    // AttnParams.src32: fp32 storage read directly, fp32 output (1), with the probability pairs (2)
  int out32;    // AttnParams.out32: 16-bit storage with the output taken from the fp32 accumulators (include/oeh.h: o_dtype)
  int pv2;      // the probability pairs are on (include/oeh.h: oeh_attn_opts.pv_pairs)
  int nt;       // 16-key tiles of a full row, as the names print it
};

// The checks in the order the ABI promises (the first refusal wins).  name_only (oeh_attn_variant[_ex], host only: q .. o are null):
// the sizes / dtype / option words instead of validate(), and the plan ends with the variant - a name exists also where steps 5 - 6 refuse.
AttnPlan plan_attn(const oeh_attn_desc* d, const oeh_attn_opts* opts, const void* q, const void* k, const void* v, void* o,
                   const oeh_fq_desc* fq, bool name_only) {
  AttnPlan pl = {};
  // 1 - 3. reserved option words (before any other check), the descriptor, what the probability pairs do not cover
  if (opts != nullptr && (opts->reserved[0] != 0 || opts->reserved[1] != 0 || opts->reserved[2] != 0)) pl.rc = OEH_EINVAL;
  else pl.rc = name_only ? (desc_sane(d, true, true) ? OEH_OK : OEH_EINVAL) : validate(d, q, k, v, o, fq);
  if (pl.rc != OEH_OK) return pl;
  if (opts != nullptr && opts->pv_pairs != 0) {
    if (d->dtype != OEH_F32 || any_fq(fq) || gate_in_kernel(d)) { pl.rc = OEH_ENOTSUP; return pl; }
    pl.pv2 = 1;
  }
  // 4. the variant.  With the probability pairs, a problem the general kernel would take (its fp32 form rounds P to one fp16 operand) goes to
  // the any-shape kernel (fp32 FMA); the one-pass and full-row kernels run their PV2 forms, the small-shape kernel is fp32-exact as it is.
  pl.out32 = (d->dtype == OEH_F16 || d->dtype == OEH_BF16) && d->o_dtype == OEH_F32;
  pl.var = pick_variant(d, q, k, v, o, fq, pl.out32);
  if (pl.pv2 && pl.var == V_MFMA) pl.var = (generic_can(d) && !(g_hooks.off & (1 << V_GENERIC))) ? V_GENERIC : V_NONE;
  if (pl.var == V_NONE) { pl.rc = OEH_ENOTSUP; return pl; }
  const bool matrix16 = pl.var == V_FLASH || pl.var == V_FAST;
  pl.src32 = (d->dtype == OEH_F32 && matrix16) ? (pl.pv2 ? 2 : 1) : 0;
  pl.nt = d->Sk <= 128 ? 8 : (d->Sk <= 256 ? 16 : 32);
  pl.mq = pl.var == V_FLASH ? flash_mq(d, pl.pv2) : 0;  // 7. (before 5 - 6: the names print it, and the fp32-output rule reads it)
  if (name_only) return pl;
  // 5. fused gate predictor: 16-bit MFMA variants, 16-B aligned rows
  if (gate_in_kernel(d)) {
    // up to four 16-unit MFMA tiles of hidden units; fp32 storage: the full-row kernel's operand-pair form only
    if (!matrix16 || d->gate_units > 64 || (d->dtype == OEH_F32 && pl.var != V_FAST)) { pl.rc = OEH_ENOTSUP; return pl; }
    const int geb = d->dtype == OEH_F32 ? 4 : 2;
    if (!all16(addr(d->gate_hidden) | (uintptr_t)(d->gate_hidden_stride[0] * geb) | (uintptr_t)(d->gate_hidden_stride[1] * geb))) { pl.rc = OEH_EALIGN; return pl; }
    if (d->gate_hidden_stride[1] <= 0 || d->gate_hidden_stride[1] >= (1 << 24)) { pl.rc = OEH_ENOTSUP; return pl; }  // (32-bit lane offsets of the input rows' LDS-DMA)
  }
  // 6. fp32 output
  if (pl.out32) {
    // the accumulators themselves - sibling instantiations (O32) of what the 16-bit workloads of BASELINE.json run.  Head dim 64: the one-pass
    // kernel's plain form with masks none / causal / key padding / a (B,1,Sq,Sk) mask, or with the in-kernel gate predictor (not both);
    // the full-row kernel's plain and clipped forms (+ key padding), the plain form with the in-kernel gate predictor.  Head dim 128
    // (round 5): the plain forms of both (one block per wave in the one-pass kernel), gate values only.
    const bool masked = d->key_pad_mask != nullptr || d->full_mask != nullptr;
    bool ok = !any_fq(fq) && matrix16;
    if (d->D == 64) ok = ok && (pl.var == V_FLASH ? !d->clip && !(masked && gate_in_kernel(d)) : !(d->clip && gate_in_kernel(d)));
    else if (d->D == 128) ok = ok && !d->clip && !gate_in_kernel(d) && (pl.var == V_FAST || (!masked && pl.mq == 1));
    else ok = false;
    if (!ok) pl.rc = OEH_ENOTSUP;
  }
  return pl;
}

const char* variant_name(const AttnPlan& pl, const oeh_attn_desc* d, bool fq) {
  static thread_local char buf[64];
  const char* dt = oeh::dtype_name(d->dtype);  // (not used by V_I8, whose dtype is none of the three)
  const char* pv2 = pl.pv2 ? "+pv2" : "";
  switch (pl.var) {
    case V_NONE: return nullptr;
    case V_GENERIC: return "generic";
    case V_I8:
      std::snprintf(buf, sizeof(buf), "i8mfma/NT%d/D64/%s", pl.nt, d->o_dtype == OEH_F16 ? "f16" : (d->o_dtype == OEH_BF16 ? "bf16" : (d->o_dtype == OEH_I8 ? "i8" : "f32")));
      break;
    case V_SMALL: std::snprintf(buf, sizeof(buf), "small/ST%d/D%d/%s", d->Sk <= 32 ? 2 : 4, d->D, dt); break;
    case V_FLASH: std::snprintf(buf, sizeof(buf), "flash16/MQ%d/D%d/%s%s%s", pl.mq, d->D, dt, fq ? "/fq2p" : (d->clip ? "/clip2p" : ""), pv2); break;
    case V_FAST: std::snprintf(buf, sizeof(buf), "fast16/NT%d/D%d/%s%s%s%s", pl.nt, d->D, dt, d->clip ? "/clip" : "", fq ? "/fq" : "", pv2); break;
    case V_MFMA: std::snprintf(buf, sizeof(buf), "mfma16/NT%d/D%d/%s%s", pl.nt, d->D, dt, fq ? "/fq" : ""); break;
  }
  return buf;
}

// the head-dim units of a kernel family (D is 32, 64 or 128 here: pick_variant's d_ok)
#define OEH_LAUNCH_BY_D(family, ...) \
  (desc->D == 32 ? oeh::launch_attn_##family##_d32(__VA_ARGS__) : desc->D == 64 ? oeh::launch_attn_##family##_d64(__VA_ARGS__) : oeh::launch_attn_##family##_d128(__VA_ARGS__))

}  // namespace

extern "C" {

int oeh_attn_fwd_ex(const oeh_attn_desc* desc, const oeh_attn_opts* opts, const void* q, const void* k, const void* v, void* o,
                    const oeh_fq_desc* fq, void* stream) {
  const AttnPlan pl = plan_attn(desc, opts, q, k, v, o, fq, false);
  if (pl.rc != OEH_OK) return pl.rc;
  AttnParams P;
  fill_params(P, desc, q, k, v, o, fq);
  P.src32 = pl.src32;
  P.out32 = pl.out32;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if ((pl.var == V_FLASH || pl.var == V_FAST) && desc->scale_div != 0.0f) { P.scale = 1.0f / desc->scale_div; P.scale_div = 0.0f; }  // (fast_can: exact for a power of two)
  switch (pl.var) {
    case V_SMALL: return oeh::launch_attn_small(P, desc->dtype, st);
    case V_I8: {
      const double mult = desc->scale_div != 0.0f ? 1.0 / (double)desc->scale_div : (double)desc->scale;
      P.i8_cq = 128 - (int)desc->q_grid.zero_point; P.i8_ck = 128 - (int)desc->k_grid.zero_point;
      P.i8_cv = 128 - (int)desc->v_grid.zero_point; P.i8_cp = 128 - (int)fq->probs.zero_point;
      P.i8_k1 = (float)((double)desc->q_grid.scale * (double)desc->k_grid.scale * mult / (double)fq->scores.scale);
      P.i8_so = (float)((double)fq->probs.scale * (double)desc->v_grid.scale);
      P.nBHpad = (P.nBH + 15) & ~15;  // head pairs on one XCD (oeh_attn_i8.hip)
      P.magic_nbh = (unsigned)(0x100000000ULL / (unsigned long long)P.nBHpad);
      return oeh::launch_attn_i8(P, desc->o_dtype, st);
    }
    case V_FLASH: {
      P.nQT = (desc->Sq + 64 * pl.mq - 1) / (64 * pl.mq);
      oeh::AttnHot hot;
      const bool with_hot = fill_hot(hot, P);
      if (with_hot) ++g_hooks.hot_launches;  // (process-global like the hooks that read it: include/oeh_debug.h)
      return OEH_LAUNCH_BY_D(flash, P, with_hot ? &hot : nullptr, desc->dtype, pl.mq, st);
    }
    case V_FAST: return OEH_LAUNCH_BY_D(fast, P, desc->dtype, st);
    case V_MFMA: return OEH_LAUNCH_BY_D(mfma, P, desc->dtype, any_fq(fq), st);
    default: return oeh::launch_attn_generic(P, desc->dtype, st);
  }
}

int oeh_attn_fwd(const oeh_attn_desc* desc, const void* q, const void* k, const void* v, void* o, const oeh_fq_desc* fq,
                 void* stream) {
  return oeh_attn_fwd_ex(desc, nullptr, q, k, v, o, fq, stream);
}

const char* oeh_attn_variant_ex(const oeh_attn_desc* desc, const oeh_attn_opts* opts, const oeh_fq_desc* fq) {
  const AttnPlan pl = plan_attn(desc, opts, nullptr, nullptr, nullptr, nullptr, fq, true);
  return pl.rc == OEH_OK ? variant_name(pl, desc, any_fq(fq)) : nullptr;
}

const char* oeh_attn_variant(const oeh_attn_desc* desc, const oeh_fq_desc* fq) { return oeh_attn_variant_ex(desc, nullptr, fq); }

int oeh_attn_calibrate(const oeh_attn_desc* desc, const void* q, const void* k, const void* v, float* ctx_out, int32_t which,
                       const double* scores_range, const double* probs_range, int32_t n_bits, double eps, double q_lo, double q_hi,
                       double momentum, int32_t first, double* state, void* work, void* stream) {
  if (q == nullptr || k == nullptr || !desc_sane(desc, false, false)) return OEH_EINVAL;
  if (which < OEH_CALIB_SCORES || which > OEH_CALIB_CONTEXT || n_bits < 1 || n_bits > 16 || !(eps > 0.0)) return OEH_EINVAL;
  if (which == OEH_CALIB_CONTEXT ? (v == nullptr || ctx_out == nullptr) : (state == nullptr || work == nullptr)) return OEH_EINVAL;
  if (!softmax_base_ok(desc->softmax_base) || !oeh::key_pad_ok(desc) || !oeh::full_mask_ok(desc)) return OEH_EINVAL;
  if (!(desc->D == 32 || desc->D == 64 || desc->D == 128)) return OEH_ENOTSUP;
  if (which != OEH_CALIB_CONTEXT) {
    if (!(q_lo >= 0.0 && q_lo <= 100.0 && q_hi >= 0.0 && q_hi <= 100.0) || !(momentum >= 0.0 && momentum <= 1.0)) return OEH_EINVAL;
    if ((int64_t)desc->B * desc->H * desc->Sq * desc->Sk >= ((int64_t)1 << 32)) return OEH_ENOTSUP;
    if ((reinterpret_cast<uintptr_t>(work) & 7) != 0 || (reinterpret_cast<uintptr_t>(state) & 7) != 0) return OEH_EALIGN;
  }
  const int eb = elem_bytes(desc->dtype);
  if (!aligned16(q, desc->q_stride, eb) || !aligned16(k, desc->k_stride, eb)) return OEH_EALIGN;
  if (which == OEH_CALIB_CONTEXT && (!aligned16(v, desc->v_stride, eb) || !aligned16(ctx_out, desc->o_stride, 4))) return OEH_EALIGN;
  AttnParams P;
  fill_params(P, desc, q, k, v, ctx_out, nullptr);
  return oeh::launch_attn_calibrate(P, desc->dtype, which, scores_range, probs_range, (float)((1 << n_bits) - 1), eps, q_lo, q_hi, momentum, first ? 1 : 0,
                                    state, work, reinterpret_cast<hipStream_t>(stream));
}

// Diagnostic hooks: include/oeh_debug.h (NOT part of the product ABI; inert unless OEH_DEBUG_HOOKS=1 in the environment)
static bool debug_hooks_on() {
  static const bool on = [] { const char* e = std::getenv("OEH_DEBUG_HOOKS"); return e != nullptr && e[0] == '1'; }();
  return on;
}
int oeh_debug_set_variant(int off_mask, int flash_mq_force) {
  if (!debug_hooks_on()) return OEH_ENOTSUP;
  g_hooks.off = off_mask & HOOK_ALL;
  g_hooks.flash_mq = flash_mq_force;
  { const char* e = std::getenv("OEH_HEAD_GROUP"); g_hooks.head_group = e != nullptr ? (std::atoi(e) & ~7) : 0; }
  return OEH_OK;
}
int oeh_debug_set_stamps(void* device_buffer) {
  if (!debug_hooks_on()) return OEH_ENOTSUP;
  g_hooks.stamps = static_cast<unsigned long long*>(device_buffer);
  return OEH_OK;
}

long oeh_debug_hot_launches(void) { return debug_hooks_on() ? g_hooks.hot_launches : (long)OEH_ENOTSUP; }

int oeh_abi_version(void) { return OEH_ABI_VERSION; }

const char* oeh_build_info(void) {
  return "liboeh_hip gfx950 (MI355X, CDNA4) v_mfma_f32_16x16x32_{f16,bf16} + v_mfma_f32_16x16x4_f32 + v_mfma_i32_16x16x64_i8; built " __DATE__ " " __TIME__ " hipcc " __VERSION__;
}

const char* oeh_strerror(int code) {
  switch (code) {
    case OEH_OK: return "ok";
    case OEH_EINVAL: return "invalid argument";
    case OEH_ENOTSUP: return "shape/dtype/option combination not supported";
    case OEH_EALIGN: return "pointer or stride not 16-byte aligned";
    case OEH_ELAUNCH: return "HIP kernel launch failed";
    case OEH_ENODEV: return "no gfx950 device";
    default: return "unknown error";
  }
}

}  // extern "C"
