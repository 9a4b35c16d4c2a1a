// One-pass ("online") fused attention for the PLAIN softmax / softmax_1 case, 16-bit storage - the headline
// configuration (OPT-125m softmax1, gated variants, long BERT/ViT rows).
//
// Why a second structure: the full-row kernel (oeh_attn_fast.inl) must keep a query block's complete score row in
// registers because clipping and fake-quant are non-linear in the final probability; that caps a workgroup at 64
// query rows, so a head's K/V is re-streamed through LDS once per 64 rows (4.5x for causal S=512) and the in-kernel
// timeline (tools/timeline.py) shows its K and V phases paced by that LDS-DMA traffic.  Plain softmax_n has no such
// constraint (hard part 1): with a per-row reference score, exp(x - reference) is accumulated tile by tile
// and the sums rescaled when the reference moves.  softmax_1's "+1" is exp(0 - reference) added to the row sum once
// at the end - the reference formula, including rows that are exactly 0 when every key is masked.  Hence:
//   * one workgroup = 4 waves x MQ query blocks of 16 rows (MQ=2: 128 rows) -> K/V stream 2.3x smaller, and K and V
//     tiles arrive TOGETHER: one barrier per 64 keys instead of two;
//   * registers: Q, O and one 64-key score tile per block only (no Sk limit);
//   * every K fragment read from LDS feeds MQ MFMAs and every V^T fragment feeds MQ MFMAs (LDS bandwidth / MQ);
//   * row max all-reduce by v_permlane16_swap / v_permlane32_swap (VALU), not ds_bpermute (LDS round trip);
//   * row sums by one extra MFMA per 32 keys against a ones operand (sums exactly the rounded P the second product
//     uses, and frees 16 v_add per block and tile - the loop is VALU-issue bound, not MFMA bound);
//   * lazy reference: it moves only when a row's tile maximum exceeds it by 2^8, so the O/l rescale (20 multiplies per
//     block) almost never runs after the first tiles;
//   * Q arrives by LDS-DMA ahead of the first stages and tile 0 starts on Q + K tile 0 alone; O leaves as whole rows,
//     write-through (oeh_common.h: store_wt16 - a plain store parks the output in L2 until the end-of-kernel release);
//   * key padding (PAD variant): the padding row sits in LDS and trailing fully padded key tiles are not streamed.
// Same swapped products (S^T = K Q^T, O^T = V^T P^T on v_mfma_f32_16x16x32), LDS images, swizzles and LDS-DMA ring
// as the full-row kernel.  Masks: none | analytic causal | key padding (softmax_1 only: a fully masked row must be 0).
#pragma once
#include "oeh_attn_fast.inl"

#include <type_traits>

namespace oeh {

// all-reduce over the 4 lanes (c, c+16, c+32, c+48) that hold one query row, without LDS
__device__ __forceinline__ float row_allreduce_max(float x) {
  auto a = __builtin_amdgcn_permlane16_swap(f32_bits(x), f32_bits(x), false, false);
  x = __builtin_fmaxf(bits_f32(a[0]), bits_f32(a[1]));
  auto b = __builtin_amdgcn_permlane32_swap(f32_bits(x), f32_bits(x), false, false);
  return __builtin_fmaxf(bits_f32(b[0]), bits_f32(b[1]));
}

template <int D, int MQ, bool SRC32>
constexpr int flash_occupancy() { return D >= 128 ? 1 : (SRC32 ? 2 : 3); }  // fp32 forms: operand pairs + the staged stage, 2 waves per SIMD

// GATE: the conditional per-token gate is computed in the kernel exactly as in the full-row kernel (oeh_attn_fast.inl:
// layer-input rows as K-shaped LDS-DMA tiles, first predictor layer on the matrix cores).  The input rows borrow stage 1
// at start-up, so stage 1 of the K/V stream is issued later (with stage 2, once the gate has been formed).
// SRC32: q, k, v and o are fp32 (the reference's validate_* scripts run fp32 models).  The tiles then come through
// registers - 32 B of fp32 per lane and piece, split into the fp16 operand pair (hi, lo) of oeh_common.h: split8 and written
// as two LDS images in the layout the DMA produces - one 64-key stage ahead: the loads of stage i+1 are issued right after
// the barrier of tile i and committed to LDS at the top of tile i+1, so they have a tile of compute to land; one barrier
// per tile as before, two ring slots (a slot's readers are all behind the barrier that precedes its next commit).  Scores
// from three MFMAs per k-step (q.k = qh.kh + 2^-11 (qh.kl + ql.kh)), the context from two (P is an fp16 operand, V the pair):
// fp32 accuracy on the scores, fp32 accumulation and fp32 output straight from the accumulators (OUT32); Q goes global ->
// registers directly.  No conversion pre-pass (which costs more HBM time than the attention itself).
// CLIP: clipped softmax (softmax.py:10-19: clip(p (eta - gamma) + gamma, 0, 1)) needs the finished denominator before any
// probability can enter the second product, so the key stream runs TWICE: a statistics pass (scores, lazy reference, row
// sums of the exponentials - no V product) and a final pass that recomputes the scores against the now final reference,
// forms p = e / den, clips and multiplies by V.  Rows of any length (the full-row kernel holds at most 512 scores per row in
// registers and is the faster form up to there: it computes the scores once); masked keys have e = 0 and stay 0 (gamma <= 0).
// TP = 2: the fused INT8 chain on the quantiser grid (oeh_attn_fast.inl, FQ == 1: rel = clamp(rint(s k1)), exp2((rel - rel_max) c2),
// index of the probability from e * RN(1 / (den scale_p))) in the same two passes: the statistics pass keeps a running maximum
// and sum per LANE (no cross-lane step inside the loop), the final pass recomputes rel against the row's maximum and feeds the
// integer-valued probability to the second product; context quantiser and gate in the epilogue.  Rows of any length.
// O32: 16-bit storage with the output taken from the fp32 accumulators (include/oeh.h: o_dtype = OEH_F32) - the same loop, only the
// epilogue's store differs (as a runtime switch in the epilogue it cost the production launches +0.7 ... +3 %, round 4).
// PV2 (fp32 storage, plain and clipped forms; include/oeh.h: oeh_attn_opts.pv_pairs): the context to fp32 accuracy as well.  Each fp32
// probability tile is split in registers like the operands, p = P_hi + P_lo 2^-11 (oeh_common.h: split8), and the second product becomes
// o += V_hi P_hi, ox += V_lo P_hi + V_hi P_lo (ox is scaled by 2^-11 in the epilogue; V_lo P_lo, 2^-22 relative, is dropped): one more MFMA
// per V fragment.  The one-pass form's row sums stay the sums of exactly what the numerator multiplies: a second ones-MFMA, on P_lo with
// a ones operand of 2^-11, adds the lo part into the same accumulator.  The clipped form's denominator is the fp32 sum of the
// exponentials (statistics pass) and does not change.
//
// The kernel body (oeh_attn_flash_body.inl) has two entries.  What the block-id decode and the Q / K / V requests read is OEH_HOT(field), the rest P:
//   * oeh_attn_flash_kernel(AttnParams): OEH_HOT is P's own fields, requested with one round of scalar loads at entry - every form;
//   * oeh_attn_flash_hot_kernel(14 leading scalar dwords, AttnParams) (PFX): it is the hot argument prefix (oeh_attn_params.h: AttnHot), which
//     gfx950 hands over in user SGPRs at wave launch (kernarg preload; csrc/Makefile: PRELOAD_FLAGS), so the first requests are issued
//     without a memory round trip; P's round of loads is awaited behind them.  The plain 16-bit forms (no PAD, no GATE) only.
struct FlashHot {
  const void *q, *k, *v;
  int nBHpad, nBH;
  unsigned magic_nbh, magic_h;
  int H, nQT, causal, snake, Sq, Sk;
  long qs_b, qs_h, qs_s, ks_b, ks_h, ks_s, vs_b, vs_h, vs_s;
};

// Diagnostic build (tools/timeline.py): s_memrealtime and s_memtime as the kernel's first two instructions, before any argument is used, kept in
// SGPRs and stored with the other stamps behind the first requests.  The compiler places the loads of by-value kernel arguments at the top of
// the kernel whatever the source order, so the AttnParams-only entry reads its block through the kernarg segment pointer made opaque BY the
// stamp statement (kp: in and out) - no argument load can be issued in front of it.  (The wait is part of the statement: the compiler does not
// track the return of scalar-memory results of inline asm.)
#ifdef OEH_TIMELINE
#define OEH_ENTRY_STAMPS(kp)                 \
  unsigned long long t_real0, t_entry;       \
  asm volatile("s_memrealtime %1\n\ts_memtime %2\n\ts_waitcnt lgkmcnt(0)" : "+s"(kp), "=s"(t_real0), "=s"(t_entry) : : "memory")
#endif

template <int D, int IN, int MQ, bool PAD, bool GATE, bool SRC32 = false, int TP = 0, bool O32 = false, bool PV2 = false>
#ifdef OEH_TIMELINE
__global__ __launch_bounds__(256, (flash_occupancy<D, MQ, SRC32>())) void oeh_attn_flash_kernel(const AttnParams) {
  auto kp = __builtin_amdgcn_kernarg_segment_ptr();
  OEH_ENTRY_STAMPS(kp);
  const AttnParams& P = *(const AttnParams*)kp;
#else
__global__ __launch_bounds__(256, (flash_occupancy<D, MQ, SRC32>())) void oeh_attn_flash_kernel(const AttnParams P) {
#endif
  constexpr bool PFX = false;
#define OEH_HOT(f) P.f
#include "oeh_attn_flash_body.inl"
#undef OEH_HOT
}

// The hot-prefix entry of the plain 16-bit forms.  The parameter list is AttnHot, field by field (a struct would not be preloaded).
template <int D, int IN, int MQ>
__global__ __launch_bounds__(256, (flash_occupancy<D, MQ, false>())) void oeh_attn_flash_hot_kernel(OEH_HOT_PARAMS, const AttnParams P) {
#ifdef OEH_TIMELINE
  OEH_ENTRY_STAMPS(hq);
#endif
  const int nbhpad = (h_nbh + 7) & ~7;
  const long sb = (long)h_sb, sh = (long)h_sh, ss = (long)h_ss;
  const FlashHot Hh = {hq, hk, hv, nbhpad, h_nbh, h_mnbh, h_mh, (int)(h_geom & 0xffffu), (int)((h_geom >> 16) & 0xfffu), (int)((h_geom >> 30) & 1u), (int)(h_geom >> 31),
                       (int)(h_sqsk & 0xffffu), (int)(h_sqsk >> 16), sb, sh, ss, sb, sh, ss, sb, sh, ss};
  constexpr bool PFX = true, PAD = false, GATE = false, SRC32 = false, O32 = false, PV2 = false;
  constexpr int TP = 0;
#define OEH_HOT(f) Hh.f
#include "oeh_attn_flash_body.inl"
#undef OEH_HOT
}

// One launch of the ladder below: true = launched.  A combination without a branch returns false (OEH_ENOTSUP in the wrapper): the plan
// (oeh_api.hip: plan_attn) never selects one, and a future change that does shall not pass for a launch.
#define OEH_GO(...) (oeh_attn_flash_kernel<D, IN, MQ, __VA_ARGS__><<<dim3(grid), dim3(256), 0, st>>>(P), true)
#define OEH_GO_HOT() (oeh_attn_flash_hot_kernel<D, IN, MQ><<<dim3(grid), dim3(256), 0, st>>>(OEH_HOT_ARGS(*hot), P), true)
template <int D, int MQ, int IN>
static bool launch_flash_d_mq_in(const AttnParams& P, const AttnHot* hot, unsigned grid, hipStream_t st) {
  const bool pad = P.pad != nullptr || P.full != nullptr, gate = P.gh != nullptr;  // (the PAD variants also serve a (B,1,Sq,Sk) mask)
  if (P.src32) {  // fp32 storage read directly, fp32 output; no in-kernel gate predictor on this path (AttnPlan.src32: only with f32 storage, IN_F16)
    if constexpr (IN == IN_F16 && !(D == 128 && MQ == 2)) {  // (d = 128 with two blocks per wave: AttnPlan.mq is 1 there, flash_mq)
      if (P.src32 == 2) {  // PV2: the probability pairs (AttnPlan.pv2 excludes the fake-quant chain)
        if constexpr (!(D == 64 && MQ == 2)) {  // (d = 64 with padding: AttnPlan.mq is 1, flash_mq)
          if (pad) return P.clip ? OEH_GO(true, false, true, 1, false, true) : OEH_GO(true, false, true, 0, false, true);
        }
        if (!pad) return P.clip ? OEH_GO(false, false, true, 1, false, true) : OEH_GO(false, false, true, 0, false, true);
        return false;
      }
      if (P.fq_s.en) return pad ? OEH_GO(true, false, true, 2) : OEH_GO(false, false, true, 2);
      if (P.clip) return pad ? OEH_GO(true, false, true, 1) : OEH_GO(false, false, true, 1);
      return pad ? OEH_GO(true, false, true) : OEH_GO(false, false, true);
    }
    return false;
  }
  // (flash_two_pass_can - the grid chain: no clip, no in-kernel predictor; key padding as a 0 / <= -1e4 vector)
  if (P.fq_s.en) return pad ? OEH_GO(true, false, false, 2) : OEH_GO(false, false, false, 2);
  if (P.clip) return pad ? OEH_GO(true, false, false, 1) : OEH_GO(false, false, false, 1);  // (flash_two_pass_can - no in-kernel predictor)
  if (P.out32) {  // (AttnPlan.out32, plan_attn step 6)
    if constexpr (D == 64) {  // head dim 64: plain, + key padding / a (B,1,Sq,Sk) mask, + the in-kernel gate predictor
      if (pad) return OEH_GO(true, false, false, 0, true);
      return gate ? OEH_GO(false, true, false, 0, true) : OEH_GO(false, false, false, 0, true);
    }
    if constexpr (D == 128 && MQ == 1) return OEH_GO(false, false, false, 0, true);  // head dim 128: the plain form, AttnPlan.mq == 1
    return false;
  }
  if (pad) return gate ? OEH_GO(true, true) : OEH_GO(true, false);
  if (gate) return OEH_GO(false, true);
  // the plain form: with the hot argument prefix where the host could fill one (oeh_api.hip: fill_hot), else from the AttnParams block alone
  return hot != nullptr ? OEH_GO_HOT() : OEH_GO(false, false);
}
#undef OEH_GO_HOT
#undef OEH_GO

template <int D, int MQ>
static int launch_flash_d_mq(const AttnParams& P, const AttnHot* hot, int in, hipStream_t st) {
  const unsigned grid = (unsigned)(P.nQT * P.nBHpad);
  const bool launched = in == IN_BF16 ? launch_flash_d_mq_in<D, MQ, IN_BF16>(P, hot, grid, st) : launch_flash_d_mq_in<D, MQ, IN_F16>(P, hot, grid, st);
  if (!launched) return -95;  // OEH_ENOTSUP
  return launch_status();
}

// P.nQT = ceil(Sq / (64*MQ)) workgroups per head; MQ is AttnPlan.mq (oeh_api.hip: flash_mq)
template <int D>
static int launch_flash_d(const AttnParams& P, const AttnHot* hot, int in, int mq, hipStream_t st) {
  if (mq == 1) return launch_flash_d_mq<D, 1>(P, hot, in, st);
  return launch_flash_d_mq<D, 2>(P, hot, in, st);
}

}  // namespace oeh
