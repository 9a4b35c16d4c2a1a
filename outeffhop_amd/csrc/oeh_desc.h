// The attention descriptor (include/oeh.h: oeh_attn_desc, oeh_fq_desc) on the host: one text for every rule that the attention entry points
// share - what a sane descriptor is, which strides and rows the kernels can address, what a quantiser grid is, when causal tiles may be
// skipped, and how the descriptor becomes the problem part of a kernel-argument block - and the small storage-type predicates every entry
// point of the library uses (dtype_ok, elem_bytes, vec16_elems, dtype_name, addr, all16).  Only the predicates live here: each entry point
// keeps the ORDER of its refusals and its codes where they can be read (oeh_api.hip: validate / plan_attn, oeh_attn_decode.hip: plan_decode,
// oeh_attn_bwd.hip: check_desc / fwd_train / bwd_run, and the *_check function next to every other entry point).  Host only, no device code.
#pragma once
#include "../../include/oeh.h"
#include "oeh_attn_params.h"

#include <cmath>

namespace oeh {

inline bool dtype_ok(int d) { return d == OEH_F16 || d == OEH_BF16 || d == OEH_F32; }
// of a storage type: bytes per element, elements per 16-byte vector, and its name in the *_variant strings
inline int elem_bytes(int d) { return d == OEH_F32 ? 4 : d == OEH_I8 ? 1 : 2; }
inline int vec16_elems(int d) { return d == OEH_F32 ? 4 : 8; }
inline const char* dtype_name(int d) { return d == OEH_F32 ? "f32" : d == OEH_BF16 ? "bf16" : "f16"; }
inline bool softmax_base_ok(int base) { return base == OEH_SOFTMAX_VANILLA || base == OEH_SOFTMAX_ONE; }

// The descriptor sanity every entry point starts with: positive sizes (the head dim where the caller does not judge it itself) and a
// storage type (INT8 where the caller takes it - or refuses it later with its own code)
inline bool desc_sizes_ok(const oeh_attn_desc* d, bool with_D) {
  return d != nullptr && d->B > 0 && d->H > 0 && d->Sq > 0 && d->Sk > 0 && (!with_D || d->D > 0);
}
inline bool desc_sane(const oeh_attn_desc* d, bool with_D, bool with_i8) {
  return desc_sizes_ok(d, with_D) && (dtype_ok(d->dtype) || (with_i8 && d->dtype == OEH_I8));
}

// additive masks are fp16 or fp32 (judged only where the mask is given)
inline bool mask_dtype_ok(const void* mask, int dtype) { return mask == nullptr || dtype == OEH_F16 || dtype == OEH_F32; }
inline bool key_pad_ok(const oeh_attn_desc* d) { return mask_dtype_ok(d->key_pad_mask, d->key_pad_dtype); }
inline bool full_mask_ok(const oeh_attn_desc* d) { return mask_dtype_ok(d->full_mask, d->full_mask_dtype); }

// Strides are element counts in [0, 2^32): every kernel forms its batch / head offsets from two 32 x 32 -> 64-bit products of the low
// words (oeh_common.h: bh_offset).  Views with negative strides are not a layout any caller of the reference produces.
inline bool strides_in_range(const int64_t st[3]) {
  for (int i = 0; i < 3; ++i)
    if (st[i] < 0 || st[i] >= ((int64_t)1 << 32)) return false;
  return true;
}
inline bool desc_strides_in_range(const oeh_attn_desc* d) {
  return strides_in_range(d->q_stride) && strides_in_range(d->k_stride) && strides_in_range(d->v_stride) && strides_in_range(d->o_stride);
}

// 16-byte alignment of an OR of addresses and byte counts; of a tensor's rows: the pointer and its three strides (elements of eb bytes),
// for the matrix-core paths' 16-B loads / 8..16-B stores
inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }
inline bool all16(uintptr_t ored) { return (ored & 15) == 0; }
inline bool aligned16(const void* p, const int64_t* st, int eb) {
  return all16(addr(p) | (uintptr_t)(st[0] * eb) | (uintptr_t)(st[1] * eb) | (uintptr_t)(st[2] * eb));
}

inline bool any_fq(const oeh_fq_desc* fq) { return fq != nullptr && (fq->scores.enable || fq->probs.enable || fq->ctx.enable); }

// Is (scale, zero_point, qmax) a quantiser grid: a positive step, at least two levels, the zero point on the grid.  finite: also a finite
// step and top level and no NaN zero point - oeh_attn_decode_fq[_variant] ask for that (check_fq); oeh_attn_fwd[_ex] (validate) and
// oeh_fake_quant keep the looser form they shipped with, which lets an infinite step or top level and a NaN zero point through.
inline bool fq_grid_ok(float scale, float zero_point, float qmax, bool finite) {
  if (!(scale > 0.0f) || !(qmax >= 1.0f)) return false;
  if (finite) return std::isfinite(scale) && std::isfinite(qmax) && zero_point >= 0.0f && zero_point <= qmax;
  return !(zero_point < 0.0f || zero_point > qmax);
}
inline bool fq_grid_ok(const oeh_fq& f, bool finite) { return fq_grid_ok(f.scale, f.zero_point, f.qmax, finite); }
// the test-only index dumps are bytes
inline bool fq_dump_fits(const oeh_fq& f) { return f.dump_idx == nullptr || !(f.qmax > 255.0f); }

// Causal tiles strictly above the diagonal contribute exactly 0 to P@V, to the row statistics and to every gradient, and may be skipped
// when: masked probabilities are exactly 0 before the clip and the clip maps 0 to 0 with zero gradient (gamma <= 0); the row can never be
// fully masked under the vanilla softmax (which would make it uniform over ALL keys) - guaranteed by the diagonal unless another mask is
// present; and no index dump wants every element (index_dumps: the inference forward's scores / probability dumps; the training kernels
// have none).  The backward recomputes the forward's probabilities: both MUST decide this by the same rule.
inline bool causal_skip_ok(const oeh_attn_desc* d, bool index_dumps) {
  const bool other_mask = d->key_pad_mask != nullptr || d->full_mask != nullptr;
  return d->causal && d->Sq <= d->Sk && (!d->clip || d->gamma <= 0.0f) && !index_dumps && (d->softmax_base == OEH_SOFTMAX_ONE || !other_mask) &&
         std::isfinite(d->mask_min) && d->mask_min < -1e4f;
}

// The problem part of a kernel-argument block (AttnParams, bwd::Params: the fields both spell alike) from the descriptor.  No pointers of
// the call, no head dim, no launch geometry, and no scale: the inference, decode and training paths each fold a divisor their own way.
// (The (B,1,Sq,Sk) mask's type and strides only with the mask: a block without one keeps them zero.)
template <class P>
inline void fill_problem(P& p, const oeh_attn_desc* d) {
  p.B = d->B; p.H = d->H; p.Sq = d->Sq; p.Sk = d->Sk;
  p.qs_b = d->q_stride[0]; p.qs_h = d->q_stride[1]; p.qs_s = d->q_stride[2];
  p.ks_b = d->k_stride[0]; p.ks_h = d->k_stride[1]; p.ks_s = d->k_stride[2];
  p.vs_b = d->v_stride[0]; p.vs_h = d->v_stride[1]; p.vs_s = d->v_stride[2];
  p.os_b = d->o_stride[0]; p.os_h = d->o_stride[1]; p.os_s = d->o_stride[2];
  p.base = d->softmax_base;
  p.clip = d->clip ? 1 : 0;
  // (eta - gamma) is formed in double and rounded to fp32 once, as the Python scalar the reference multiplies by
  p.clip_w = (float)((double)d->eta - (double)d->gamma);
  p.clip_g = d->gamma;
  p.pad = d->key_pad_mask; p.pad_f16 = d->key_pad_dtype == OEH_F16; p.pad_sb = d->key_pad_stride;
  if (d->full_mask != nullptr) {
    p.full = d->full_mask; p.full_f16 = d->full_mask_dtype == OEH_F16;
    p.full_sb = d->full_mask_stride[0]; p.full_sq = d->full_mask_stride[1];
  }
  p.causal = d->causal ? 1 : 0; p.clamp_min = d->clamp_min ? 1 : 0; p.mask_min = d->mask_min;
}

}  // namespace oeh
