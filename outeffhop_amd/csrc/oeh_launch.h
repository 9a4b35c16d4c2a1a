// The host side that every unit with a launcher shares: the status of a launch chain, the storage-type dispatchers, and the prototypes of the
// attention launchers that oeh_api.hip calls ACROSS units - declared HERE and nowhere else, and included by the unit that defines each of
// them as well as by oeh_api.hip: one text for both sides (a definition whose return type drifts no longer compiles; one whose parameters
// drift is an unresolved symbol of the library).  Nothing else: an op outside the attention forward family keeps its extern "C" entry
// point, its argument block and its launcher in the unit that owns its kernels, file-local.  No device code.
#pragma once
#include "../../include/oeh.h"
#include "oeh_attn_params.h"

#include <type_traits>

namespace oeh {

// OEH_OK, or OEH_ELAUNCH if any launch of the chain since the last look failed
inline int launch_status() { return hipGetLastError() == hipSuccess ? OEH_OK : OEH_ELAUNCH; }

// f(std::integral_constant<int, IN>{}) for the storage type `in` (anything that is not IN_F16 / IN_BF16 is fp32, as in every launcher
// before this header): dispatch_in(in, [&](auto t) { constexpr int IN = decltype(t)::value; hipLaunchKernelGGL(k<IN>, ...); });
template <class F>
inline auto dispatch_in(const int in, F&& f) {
  switch (in) {
    case IN_F16: return f(std::integral_constant<int, IN_F16>{});
    case IN_BF16: return f(std::integral_constant<int, IN_BF16>{});
    default: return f(std::integral_constant<int, IN_F32>{});
  }
}

// The callers pass a descriptor's OEH_* storage type as `in`: the ABI's values and the kernels' template arguments are the same numbers
static_assert(IN_F16 == OEH_F16 && IN_BF16 == OEH_BF16 && IN_F32 == OEH_F32, "dispatch_in[16] take an oeh_attn_desc.dtype");

// The 16-bit sibling, for kernels without an fp32-storage form (training, decode: dispatch_in would instantiate one): IN_BF16 or (anything
// else) IN_F16.  With `flag`: a second compile-time switch, f(std::integral_constant<int, IN>{}, std::bool_constant<FLAG>{})
template <class F>
inline auto dispatch_in16(const int in, F&& f) {
  return in == IN_BF16 ? f(std::integral_constant<int, IN_BF16>{}) : f(std::integral_constant<int, IN_F16>{});
}
template <class F>
inline auto dispatch_in16(const int in, const bool flag, F&& f) {
  return dispatch_in16(in, [&](auto t) { return flag ? f(t, std::true_type{}) : f(t, std::false_type{}); });
}

// oeh_attn_mfma_d*.hip, oeh_attn_fast_d*.hip, oeh_attn_flash_d*.hip
int launch_attn_mfma_d32(const AttnParams& P, int in, bool fq, hipStream_t st);
int launch_attn_mfma_d64(const AttnParams& P, int in, bool fq, hipStream_t st);
int launch_attn_mfma_d128(const AttnParams& P, int in, bool fq, hipStream_t st);
int launch_attn_fast_d32(const AttnParams& P, int in, hipStream_t st);
int launch_attn_fast_d64(const AttnParams& P, int in, hipStream_t st);
int launch_attn_fast_d128(const AttnParams& P, int in, hipStream_t st);
int launch_attn_flash_d32(const AttnParams& P, const AttnHot* hot, int in, int mq, hipStream_t st);
int launch_attn_flash_d64(const AttnParams& P, const AttnHot* hot, int in, int mq, hipStream_t st);
int launch_attn_flash_d128(const AttnParams& P, const AttnHot* hot, int in, int mq, hipStream_t st);
// oeh_attn_generic.hip, oeh_attn_small.hip, oeh_attn_i8.hip
int launch_attn_generic(const AttnParams& P, int in, hipStream_t st);
int launch_attn_small(const AttnParams& P, int in, hipStream_t st);
int launch_attn_i8(const AttnParams& P, int out, hipStream_t st);
// oeh_calib.hip (oeh_attn_calibrate takes an oeh_attn_desc and fills the AttnParams block in oeh_api.hip)
int launch_attn_calibrate(const AttnParams& P, int in, int which, const double* s_range, const double* p_range, float qmax, double eps, double q_lo,
                          double q_hi, double momentum, int first, double* state, void* work, hipStream_t st);

}  // namespace oeh
