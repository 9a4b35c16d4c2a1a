// The elementwise tail of a QuantLinear with an activation function (hijacker.py:78-134: F.linear -> activation -> output quantiser; OPT's
// fc1 + ReLU, quantized_opt.py:292-294; BERT's intermediate dense + GELU, quantized_bert.py:609-617) as ONE pass over the GEMM's output:
// [alpha * x + bias] -> activation -> [round to the storage type] -> frozen 8-bit asymmetric quantiser -> the dequantised values and / or
// the centred int8 indices that the integer matrix cores take (oeh_proj_quant_i8, pairs == 3).  HBM-bound: 16-byte loads, write-through
// stores, no LDS, no atomics; every element is computed by one thread from its own input alone, so the result is bitwise reproducible.
#include "oeh_stream.h"
#include "oeh_launch.h"
#include "oeh_desc.h"

#include <cmath>
#include <cstdio>

namespace oeh {

// one activation, fp32, every operation rounded on its own
template <int ACT>
__device__ __forceinline__ float act_apply(float v) {
  if constexpr (ACT == OEH_ACT_RELU) {
    return v < 0.0f ? 0.0f : v;  // (a NaN compares false and stays, as torch.relu's does)
  } else if constexpr (ACT == OEH_ACT_GELU) {
    return (0.5f * v) * (1.0f + erff(v * (float)M_SQRT1_2));  // torch's erf form (0.5 v is exact: the order of the two products is free)
  } else {
    return v;
  }
}

// A thread-iteration = 16 consecutive columns of one row (cols % 16 == 0: a chunk never crosses a row): 4 (fp32) or 2 (16-bit) 16-byte
// loads, one 16-byte index store, 4 or 2 16-byte value stores.  Chunks are numbered row-major and dealt grid-stride; row offsets are 64-bit.
template <int IN, int ACT>
__global__ __launch_bounds__(256) void oeh_act_quant_kernel(const void* __restrict__ xin, signed char* __restrict__ out, void* __restrict__ yout,
                                                            long rows, int cols, long x_sr, long y_sr, FqP f, float alpha,
                                                            const float* __restrict__ bias) {
  constexpr int N = Vec16<IN>::N, NV = 16 / N, EB = In<IN>::bytes;
  const long chunks_per_row = cols / 16;
  const long total = rows * chunks_per_row;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = i / chunks_per_row;
    const int c0 = (int)(i - r * chunks_per_row) * 16;
    const unsigned char* xp = reinterpret_cast<const unsigned char*>(xin) + (r * x_sr + c0) * EB;
    float v[16];
#pragma unroll
    for (int q = 0; q < NV; ++q) Vec16<IN>::load(xp + 16 * q, v + N * q);
    if (bias != nullptr) {  // (uniform over the launch) a raw accumulator comes in: the projection's scale and bias, oeh_quantize_heads_i8's form
      const f4* bp = reinterpret_cast<const f4*>(bias + c0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f4 t = bp[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = __builtin_fmaf(v[4 * q + e], alpha, t[e]);
      }
    }
    unsigned int w[4];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float a = act_apply<ACT>(v[k]);
      if constexpr (ACT != OEH_ACT_NONE && IN != IN_F32) a = In<IN>::to_f32(In<IN>::from_f32(a));  // what the chain's activation op stores
      const float rel = fq_rel_sat(a, f);
      const unsigned int idx = (unsigned int)(rel + f.zp);
      if ((k & 3) == 0) w[k >> 2] = 0u;
      w[k >> 2] |= (idx ^ 0x80u) << (8 * (k & 3));
      v[k] = f.scale * rel;
    }
    if (out != nullptr) store_wt16(out + r * cols + c0, u4{w[0], w[1], w[2], w[3]});
    if (yout != nullptr) {
      unsigned char* yp = reinterpret_cast<unsigned char*>(yout) + (r * y_sr + c0) * EB;
#pragma unroll
      for (int q = 0; q < NV; ++q) store_wt16(yp + 16 * q, pack16<IN>(v + N * q));
    }
  }
}

// the most workgroups of a launch: 8 per CU of a 256-CU part; beyond kActQuantMaxBlocks * 256 chunks a thread takes several ("loop")
constexpr long kActQuantMaxBlocks = 2048;

static long act_quant_blocks(long rows, int cols, bool* loop) {
  const long total = rows * (cols / 16);
  long blocks = (total + 255) / 256;
  *loop = blocks > kActQuantMaxBlocks;
  if (*loop) blocks = kActQuantMaxBlocks;
  return blocks < 1 ? 1 : blocks;
}

static int launch_act_quant(const void* x, signed char* out, void* y, long rows, int cols, long x_sr, long y_sr, int in, int act, FqP f,
                            float alpha, const float* bias, hipStream_t st) {
  bool loop;
  const unsigned blocks = (unsigned)act_quant_blocks(rows, cols, &loop);
  dispatch_in(in, [&](auto t) {
    constexpr int IN = decltype(t)::value;
#define OEH_AQ(ACT_) hipLaunchKernelGGL((oeh_act_quant_kernel<IN, ACT_>), dim3(blocks), dim3(256), 0, st, x, out, y, rows, cols, x_sr, y_sr, f, alpha, bias)
    if (act == OEH_ACT_RELU) OEH_AQ(OEH_ACT_RELU);
    else if (act == OEH_ACT_GELU) OEH_AQ(OEH_ACT_GELU);
    else OEH_AQ(OEH_ACT_NONE);
#undef OEH_AQ
  });
  return launch_status();
}

static const char* act_name(int act) { return act == OEH_ACT_RELU ? "relu" : act == OEH_ACT_GELU ? "gelu" : "none"; }

// oeh_act_quant / oeh_act_quant_variant: the refusals that need no pointer, in the documented order
static int act_quant_check(int64_t rows, int32_t cols, int64_t x_stride, int64_t y_stride, bool with_y, int32_t dtype, int32_t act, float scale,
                           float zero_point) {
  if (rows < 0 || cols <= 0 || !dtype_ok(dtype) || x_stride < 0 || y_stride < 0) return OEH_EINVAL;
  if (act != OEH_ACT_NONE && act != OEH_ACT_RELU && act != OEH_ACT_GELU) return OEH_EINVAL;
  if (!(scale > 0.0f) || zero_point < 0.0f || zero_point > 255.0f || zero_point != std::nearbyint(zero_point)) return OEH_EINVAL;
  if (with_y && rows > 1 && y_stride < cols) return OEH_EINVAL;  // rows of the output would overlap
  if ((cols & 15) != 0) return OEH_ENOTSUP;
  const int eb = elem_bytes(dtype);
  if (!all16((uintptr_t)(x_stride * eb) | (with_y ? (uintptr_t)(y_stride * eb) : 0))) return OEH_EALIGN;
  return OEH_OK;
}

}  // namespace oeh

using namespace oeh;

extern "C" {

int oeh_act_quant(const void* x, int8_t* out, void* y, int64_t rows, int32_t cols, int64_t x_stride, int64_t y_stride, int32_t dtype, int32_t act,
                  float scale, float zero_point, float alpha, const float* bias, void* stream) {
  if (x == nullptr || (out == nullptr && y == nullptr)) return OEH_EINVAL;
  const int rc = act_quant_check(rows, cols, x_stride, y_stride, y != nullptr, dtype, act, scale, zero_point);
  if (rc != OEH_OK) return rc;
  if (!all16(addr(x) | addr(out) | addr(y) | addr(bias))) return OEH_EALIGN;
  if (rows == 0) return OEH_OK;
  const oeh_fq f = {1, scale, zero_point, 255.0f, nullptr};
  return launch_act_quant(x, reinterpret_cast<signed char*>(out), y, rows, cols, x_stride, y_stride, dtype, act, make_fq(&f), alpha, bias,
                          reinterpret_cast<hipStream_t>(stream));
}

const char* oeh_act_quant_variant(int64_t rows, int32_t cols, int64_t x_stride, int64_t y_stride, int32_t dtype, int32_t act, int32_t want_y,
                                  int32_t want_out) {
  static thread_local char name[48];
  if (!want_y && !want_out) return nullptr;
  if (act_quant_check(rows, cols, x_stride, y_stride, want_y != 0, dtype, act, 1.0f, 0.0f) != OEH_OK) return nullptr;
  bool loop;
  act_quant_blocks(rows, cols, &loop);
  std::snprintf(name, sizeof name, "actq/%s/%s/%s/%s", act_name(act), dtype_name(dtype), want_y ? (want_out ? "y+i8" : "y") : "i8", loop ? "loop" : "once");
  return name;
}

}  // extern "C"
