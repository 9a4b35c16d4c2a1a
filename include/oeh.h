/*
 * oeh.h - C ABI of liboeh_hip.so: the MI355X (gfx950) implementation of OutEffHop's
 * modified-softmax attention hot path.
 *
 * The reference (MAGICS-LAB/OutEffHop) is pure PyTorch eager code and has NO native / FFI
 * boundary of its own ("Native-code inventory"); its plugin surface is Python
 * (SOFTMAX_MAPPING, AttentionGateType, the *WithExtras modules).  This header is therefore the
 * boundary a maintainer would bind from that Python surface (ctypes stub in INTEGRATION.md);
 * each entry point names the reference op chain it replaces.
 *
 * Conventions: plain pointers and sizes only (no torch / HIP types: `stream` is a hipStream_t
 * passed as void*); every pointer is a DEVICE pointer unless said otherwise; calls enqueue on
 * `stream` and return immediately; no allocation, no ownership transfer, no host synchronisation
 * (graph-capture safe); return 0 on success or a negative OEH_E* code, never throw.
 */
#ifndef OEH_H_
#define OEH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OEH_ABI_VERSION 6

/* error codes (negative errno style) */
#define OEH_OK 0
#define OEH_EINVAL (-22)     /* bad argument (null pointer, non-positive size, bad enum) */
#define OEH_ENOTSUP (-95)    /* shape / dtype / option combination not implemented */
#define OEH_EALIGN (-14)     /* pointer or stride not aligned as required (16 B rows) */
#define OEH_ELAUNCH (-5)     /* HIP reported a launch error */
#define OEH_ENODEV (-19)     /* no gfx950 device / code object not loadable */

/* storage dtypes of q, k, v, o (arithmetic is always fp32 accumulate) */
#define OEH_F16 0
#define OEH_BF16 1
#define OEH_F32 2
#define OEH_I8 3 /* oeh_attn_fwd only: q, k, v are CENTRED 8-bit quantiser indices (see oeh_attn_desc.q_grid) */

/* softmax base: softmax_n with n = 0 (torch softmax) or n = 1 (softmax_1) */
#define OEH_SOFTMAX_VANILLA 0
#define OEH_SOFTMAX_ONE 1

/* One per-tensor asymmetric uniform fake-quantiser in fixed-range mode
 * (AsymmetricUniformQuantizer.forward, OutEffHop/quantization/quantizers/uniform_quantizers.py:119-148;
 *  QuantizationManager in Qstates.fix_ranges, quantization_manager.py:94-102):
 *    idx = clamp(rint(x / scale) + zero_point, 0, qmax);  x_q = scale * (idx - zero_point)
 * scale = float32(max(delta, 1e-8)), zero_point = clamp(rint(zero_float), 0, qmax), qmax = 2^n_bits - 1,
 * all computed on the host from the calibrated (_delta, _zero_float) buffers.  The division is a
 * true IEEE fp32 division and rint is round-half-to-even (torch.round). */
typedef struct oeh_fq {
  int32_t enable;
  float scale;
  float zero_point;
  float qmax;
  uint8_t* dump_idx; /* optional (tests): receives idx as uint8, dense row-major in the tensor's logical shape */
} oeh_fq;

/* The three activation quantisers inside the attention class
 * (quantized_opt.py:154,182,210; quantized_bert.py:363,374,434). */
typedef struct oeh_fq_desc {
  oeh_fq scores;                 /* on QK^T (after scaling), BEFORE the mask is added; dump shape (B,H,Sq,Sk) */
  oeh_fq probs;                  /* on the softmax output (after clipping);              dump shape (B,H,Sq,Sk) */
  oeh_fq ctx;                    /* on P@V;                                              dump shape (B,H,Sq,D)  */
  int32_t ctx_quant_before_gate; /* 1: OPT order (quantized_opt.py:210 then gate :224-261);
                                    0: BERT order (gate quantized_bert.py:389-426 then quant :434) */
  int32_t ctx_emit_index;        /* 1: o receives the context quantiser's INTEGERS idx - zero_point (exact in every output
                                    dtype, |.| <= 255) instead of scale * (idx - zero_point).  For a consumer that is a
                                    QuantLinear (OPT's out_proj, quantized_opt.py:271 - integer weights): the projection is
                                    then ONE 16-bit GEMM of integers, exact products, with scale_ctx * scale_w folded into its
                                    output pass - no fp32 GEMM, no operand pairs.  Needs ctx.enable and the quantiser as the
                                    last op of the core (no gate after it), else OEH_EINVAL. */
} oeh_fq_desc;

/* Attention problem descriptor.  Tensors are (B,H,S,D) VIEWS given by element strides for
 * (batch, head, sequence); the head dim is contiguous.  This covers the reference's layouts:
 * BERT's permuted view of (B,S,H*D) (bert_attention.py:164-167), OPT's contiguous (B*H,S,D)
 * (opt_attention.py:146-147,198-201), ViT's qkv unbind (vit_attention.py:205-206) and STanHop's
 * (B,L,H,E) (hopfield.py:43-49).  The output is normally given (B,S,H,D) strides so the head merge
 * (bert_attention.py:335-337, opt_attention.py:318-322) costs nothing. */
typedef struct oeh_attn_desc {
  int32_t B, H, Sq, Sk, D;
  int32_t dtype;                 /* OEH_F16 | OEH_BF16 | OEH_F32 : q, k, v and o;  OEH_I8 : q, k, v are centred 8-bit indices on
                                    q_grid / k_grid / v_grid (v transposed) and o is o_dtype - see the ABI-3 fields below */
  int64_t q_stride[3];           /* elements: batch, head, seq */
  int64_t k_stride[3];
  int64_t v_stride[3];
  int64_t o_stride[3];

  /* scores = (q.k) * scale          when scale_div == 0  (OPT: scale = 1, q pre-scaled, opt_attention.py:167;
   *                                  ViT vit_attention.py:71; Association hopfield.py:48)
   * scores = (q.k) / scale_div      when scale_div != 0  (BERT: / sqrt(d), bert_attention.py:265) */
  float scale;
  float scale_div;

  int32_t softmax_base;          /* OEH_SOFTMAX_VANILLA | OEH_SOFTMAX_ONE (vutils/softmax_1.py:4-28) */
  int32_t clip;                  /* 1: p = clip(p*(eta-gamma)+gamma, 0, 1) (models/softmax.py:10-19) */
  float gamma, eta;

  /* additive masks, applied in this order after the scores fake-quant:
   *   key_pad_mask (B,Sk): BERT's (B,1,1,S) extended mask (bert_attention.py:270-272)
   *   full_mask (B,1,Sq,Sk): OPT's causal+padding mask (opt_attention.py:215-220)
   *   causal: analytic causal mask, adds mask_min where k > q + (Sk - Sq)
   *   clamp_min: then max(x, mask_min) (opt_attention.py:221-223) */
  const void* key_pad_mask;
  int32_t key_pad_dtype;         /* OEH_F16 | OEH_F32 */
  int64_t key_pad_stride;        /* elements between batches */
  const void* full_mask;
  int32_t full_mask_dtype;       /* OEH_F16 | OEH_F32 */
  int64_t full_mask_stride[2];   /* elements: batch, query row; keys contiguous */
  int32_t causal;
  int32_t clamp_min;
  float mask_min;                /* finfo.min of the dtype the reference would hold the scores in */

  /* gate: fp32 values already multiplied by gate_scaling_factor, broadcast by zero strides
   * (context *= gate * scaling, bert_attention.py:327; opt_attention.py:309).  NULL = no gate. */
  const float* gate;
  int64_t gate_stride[3];        /* elements: batch, head, query row */

  /* OR the conditional per-token gate computed INSIDE the kernel from the layer input (bert_attention.py:301-327,
   * opt_attention.py:283-309), used when gate == NULL and gate_hidden != NULL: per head h the predictor acts on
   * gate_hidden[b, t, h*D:(h+1)*D] (same dtype as q, D contiguous, rows 16-byte aligned); weights are fp32
   * device arrays laid out as for oeh_gate_fwd (gate_units == 0: Linear(D,1): w1 (H,D), b1 (H); gate_units = m > 0:
   * Linear(D,m), ReLU, Linear(m,1): w1 (H,m,D), b1 (H,m), w2 (H,m), b2 (H)); context *= sigmoid(logit) * gate_scaling.
   * The first layer runs on the matrix cores with the weights rounded to the storage dtype and fp32 accumulation -
   * what the reference's own Linear does in a 16-bit model - so values agree with oeh_gate_fwd (fp32 weights) to
   * ~1e-4, not bit for bit.  gate_out (B,H,Sq) fp32, optional, receives sigmoid(logit) without the scaling (the
   * modules' last_gate_all_probs bookkeeping).  At most 64 hidden units (attn_gate_mlp2: head_dim); the 16-bit MFMA variants
   * ("fast16/...", "flash16/...") and, on fp32 storage, the full-row kernel (rows of <= 512 keys; weights and input as fp16
   * operand pairs: the logits are fp32-accurate, as the reference's fp32 Linear): OEH_ENOTSUP otherwise (use oeh_gate_fwd +
   * `gate`). */
  const void* gate_hidden;
  int64_t gate_hidden_stride[2]; /* elements: batch, token */
  const float* gate_w1;
  const float* gate_b1;
  const float* gate_w2;
  const float* gate_b2;
  int32_t gate_units;
  float gate_scaling;
  float* gate_out;

  /* dtype == OEH_I8 (ABI 3) - the INT8 configuration with q, k, v as the 8-bit indices the reference's QuantLinear
   * projections put them on (hijacker.py:78-127; quantized_opt.py:67-75: q_proj / k_proj / v_proj are QuantLinear, their
   * outputs fake-quantised per tensor before the bmm at :151), both products on the integer matrix cores:
   *   an element is the int8 value c = idx - 128 of the index idx in [0, 255]; its value is grid.scale * (c + 128 - grid.zero_point)
   *   (for q: AFTER OPT's `* scaling`, i.e. fold head_dim^-0.5 into q_grid.scale or pass it as `scale`);
   *   q, k: (B,H,S,D) views as usual (strides in elements = bytes); v TRANSPOSED: a (B,H,D,Sk) view, keys contiguous,
   *   v_stride = (batch, head, d row) - the second product sums over keys;
   *   o has dtype o_dtype (OEH_F16 | OEH_BF16 | OEH_F32; ABI 6: OEH_I8 with oeh_fq_desc.ctx_emit_index on a full 8-bit context grid with a
   *   whole zero point - o then holds the context quantiser's CENTRED indices idx - 128 as int8, what oeh_proj_quant_i8 takes with pairs == 3).
   * Requires D == 64, Sk <= 512 and a multiple of 16, 16-byte aligned rows, masks none | causal | key_pad_mask (with or
   * without causal) whose entries are 0 (visible) or <= -1e4 (padded: HF's extended masks hold 0 / finfo.min) - a padded key is
   * dropped exactly like a causally hidden one, other mask values are NOT added to the scores on this path -, clipping only with gamma <= 0 (the reference's registry), and `fq`
   * with scores and probabilities enabled (probabilities on a full 8-bit grid, qmax == 255; whole-number zero points, as
   * uniform_quantizers.py:79 makes them): OEH_ENOTSUP otherwise (run the fake-quant variants on dequantised values).
   * The test-only index dumps (oeh_fq.dump_idx) are honoured with o_dtype == OEH_F32: scores for every key (the reference
   * quantises before the mask is added), probabilities, context - same layouts as everywhere. */
  struct { float scale; float zero_point; } q_grid, k_grid, v_grid;
  int32_t o_dtype;               /* dtype == OEH_I8: the output's dtype.  dtype OEH_F16 / OEH_BF16 (ABI 5): OEH_F32 here asks for the
                                    output straight from the kernel's fp32 accumulators (o is then fp32, strides in fp32 elements) - the
                                    arithmetic of the kernel that ships before its output rounding, for the "within 1e-3" checks: sibling
                                    instantiations that differ in the epilogue's store only.  Head dim 64: the one-pass kernel's plain
                                    form (masks none / causal / key padding / a (B,1,Sq,Sk) mask; or with the in-kernel gate predictor,
                                    unmasked / causal) and the full-row kernel's plain / clipped forms (+ key padding; the plain form also
                                    with the in-kernel gate predictor).  Head dim 128 (round 5): the plain forms of both (the one-pass
                                    kernel with one block per wave, unmasked / causal).  OEH_ENOTSUP elsewhere.  Any other value: o has `dtype`. */

  /* (appended in ABI 4: fields are only ever added at the end of a descriptor) */
  int32_t key_pad_boolean;       /* key_pad_mask: the caller's promise that every entry is 0 or <= -1e4 (HF's extended masks: 0 / finfo.min):
                                    a padded key is then simply invisible and the INT8 chain can stay on the quantiser grid with
                                    key padding too (full-row kernel's grid form, two-pass form for rows of more than 512 keys)
                                    instead of the reference's op order on dequantised values.  With moderate negative entries
                                    (an additive bias rather than a mask) leave it 0.  Same result as the literal order except
                                    for a row WITHOUT any visible key whose mask entries are not absorbing (> -1e30): such a
                                    row comes out as with finfo.min entries.  dtype OEH_I8 always reads the mask this way. */
} oeh_attn_desc;

/* QK^T -> scale -> [fq] -> mask -> softmax / softmax_1 -> [clip] -> [fq] -> PV -> [fq] -> gate -> [fq]
 * in ONE kernel.  Replaces bert_attention.py:222-337, opt_attention.py:204-322,
 * vit_attention.py:54-75/215-266, hopfield.py:47-49 and, with `fq`, quantized_bert.py:317-434 /
 * quantized_opt.py:151-270.  `fq` may be NULL.  Dropout and head_mask are inference no-ops in the
 * reference and are not part of this path (callers must not be training with p_drop > 0). */
int oeh_attn_fwd(const oeh_attn_desc* desc, const void* q, const void* k, const void* v, void* o,
                 const oeh_fq_desc* fq, void* stream);

/* Row-wise softmax family on a dense (rows, cols) array: the SOFTMAX_MAPPING callables
 * (models/softmax.py:22-64; vutils/softmax_1.py:24-28).  x and y may alias.  dtype of x and y. */
int oeh_softmax_rows(const void* x, void* y, int64_t rows, int32_t cols, int32_t dtype, int32_t softmax_base,
                     int32_t clip, float gamma, float eta, void* stream);

/* Stand-alone per-tensor asymmetric fake-quant (QuantizedActivation in fixed-range mode,
 * base_quantized_classes.py:182-199).  y (same dtype as x) and/or idx (uint8) may be NULL. */
int oeh_fake_quant(const void* x, void* y, uint8_t* idx, int64_t n, int32_t dtype, float scale, float zero_point,
                   float qmax, void* stream);

/* Gate probabilities for the conditional gates (bert_attention.py:301-327):
 *   hidden (B,T,E) [dtype], E = H*d; per-head predictor fc_h on hidden[:, :, h*d:(h+1)*d]:
 *     hidden_units == 0 : Linear(d,1)            w1 (H,d)        b1 (H)          (w2,b2 NULL)
 *     hidden_units  > 0 : Linear(d,m),ReLU,Linear(m,1)  w1 (H,m,d) b1 (H,m) w2 (H,m) b2 (H)
 *   per_head_pool: average the logits over T before the sigmoid (conditional_per_head, :321-322)
 *   gate_out (B,H,T) fp32 (or (B,H,1) when pooling) = sigmoid(logit) * scaling.
 * Weights are fp32 device arrays. */
int oeh_gate_fwd(const void* hidden, int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t d,
                 int64_t hidden_stride_b, int64_t hidden_stride_t, const float* w1, const float* b1, const float* w2,
                 const float* b2, int32_t hidden_units, int32_t per_head_pool, float scaling, float* gate_out,
                 void* stream);

/* min and max of a dense array -> out[0], out[1] (fp32 device scalars): the CurrentMinMax / RunningMinMax
 * (no percentile) range statistics (range_estimators.py:71-72,96-97) without a device->host copy. */
int oeh_minmax(const void* x, int64_t n, int32_t dtype, float* out2, void* stream);

/* Percentile range statistics with the running average, entirely in device memory: RunningMinMaxEstimator with
 * `percentile` (range_estimators.py:83-106; the --est_ranges_pct flow of validate_clm.py:450-454 through
 * pass_data_for_range_estimation, transformers_language/utils.py:50-71), replacing the reference's device->host copy +
 * np.percentile per quantiser and batch:
 *   lo = np.percentile(x, q_lo), hi = np.percentile(x, q_hi)   (percents; "linear" interpolation between the two order
 *        statistics around each rank, float64 - what numpy returns for float32 data; exact, by radix selection)
 *   state[0..1] = first ? (lo, hi) : (1 - momentum) * (lo, hi) + momentum * state[0..1]
 * state: device double[2].  work: device scratch of OEH_CALIB_WORK_BYTES (8-byte aligned; contents irrelevant before and
 * after).  n < 2^32.  No host synchronisation. */
#define OEH_CALIB_WORK_BYTES 36864
int oeh_percentile_ema(const void* x, int64_t n, int32_t dtype, double q_lo, double q_hi, double momentum, int32_t first,
                       double* state, void* work, void* stream);

/* The activation quantiser's forward while ranges are still being estimated (QuantizationManager.forward in
 * Qstates.estimate_ranges, quantization_manager.py:104-112): the grid is derived IN the kernel from the float64
 * (x_min, x_max) pair in device memory exactly as set_quant_range does (uniform_quantizers.py:72-82:
 * x_min <- min(x_min, 0), x_max <- max(x_max, eps), delta = (x_max - x_min) / (2^n_bits - 1), zero = -x_min / delta,
 * scale = float32(max(delta, eps)), zero_point = clamp(rint(zero), 0, 2^n_bits - 1)), then y = scale * (idx - zero_point). */
int oeh_fake_quant_range(const void* x, void* y, int64_t n, int32_t dtype, const double* xmin_xmax, int32_t n_bits, double eps,
                         void* stream);

/* Range estimation of the attention core's activation quantisers WITHOUT materialising the (B,H,Sq,Sk) tensors.  In
 * Qstates.estimate_ranges the reference hands the whole score tensor and then the whole probability tensor to np.percentile
 * (range_estimators.py:83-106 from quantized_opt.py:154,182 / quantized_bert.py:363,374; 201 MB each per OPT-125m layer and
 * batch).  This entry point RECOMPUTES the values tile by tile - fp32 throughout, both products on the fp32 matrix-core
 * instruction, the elementwise chain in the reference's op order - and feeds them to the exact radix selection of
 * oeh_percentile_ema, once per selection pass; nothing of size Sq x Sk is stored.  `desc` as for oeh_attn_fwd (dtype
 * OEH_F16 | OEH_BF16 | OEH_F32, D in {32, 64, 128}, any Sq / Sk, masks key_pad_mask / full_mask / causal, scale or scale_div,
 * softmax_base, clip; gate fields are ignored):
 *   which == OEH_CALIB_SCORES : state <- percentile pair [+ running average] of the scaled scores (before quantiser and masks)
 *   which == OEH_CALIB_PROBS  : scores fake-quantised on the grid of `scores_range` (NULL: not quantised), masks, softmax, clip;
 *                               state <- percentile pair [+ running average] of the probabilities
 *   which == OEH_CALIB_CONTEXT: ... probabilities fake-quantised on the grid of `probs_range` (NULL: not), P V -> ctx_out
 *                               (fp32, o_stride of desc in fp32 elements); no statistics (state / work unused) - the context is
 *                               small, its quantiser runs oeh_percentile_ema / oeh_fake_quant_range on it
 * scores_range / probs_range: device double[2] = (x_min, x_max), e.g. the `state` of the previous call; the grids are derived
 * in the kernel as oeh_fake_quant_range does (n_bits, eps).  q_lo, q_hi, momentum, first, state, work: as oeh_percentile_ema.
 * No host synchronisation; safe under hipGraph capture. */
#define OEH_CALIB_SCORES 0
#define OEH_CALIB_PROBS 1
#define OEH_CALIB_CONTEXT 2
int oeh_attn_calibrate(const oeh_attn_desc* desc, const void* q, const void* k, const void* v, float* ctx_out, int32_t which,
                       const double* scores_range, const double* probs_range, int32_t n_bits, double eps, double q_lo, double q_hi,
                       double momentum, int32_t first, double* state, void* work, void* stream);

/* The producer side of the INT8-storage attention core (oeh_attn_fwd with dtype OEH_I8): a QuantLinear projection's output
 * quantiser (hijacker.py:78-127; AsymmetricUniformQuantizer.forward, uniform_quantizers.py:119-148) that writes what the core
 * consumes - the centred int8 index c = clamp(rint(x / scale) + zero_point, 0, 255) - 128 - instead of a fake-quantised
 * float tensor, split into heads of 64:
 *   x: (B, S, H*64) values in `dtype`, last dim contiguous, x_stride = (batch, row) in elements;
 *   transpose == 0: out is (B, S, H*64) int8 in x's element order (q, k; needs x_stride[0] == S * x_stride[1]);
 *   transpose == 1: out is (B, H, 64, S) int8, keys contiguous (v: the layout the second product wants; S % 16 == 0);
 *   y (optional, may be NULL): the dequantised values scale * (idx - zero_point) in `dtype`, y_stride like x_stride - what a
 *   decoder keeps as its (k, v) cache - in the same pass; with transpose == 0, out may be NULL when y is given: the values
 *   only, i.e. a QuantLinear's scale + bias + output fake-quant in one pass over the GEMM accumulator (out_proj);
 *   bias (optional, fp32 device array of H*64, may be NULL): x is a raw GEMM accumulator and the value that is quantised is
 *   alpha * x + bias[column] - the projection's weight scale and bias folded into this pass (oeh_split_pairs' GEMM);
 *   bias == NULL: x is quantised as it is (alpha ignored).
 * x, out, y and bias must be 16-byte aligned, and so must the row and batch strides of x and y in bytes (16-byte vector
 * accesses): OEH_EALIGN otherwise.
 * One launch per projection instead of fake-quant + index conversion + transpose copy. */
int oeh_quantize_heads_i8(const void* x, int8_t* out, void* y, int64_t B, int32_t S, int32_t H, const int64_t x_stride[2],
                          const int64_t y_stride[2], int32_t dtype, float scale, float zero_point, int32_t transpose, float alpha,
                          const float* bias, void* stream);

/* fp32 activations as fp16 operand pairs for a library GEMM either side of the attention core (the q/k/v and output
 * projections of an fp32 model, opt_attention.py:167-201,318-324 / quantized_opt.py:67-75): out[r][0:K] = hi = RN16(x[r]),
 * out[r][K:2K] = lo = RN16((x[r] - hi) * 2^11); with the weight matrix stacked as [W ; W * 2^-11] one fp16 GEMM with fp32
 * accumulation gives x.W to ~2^-22 relative (the weight side exactly when W holds 8-bit integers, as QuantLinear's weights
 * do up to their scale) at fp16 matrix-core speed.  x: (rows, K) fp32, K % 8 == 0, 16-byte aligned rows; out: (rows, 2K) fp16. */
int oeh_split_pairs(const float* x, void* out_f16, int64_t rows, int32_t K, int64_t x_stride_row, void* stream);

/* The same prologue for Linears with GENERAL fp32 weights (the unquantised fp32 models of validate_clm.py / validate_mlm_config.py:
 * q_proj / k_proj / v_proj / out_proj, query / key / value - opt_attention.py:167-201,318-324, bert_attention.py:183-208): with
 * x = xh + xl 2^-11, W = Wh + Wl 2^-11, b = bh + bl 2^-11 (all halves fp16),
 *     x W^T + b  =  [ xh | xh 2^-5 | xl 2^-5 | 1, 2^-5, 0 x6 ]  @  [ Wh ; Wl 2^-6 ; Wh 2^-6 ; bh ; bl 2^-6 ; 0 x6 ]   (+ O(2^-22) relative)
 * i.e. ONE fp16 GEMM with fp32 accumulation over K' = 3K + 8, bias included - measured closer to the float64 result than the fp32
 * library GEMM and about twice as fast (M = 8192, K = 768: N = 768 46 us against 89 us, N = 2304 122 us against 231 us).
 * This entry writes the activation side: x (rows, K) fp32 with row stride x_stride_row (elements) -> out_f16 (rows, 3K + 8) fp16,
 * contiguous; K % 8 == 0, 16-byte aligned rows.  Values beyond the fp16 range saturate (as in oeh_split_pairs). */
int oeh_split_triples(const float* x, void* out_f16, int64_t rows, int32_t K, int64_t x_stride_row, void* stream);

/* The q / k / v projections of a QuantLinear model as ONE matrix-core GEMM with the output quantisers in its epilogue (SURVEY 8f-1;
 * quantized_opt.py:67-75 q_proj / k_proj / v_proj, quantized_bert.py:236-238 query / key / value: QuantLinear = weight fake-quant +
 * F.linear + output fake-quant, hijacker.py:78-127): what a library GEMM over the stacked weights followed by three
 * oeh_quantize_heads_i8 passes computes, without the (B*S, n_seg*E) accumulator ever reaching memory.
 *   a: the activations (B*S rows, row stride lda elements, 16-byte aligned rows) - pairs == 0: fp16 (rows, K); pairs == 1: fp16
 *      (rows, 2K), the operand pairs [hi | lo] that oeh_split_pairs writes for an fp32 model; pairs == 2: the fp32 activations (rows, K)
 *      themselves - the kernel forms a (hi, lo) pair when a wave reads its operand fragments, without the split pass: 64 x = hi + lo with the
 *      residual unscaled (|x - pair| <= 2^-31: 22 bits down to |x| = 2^-9, as pairs == 1 above that; |x| <= 2 047, saturating beyond), so an index
 *      differs from the pairs == 1 call's only where the value sits on a rounding boundary to within the fp32 accumulation error; pairs == 3: int8 (rows, K) - e.g. the centred indices idx - 128 of the producer's 8-bit
 *      quantiser (oeh_attn_fwd, dtype OEH_I8, o_dtype OEH_I8) - against int8 weights on the integer matrix cores (K % 64 == 0): exact
 *      int32 sums; with acc_add[n] = (128 - zero_point) * sum_k w[n][k] the accumulator is the sum over idx - zero_point;
 *   w: (n_seg*E, K) fp16 (int8 with pairs == 3), row stride ldw: the QuantLinear weights' INTEGERS (w / weight scale: exact in fp16), the segments' rows
 *      one after the other; pairs == 1 multiplies the lo half against w * 2^-11, formed in registers (exact on integers);
 *   bias: (n_seg*E) fp32; segment i covers output columns [i*E, (i+1)*E) and turns the fp32 accumulator into
 *      value = alpha * acc + bias[column],  c = clamp(rint(value / scale) + zero_point, 0, 255) - 128:
 *      out  (may be NULL when y is given): int8, (B, S, E) [transpose == 0: q, k] or (B, E/64, 64, S) [transpose == 1: v, keys
 *           contiguous] - the layouts oeh_attn_fwd takes with dtype OEH_I8; 16-byte aligned;
 *      y    (optional): the dequantised values scale * (c + 128 - zero_point) as fp32, (B*S, E) with row stride y_stride_row
 *           elements - a decoder's (k, v) cache.
 * K % 32 == 0, E % 64 == 0, S % 16 == 0 (and every 32-bit lane offset of a, w and y below 4 GiB): OEH_ENOTSUP otherwise; n_seg outside
 * 1..3: OEH_EINVAL.  Same formulas as oeh_quantize_heads_i8; the
 * accumulation order differs from a library GEMM's, so an index may differ by one step where the value sits on a rounding
 * boundary to within the fp32 accumulation error (both are fp32-grade: |acc - exact| <~ 1e-6 of the row's scale). */
typedef struct {
  float alpha;
  float scale, zero_point;
  int8_t* out;
  float* y;
  int64_t y_stride_row;
  int32_t transpose;
  const int32_t* acc_add;   /* pairs == 3 only: E integers added to the int32 accumulator before alpha (NULL: none) */
} oeh_proj_seg;
int oeh_proj_quant_i8(const void* a, int32_t pairs, const void* w, const float* bias, int64_t B, int32_t S, int32_t K, int32_t E, int32_t n_seg,
                      const oeh_proj_seg* segs, int64_t lda, int64_t ldw, void* stream);

/* The elementwise tail of a QuantLinear WITH an activation function (oeh_act_quant.hip) - OPT's fc1 + ReLU (quantized_opt.py:292-294), BERT's
 * intermediate dense + GELU (quantized_bert.py:609-617); hijacker.py:78-134: F.linear -> activation -> output quantiser - in ONE pass over
 * the (rows, cols) output of the GEMM, x in `dtype`, columns contiguous, x_stride elements between rows.  Per element, every operation
 * rounded on its own:
 *   v = fma(x, alpha, bias[column])        bias given (cols fp32 values): x is a raw accumulator - oeh_quantize_heads_i8's form;
 *   v = x                                  bias == NULL (alpha ignored)
 *   a = v | max(v, 0) | 0.5 v (1 + erf(v / sqrt 2))        act = OEH_ACT_NONE | OEH_ACT_RELU (a NaN stays a NaN) | OEH_ACT_GELU (the erf
 *                                          form, in fp32; the tanh form is not implemented)
 *   a = RN_dtype(a)                        16-bit `dtype` with an activation: what the separate activation op stores
 *   c = clamp(rint(a / scale) + zero_point, 0, 255)         oeh_fake_quant's arithmetic (8-bit grid)
 *   y   (optional): scale * (c - zero_point) in `dtype`, y_stride elements between rows;
 *   out (optional): c - 128 as int8, (rows, cols) contiguous - the operand of oeh_proj_quant_i8 with pairs == 3.
 * A NaN takes index 0, +-inf saturate (oeh_fake_quant's behaviour).  Bitwise reproducible, no work buffer, safe under graph capture.
 * Launch forms (oeh_act_quant_variant: "actq/relu/f32/y+i8/once", "actq/gelu/f16/i8/loop"; host only, NULL if refused, the string lives
 * in thread-local storage until the next call on this thread; it assumes 16-byte aligned pointers): a thread takes 16 consecutive columns;
 * "loop" when the 2048 workgroups of a launch take more than one such chunk per thread.
 * Refusals, before any launch, in this order: OEH_EINVAL - x NULL, out and y both NULL, rows < 0, cols < 1, a dtype other than OEH_F16 /
 * OEH_BF16 / OEH_F32, a negative stride, an unknown activation, scale <= 0, a zero point that is no integer in [0, 255], y_stride < cols
 * with rows > 1; OEH_ENOTSUP - cols % 16 != 0; OEH_EALIGN - x, out, y or bias not 16-byte aligned, a row stride of x or y that is no
 * multiple of 16 bytes.  rows == 0: OEH_OK without a launch. */
#define OEH_ACT_NONE 0
#define OEH_ACT_RELU 1
#define OEH_ACT_GELU 2
int oeh_act_quant(const void* x, int8_t* out /* may be NULL */, void* y /* may be NULL */, int64_t rows, int32_t cols, int64_t x_stride,
                  int64_t y_stride, int32_t dtype, int32_t act, float scale, float zero_point, float alpha, const float* bias /* may be NULL */,
                  void* stream);
const char* oeh_act_quant_variant(int64_t rows, int32_t cols, int64_t x_stride, int64_t y_stride, int32_t dtype, int32_t act, int32_t want_y,
                                  int32_t want_out);  /* which launch form, or NULL if refused; host only */

/* Attention core for TRAINING (oeh_attn_bwd.hip): the forward with its row statistic, and the fused backward that recomputes the
 * probabilities from it - nothing of size Sq x Sk is stored.  Replaces the torch-op chain opt_attention.py:204-263 /
 * bert_attention.py:222-292 under autograd.  `desc` as for oeh_attn_fwd with: dtype OEH_F16 | OEH_BF16, D == 64, softmax_base and
 * clip (gamma, eta), scale / scale_div, key_pad_mask, full_mask, causal, clamp_min + mask_min; fp32 or INT8 storage, another head
 * dim, a gate (gate or gate_hidden) or o_dtype OEH_F32: OEH_ENOTSUP (the gate stays outside the differentiable core, as a torch
 * multiply; fake-quant has no parameter here).  q, k, v, o (and do_, dq, dk, dv) rows must be 16-byte aligned: OEH_EALIGN.
 *
 * oeh_attn_fwd_train: o as oeh_attn_fwd (o_stride), and lse (B,H,Sq) fp32 contiguous: the per-row statistic
 *   lse = m' + log(sum_k e^(x_k - m') + [softmax_1] e^(-m')),  m' = max(m, 0) for softmax_1, m for softmax
 * so that p = e^(x - lse) for either base (a fully masked softmax_1 row: p = 0; a fully masked vanilla row: uniform).
 * oeh_attn_bwd: do_, dq, dk, dv in desc->dtype with their own (batch, head, seq) element strides; o and lse from
 *   oeh_attn_fwd_train; work: caller-provided fp32 scratch of oeh_attn_bwd_work_bytes(desc) bytes (two terms per query row: delta, and
 *   log(den) of a row whose fp32 lse cannot hold it - a vanilla row at finfo.min of bf16 / fp32).  Two kernels
 *   (dq, then dk / dv), no allocation, no atomics: the gradients are bitwise reproducible; graph-capture safe.
 * oeh_attn_bwd_work_bytes: bytes of `work`, or the negative OEH_E* code of an unsupported / invalid descriptor. */
int oeh_attn_fwd_train(const oeh_attn_desc* desc, const void* q, const void* k, const void* v, void* o, float* lse, void* stream);
int64_t oeh_attn_bwd_work_bytes(const oeh_attn_desc* desc);
int oeh_attn_bwd(const oeh_attn_desc* desc, const void* q, const void* k, const void* v, const void* o, const void* do_,
                 const int64_t do_stride[3], const float* lse, void* dq, const int64_t dq_stride[3], void* dk, const int64_t dk_stride[3],
                 void* dv, const int64_t dv_stride[3], void* work, void* stream);

/* Attention dropout inside the training kernels (oeh_attn_bwd.hip, oeh_philox.h): the probabilities after the clip (y, or p without
 * the clip) are multiplied by keep / (1 - p) before the product with V - where nn.Dropout sits in bert_attention.py /
 * opt_attention.py - and both backward kernels regenerate the same bits; nothing of size Sq x Sk is stored and lse is unchanged.
 * The keep bit of element (b, h, i, j) (query row i, key column j of the logical problem) is Philox4x32-10 with key
 * (seed & 0xffffffff, seed >> 32), counter (j >> 2, i, b * H + h, 0), output word j & 3: kept iff word >= floor(p * 2^32).
 * p outside [0, 1) or NaN: OEH_EINVAL, before any other check or device work; p == 0: exactly the entry points above.
 * oeh_attn_fwd_train_dropout / oeh_attn_bwd_dropout: as oeh_attn_fwd_train / oeh_attn_bwd (same scope rules, same scratch
 *   oeh_attn_bwd_work_bytes(desc)); the backward must get the forward's drop.
 * oeh_attn_dropout_mask: the (B,H,Sq,Sk) contiguous keep mask (1 kept, 0 dropped) of desc's B, H, Sq, Sk from the same generator. */
typedef struct oeh_dropout {
  float p;
  uint32_t reserved;
  uint64_t seed;
} oeh_dropout;
int oeh_attn_fwd_train_dropout(const oeh_attn_desc* desc, const oeh_dropout* drop, const void* q, const void* k, const void* v, void* o, float* lse,
                               void* stream);
int oeh_attn_bwd_dropout(const oeh_attn_desc* desc, const oeh_dropout* drop, const void* q, const void* k, const void* v, const void* o,
                         const void* do_, const int64_t do_stride[3], const float* lse, void* dq, const int64_t dq_stride[3], void* dk,
                         const int64_t dk_stride[3], void* dv, const int64_t dv_stride[3], void* work, void* stream);
int oeh_attn_dropout_mask(const oeh_attn_desc* desc, const oeh_dropout* drop, uint8_t* keep, void* stream);

/* Options of the forward beyond oeh_attn_desc (ABI 6 and the descriptor stay as they are).
 * pv_pairs != 0: fp32 storage (dtype OEH_F32) computes the CONTEXT to fp32 accuracy as well as the scores.  The one-pass and full-row
 *   kernels split each fp32 probability tile in registers into fp16 operands p = P_hi + P_lo 2^-11 and accumulate
 *   V P = V_hi P_hi + 2^-11 (V_lo P_hi + V_hi P_lo) - without it P enters the second product as ONE fp16 operand (~1e-4 relative on the
 *   context).  The one-pass kernel's row sums include P_lo, so the denominator is the sum of what the numerator multiplied.  The
 *   small-shape kernel (fp32 matrix-core operands) and the any-shape kernel (fp32 FMA) are fp32-exact already and run unchanged; a problem
 *   that would reach the general kernel (fp16 probability operand) runs on the any-shape kernel instead.  Not with fake-quant (`fq`
 *   enabled: the probability operand is a grid value), the in-kernel gate predictor (gate_hidden; `gate` is fine) or 16-bit storage
 *   (including o_dtype OEH_F32): OEH_ENOTSUP.
 * reserved: must be 0 (else OEH_EINVAL, before any other check or device work).
 * oeh_attn_fwd_ex / oeh_attn_variant_ex with opts == NULL or pv_pairs == 0: exactly oeh_attn_fwd / oeh_attn_variant.  The variant name
 * of a form with probability pairs ends in "+pv2" ("flash16/MQ2/D64/f32+pv2"). */
typedef struct oeh_attn_opts {
  int32_t pv_pairs;
  int32_t reserved[3];
} oeh_attn_opts;
int oeh_attn_fwd_ex(const oeh_attn_desc* desc, const oeh_attn_opts* opts, const void* q, const void* k, const void* v, void* o,
                    const oeh_fq_desc* fq, void* stream);
const char* oeh_attn_variant_ex(const oeh_attn_desc* desc, const oeh_attn_opts* opts, const oeh_fq_desc* fq);

/* Split-key decode attention (oeh_attn_decode.hip): a generation step against a key / value cache - 1 <= Sq <= 16 query rows, any Sk >= 1 - with
 * the KEYS of one (batch, head) split over up to OEH_DECODE_MAX_SPLITS workgroups and the partial results combined by a second small launch.
 * oeh_attn_fwd gives such a problem one workgroup per (batch, head) that walks the whole cache serially; this entry point fills the chip.
 * `desc` as for oeh_attn_fwd with: dtype OEH_F16 | OEH_BF16, D == 64, both softmax bases, clip with gamma <= 0, scale or a positive finite
 * scale_div, key_pad_mask (f16 / f32), causal (the Sk - Sq offset; only Sq <= Sk), clamp_min + mask_min, gate values with their strides,
 * o_dtype == OEH_F32 (fp32 output from the accumulators, written by the combine pass).  oeh_attn_decode takes no fake-quant argument;
 * oeh_attn_decode_fq below is the same entry point with one.
 * Refusals, in this order: OEH_EINVAL - null pointers, non-positive sizes, splits < 0 or > OEH_DECODE_MAX_SPLITS; OEH_ENOTSUP - full_mask,
 * gate_hidden, fp32 or INT8 storage, another head dim, Sq > 16, clip with gamma > 0, causal with Sq > Sk; OEH_EALIGN - q, k, v or o rows (or
 * `work`) not 16-byte aligned.
 * splits == 0: the library chooses (oeh_attn_decode.hip, default_splits, with the measurements it was chosen from).  Otherwise the chunk is
 * C = roundup64(ceil(Sk / splits)) keys and the effective count n = ceil(Sk / C); the variant name prints n:
 * "decode16/SP<n>/D64/<f16|bf16>[/clip]".
 * work: caller-provided device scratch of oeh_attn_decode_work_bytes(desc, splits) bytes, 16-byte aligned; contents irrelevant before and
 * after.  Per (batch, head, split, query row): the running maximum m and the sum l = sum e^(x - m) of the split's scores, and 64 fp32
 * accumulators sum e^(x - m) v.  The combine pass forms M = max_s m_s (softmax_1: max(., 0)), den = sum_s l_s e^(m_s - M) (+ e^(-M)) and
 * o = sum_s acc_s e^(m_s - M) / den - M and den as TWO numbers, never one lse = M + log(den): a vanilla row without a visible key sits at
 * finfo.min, where that sum rounds back to M and every key would get probability 1 (the same trap as the backward's scratch above).
 * The clipped forms run three launches (statistics; y = clip((eta - gamma) e^(x - M) / den + gamma, 0, 1) times V per split; the sum).
 * No allocation, no host synchronisation, no atomics, a fixed split order: bitwise reproducible; graph-capture safe (a linear chain of
 * launches).  The masks are added literally in fp32 and no chunk is skipped (a vanilla row without a visible key is uniform over ALL keys).
 * oeh_attn_decode_work_bytes: bytes of `work`, or the negative OEH_E* code.  oeh_attn_decode_variant: host only; NULL if refused; the
 * string lives in thread-local storage until the next call on this thread. */
#define OEH_DECODE_MAX_SPLITS 64
int64_t oeh_attn_decode_work_bytes(const oeh_attn_desc* desc, int32_t splits);
int oeh_attn_decode(const oeh_attn_desc* desc, int32_t splits, const void* q, const void* k, const void* v, void* o, void* work, void* stream);
const char* oeh_attn_decode_variant(const oeh_attn_desc* desc, int32_t splits);
/* The same with the fused INT8 chain of oeh_attn_fwd - QK^T -> scale -> [fq scores] -> masks -> softmax / softmax_1 -> [clip] -> [fq probs] -> PV ->
 * [fq ctx | gate, in the order of ctx_quant_before_gate] - for a quantised decoder's generation step; any subset of the three quantisers.
 * `desc`, `splits` (the same rule), the scope and `work` - layout and size of oeh_attn_decode_work_bytes(desc, splits), the same (m, l) pairs
 * and accumulators; there is no second size function - as for oeh_attn_decode.  With fq == NULL or no quantiser enabled the call IS
 * oeh_attn_decode, bit for bit.
 * The scores are quantised right after the scaling (scale_div: a true division) and before the masks, which are added literally
 * (key_pad_boolean is accepted and not needed); a key beyond Sk stays invisible, a zero K row quantises to a grid point.  With the probability
 * quantiser (as with the clip) the three-launch form runs: statistics; a product pass that forms p = e^(x - M) / den, clips, and feeds the
 * integers idx - zero_point (exact in fp16 and bf16) to the second product; a sum that applies the probability scale in fp32.  Otherwise the
 * two-launch form, the scores quantiser in the partial pass.  The context quantiser and the gate sit in the last launch; o_dtype == OEH_F32
 * stays available.  Index dumps (oeh_fq.dump_idx, tests): scores and probabilities dense (B,H,Sq,Sk), each split writing its own keys; context
 * (B,H,Sq,64).  Still plain launches in a fixed split order: bitwise reproducible, graph-capture safe.
 * Refusals: those of oeh_attn_decode first, in its order (full_mask, gate_hidden, fp32 / INT8 storage, another head dim, Sq > 16 ... are
 * OEH_ENOTSUP here too); then OEH_EINVAL - an enabled quantiser whose scale is not positive and finite, whose qmax is not finite and >= 1 or
 * whose zero point lies outside [0, qmax]; then OEH_ENOTSUP - ctx_emit_index (oeh_attn_fwd has it), a uint8 dump of a grid with qmax > 255.
 * oeh_attn_decode_fq_variant: the decode name with "/fq" appended when a quantiser is enabled ("decode16/SP8/D64/f16/fq", ".../clip/fq");
 * NULL if refused; thread-local storage as above. */
int oeh_attn_decode_fq(const oeh_attn_desc* desc, const oeh_fq_desc* fq, int32_t splits, const void* q, const void* k, const void* v, void* o,
                       void* work, void* stream);
const char* oeh_attn_decode_fq_variant(const oeh_attn_desc* desc, const oeh_fq_desc* fq, int32_t splits);

/* Outlier statistics (oeh_stats.hip): the two numbers the reference reports its results in - the maximum infinity norm and the average
 * kurtosis of layer outputs (validate_clm.py:565-621, validate_mlm.py:497-533, validate_vit1.py:620-693, run_clm_ddp.py:735-760, with
 * `kurtosis` of transformers_language/utils.py:9-20) - for every row of a (rows, cols) array in ONE pass over HBM, replacing the eager
 * chain x.norm(p=inf), mean, std, (x - mu) ** 4, mean and its one .item() per sample and statistic.
 * x: fp16 / bf16 / fp32, element (r, c) at x[r * row_stride + c], row_stride >= cols; rows may start at any element (no 16-byte rule).
 * stats: (rows, 4) fp32, 16-byte aligned:
 *   [0] inf_norm = max |x|                                  (bit for bit)
 *   [1] kurtosis = mean((x - mu)^4) / (std^4 + eps)         (utils.py:9-20)
 *   [2] mean
 *   [3] std, unbiased: sqrt(sum (x - mu)^2 / (cols - 1))    (torch.std)
 * evaluated from central moments about per-chunk means in fp32 (never raw power sums), corrected and merged in float64 (Chan / Pebay
 * pairwise updates) in a fixed order: bitwise reproducible.  The values are the float64 results rounded to fp32 for 16-bit inputs too;
 * the reference would evaluate (x - mu)^4 in the storage type there and overflow fp16.
 * Special values: a NaN in a row -> inf_norm = NaN, kurtosis = NaN; a +-inf (and no NaN) -> inf_norm = +inf, kurtosis = NaN (mean and std
 * are NaN in both cases); a constant row -> std = 0 and kurtosis = 0 exactly (eps > 0); cols == 1 -> inf_norm = |x|, mean = x, std and
 * kurtosis NaN.  fp32 data with |x - mean| >= 2^31 overflows the fourth power as it does in the reference: no accuracy is promised, the
 * call returns normally.
 * meter (or NULL): device double[4] = {sum_inf, n_inf, sum_kurt, n_kurt}, 8-byte aligned - the running sums that the reference's
 * AverageMeter.update(v.item()) forms on the host.  The last launch of the call adds this call's rows, in ascending order, in float64,
 * as selected by `accumulate`: bit 0 (1) the inf-norms, bit 1 (2) the kurtoses; 0 leaves meter untouched.
 * Rows of at most OEH_STATS_WAVE_COLS elements: one wave per row, one launch, no work buffer.  Longer rows: one workgroup per
 * (row, chunk of OEH_STATS_CHUNK elements, cut at the row's own 16-byte boundaries) writes a record of OEH_STATS_RECORD_BYTES to `work`
 * and a second launch merges them.  work: device scratch of oeh_outlier_stats_work_bytes(rows, cols) bytes (0 for the short-row form; 0
 * for rows or cols < 1), 8-byte aligned, contents irrelevant before and after.  Plain launches in a linear chain: no atomics, no
 * allocation, no host synchronisation, graph-capture safe.
 * Refusals, before any launch: OEH_EINVAL - x or stats NULL, rows < 1 or cols < 1, row_stride < cols, a dtype other than OEH_F16 /
 * OEH_BF16 / OEH_F32, eps < 0 or NaN, accumulate outside 0..3 or non-zero with meter == NULL, work == NULL where work_bytes > 0;
 * OEH_EALIGN - stats not 16-byte aligned, meter or work not 8-byte aligned, x not aligned to its element; OEH_ENOTSUP - 2^31 or more
 * (row, chunk) pairs. */
#define OEH_STATS_WAVE_COLS 2040
#define OEH_STATS_CHUNK 8192
#define OEH_STATS_RECORD_BYTES 48
size_t oeh_outlier_stats_work_bytes(int64_t rows, int64_t cols);
int oeh_outlier_stats(const void* x, int64_t rows, int64_t cols, int64_t row_stride, int32_t dtype, double eps, float* stats, double* meter,
                      int32_t accumulate, void* work, void* stream);

/* Quantisation-error search (oeh_qmse.hip): the squared error of K candidate quantiser grids on one array, every candidate from ONE
 * read of the data - the loss_fx of the reference's MSE range estimator (quantization/range_estimators.py:134-142: fake-quantise,
 * subtract, square, sum, .cpu(), once per candidate range; 100 times per tensor and batch in the 1-D grid search, 100 * 64 * 2 times in
 * the 2-D search).
 * x: n elements of fp16 / bf16 / fp32, dense, starting at any element (no 16-byte rule); nothing outside [x, x + n) is read.
 * cand: K records of OEH_QMSE_CAND_BYTES = 16 bytes in device memory, 16-byte aligned, four floats each:
 *   [0] scale > 0    the grid's step (the quantiser's clamp(delta, eps))
 *   [1] lo           int_min - zero_point   (lowest index relative to the zero point)
 *   [2] hi           int_max - zero_point
 *   [3] reserved     (ignored; write 0)
 * One record type covers every grid: symmetric signed (-128, 127), symmetric unsigned (0, 255), asymmetric (-zp, qmax - zp), any
 * n_bits <= 16.  RN(1 / scale) is formed inside the kernel by a true division.  scale <= 0 is the caller's error and is not detected.
 * loss: K float64 in device memory, 8-byte aligned: loss[k] = sum_i term_i(k), or loss[k] += that sum (ONE float64 add) when
 * `accumulate` is not 0.  The term is defined in fp32, each operation rounded separately, exactly as the reference's eager ops round it
 * (uniform_quantizers.py:114-115,146; 16-bit elements are widened to fp32 first - the reference would square and sum in the storage
 * type there and overflow fp16):
 *   q = RN(x_i / scale_k);  r = clamp(rint(q), lo_k, hi_k)  (ties to even);  y = fl32(scale_k * r);  d = fl32(x_i - y);  term = fl32(d * d)
 * At most 32 terms are added in fp32, pairwise, before the sum continues in float64 in a fixed order:
 *   |loss[k] - L64[k]| <= 6 * 2^-24 * L64[k],   L64 = the float64 sum of the fp32 terms;   bitwise reproducible.
 * A call of K <= OEH_QMSE_F64_K candidates adds in float64 from the first term (loss[k] = L64[k] up to float64 rounding): such calls are
 * the steps of a sequential search (golden section), whose result moves with the noise of its loss - the reference's fp32 sums move the
 * range it finds by 1e-4 - and whose pass over the data is bound by the read, not by the arithmetic.
 * A non-finite element makes the losses it affects inf / NaN; the call returns normally.
 * A workgroup keeps a chunk of OEH_QMSE_CHUNK elements (cut at the array's own 16-byte boundaries) in registers and loops over the
 * candidates; at most OEH_QMSE_MAX_BLOCKS workgroups (beyond that each takes several chunks) write one float64 per candidate to `work`
 * and a merge launch adds them in a fixed order.  K is unbounded: it is cut into slices of OEH_QMSE_SLICE candidates, each a pass over the
 * data and a merge.  work: device scratch of oeh_quant_mse_work_bytes(n, K) bytes (0 for n < 1 or K < 1), 8-byte aligned, contents
 * irrelevant before and after.  Plain launches in a linear chain: no atomics, no allocation, no host synchronisation, graph-capture
 * safe; the launch geometry depends on (n, K) only.
 * Refusals, before any launch: OEH_EINVAL - x, cand, loss or work NULL, n < 1, K < 1, a dtype other than OEH_F16 / OEH_BF16 / OEH_F32;
 * OEH_EALIGN - cand not 16-byte aligned, loss or work not 8-byte aligned, x not aligned to its element. */
#define OEH_QMSE_CHUNK 8192
#define OEH_QMSE_SLICE 256
#define OEH_QMSE_MAX_BLOCKS 1024
#define OEH_QMSE_CAND_BYTES 16
#define OEH_QMSE_F64_K 4
size_t oeh_quant_mse_work_bytes(int64_t n, int32_t K);
int oeh_quant_mse(const void* x, int64_t n, int32_t dtype, const float* cand, int32_t K, double* loss, int32_t accumulate, void* work,
                  void* stream);

/* The tail of a quantised transformer block (oeh_ln.hip): residual add -> sum quantiser -> LayerNorm -> output quantiser on the rows
 * of a (rows, cols) array in ONE pass - dense -> dropout -> + input -> res_act_quantizer -> LayerNorm of QuantizedBertSelfOutput /
 * QuantizedBertOutput (quantized_bert.py:541-606), residual + x -> *_res_act_quantizer -> *_layer_norm of QuantizedOPTDecoderLayer
 * (quantized_opt.py:277-384), with QuantLayerNorm = F.layer_norm on fake-quantised gamma -> activation quantiser
 * (autoquant_utils.py:64-72, hijacker.py:78-134).  Inference only.
 * x, r, sum_out and y have `dtype` and contiguous columns; element (i, j) of each sits at base[i * stride + j].  gamma, beta: cols fp32
 * values, fake-quantised by the caller where weight quantisation is on.  Per row, every operation rounded on its own, in this order:
 *   s = RN_dtype(x + r)              one fp32 add rounded once to the storage type; s = x without r
 *   fq_sum enabled: s = RN_dtype(scale * (clamp(rint(s / scale) + zero_point, 0, qmax) - zero_point))   oeh_fake_quant's arithmetic
 *   sum_out (if given) <- s;  the LayerNorm reads this stored, rounded s - the call equals the composition of the separate ops bit for bit
 *   mean = sum(s) / cols;  var = sum((s - mean)^2) / cols (biased), fp32, two passes over the row in registers, a fixed summation order
 *   rstd = 1 / sqrt(var + eps)       correctly rounded square root and division
 *   y = ((s - mean) * rstd) * gamma + beta;  fq_out enabled: the same fake-quant;  y <- RN_dtype(.)
 * Bitwise reproducible.  qmax up to 65535 (the 16-bit final LayerNorm of quantized_opt.py:740-741).  The dump_idx fields of the two oeh_fq
 * are ignored: sum_idx / y_idx (tests; dense (rows, cols) uint8) receive the indices of the sum / output quantiser.
 * Aliasing: sum_out may be r or x, and y may be x, with the same row stride; anything else must not overlap.
 * Launch forms (oeh_resid_ln_variant: "ln/wave/CH4/f32", "ln/block/CH8/f16", "ln/scalar/CH1/bf16"; host only, NULL if refused, the
 * string lives in thread-local storage until the next call on this thread; it assumes 16-byte aligned pointers): one wave per row, four
 * rows per workgroup, for cols <= 1024; one workgroup per row up to cols <= 8192 - both with 16-byte accesses, which need every base
 * pointer (gamma and beta included) 16-byte aligned and cols and every given tensor's stride a multiple of 4 (fp32) / 8 (16-bit)
 * elements; otherwise element accesses, one workgroup per row.
 * Refusals, before any launch: OEH_EINVAL - desc, x, gamma or y NULL, cols < 1, rows < 0, a dtype other than OEH_F16 / OEH_BF16 /
 * OEH_F32, eps < 0 or NaN, reserved != 0, a negative stride, a stride of sum_out or y below cols with rows > 1, an enabled quantiser that
 * is no grid (scale <= 0, qmax < 1, zero point outside [0, qmax]), an index dump of a disabled quantiser; OEH_ENOTSUP - cols > 8192,
 * rows >= 2^31, an index dump of a grid with qmax > 255.  rows == 0: OEH_OK without a launch. */
typedef struct oeh_ln_desc {
  int64_t rows; int32_t cols; int32_t dtype;             /* OEH_F16 | OEH_BF16 | OEH_F32: x, r, sum_out and y share it */
  int64_t x_stride, r_stride, sum_stride, y_stride;      /* elements between rows; columns are contiguous */
  float eps; int32_t reserved;
  oeh_fq fq_sum, fq_out;                                 /* either may be disabled */
} oeh_ln_desc;
int oeh_resid_ln_quant(const oeh_ln_desc* d, const void* x, const void* r /* may be NULL */, const float* gamma, const float* beta /* may be NULL */,
                       void* sum_out /* may be NULL */, void* y, uint8_t* sum_idx /* tests */, uint8_t* y_idx /* tests */, void* stream);
const char* oeh_resid_ln_variant(const oeh_ln_desc* d);  /* which launch form, or NULL if refused; host only */

/* The front of a quantised model (oeh_embed.hip): 1 <= n_tab <= 3 embedding lookups -> their sums, each behind its activation quantiser ->
 * LayerNorm -> output quantiser, ONE output row per (b, s) of a (B, S) id grid in ONE pass - QuantizedBertEmbeddings (quantized_bert.py:
 * 146-218: word + token type -> sum_input_token_type_embd_act_quantizer, += position -> sum_pos_embd_act_quantizer, LayerNorm) and the OPT
 * decoder front (quantized_opt.py:27-51, 549-569: embed_tokens + embed_positions -> embed_sum_act_quantizer, no LayerNorm), on tables the
 * reference fake-quantises as whole tensors (QuantEmbedding, autoquant_utils.py:75-95).  Inference only.
 * Lookup t reads row ids[b * id_stride_b + s * id_stride_s] (int32 or int64 elements; a stride may be 0: a (1, S) id tensor broadcast over
 * the batch) of its table, n_rows rows of `cols` contiguous elements row_stride elements apart.  ids == NULL, lookup 0 only: row b * S + s
 * ("dense rows": inputs_embeds).  A table row e_t arrives in one of three forms; with RN = rounding to `dtype`, every operation rounded on
 * its own, in this order:
 *   OEH_TAB_PLAIN  `dtype` elements taken as they are
 *   OEH_TAB_GRID   `dtype` elements w, the per-tensor symmetric weight grid applied to the gathered row with the rounding points of
 *                  SymmetricUniformQuantizer.forward's torch ops on a `dtype` tensor (uniform_quantizers.py:150-186): sc = RN(scale);
 *                  q = RN(w / sc) (a true division); i = clamp(rint(q), int_min, int_max) + 0; e = RN(sc * i)
 *   OEH_TAB_I8     int8 elements i, the grid's integers: sc = RN(scale); e = RN(sc * i).  The same bits as OEH_TAB_GRID on the table the
 *                  integers were taken from (+ 0 above: an integer is never -0, where torch's scale * round(-0.3) is) at a quarter of an
 *                  fp32 table's memory and gather traffic.
 * Then per row:  s = e_0;  for t = 1 .. n_tab - 1:  s = RN(s + e_t);  fq_sum[t] enabled: s = RN(scale * (clamp(rint(s / scale) + zero_point,
 * 0, qmax) - zero_point)), oeh_fake_quant's arithmetic.  sum_out (if given) <- the final s.  gamma == NULL: y <- the final s.  Otherwise the
 * LayerNorm of that s and fq_out exactly as oeh_resid_ln_quant defines them (moments, summation order per launch form, qmax up to 65535):
 * in the same launch form the two entry points give the same bits for the same s.  Bitwise reproducible.  The dump_idx fields are ignored:
 * sum_idx / y_idx (tests; dense (B * S, cols) uint8) receive the indices of fq_sum[n_tab - 1] / fq_out.
 * Ids are data: a row with an id outside [0, n_rows) reads nothing from any table, its y (and sum_out) row is written as NaN, its index dumps
 * are not written, and *bad_rows (if given; a device int32 the caller zeroes) is incremented by one.  Nothing synchronises.
 * Launch forms (oeh_embed_sum_variant: "embed/wave/CH4/T3/f32", "embed/block/CH4/T2/f16", "embed/scalar/CH1/T1/bf16" - form, accesses per
 * thread, lookups, storage type; host only, NULL if refused, thread-local storage): those of oeh_resid_ln_quant.  The 16-byte forms need every
 * `dtype` base pointer (tables, gamma, beta, sum_out, y) 16-byte aligned and cols, every table's row stride and the output strides multiples
 * of 4 (fp32) / 8 (16-bit) elements - an int8 table: base and row stride multiples of that many BYTES; otherwise element accesses.
 * Refusals, before any launch, in this order: OEH_EINVAL - d, y or a table NULL, n_tab outside 1..3, lookup t >= 1 without ids, cols < 1,
 * B or S < 0, a negative n_rows or stride, a stride of sum_out or y below cols with more than one row, a dtype, id_dtype or form code that
 * is none, a grid table with scale <= 0 (or not finite) or int_min >= int_max, an enabled quantiser that is no grid, an enabled fq_sum[0] or
 * fq_sum[t >= n_tab], fq_out, beta or y_idx without gamma, an index dump of a disabled quantiser, reserved != 0, eps < 0 or NaN with gamma
 * given; OEH_ENOTSUP - cols > 8192, B * S >= 2^31, an int8 table with int_min < -128 or int_max > 127, an index dump of a grid with
 * qmax > 255; OEH_EALIGN - ids off their element size, an int8 table off 4 bytes, a `dtype` pointer off its element size (gamma, beta: 4).
 * B * S == 0: OEH_OK without a launch. */
#define OEH_TAB_PLAIN 0
#define OEH_TAB_GRID 1
#define OEH_TAB_I8 2
#define OEH_ID_I32 0
#define OEH_ID_I64 1
typedef struct oeh_embed_lookup {
  const void* table;                    /* n_rows x cols, `dtype` (OEH_TAB_PLAIN, OEH_TAB_GRID) or int8 (OEH_TAB_I8) */
  const void* ids;                      /* NULL (lookup 0 only): dense rows */
  int64_t n_rows, row_stride;           /* row_stride in elements of the table */
  int64_t id_stride_b, id_stride_s;     /* in id elements; 0 broadcasts */
  int32_t id_dtype, form;               /* OEH_ID_*, OEH_TAB_* */
  float scale, int_min, int_max;        /* the weight grid of OEH_TAB_GRID / OEH_TAB_I8 */
  int32_t reserved;
} oeh_embed_lookup;
typedef struct oeh_embed_desc {
  int32_t B, S, cols, dtype;            /* OEH_F16 | OEH_BF16 | OEH_F32: the float tables, sum_out and y share it */
  int32_t n_tab, reserved;
  int64_t sum_stride, y_stride;         /* elements between rows */
  float eps; int32_t reserved2;
  oeh_embed_lookup tab[3];
  oeh_fq fq_sum[3];                     /* [t]: behind the add of lookup t; [0] stays disabled */
  oeh_fq fq_out;
} oeh_embed_desc;
int oeh_embed_sum_quant(const oeh_embed_desc* d, const float* gamma /* may be NULL */, const float* beta /* may be NULL */, void* sum_out /* may be NULL */,
                        void* y, uint8_t* sum_idx /* tests */, uint8_t* y_idx /* tests */, int32_t* bad_rows /* may be NULL */, void* stream);
const char* oeh_embed_sum_variant(const oeh_embed_desc* d);  /* which launch form for d's pointers and strides, or NULL if refused; host only */

/* Cross-entropy over a vocabulary (oeh_xent.hip): the loss both language models end in - CrossEntropyLoss on the shifted logits
 * (quantized_opt.py:868-877), on -100 labels (quantized_bert.py:910-915), exp(mean of the batch losses) as perplexity (validate_clm.py:
 * 556-594), label_smoothing (run_vit.py) - with every logit read ONCE forward, and read once and written once backward.
 * logits: a (B, S, V) view, element (b, s, j) at logits[b * x_stride[0] + s * x_stride[1] + j]; labels: a (B, S) view of int32 or int64
 * with label_stride.  The reference's shift is logits as they are with S - 1 rows per batch and labels + 1: no copy.  A row may start at
 * any element; it is read with 16-byte loads on its own 16-byte boundaries, and nothing outside [row, row + V) is read except inside the
 * 16-byte slots that hold the row's first and last element.
 * Forward, per row with label y (fp32 arithmetic, bitwise reproducible, a fixed order of every sum):
 *   lse = M + log(L),  M = max_j x_j,  L = sum_j exp(x_j - M) by an online (max, sum) per thread, merged over the workgroup
 *   row_loss = lse - x_y                                              one fp32 subtraction
 *   label_smoothing = e > 0:  row_loss = (1 - e) * (lse - x_y) + e * (lse - sum_j x_j / V)       torch's definition
 *   y == ignore_index: no logit is read, lse = row_loss = 0, the row is not counted
 *   y outside [0, V) otherwise (found before any address is formed): lse = row_loss = NaN, the row IS counted
 * then ONE more launch of one workgroup: out2[0] = the float64 sum of the counted rows' fp32 losses, out2[1] = their number,
 * *mean = fp32(out2[0] / out2[1]) (NaN without a counted row, as torch), meter (if given; a device double[2] the caller zeroes once):
 * meter[0] += out2[0] / out2[1]; meter[1] += 1 - what validate_clm.py:561-591 accumulates on the host, so that a validation run needs
 * one device-to-host copy at its end; *bad_rows (if given; a device int32 the caller zeroes) += the number of rows with a label that
 * is none.  lse and row_loss: B * S fp32 values, row b * S + s.  row_loss may be NULL without label smoothing: the reduce launch then
 * forms lse - x_y itself (the same bits).  No atomics, no allocation, no host synchronisation.  B * S == 0: the reduce launch alone
 * (sum 0, count 0, mean NaN).
 * Backward, per element:  dlogits[j] = RN_dtype((exp(x_j - lse) - (1 - e) * [j == y] - e / V) * g), each operation rounded on its own,
 * the third term only with smoothing; g = grad[row * grad_stride] (fp32, read on the device; grad_stride == 0 broadcasts one scalar),
 * with mean_reduction != 0 g = fp32(g / out2[1]).  lse and out2 are the forward's.  An ignored row is written as zeros without reading
 * its logits, a row with a label that is none as NaN.  dlogits has the logits' dtype and dx_stride; it may BE logits (the same pointer and
 * strides: every thread reads its elements before it writes them), otherwise the two must not overlap.  Stores are 16 bytes wide when
 * every dlogits row sits as far from a 16-byte boundary as its logits row, else per element (variant name ends in "/el").
 * oeh_xent_variant: "xent/block/CH4/f16", "xent/block/CH4/f32/ls", "xent/block/CH4/bf16/ls/el" - one 256-thread workgroup per row, CH
 * (= OEH_XENT_SLOTS) 16-byte slots per thread and loop step, i.e. 256 * CH * (4 fp32 | 8 16-bit) elements per step; "/el" only with
 * dlogits given.  Host only, NULL if refused, thread-local storage.
 * Refusals, before any launch, in this order: OEH_EINVAL - d, logits, labels, lse or out2 NULL (backward: grad or dlogits too), row_loss
 * NULL with label smoothing, V < 1, B or S < 0, a dtype other than OEH_F16 / OEH_BF16 / OEH_F32, a label_dtype that is none, a negative
 * stride, a dx_stride below V with more than one row along it (backward), label_smoothing outside [0, 1) or NaN, reserved != 0;
 * OEH_ENOTSUP - B * S >= 2^31; OEH_EALIGN - logits or dlogits off their element size, labels off theirs, lse / row_loss / mean / grad /
 * bad_rows off 4 bytes, out2 / meter off 8 bytes. */
#define OEH_XENT_SLOTS 4
typedef struct oeh_xent_desc {
  int32_t B, S, V, dtype;              /* OEH_F16 | OEH_BF16 | OEH_F32: logits and dlogits */
  int32_t label_dtype, mean_reduction; /* OEH_ID_I32 | OEH_ID_I64;  backward: divide grad by out2[1] */
  int64_t x_stride[2], label_stride[2], dx_stride[2];   /* elements: batch, row */
  int64_t ignore_index;
  float label_smoothing; int32_t reserved;
} oeh_xent_desc;
int oeh_xent_fwd(const oeh_xent_desc* d, const void* logits, const void* labels, float* lse, float* row_loss /* may be NULL */,
                 double* out2, float* mean /* may be NULL */, double* meter /* may be NULL */, int32_t* bad_rows /* may be NULL */, void* stream);
int oeh_xent_bwd(const oeh_xent_desc* d, const void* logits, const void* labels, const float* lse, const double* out2,
                 const float* grad, int64_t grad_stride, void* dlogits, void* stream);
const char* oeh_xent_variant(const oeh_xent_desc* d, const void* logits, const void* dlogits /* may be NULL */);

/* The tail of a transformer block in training (oeh_ln_train.hip): dropout -> residual add -> LayerNorm on the rows of a (rows, cols)
 * array, forward in ONE pass and backward in one pass plus a column reduction - dense -> dropout -> + input -> LayerNorm of BertSelfOutput
 * / BertOutput (the fp32 shape of quantized_bert.py:541-606) and residual + dropout(h) in front of the next LayerNorm of the OPT decoder
 * layer (quantized_opt.py:277-384), whose residual stream is sum_out.
 * Every row tensor has `dtype` and contiguous columns; element (i, j) sits at base[i * stride + j].  The descriptor's strides belong to
 * x, r, sum_out, y in the forward and to dx, dr, s, dy (and dsum_stride to dsum) in the backward.  gamma, beta, mean, rstd, dgamma, dbeta: fp32.
 * Forward, per element (i, j), every operation rounded on its own, in this order:
 *   d = keep(i, j) ? fp32(x) * inv : 0        inv = 1 / (1 - p), formed once in fp32; p == 0: d = fp32(x), no generator work
 *   s = RN_dtype(d + fp32(r))                 one rounding to the storage type; r == NULL: s = RN_dtype(d)
 *   sum_out <- s                              required: the backward reads it, and pre-LN blocks carry it on as the residual stream
 *   y = ((s - mean) * rstd) * gamma + beta from the stored s exactly as oeh_resid_ln_quant defines it without quantisers (its fp32 moments,
 *   the same summation order per launch form: with p == 0 the two entry points give the same bits)
 *   mean[i], rstd[i] <- the row's mean and 1 / sqrt(var + eps) formed in float64 and rounded to fp32 once: what the backward reads
 * Keep bit: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32), counter (j >> 2, i & 0xffffffff, i >> 32, 1), output word j & 3:
 * kept iff word >= floor(p * 2^32).  The fourth counter word is 1 where attention dropout's is 0 (oeh_dropout): one seed serves both
 * without a shared stream.  The mask depends on (seed, i, j) only - not on the launch form, not on strides.
 * oeh_drop_resid_ln_mask: the dense (rows, cols) keep mask (1 kept, 0 dropped) of d's rows, cols and drop from the same generator.
 * Backward, from the forward's s, mean, rstd and drop, per row in fp32:
 *   xhat = (s - mean) * rstd;  g = dy * gamma;  c1 = sum(g) / cols;  c2 = sum(g * xhat) / cols
 *   ds = rstd * ((g - c1) - xhat * c2);  dsum given (the gradient that arrived on sum_out): ds = ds + fp32(dsum)
 *   dr (if given) <- RN_dtype(ds);  dx <- RN_dtype(keep(i, j) ? ds * inv : 0)
 *   dgamma[j] = sum_i dy * xhat;  dbeta[j] (if given) = sum_i dy        both summed in float64 and rounded once to fp32, with xhat for
 *   THESE sums from a mean and rstd = 1 / sqrt(var + eps) the kernel forms again from s in float64 (eps: the forward's): an entry that one
 *   row dominates would otherwise carry the rounding of that row's fp32 rstd
 * Two kernels, no atomics, bitwise reproducible: the row kernel runs at most OEH_LN_TRAIN_MAX_GROUPS workgroups (two per CU), each of which -
 * in the one-wave-per-row form each of its four waves - walks a contiguous slab of rows with its columns' two sums in registers and leaves
 * one (2, cols) float64 partial in `work`; the column kernel adds the partials in a fixed order.  work: oeh_drop_resid_ln_bwd_work_bytes(d)
 * bytes (a multiple of 16; 0 for a refused descriptor), 8-byte aligned, the caller's, not shared between streams.
 * Aliasing: sum_out may be r, y may be x, dx may be dy, dr may be dsum - each pair with equal row strides; anything else must not overlap.
 * Launch forms: those of oeh_resid_ln_quant, with its alignment rule over every given row tensor, gamma, beta (and the backward's work).
 * oeh_drop_resid_ln_variant: "ln_train/fwd/wave/CH2/f16/drop", "ln_train/bwd/block/CH8/f32/G512x2" (backward: workgroups x rows per
 * slab); host only, NULL if refused, thread-local storage; it takes every optional tensor as given and 16-byte aligned.
 * Refusals, before any launch: OEH_EINVAL - p outside [0, 1) or NaN or drop.reserved != 0 (checked first), then d or a required pointer
 * NULL (forward: x, gamma, sum_out, y, mean, rstd; backward: dy, s, gamma, mean, rstd, dx, dgamma, work), cols < 1, rows < 0, a dtype other
 * than OEH_F16 / OEH_BF16 / OEH_F32, eps < 0 or NaN, reserved != 0, a negative stride, a stride of an output (sum_out, y; dx, dr) below
 * cols with rows > 1; OEH_ENOTSUP - cols > 8192, rows >= 2^31.  rows == 0: OEH_OK without a launch; the backward still zeroes dgamma and
 * dbeta. */
#define OEH_LN_TRAIN_MAX_GROUPS 512
typedef struct oeh_ln_train_desc {
  int64_t rows; int32_t cols; int32_t dtype;           /* OEH_F16 | OEH_BF16 | OEH_F32 */
  int64_t x_stride, r_stride, sum_stride, y_stride;    /* forward: x, r, sum_out, y;  backward: dx, dr, s, dy */
  int64_t dsum_stride;                                 /* backward only */
  float eps; int32_t reserved;
  oeh_dropout drop;                                    /* p == 0: no dropout */
} oeh_ln_train_desc;
int oeh_drop_resid_ln_fwd(const oeh_ln_train_desc* d, const void* x, const void* r /* may be NULL */, const float* gamma, const float* beta /* may be NULL */,
                          void* sum_out, void* y, float* mean, float* rstd, void* stream);
size_t oeh_drop_resid_ln_bwd_work_bytes(const oeh_ln_train_desc* d);
int oeh_drop_resid_ln_bwd(const oeh_ln_train_desc* d, const void* dy, const void* dsum /* may be NULL */, const void* s, const float* gamma,
                          const float* mean, const float* rstd, void* dx, void* dr /* may be NULL */, float* dgamma, float* dbeta /* may be NULL */,
                          void* work, void* stream);
int oeh_drop_resid_ln_mask(const oeh_ln_train_desc* d, uint8_t* keep /* dense (rows, cols) */, void* stream);   /* tests */
const char* oeh_drop_resid_ln_variant(const oeh_ln_train_desc* d, int backward);   /* host only, NULL if refused */

/* The softmax rows of the unfused attention path in training (oeh_softmax_train.hip): scale -> additive mask -> clamp -> softmax /
 * softmax_1 -> clip -> dropout over (B,H,Sq,Sk) scores in ONE pass, and a backward that recomputes the probabilities from the scores and
 * two fp32 numbers per row - the span of attention.unfused_core between the score product and the product with V (opt_attention.py:215-224
 * with the clamp, bert_attention.py:265-292), and softmax.softmax_autograd on plain (rows, cols) data (B = H = 1).
 * A row is (b, h, i); element j of a tensor t sits at t[b * stride[0] + h * stride[1] + i * stride[2] + j] (element strides, the last
 * dimension contiguous).  x and dx have x_dtype; y, u, dy and du have y_dtype (x_dtype, or OEH_F32: what torch.result_type gives fp16 scores
 * under an fp32 mask); the mask has mask_dtype and any of its strides may be 0 ((B,1,1,Sk), (B,1,Sq,Sk), (1,1,Sq,Sk)).
 * Forward, per row in fp32, every operation rounded on its own:
 *   z = fp32(x) * scale, or fp32(x) / scale_div when scale_div > 0 (as oeh_attn_desc);  z = z + fp32(mask);  clamp: z = max(z, clamp_min)
 *   m = max_j z;  e = exp(z - m);  den = sum e (softmax_1: + exp(-m));  p = e / den - oeh_softmax_rows' arithmetic and, per launch form, its
 *   order of summation: without scale, mask, clamp and dropout and with y_dtype == x_dtype, y has oeh_softmax_rows' bits; den = inf: p = 0
 *   clip: y = clamp(p * (eta - gamma) + gamma, 0, 1);  y <- RN_y_dtype(y);  u <- RN_y_dtype(keep ? fp32(stored y) * inv : 0), inv = 1 / (1 - p_drop)
 *   in fp32: nn.Dropout on the stored probabilities.  stats[row] <- (m, den) as formed (no lse: an fp32 lse loses log(den) on a saturated row).
 * Keep bit: the ATTENTION dropout stream of oeh_dropout - counter (j >> 2, i, b * H + h, 0), word j & 3, kept iff word >= floor(p * 2^32):
 * one seed gives this path and the fused attention kernels the same mask (oeh_attn_dropout_mask).
 * At least one of y, u; u only with p_drop > 0.
 * Backward, from x, mask, stats and the descriptor (nothing else of size Sq x Sk from the forward), per row in fp32:
 *   z, p = exp(z - m) / den as above - the forward's fp32 p bit for bit;  g = fp32(dy) + (keep ? fp32(du) * inv : 0), either may be NULL
 *   clip: g = (eta - gamma) * g where 0 <= p * (eta - gamma) + gamma <= 1 (closed, torch.clip), else 0
 *   delta = sum_j p g;  dz = p * (g - delta);  clamp: dz *= 1 above the floor, 0 below, 1/2 at a tie (torch.max);  dx <- RN_x_dtype(dz * scale
 *   or dz / scale_div)
 * A row with den = inf (softmax_1 below the exp range, a fully masked softmax_1 row): p = 0, dx = 0 - where the torch chain has a NaN at
 * the maximum's position; the fused attention backward's convention.  A row with a NaN (or +inf) z: stats, y, u and dx of that row are NaN.
 * No atomics: every sum by one wave's butterflies or the fixed four-wave step behind them; two calls are bitwise equal.
 * Launch forms (oeh_softmax_train_variant: "softmax_train/fwd/lanes/G4x8/f16/softmax1/clip/mask/clamp/drop", ".../wave/CH2/...",
 * ".../block/..."; f16>f32: y_dtype differs): lanes - the row over G lanes of a wave, 64 / G rows per wave: rows of up to 32 of x's 16-byte
 * vectors with one vector per lane (Sk <= 256 16-bit / 128 fp32 elements), and Sk <= 64 with one element per lane where Sk is no multiple
 * of the vector or a row of a given tensor is off 16 bytes; wave - one wave per row in registers, 16-byte accesses, up to 512 vectors (4096
 * 16-bit / 2048 fp32 elements); block - a workgroup per row staged in LDS, everything else.  The variant function takes y / dy as given, u / du with p_drop > 0, a mask where mask_dtype is a storage type, and
 * every pointer as 16-byte aligned; host only, thread-local storage.
 * Refusals, before any launch: OEH_EINVAL - p_drop outside [0, 1) or NaN, drop.reserved or reserved != 0 (checked first); desc, x, stats
 * (backward: dx) NULL; neither y nor u, u (du) with p_drop == 0; the backward with neither dy nor du; a dtype that is none of the three
 * (mask_dtype only with a mask), y_dtype neither x_dtype nor OEH_F32; Sk < 1, a negative extent or stride; a stride of an output (y, u; dx)
 * below Sk in a dimension of extent > 1; a bad softmax_base; clip with eta <= gamma; scale_div < 0 or NaN; NaN scale, gamma or eta.
 * OEH_ENOTSUP - Sk > OEH_SOFTMAX_TRAIN_MAX_COLS, B * H * Sq >= 2^31.  B * H * Sq == 0: OEH_OK without a launch. */
#define OEH_SOFTMAX_TRAIN_MAX_COLS 15872
typedef struct oeh_softmax_train_desc {
  int32_t B, H, Sq, Sk;
  int32_t x_dtype, y_dtype, mask_dtype;                /* OEH_F16 | OEH_BF16 | OEH_F32 */
  int32_t softmax_base, clip;
  float gamma, eta;
  float scale, scale_div;
  int32_t clamp; float clamp_min;
  int32_t reserved;
  int64_t x_stride[3], y_stride[3], u_stride[3], mask_stride[3];
  int64_t dy_stride[3], du_stride[3], dx_stride[3];   /* backward only */
  oeh_dropout drop;                                    /* p == 0: no dropout */
} oeh_softmax_train_desc;
int oeh_softmax_train_fwd(const oeh_softmax_train_desc* d, const void* x, const void* mask /* may be NULL */, void* y /* may be NULL */,
                          void* u /* may be NULL */, float* stats, void* stream);
int oeh_softmax_train_bwd(const oeh_softmax_train_desc* d, const void* x, const void* mask /* may be NULL */, const float* stats,
                          const void* dy /* may be NULL */, const void* du /* may be NULL */, void* dx, void* stream);
const char* oeh_softmax_train_variant(const oeh_softmax_train_desc* d, int backward);   /* host only, NULL if refused */

/* The optimizer phase of a training step (oeh_optim.hip): the global gradient norm with its clip coefficient, and a decoupled-weight-decay
 * Adam step over ALL parameter tensors of a model in one launch - what the reference's loops do after backward()
 * (run_clm.py:440-462 torch.optim.AdamW over a decay and a no-decay group, :589-601 accelerator.clip_grad_norm_ then optimizer.step()).
 * A call works on a PLAN: a table the host builds once from the tensor list, copies to the device and reuses while the pointers stay the same.
 *   oeh_mt_plan(t, n_tensors, plan_host, n_chunks): host only.  Writes oeh_mt_plan_bytes(t, n_tensors) bytes into plan_host (8-byte
 *   aligned; NULL: only *n_chunks is formed): first one 16-byte chunk entry per workgroup {int32 tensor, int32 count, int64 offset} - tensor
 *   i's elements [offset, offset + count), count <= OEH_MT_CHUNK, the tensors in the order given and a tensor's chunks ascending - then one
 *   56-byte record per tensor {p, g, m, v, int64 n, int32 g_dtype, int32 group, int32 vec16, int32 0}.  A tensor with n == 0 has a record and
 *   no chunk.  Offsets are 64-bit throughout.
 *   p, m, v: fp32.  g: g_dtype (OEH_F16 | OEH_BF16 | OEH_F32).  group: which column of oeh_adamw_desc the tensor is stepped with.
 *   A tensor takes the 16-byte form ("vec16") when p, m and v are 16-byte aligned and g is aligned to four of its elements (16 bytes fp32,
 *   8 bytes 16-bit): thread t of a chunk owns the elements [4 (k * 256 + t), + 4), k = 0..3, as one access per tensor.  The ragged end of a
 *   vec16 tensor's last chunk is done by the same kernel element by element.  Any other tensor takes the element form ("elem"): one element
 *   per access.  Both forms compute the same bits.  oeh_mt_variant: which one, NULL for a refused tensor; host only.
 *   Refusals: OEH_EINVAL - t NULL with n_tensors > 0, n_tensors < 0, n_chunks NULL, n < 0, a NULL p / g / m / v, group outside
 *   [0, OEH_MT_MAX_GROUPS), a g_dtype that is none of the three; OEH_EALIGN - p, m or v off 4 bytes, g off its element size; OEH_ENOTSUP -
 *   2^31 or more chunks.  oeh_mt_plan_bytes: -1 for a refused list.
 * oeh_grad_norm: two launches.  One workgroup per chunk writes the float64 partial sum of (double)g * (double)g (every product exact) into
 *   work (oeh_grad_norm_work_bytes(n_chunks) bytes, 8-byte aligned); one workgroup of 1024 threads then adds the partials - thread t the
 *   partials t, t + 1024, ... ascending, the wave butterflies, the 16 waves as a pairwise tree - and writes
 *     out4 = {sumsq, norm = sqrt(sumsq), coef, 0},  coef = min(1, max_norm / (norm + 1e-6)) in float64 (torch's clip_grad_norm_)
 *   max_norm <= 0, NaN or +inf: coef = 1.  A non-finite gradient gives a non-finite sumsq and the coef that formula then gives (NaN for NaN):
 *   torch's error_if_nonfinite=False.  No atomics: the same bits on every call.  n_chunks == 0: the second launch alone, sumsq = 0.
 * oeh_grad_scale: g <- RN_dtype(fp32(g) * c) in place, c = clip4[2] rounded to fp32 once; clip4 is device memory (an out4).
 * oeh_adamw_step: one launch over the chunks.  c = clip4[2] rounded to fp32 once (clip4 NULL: c = 1, nothing read).  Per element in fp32,
 *   every operation rounded on its own, `/` and sqrt correctly rounded, denormals kept; RN32: a constant the host forms in double from the
 *   descriptor's fp32 fields and rounds to fp32 once; t = step[group], the step number AFTER the increment (torch's), the powers by pow():
 *     g' = fp32(g) * c
 *     p1 = p * RN32(1 - lr * wd)
 *     m' = m + (g' - m) * RN32(1 - beta1)
 *     v' = v * beta2 + (g' * g') * RN32(1 - beta2)
 *     den = sqrt(v') / RN32(sqrt(1 - beta2^t)) + eps
 *     p' = p1 - RN32(lr / (1 - beta1^t)) * (m' / den)
 *   p, m, v are written; g is NOT (the clip is folded in: the difference from torch's clip_grad_norm_ + step pair).  A thread reads its
 *   elements of a chunk before it writes them.  Tensors of a plan must not overlap each other.
 *   Refusals: OEH_EINVAL - d NULL, n_groups outside [1, OEH_MT_MAX_GROUPS], reserved != 0, and for a group below n_groups: step < 1, lr, eps
 *   or weight_decay negative or NaN, a beta outside [0, 1); n_chunks < 0; plan_dev NULL with n_chunks > 0 (all three entry points; oeh_grad_norm:
 *   out4 NULL, work NULL with n_chunks > 0; oeh_grad_scale: clip4 NULL); OEH_EALIGN - work, out4 or clip4 off 8 bytes; OEH_ENOTSUP - n_chunks >= 2^31.
 *   n_chunks == 0: OEH_OK without a launch (oeh_adamw_step, oeh_grad_scale).  The plan lives on the device and is not looked at by the host: a
 *   tensor whose group is not below n_groups is no refusal - the kernel leaves its p, m and v untouched.
 *   oeh_grad_norm and oeh_grad_scale read and write g alone.  A caller who plans for them only still has to name p, m and v (NULL is
 *   refused): any 4-byte aligned addresses serve, 16-byte aligned ones leave the access form to g; such a plan must not be stepped. */
#define OEH_MT_CHUNK 4096        /* elements of one tensor covered by one workgroup */
#define OEH_MT_MAX_GROUPS 8
#define OEH_MT_ENTRY_BYTES 16
#define OEH_MT_RECORD_BYTES 56
typedef struct oeh_mt_tensor {
  void* p; const void* g; void* m; void* v;
  int64_t n; int32_t g_dtype; int32_t group;
} oeh_mt_tensor;
typedef struct oeh_adamw_desc {
  float lr[8], beta1[8], beta2[8], eps[8], weight_decay[8];
  int64_t step[8];
  int32_t n_groups, reserved;
} oeh_adamw_desc;
int64_t oeh_mt_plan_bytes(const oeh_mt_tensor* t, int32_t n_tensors);                                        /* host only */
int oeh_mt_plan(const oeh_mt_tensor* t, int32_t n_tensors, void* plan_host /* may be NULL */, int64_t* n_chunks);   /* host only */
const char* oeh_mt_variant(const oeh_mt_tensor* t);                                                          /* host only */
int64_t oeh_grad_norm_work_bytes(int64_t n_chunks);
int oeh_grad_norm(const void* plan_dev, int64_t n_chunks, double max_norm, void* work, double* out4, void* stream);
int oeh_grad_scale(const void* plan_dev, int64_t n_chunks, const double* clip4, void* stream);
int oeh_adamw_step(const void* plan_dev, int64_t n_chunks, const oeh_adamw_desc* d, const double* clip4 /* may be NULL */, void* stream);

/* The same phase under fp16 loss scaling (run_clm.py:587-606, a GradScaler loop): the unscale is folded into the clip coefficient, the
 * overflow check is the norm's own float64 sum, a skipped step is one uniform early return, and the step counters live on the device -
 * whether a step was skipped is known only there.  Nothing here reads anything back.
 * oeh_grad_norm_amp: oeh_grad_norm's two launches (the same per-chunk partials pass, then a finalize of the same sum).  grad_scale, found_in
 *   and found_acc are device pointers to one fp32 each; each may be NULL.  With s = (double)*grad_scale (NULL: 1) and
 *     found = !isfinite(sumsq) || (found_in && *found_in != 0) || !(s > 0 && isfinite(s))
 *   the finalize writes
 *     out4 = {sumsq of the gradients as stored, norm = sqrt(sumsq) / s, coef = clipc / s, found ? 1.0 : 0.0}
 *   clipc = min(1, max_norm / (norm + 1e-6)) from THAT norm, 1 for max_norm <= 0, NaN or +inf.  A power-of-two s changes neither norm nor
 *   clipc by a bit.  If found and found_acc is not NULL the one finalizing thread stores *found_acc = 1.0f; nothing is stored there
 *   otherwise (several optimizers may share one accumulator: it holds the OR of their flags).
 *   Refusals: oeh_grad_norm's, and OEH_EALIGN for grad_scale, found_in or found_acc off 4 bytes.
 * oeh_adamw_step_amp: two launches, `advance` then `step`.  d->step[] is not read: the counters are steps[], fp32 and integer-valued on the
 *   device (torch's fused / capturable convention), and slot[i] (int32, device) is the counter of plan record i.  No two records may share
 *   a slot - the device cannot tell.  clip4 is required: an out4 of oeh_grad_norm_amp.  work: oeh_adamw_amp_work_bytes(n_tensors) = 8
 *   bytes per record, 4-byte aligned, device.
 *   advance: one thread per record i, j = slot[i].  A record whose group is not below n_groups is left alone, counter included.  Otherwise
 *     t = steps[j] + (clip4[3] != 0 ? 0 : 1);  steps[j] = t is stored only when clip4[3] == 0;
 *     work[i] = {bc2 = RN32(sqrt(1 - pw(beta2, t))), ss = RN32(lr / (1 - pw(beta1, t)))}   (two fp32; zeros when t < 1)
 *   in double from the descriptor's fp32 fields, plain `/` and sqrt, and pw binary exponentiation - IEEE multiplications only:
 *     r = 1; base = beta; n = (int64)t;  while (n) { if (n & 1) r *= base;  n >>= 1;  if (n) base *= base; }
 *   It depends on t alone: a resumed run equals an uninterrupted one.
 *   step: if (clip4[3] != 0) return; first - uniform, one scalar load: on a skipped step p, m and v are neither read nor written.  Then
 *   oeh_adamw_step's arithmetic, operation for operation, with bc2 and ss from work[record] and c = clip4[2] rounded to fp32 once; the
 *   other five constants are the host's, as there.
 *   Refusals: oeh_adamw_step's without the step < 1 rule; OEH_EINVAL - n_tensors < 0, or clip4, steps, slot or work NULL with n_chunks > 0;
 *   OEH_EALIGN - clip4 off 8 bytes, steps, slot or work off 4.  n_chunks == 0: OEH_OK without a launch.
 * oeh_loss_scale_update: state4 = {scale, growth_tracker, found, skipped}, four fp32 on the device, integer-valued where they count.  One
 *   thread applies torch's _amp_update_scale_ rule:
 *     found != 0:               scale = RN32(scale * (float)backoff_factor), tracker = 0, skipped += 1
 *     tracker + 1 == interval:  ns = RN32(scale * (float)growth_factor); scale = ns when ns is finite; tracker = 0
 *     otherwise:                tracker += 1
 *   and then found = 0.  Refusals: OEH_EINVAL - state4 NULL, a factor that is not positive and finite, growth_interval < 1; OEH_EALIGN -
 *   state4 off 4 bytes. */
int oeh_grad_norm_amp(const void* plan_dev, int64_t n_chunks, double max_norm, const float* grad_scale /* may be NULL */,
                      const float* found_in /* may be NULL */, float* found_acc /* may be NULL */, void* work, double* out4, void* stream);
int64_t oeh_adamw_amp_work_bytes(int32_t n_tensors);
int oeh_adamw_step_amp(const void* plan_dev, int64_t n_chunks, int32_t n_tensors, const oeh_adamw_desc* d, const double* clip4, float* steps,
                       const int32_t* slot, void* work, void* stream);
int oeh_loss_scale_update(float* state4, double growth_factor, double backoff_factor, int32_t growth_interval, void* stream);

/* The conditional per-token gate in TRAINING (oeh_gate_train.hip): the per-head predictors, the sigmoid and the product with the context in
 * one entry point per direction - what attention.gate_autograd (H small Linear / Linear-ReLU-Linear modules on strided slices, stack,
 * sigmoid) and attention.gated_merge (context * gate) do as torch ops, with autograd's chain behind them (bert_attention.py:294-331).
 * hidden (B,T,H*d): element strides for batch and token, last dimension contiguous.  ctx (B,H,T,d) and dctx by (batch, head, token) element
 * strides; out, dout and dhidden (B,T,H*d) by (batch, token) strides.  All five have `dtype`.  The predictor weights are fp32 device arrays
 * laid out as for oeh_gate_fwd (units == 0: w1 (H,d), b1 (H); units = m > 0: w1 (H,m,d), b1 (H,m), w2 (H,m), b2 (H)).
 * Forward (two launches): gate_out (B,H,T) fp32 contiguous <- sigmoid(logit) WITHOUT the scaling - oeh_gate_fwd's own launch with scaling 1,
 *   so its bits; out[b, t, h d + j] <- RN_dtype(fp32(ctx[b,h,t,j]) * (gate_out[b,h,t] * scaling)).
 * Backward (two launches), s = scaling:
 *   dctx <- RN_dtype(fp32(dout) * (gate_out * s)): the forward's product applied to dout, fp32, one rounding.
 *   Everything that feeds a sum over tokens is formed in FLOAT64 from the stored inputs, each operation rounded on its own:
 *     dot = sum_j dout_j * ctx_j, j ascending (the products are exact);  the logit z once more from hidden (nothing of the hidden layer is
 *     stored): units == 0: z = sum_k x_k w1[h][k] + b1[h], k ascending;  units > 0: a_j = sum_k x_k w1[h][j][k], u_j = a_j + b1_j,
 *     r_j = max(u_j, 0), z = sum_j r_j w2_j + b2, j ascending;  pi = 1 / (1 + exp(-z));  dz = ((s * dot) * pi) * (1 - pi)
 *   units == 0:  dw1[h] = sum_{b,t} dz * x;  db1[h] = sum dz;  dhidden_h = RN_fp32(dz) * w1[h]
 *   units  > 0:  dw2_j = sum dz * r_j;  db2 = sum dz;  dw1[j] = w2_j * sum [u_j > 0] dz * x;  db1_j = w2_j * sum [u_j > 0] dz (the ReLU passes
 *                nothing at 0, as torch's);  dhidden_h = sum_j da_j * w1[j] in fp32, j ascending, da_j = [u_j > 0] RN_fp32(dz) * w2_j
 *   dhidden (may be NULL: skipped, the other outputs keep their bits) <- RN_dtype.  The sums over (b, t): a workgroup (one wave, 64 tokens
 *   of one head per tile) walks `tiles per workgroup` consecutive tiles and adds its tokens in ascending order in float64, then leaves ONE
 *   record per head in `work`; at most OEH_GATE_TRAIN_MAX_GROUPS workgroups per launch.  The second launch adds the records of an output
 *   element over the workgroups - 16 slices of the list, each in ascending order, then a pairwise tree - in float64 and rounds to fp32
 *   once: each parameter gradient is the fp32 number next to the float64 result.  No atomics: two calls give the same bits.
 *   (A per-token chain in fp32 in front of float64 sums was measured first: a sum of n fp32 dz values carries the square root of n of
 *   their roundings, several times what a CPU fp32 evaluation of a one-element output happens to be off by - DESIGN.md 20.  The pi formed
 *   here differs from the stored gate_out by that one's fp32 rounding; dctx uses the stored one.)
 * work: oeh_gate_apply_bwd_work_bytes(B, T, H, d, units) bytes (or a negative OEH_E* code), 8-byte aligned, the caller's, one per stream.
 * oeh_gate_apply_variant: "gate_train/fwd/D64/M16/f16", "gate_train/bwd/D64/M16/f16/G64x2" (backward: workgroups per head x tiles per
 * workgroup); host only, NULL if refused, thread-local storage; every pointer taken as given and aligned.
 * Refusals, before any launch, in this order: OEH_EINVAL - d or a required pointer NULL (forward: hidden, w1, b1, ctx, gate_out, out;
 * backward: dout, ctx, hidden, gate_out, w1, b1, dctx, dw1, db1, work; with units > 0 also w2, b2 and backward dw2, db2), B, T, H or d < 1,
 * units < 0, a dtype that is none of the three, reserved != 0, a negative stride, a scaling that is not finite; OEH_ENOTSUP - d not 32 or
 * 64, units > 64, H > 65535 (the head is a grid dimension), B * T * H >= 2^31; OEH_EALIGN - a row of hidden, ctx, out / dout, dctx or dhidden (pointer or stride) off 16 bytes, work
 * off 8 bytes. */
#define OEH_GATE_TRAIN_MAX_GROUPS 1024
typedef struct oeh_gate_train_desc {
  int32_t B, T, H, d;
  int32_t units; int32_t dtype;                        /* OEH_F16 | OEH_BF16 | OEH_F32 */
  float scaling; int32_t reserved;
  int64_t hidden_stride[2];                            /* batch, token */
  int64_t ctx_stride[3];                               /* batch, head, token */
  int64_t out_stride[2];                               /* forward: out;  backward: dout */
  int64_t dctx_stride[3], dhidden_stride[2];           /* backward only */
} oeh_gate_train_desc;
int oeh_gate_apply_fwd(const oeh_gate_train_desc* d, const void* hidden, const float* w1, const float* b1, const float* w2 /* units > 0 */,
                       const float* b2 /* units > 0 */, const void* ctx, float* gate_out, void* out, void* stream);
int64_t oeh_gate_apply_bwd_work_bytes(int32_t B, int32_t T, int32_t H, int32_t d, int32_t units);
int oeh_gate_apply_bwd(const oeh_gate_train_desc* d, const void* dout, const void* ctx, const void* hidden, const float* gate_out, const float* w1,
                       const float* b1, const float* w2, const float* b2, void* dctx, void* dhidden /* may be NULL */, float* dw1, float* db1,
                       float* dw2, float* db2, void* work, void* stream);
const char* oeh_gate_apply_variant(const oeh_gate_train_desc* d, int backward);   /* host only, NULL if refused */

/* library information (host side, no device work) */
int oeh_abi_version(void);
const char* oeh_build_info(void);       /* "gfx950 hipcc <version> ..." */
const char* oeh_strerror(int code);
/* name of the kernel variant oeh_attn_fwd would launch for `desc` ("flash16/MQ2/D64/f16" one-pass kernel,
 * "fast16/NT32/D64/f16/clip" full-row kernel, "mfma16/NT32/D64/f16/fq" general kernel, "generic") or NULL if
 * unsupported; host only.  The returned string lives in thread-local storage until the next call on this thread. */
const char* oeh_attn_variant(const oeh_attn_desc* desc, const oeh_fq_desc* fq);
#ifdef __cplusplus
}
#endif
#endif /* OEH_H_ */
