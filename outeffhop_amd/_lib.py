"""ctypes binding of liboeh_hip.so (C ABI: include/oeh.h).

The HIP library IS the product path: if it cannot be loaded this module raises - there is no CPU or
PyTorch fallback behind any op in this package.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OEH_LIB: explicit path of another build of the same library (A/B timing of compiler flags; tools/ only)
LIB_PATH = os.environ.get("OEH_LIB") or os.path.join(_HERE, "lib", "liboeh_hip.so")

ABI_VERSION = 6  # include/oeh.h: OEH_ABI_VERSION
CALIB_WORK_BYTES = 36864  # include/oeh.h: OEH_CALIB_WORK_BYTES
DECODE_MAX_SPLITS = 64  # include/oeh.h: OEH_DECODE_MAX_SPLITS
STATS_WAVE_COLS, STATS_CHUNK, STATS_RECORD_BYTES = 2040, 8192, 48  # include/oeh.h: OEH_STATS_WAVE_COLS, OEH_STATS_CHUNK, OEH_STATS_RECORD_BYTES
QMSE_CHUNK, QMSE_SLICE, QMSE_MAX_BLOCKS, QMSE_CAND_BYTES, QMSE_F64_K = 8192, 256, 1024, 16, 4  # include/oeh.h: OEH_QMSE_CHUNK, OEH_QMSE_SLICE, OEH_QMSE_MAX_BLOCKS, OEH_QMSE_CAND_BYTES, OEH_QMSE_F64_K
OEH_F16, OEH_BF16, OEH_F32, OEH_I8 = 0, 1, 2, 3
OEH_SOFTMAX_VANILLA, OEH_SOFTMAX_ONE = 0, 1
OEH_ACT_NONE, OEH_ACT_RELU, OEH_ACT_GELU = 0, 1, 2  # include/oeh.h: the activations of oeh_act_quant


class OehError(RuntimeError):
    code = 0  # the negative OEH_E* code when the error came from the library


class oeh_fq(C.Structure):
    _fields_ = [
        ("enable", C.c_int32),
        ("scale", C.c_float),
        ("zero_point", C.c_float),
        ("qmax", C.c_float),
        ("dump_idx", C.c_void_p),
    ]


class oeh_fq_desc(C.Structure):
    _fields_ = [("scores", oeh_fq), ("probs", oeh_fq), ("ctx", oeh_fq), ("ctx_quant_before_gate", C.c_int32), ("ctx_emit_index", C.c_int32)]


class oeh_grid(C.Structure):
    _fields_ = [("scale", C.c_float), ("zero_point", C.c_float)]


class oeh_attn_desc(C.Structure):
    _fields_ = [
        ("B", C.c_int32), ("H", C.c_int32), ("Sq", C.c_int32), ("Sk", C.c_int32), ("D", C.c_int32),
        ("dtype", C.c_int32),
        ("q_stride", C.c_int64 * 3), ("k_stride", C.c_int64 * 3), ("v_stride", C.c_int64 * 3), ("o_stride", C.c_int64 * 3),
        ("scale", C.c_float), ("scale_div", C.c_float),
        ("softmax_base", C.c_int32), ("clip", C.c_int32), ("gamma", C.c_float), ("eta", C.c_float),
        ("key_pad_mask", C.c_void_p), ("key_pad_dtype", C.c_int32), ("key_pad_stride", C.c_int64),
        ("full_mask", C.c_void_p), ("full_mask_dtype", C.c_int32), ("full_mask_stride", C.c_int64 * 2),
        ("causal", C.c_int32), ("clamp_min", C.c_int32), ("mask_min", C.c_float),
        ("gate", C.c_void_p), ("gate_stride", C.c_int64 * 3),
        ("gate_hidden", C.c_void_p), ("gate_hidden_stride", C.c_int64 * 2),
        ("gate_w1", C.c_void_p), ("gate_b1", C.c_void_p), ("gate_w2", C.c_void_p), ("gate_b2", C.c_void_p),
        ("gate_units", C.c_int32), ("gate_scaling", C.c_float), ("gate_out", C.c_void_p),
        ("q_grid", oeh_grid), ("k_grid", oeh_grid), ("v_grid", oeh_grid), ("o_dtype", C.c_int32),
        ("key_pad_boolean", C.c_int32),
    ]


class oeh_dropout(C.Structure):
    """include/oeh.h: attention dropout of the training kernels (p in [0, 1), Philox key seed)."""
    _fields_ = [("p", C.c_float), ("reserved", C.c_uint32), ("seed", C.c_uint64)]


class oeh_attn_opts(C.Structure):
    """include/oeh.h: options of oeh_attn_fwd_ex (pv_pairs: the probability operand as an fp16 pair on fp32 storage)."""
    _fields_ = [("pv_pairs", C.c_int32), ("reserved", C.c_int32 * 3)]


class oeh_proj_seg(C.Structure):
    """include/oeh.h: one column segment (a projection) of oeh_proj_quant_i8."""
    _fields_ = [("alpha", C.c_float), ("scale", C.c_float), ("zero_point", C.c_float), ("out", C.c_void_p), ("y", C.c_void_p),
                ("y_stride_row", C.c_int64), ("transpose", C.c_int32), ("acc_add", C.c_void_p)]


class oeh_ln_desc(C.Structure):
    """include/oeh.h: the rows of oeh_resid_ln_quant (residual + sum quantiser + LayerNorm + output quantiser)."""
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int32), ("dtype", C.c_int32),
                ("x_stride", C.c_int64), ("r_stride", C.c_int64), ("sum_stride", C.c_int64), ("y_stride", C.c_int64),
                ("eps", C.c_float), ("reserved", C.c_int32), ("fq_sum", oeh_fq), ("fq_out", oeh_fq)]


OEH_TAB_PLAIN, OEH_TAB_GRID, OEH_TAB_I8 = 0, 1, 2  # include/oeh.h: the forms of an embedding table
OEH_ID_I32, OEH_ID_I64 = 0, 1


class oeh_embed_lookup(C.Structure):
    """include/oeh.h: one lookup of oeh_embed_sum_quant (table, ids, strides, the table's form and weight grid)."""
    _fields_ = [("table", C.c_void_p), ("ids", C.c_void_p), ("n_rows", C.c_int64), ("row_stride", C.c_int64),
                ("id_stride_b", C.c_int64), ("id_stride_s", C.c_int64), ("id_dtype", C.c_int32), ("form", C.c_int32),
                ("scale", C.c_float), ("int_min", C.c_float), ("int_max", C.c_float), ("reserved", C.c_int32)]


class oeh_embed_desc(C.Structure):
    """include/oeh.h: the rows of oeh_embed_sum_quant (lookups + sum quantisers + LayerNorm + output quantiser)."""
    _fields_ = [("B", C.c_int32), ("S", C.c_int32), ("cols", C.c_int32), ("dtype", C.c_int32), ("n_tab", C.c_int32), ("reserved", C.c_int32),
                ("sum_stride", C.c_int64), ("y_stride", C.c_int64), ("eps", C.c_float), ("reserved2", C.c_int32),
                ("tab", oeh_embed_lookup * 3), ("fq_sum", oeh_fq * 3), ("fq_out", oeh_fq)]


XENT_SLOTS = 4  # include/oeh.h: OEH_XENT_SLOTS


class oeh_xent_desc(C.Structure):
    """include/oeh.h: the rows of oeh_xent_fwd / oeh_xent_bwd (cross-entropy over (B, S, V) logits and (B, S) labels, both by strides)."""
    _fields_ = [("B", C.c_int32), ("S", C.c_int32), ("V", C.c_int32), ("dtype", C.c_int32), ("label_dtype", C.c_int32), ("mean_reduction", C.c_int32),
                ("x_stride", C.c_int64 * 2), ("label_stride", C.c_int64 * 2), ("dx_stride", C.c_int64 * 2), ("ignore_index", C.c_int64),
                ("label_smoothing", C.c_float), ("reserved", C.c_int32)]


LN_TRAIN_MAX_GROUPS = 512  # include/oeh.h: OEH_LN_TRAIN_MAX_GROUPS


class oeh_ln_train_desc(C.Structure):
    """include/oeh.h: the rows of oeh_drop_resid_ln_fwd / oeh_drop_resid_ln_bwd (dropout + residual + LayerNorm for training)."""
    _fields_ = [("rows", C.c_int64), ("cols", C.c_int32), ("dtype", C.c_int32),
                ("x_stride", C.c_int64), ("r_stride", C.c_int64), ("sum_stride", C.c_int64), ("y_stride", C.c_int64),
                ("dsum_stride", C.c_int64), ("eps", C.c_float), ("reserved", C.c_int32), ("drop", oeh_dropout)]


SOFTMAX_TRAIN_MAX_COLS = 15872  # include/oeh.h: OEH_SOFTMAX_TRAIN_MAX_COLS


class oeh_softmax_train_desc(C.Structure):
    """include/oeh.h: the rows of oeh_softmax_train_fwd / oeh_softmax_train_bwd (mask + softmax / softmax_1 + clip + dropout for training)."""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("Sq", C.c_int32), ("Sk", C.c_int32),
                ("x_dtype", C.c_int32), ("y_dtype", C.c_int32), ("mask_dtype", C.c_int32),
                ("softmax_base", C.c_int32), ("clip", C.c_int32), ("gamma", C.c_float), ("eta", C.c_float),
                ("scale", C.c_float), ("scale_div", C.c_float), ("clamp", C.c_int32), ("clamp_min", C.c_float), ("reserved", C.c_int32),
                ("x_stride", C.c_int64 * 3), ("y_stride", C.c_int64 * 3), ("u_stride", C.c_int64 * 3), ("mask_stride", C.c_int64 * 3),
                ("dy_stride", C.c_int64 * 3), ("du_stride", C.c_int64 * 3), ("dx_stride", C.c_int64 * 3), ("drop", oeh_dropout)]


GATE_TRAIN_MAX_GROUPS = 1024  # include/oeh.h: OEH_GATE_TRAIN_MAX_GROUPS


class oeh_gate_train_desc(C.Structure):
    """include/oeh.h: the tensors of oeh_gate_apply_fwd / oeh_gate_apply_bwd (per-token gate predictors + context * gate for training)."""
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("d", C.c_int32), ("units", C.c_int32), ("dtype", C.c_int32),
                ("scaling", C.c_float), ("reserved", C.c_int32),
                ("hidden_stride", C.c_int64 * 2), ("ctx_stride", C.c_int64 * 3), ("out_stride", C.c_int64 * 2),
                ("dctx_stride", C.c_int64 * 3), ("dhidden_stride", C.c_int64 * 2)]


MT_CHUNK, MT_MAX_GROUPS, MT_ENTRY_BYTES, MT_RECORD_BYTES = 4096, 8, 16, 56  # include/oeh.h: OEH_MT_CHUNK, OEH_MT_MAX_GROUPS, OEH_MT_ENTRY_BYTES, OEH_MT_RECORD_BYTES


class oeh_mt_tensor(C.Structure):
    """include/oeh.h: one parameter tensor of a multi-tensor plan (fp32 p, m, v; g in g_dtype; the hyper-parameter group it is stepped with)."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64), ("g_dtype", C.c_int32), ("group", C.c_int32)]


class oeh_adamw_desc(C.Structure):
    """include/oeh.h: the hyper-parameters and step numbers of oeh_adamw_step, one column per group."""
    _fields_ = [("lr", C.c_float * 8), ("beta1", C.c_float * 8), ("beta2", C.c_float * 8), ("eps", C.c_float * 8), ("weight_decay", C.c_float * 8),
                ("step", C.c_int64 * 8), ("n_groups", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/oeh.h declares (tests/test_abi.py checks the .so exports exactly these)
EXPORTS = (
    "oeh_attn_fwd", "oeh_softmax_rows", "oeh_fake_quant", "oeh_gate_fwd", "oeh_minmax", "oeh_percentile_ema", "oeh_fake_quant_range", "oeh_attn_calibrate", "oeh_quantize_heads_i8", "oeh_split_pairs", "oeh_split_triples", "oeh_proj_quant_i8",
    "oeh_attn_fwd_train", "oeh_attn_bwd_work_bytes", "oeh_attn_bwd",
    "oeh_attn_fwd_train_dropout", "oeh_attn_bwd_dropout", "oeh_attn_dropout_mask",
    "oeh_abi_version", "oeh_build_info", "oeh_strerror", "oeh_attn_variant",
    "oeh_attn_fwd_ex", "oeh_attn_variant_ex",
    "oeh_attn_decode_work_bytes", "oeh_attn_decode", "oeh_attn_decode_variant", "oeh_attn_decode_fq", "oeh_attn_decode_fq_variant",
    "oeh_outlier_stats_work_bytes", "oeh_outlier_stats",
    "oeh_quant_mse_work_bytes", "oeh_quant_mse",
    "oeh_resid_ln_quant", "oeh_resid_ln_variant",
    "oeh_xent_fwd", "oeh_xent_bwd", "oeh_xent_variant",
    "oeh_drop_resid_ln_fwd", "oeh_drop_resid_ln_bwd_work_bytes", "oeh_drop_resid_ln_bwd", "oeh_drop_resid_ln_mask", "oeh_drop_resid_ln_variant",
    "oeh_softmax_train_fwd", "oeh_softmax_train_bwd", "oeh_softmax_train_variant",
    "oeh_mt_plan_bytes", "oeh_mt_plan", "oeh_mt_variant", "oeh_grad_norm_work_bytes", "oeh_grad_norm", "oeh_grad_scale", "oeh_adamw_step",
    "oeh_grad_norm_amp", "oeh_adamw_amp_work_bytes", "oeh_adamw_step_amp", "oeh_loss_scale_update",
    "oeh_act_quant", "oeh_act_quant_variant",
    "oeh_gate_apply_fwd", "oeh_gate_apply_bwd_work_bytes", "oeh_gate_apply_bwd", "oeh_gate_apply_variant",
    "oeh_embed_sum_quant", "oeh_embed_sum_variant",
)

_lib = None


def load() -> C.CDLL:
    """Load liboeh_hip.so once.  torch (if it is going to be used) must be imported first so that both
    share ONE HIP runtime: the library's DT_NEEDED libamdhip64.so.7 then resolves to the copy torch loaded."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OehError(
            f"{LIB_PATH} is missing: build it with `make -C outeffhop_amd/csrc -j8` (or `python -c 'import "
            "__graft_entry__ as g; g.build()'`).  outeffhop_amd has no CPU/PyTorch fallback."
        )
    try:
        import torch  # noqa: F401  (brings in torch's libamdhip64 first)
    except Exception:  # pragma: no cover - library is usable from plain C hosts too
        pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.oeh_attn_fwd.argtypes = [C.POINTER(oeh_attn_desc), vp, vp, vp, vp, C.POINTER(oeh_fq_desc), vp]
    lib.oeh_attn_fwd.restype = C.c_int
    lib.oeh_softmax_rows.argtypes = [vp, vp, i64, i32, i32, i32, i32, f32, f32, vp]
    lib.oeh_softmax_rows.restype = C.c_int
    lib.oeh_fake_quant.argtypes = [vp, vp, vp, i64, i32, f32, f32, f32, vp]
    lib.oeh_fake_quant.restype = C.c_int
    lib.oeh_gate_fwd.argtypes = [vp, i32, i32, i32, i32, i32, i64, i64, vp, vp, vp, vp, i32, i32, f32, vp, vp]
    lib.oeh_gate_fwd.restype = C.c_int
    lib.oeh_minmax.argtypes = [vp, i64, i32, vp, vp]
    lib.oeh_minmax.restype = C.c_int
    f64 = C.c_double
    lib.oeh_percentile_ema.argtypes = [vp, i64, i32, f64, f64, f64, i32, vp, vp, vp]
    lib.oeh_percentile_ema.restype = C.c_int
    lib.oeh_fake_quant_range.argtypes = [vp, vp, i64, i32, vp, i32, f64, vp]
    lib.oeh_fake_quant_range.restype = C.c_int
    lib.oeh_attn_calibrate.argtypes = [C.POINTER(oeh_attn_desc), vp, vp, vp, vp, i32, vp, vp, i32, f64, f64, f64, f64, i32, vp, vp, vp]
    lib.oeh_attn_calibrate.restype = C.c_int
    lib.oeh_quantize_heads_i8.argtypes = [vp, vp, vp, i64, i32, i32, C.POINTER(i64), C.POINTER(i64), i32, f32, f32, i32, f32, vp, vp]
    lib.oeh_quantize_heads_i8.restype = C.c_int
    lib.oeh_split_pairs.argtypes = [vp, vp, i64, i32, i64, vp]
    lib.oeh_split_pairs.restype = C.c_int
    lib.oeh_split_triples.argtypes = [vp, vp, i64, i32, i64, vp]
    lib.oeh_split_triples.restype = C.c_int
    lib.oeh_proj_quant_i8.argtypes = [vp, i32, vp, vp, i64, i32, i32, i32, i32, C.POINTER(oeh_proj_seg), i64, i64, vp]
    lib.oeh_proj_quant_i8.restype = C.c_int
    lib.oeh_attn_fwd_train.argtypes = [C.POINTER(oeh_attn_desc), vp, vp, vp, vp, vp, vp]
    lib.oeh_attn_fwd_train.restype = C.c_int
    lib.oeh_attn_bwd_work_bytes.argtypes = [C.POINTER(oeh_attn_desc)]
    lib.oeh_attn_bwd_work_bytes.restype = C.c_int64
    lib.oeh_attn_bwd.argtypes = [C.POINTER(oeh_attn_desc), vp, vp, vp, vp, vp, C.POINTER(i64), vp, vp, C.POINTER(i64), vp, C.POINTER(i64), vp,
                                 C.POINTER(i64), vp, vp]
    lib.oeh_attn_bwd.restype = C.c_int
    lib.oeh_attn_fwd_train_dropout.argtypes = [C.POINTER(oeh_attn_desc), C.POINTER(oeh_dropout), vp, vp, vp, vp, vp, vp]
    lib.oeh_attn_fwd_train_dropout.restype = C.c_int
    lib.oeh_attn_bwd_dropout.argtypes = [C.POINTER(oeh_attn_desc), C.POINTER(oeh_dropout), vp, vp, vp, vp, vp, C.POINTER(i64), vp, vp, C.POINTER(i64), vp,
                                         C.POINTER(i64), vp, C.POINTER(i64), vp, vp]
    lib.oeh_attn_bwd_dropout.restype = C.c_int
    lib.oeh_attn_dropout_mask.argtypes = [C.POINTER(oeh_attn_desc), C.POINTER(oeh_dropout), vp, vp]
    lib.oeh_attn_dropout_mask.restype = C.c_int
    lib.oeh_abi_version.restype = C.c_int
    lib.oeh_build_info.restype = C.c_char_p
    lib.oeh_strerror.argtypes = [C.c_int]
    lib.oeh_strerror.restype = C.c_char_p
    lib.oeh_attn_variant.argtypes = [C.POINTER(oeh_attn_desc), C.POINTER(oeh_fq_desc)]
    lib.oeh_attn_variant.restype = C.c_char_p
    lib.oeh_attn_fwd_ex.argtypes = [C.POINTER(oeh_attn_desc), C.POINTER(oeh_attn_opts), vp, vp, vp, vp, C.POINTER(oeh_fq_desc), vp]
    lib.oeh_attn_fwd_ex.restype = C.c_int
    lib.oeh_attn_variant_ex.argtypes = [C.POINTER(oeh_attn_desc), C.POINTER(oeh_attn_opts), C.POINTER(oeh_fq_desc)]
    lib.oeh_attn_variant_ex.restype = C.c_char_p
    lib.oeh_attn_decode_work_bytes.argtypes = [C.POINTER(oeh_attn_desc), i32]
    lib.oeh_attn_decode_work_bytes.restype = C.c_int64
    lib.oeh_attn_decode.argtypes = [C.POINTER(oeh_attn_desc), i32, vp, vp, vp, vp, vp, vp]
    lib.oeh_attn_decode.restype = C.c_int
    lib.oeh_attn_decode_variant.argtypes = [C.POINTER(oeh_attn_desc), i32]
    lib.oeh_attn_decode_variant.restype = C.c_char_p
    lib.oeh_attn_decode_fq.argtypes = [C.POINTER(oeh_attn_desc), C.POINTER(oeh_fq_desc), i32, vp, vp, vp, vp, vp, vp]
    lib.oeh_attn_decode_fq.restype = C.c_int
    lib.oeh_attn_decode_fq_variant.argtypes = [C.POINTER(oeh_attn_desc), C.POINTER(oeh_fq_desc), i32]
    lib.oeh_attn_decode_fq_variant.restype = C.c_char_p
    lib.oeh_outlier_stats_work_bytes.argtypes = [i64, i64]
    lib.oeh_outlier_stats_work_bytes.restype = C.c_size_t
    lib.oeh_outlier_stats.argtypes = [vp, i64, i64, i64, i32, f64, vp, vp, i32, vp, vp]
    lib.oeh_outlier_stats.restype = C.c_int
    lib.oeh_quant_mse_work_bytes.argtypes = [i64, i32]
    lib.oeh_quant_mse_work_bytes.restype = C.c_size_t
    lib.oeh_quant_mse.argtypes = [vp, i64, i32, vp, i32, vp, i32, vp, vp]
    lib.oeh_quant_mse.restype = C.c_int
    lib.oeh_resid_ln_quant.argtypes = [C.POINTER(oeh_ln_desc), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.oeh_resid_ln_quant.restype = C.c_int
    lib.oeh_resid_ln_variant.argtypes = [C.POINTER(oeh_ln_desc)]
    lib.oeh_resid_ln_variant.restype = C.c_char_p
    lib.oeh_embed_sum_quant.argtypes = [C.POINTER(oeh_embed_desc), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.oeh_embed_sum_quant.restype = C.c_int
    lib.oeh_embed_sum_variant.argtypes = [C.POINTER(oeh_embed_desc)]
    lib.oeh_embed_sum_variant.restype = C.c_char_p
    lib.oeh_act_quant.argtypes = [vp, vp, vp, i64, i32, i64, i64, i32, i32, f32, f32, f32, vp, vp]
    lib.oeh_act_quant.restype = C.c_int
    lib.oeh_act_quant_variant.argtypes = [i64, i32, i64, i64, i32, i32, i32, i32]
    lib.oeh_act_quant_variant.restype = C.c_char_p
    lib.oeh_xent_fwd.argtypes = [C.POINTER(oeh_xent_desc), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.oeh_xent_fwd.restype = C.c_int
    lib.oeh_xent_bwd.argtypes = [C.POINTER(oeh_xent_desc), vp, vp, vp, vp, vp, i64, vp, vp]
    lib.oeh_xent_bwd.restype = C.c_int
    lib.oeh_xent_variant.argtypes = [C.POINTER(oeh_xent_desc), vp, vp]
    lib.oeh_xent_variant.restype = C.c_char_p
    lib.oeh_drop_resid_ln_fwd.argtypes = [C.POINTER(oeh_ln_train_desc), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.oeh_drop_resid_ln_fwd.restype = C.c_int
    lib.oeh_drop_resid_ln_bwd_work_bytes.argtypes = [C.POINTER(oeh_ln_train_desc)]
    lib.oeh_drop_resid_ln_bwd_work_bytes.restype = C.c_size_t
    lib.oeh_drop_resid_ln_bwd.argtypes = [C.POINTER(oeh_ln_train_desc), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.oeh_drop_resid_ln_bwd.restype = C.c_int
    lib.oeh_drop_resid_ln_mask.argtypes = [C.POINTER(oeh_ln_train_desc), vp, vp]
    lib.oeh_drop_resid_ln_mask.restype = C.c_int
    lib.oeh_drop_resid_ln_variant.argtypes = [C.POINTER(oeh_ln_train_desc), C.c_int]
    lib.oeh_drop_resid_ln_variant.restype = C.c_char_p
    lib.oeh_softmax_train_fwd.argtypes = [C.POINTER(oeh_softmax_train_desc), vp, vp, vp, vp, vp, vp]
    lib.oeh_softmax_train_fwd.restype = C.c_int
    lib.oeh_softmax_train_bwd.argtypes = [C.POINTER(oeh_softmax_train_desc), vp, vp, vp, vp, vp, vp, vp]
    lib.oeh_softmax_train_bwd.restype = C.c_int
    lib.oeh_softmax_train_variant.argtypes = [C.POINTER(oeh_softmax_train_desc), C.c_int]
    lib.oeh_softmax_train_variant.restype = C.c_char_p
    lib.oeh_mt_plan_bytes.argtypes = [C.POINTER(oeh_mt_tensor), i32]
    lib.oeh_mt_plan_bytes.restype = C.c_int64
    lib.oeh_mt_plan.argtypes = [C.POINTER(oeh_mt_tensor), i32, vp, C.POINTER(i64)]
    lib.oeh_mt_plan.restype = C.c_int
    lib.oeh_mt_variant.argtypes = [C.POINTER(oeh_mt_tensor)]
    lib.oeh_mt_variant.restype = C.c_char_p
    lib.oeh_grad_norm_work_bytes.argtypes = [i64]
    lib.oeh_grad_norm_work_bytes.restype = C.c_int64
    lib.oeh_grad_norm.argtypes = [vp, i64, f64, vp, vp, vp]
    lib.oeh_grad_norm.restype = C.c_int
    lib.oeh_grad_scale.argtypes = [vp, i64, vp, vp]
    lib.oeh_grad_scale.restype = C.c_int
    lib.oeh_adamw_step.argtypes = [vp, i64, C.POINTER(oeh_adamw_desc), vp, vp]
    lib.oeh_adamw_step.restype = C.c_int
    lib.oeh_grad_norm_amp.argtypes = [vp, i64, f64, vp, vp, vp, vp, vp, vp]
    lib.oeh_grad_norm_amp.restype = C.c_int
    lib.oeh_adamw_amp_work_bytes.argtypes = [i32]
    lib.oeh_adamw_amp_work_bytes.restype = C.c_int64
    lib.oeh_adamw_step_amp.argtypes = [vp, i64, i32, C.POINTER(oeh_adamw_desc), vp, vp, vp, vp, vp]
    lib.oeh_adamw_step_amp.restype = C.c_int
    lib.oeh_loss_scale_update.argtypes = [vp, f64, f64, i32, vp]
    lib.oeh_loss_scale_update.restype = C.c_int
    lib.oeh_gate_apply_fwd.argtypes = [C.POINTER(oeh_gate_train_desc), vp, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.oeh_gate_apply_fwd.restype = C.c_int
    lib.oeh_gate_apply_bwd_work_bytes.argtypes = [i32, i32, i32, i32, i32]
    lib.oeh_gate_apply_bwd_work_bytes.restype = C.c_int64
    lib.oeh_gate_apply_bwd.argtypes = [C.POINTER(oeh_gate_train_desc)] + [vp] * 16
    lib.oeh_gate_apply_bwd.restype = C.c_int
    lib.oeh_gate_apply_variant.argtypes = [C.POINTER(oeh_gate_train_desc), C.c_int]
    lib.oeh_gate_apply_variant.restype = C.c_char_p
    if lib.oeh_abi_version() != ABI_VERSION:
        raise OehError(f"liboeh_hip.so ABI {lib.oeh_abi_version()} != {ABI_VERSION} (stale build?)")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        err = OehError(f"{what} failed: {load().oeh_strerror(rc).decode()} ({rc})")
        err.code = rc
        raise err
