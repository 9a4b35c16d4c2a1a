"""INT8 post-training fake-quant around the attention path, MI355X side.

Host-side mirror of the part of the reference's `quantization/` package that the attention hot path touches
(SURVEY.md section 2 rows 9-12 and the attention classes of rows 6-7):

  AsymmetricUniformQuantizer / SymmetricUniformQuantizer   quantization/quantizers/uniform_quantizers.py:12-310
  CurrentMinMaxEstimator / RunningMinMaxEstimator           quantization/range_estimators.py:54-106
  OptMethod / MSE_Estimator                                 quantization/range_estimators.py:109-395
  QuantizationManager (estimate -> fix state machine)       quantization/quantization_manager.py:11-108
  QuantizedModule / QuantizedActivation                     quantization/base_quantized_classes.py:38-199
  QuantLinear (weight + output-activation quant)            quantization/hijacker.py:27-134, autoquant_utils.py:18-20
  Quantized{Bert,OPT}...AttentionWithExtras                 models/quantized_bert.py:221-440, quantized_opt.py:54-274
  QuantLayerNorm                                            quantization/autoquant_utils.py:64-72
  QuantizedBertSelfOutput / QuantizedBertOutput             models/quantized_bert.py:541-606
  quantize_intermediate / QuantizedBertFeedForward          models/quantized_bert.py:609-700
  QuantizedOPTDecoderLayer                                  models/quantized_opt.py:277-384

Same class / attribute / buffer names (`activation_quantizer.quantizer._delta`, `_zero_float`, ...) so calibrated
state dicts are interchangeable.  Activation fake-quant runs on the GPU: fused into the attention kernel once the
three ranges are fixed (the INT8 validate path), as the stand-alone HIP kernel otherwise.  Range estimation keeps
everything on the device (the reference copies each (B,H,S,S) tensor to the host for np.percentile).
"""
from __future__ import annotations

import copy
import dataclasses
from enum import Enum
from typing import Optional

import numpy as np
import torch
from torch import nn

from . import ops
from ._lib import OehError as _OehError
from ._watch import TensorWatch, cached
from .attention import (GATE_ATTRS, AttentionGateType, BaseEnumOptions, GateBookkeeping, GateState, attention_core, classify_causal, gated_merge,
                        has_hooks, kv_source, mask_min_of, pad_is_boolean, resolve_mask, unfused_core)
from .ops import AttnFakeQuant, FakeQuantSpec
from .softmax import spec_of


class QuantizerNotInitializedError(Exception):
    def __init__(self):
        super().__init__("Quantizer has  not been initialized yet")


class Qstates(BaseEnumOptions):
    estimate_ranges = 1
    fix_ranges = 2
    learn_ranges = 4
    estimate_ranges_train = 8


def _adopt_unset_buffers(mod: nn.Module, state_dict, prefix: str) -> None:
    """A calibrated checkpoint carries range buffers that a fresh module still holds as None (`_delta`, `current_xmin` ...): give such a
    buffer the checkpoint's tensor before the loader looks, or a strict load reports the key as unexpected."""
    for name, buf in mod._buffers.items():
        if buf is None and prefix + name in state_dict and name not in mod._non_persistent_buffers_set:
            mod._buffers[name] = state_dict[prefix + name].detach().clone()


# ------------------------------------------------------------------------------------------------------------
# quantisers
# ------------------------------------------------------------------------------------------------------------
class AsymmetricUniformQuantizer(nn.Module):
    """Per-tensor asymmetric uniform fake-quant: idx = clamp(round(x/scale)+zp, 0, 2^n-1); x_q = scale*(idx-zp)."""

    def __init__(self, n_bits, scale_domain="linear", grad_scaling=False, eps=1e-8, per_channel=False, act_quant=False, **kwargs):
        super().__init__()
        if scale_domain != "linear" or per_channel or grad_scaling:
            raise NotImplementedError("only linear-domain per-tensor quantisers are on the MI355X attention path")
        self.n_bits = n_bits
        self.act_quant = act_quant
        self.per_channel = per_channel
        self.state = None
        self.x_min_fp32 = self.x_max_fp32 = None
        self.register_buffer("_delta", None)
        self.register_buffer("_zero_float", None)
        self.scale_domain = scale_domain
        self.eps = eps

    @property
    def delta(self):
        if self._delta is None:
            raise QuantizerNotInitializedError()
        return self._delta

    @property
    def zero_float(self):
        if self._zero_float is None:
            raise QuantizerNotInitializedError()
        return self._zero_float

    @property
    def is_initialized(self):
        return self._delta is not None

    @property
    def symmetric(self):
        return False

    @property
    def int_min(self):
        return 0.0

    @property
    def int_max(self):
        return 2.0 ** self.n_bits - 1

    @property
    def scale(self):
        return torch.clamp(self.delta, min=self.eps)

    @property
    def zero_point(self):
        return torch.clamp(torch.round(self.zero_float), self.int_min, self.int_max)

    @property
    def x_max(self):
        return self.scale * (self.int_max - self.zero_point)

    @property
    def x_min(self):
        return self.scale * (self.int_min - self.zero_point)

    def spec(self) -> FakeQuantSpec:
        """Host-side (scale, zero_point, qmax) for the kernels; one device->host read per range change."""
        return cached(self.__dict__, "_spec_cache", (self.n_bits, self.eps), lambda: [(self._buffers, "_delta"), (self._buffers, "_zero_float")],
                      lambda: FakeQuantSpec.from_delta(float(self._delta), float(self._zero_float), self.n_bits, self.eps))

    def to_integer_forward(self, x_float):
        _, idx = ops.fake_quant(x_float, self.spec(), want_idx=True)
        return idx.to(x_float.dtype)

    def forward(self, x_float):
        return ops.fake_quant(x_float, self.spec())

    def _tensorize_min_max(self, x_min, x_max):
        if not torch.is_tensor(x_min):
            x_min = torch.tensor(x_min).float()
            x_max = torch.tensor(x_max).float()
        if x_min.dim() > 0 and len(x_min) > 1:
            raise ValueError("x_min and x_max must be a float or 1-D Tensor for per-tensor quantization (per_channel=False)")
        x_min = torch.min(x_min, torch.zeros_like(x_min))
        x_max = torch.max(x_max, torch.ones_like(x_max) * self.eps)
        return x_min, x_max

    def set_quant_range(self, x_min, x_max):
        self.x_min_fp32, self.x_max_fp32 = x_min, x_max
        x_min, x_max = self._tensorize_min_max(x_min, x_max)
        self._delta = ((x_max - x_min) / self.int_max).detach()
        self._zero_float = (-x_min / self._delta).detach()

    def fix_ranges(self):
        pass  # ranges are plain buffers here (no learnable-range mode on this path)

    def make_range_trainable(self):
        raise NotImplementedError("learned ranges (QAT) are outside the inference hot path")

    def reset(self):
        self._delta = None
        self._zero_float = None

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        _adopt_unset_buffers(self, state_dict, prefix)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def extra_repr(self):
        return f"n_bits={self.n_bits}, per_channel={self.per_channel}, is_initalized={self.is_initialized}"


class SymmetricUniformQuantizer(AsymmetricUniformQuantizer):
    """Signed symmetric grid for WEIGHTS (quant_configs.py:26); evaluated once per weight and cached by QuantLinear,
    so plain device tensor ops are enough (not on the attention core: SURVEY 8a row a12)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.register_buffer("_signed", None)

    @property
    def signed(self):
        if self._signed is None:
            raise QuantizerNotInitializedError()
        return bool(self._signed.item())

    @property
    def symmetric(self):
        return True

    @property
    def int_min(self):
        return -(2.0 ** (self.n_bits - 1)) if self.signed else 0

    @property
    def int_max(self):
        return 2.0 ** (self.n_bits - int(self.signed)) - 1

    @property
    def zero_point(self):
        return 0.0

    def set_quant_range(self, x_min, x_max):
        self.x_min_fp32, self.x_max_fp32 = x_min, x_max
        x_min, x_max = self._tensorize_min_max(x_min, x_max)
        self._signed = x_min.min() < 0
        self._delta = (torch.max(x_min.abs(), x_max) / self.int_max).detach()

    def forward(self, x_float):
        scale = self.scale
        x_int = torch.clamp(torch.round(x_float / scale), self.int_min, self.int_max)
        return scale * x_int

    def to_integer_forward(self, x_float):
        return torch.clamp(torch.round(x_float / self.scale), self.int_min, self.int_max)


# ------------------------------------------------------------------------------------------------------------
# range estimators
# ------------------------------------------------------------------------------------------------------------
def percentile_pair(x: torch.Tensor, lo_q: float, hi_q: float):
    """np.percentile(x, (lo_q, hi_q)) (linear interpolation, float64 result) computed on the device: the tails are
    extracted with top-k instead of copying the tensor to the host and sorting it (range_estimators.py:90-94)."""
    flat = x.detach().reshape(-1).float()
    n = flat.numel()

    def one(q):
        h = (n - 1) * (q / 100.0)
        i = int(np.floor(h))
        frac = h - i
        from_top = n - 1 - i  # 0 = the maximum
        if from_top + 2 <= min(n, 1 << 20):
            vals = torch.topk(flat, min(n, from_top + 1), largest=True, sorted=True).values  # descending
            a = float(vals[from_top])
            b = float(vals[from_top - 1]) if from_top >= 1 else a
        elif i + 3 <= min(n, 1 << 20):
            vals = torch.topk(flat, min(n, i + 2), largest=False, sorted=True).values  # ascending
            a = float(vals[i])
            b = float(vals[i + 1]) if i + 1 < n else a
        else:
            srt = torch.sort(flat).values
            a = float(srt[i])
            b = float(srt[min(i + 1, n - 1)])
        # numpy's _lerp on float32 data: the difference is formed in float32, the interpolation in float64,
        # anchored at b for frac >= 0.5
        diff = np.float64(np.float32(b) - np.float32(a))
        if frac >= 0.5:
            return np.float64(np.float32(b)) - diff * (1.0 - np.float64(frac))
        return np.float64(np.float32(a)) + diff * np.float64(frac)

    return one(lo_q), one(hi_q)


class RangeEstimatorBase(nn.Module):
    def __init__(self, *args, per_channel=False, quantizer=None, **kwargs):
        super().__init__()
        if per_channel:
            raise NotImplementedError("per-channel ranges are a weights-only option outside the attention path")
        self.register_buffer("current_xmin", None)
        self.register_buffer("current_xmax", None)
        self.per_channel = per_channel
        object.__setattr__(self, "quantizer", quantizer)  # not a submodule (keeps state-dict keys like the reference's repr)
        # GPU tensors with a percentile: the (x_min, x_max) pair lives in ONE float64[2] device tensor that the HIP selection
        # kernel updates in place (ops.percentile_ema); current_xmin / current_xmax are snapshots of it.  Not a buffer: the
        # state dict keeps the reference's keys.
        self.device_state = None

    def reset(self):
        self.current_xmin = None
        self.current_xmax = None
        self.device_state = None

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        _adopt_unset_buffers(self, state_dict, prefix)
        seen = len(unexpected_keys)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        # the reference's estimator holds its quantiser as a submodule: a checkpoint of it repeats the manager's `quantizer.*` keys under
        # `range_estimator.quantizer.*` - the same object here, loaded once through the manager
        unexpected_keys[seen:] = [k for k in unexpected_keys[seen:] if not k.startswith(prefix + "quantizer.")]

    def _percentile_on_device(self, x, q_lo, q_hi, momentum):
        """(np.percentile(x, q_lo), np.percentile(x, q_hi)) [+ running average] without leaving the GPU: no topk, no host sync."""
        first = self.device_state is None or self.device_state.device != x.device
        if first:
            self.device_state = torch.empty(2, dtype=torch.float64, device=x.device)
        # (momentum None - CurrentMinMaxEstimator: no running average - is "every batch is the first one")
        ops.percentile_ema(x, q_lo, q_hi, self.device_state, momentum=0.0 if momentum is None else momentum, first=first or momentum is None)
        self.current_xmin, self.current_xmax = self.device_state[0].clone(), self.device_state[1].clone()
        return self.current_xmin, self.current_xmax


class CurrentMinMaxEstimator(RangeEstimatorBase):
    def __init__(self, *args, percentile=None, **kwargs):
        self.percentile = percentile
        super().__init__(*args, **kwargs)

    def forward(self, x):
        if self.percentile and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16, torch.float32):
            self.device_state = None  # no running average: every call starts over
            return self._percentile_on_device(x, self.percentile, 100 - self.percentile, 0.0)
        if self.percentile:
            lo, hi = percentile_pair(x, self.percentile, 100 - self.percentile)
            self.current_xmin = torch.tensor(lo).to(x.device)
            self.current_xmax = torch.tensor(hi).to(x.device)
        else:
            mm = ops.minmax(x) if x.is_cuda else torch.stack([x.min(), x.max()]).float()
            self.current_xmin, self.current_xmax = mm[0].to(x.dtype).detach(), mm[1].to(x.dtype).detach()
        return self.current_xmin, self.current_xmax


class RunningMinMaxEstimator(RangeEstimatorBase):
    def __init__(self, *args, momentum=0.9, percentile=None, **kwargs):
        self.momentum = momentum
        self.percentile = percentile
        super().__init__(*args, **kwargs)

    def forward(self, x):
        if self.percentile and x.is_cuda and x.dtype in (torch.float16, torch.bfloat16, torch.float32) and \
                (self.current_xmin is None or self.device_state is not None):
            return self._percentile_on_device(x, 100 - self.percentile, self.percentile, self.momentum)
        if self.percentile:
            lo, hi = percentile_pair(x, 100 - self.percentile, self.percentile)
            x_min, x_max = torch.tensor(lo).to(x.device), torch.tensor(hi).to(x.device)  # float64, like the reference
        else:
            mm = ops.minmax(x)
            x_min, x_max = mm[0].to(x.dtype).detach(), mm[1].to(x.dtype).detach()
        if self.current_xmin is None:
            self.current_xmin, self.current_xmax = x_min, x_max
        else:
            self.current_xmin = (1 - self.momentum) * x_min + self.momentum * self.current_xmin
            self.current_xmax = (1 - self.momentum) * x_max + self.momentum * self.current_xmax
        return self.current_xmin, self.current_xmax


class OptMethod(BaseEnumOptions):
    grid = 1
    golden_section = 2


class NoDataPassedError(Exception):
    def __init__(self):
        super().__init__("no data has been passed through the range estimator yet")


def quant_mse_eager(x: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    """What `ops.quant_mse` computes, by plain torch ops on any device, one candidate after the other: the fp32 terms of
    uniform_quantizers.py:114-115,146 (true division, round to even, clamp, scale, subtract, square) summed in float64, one host read
    per candidate as in range_estimators.py:134-142.  The path of CPU tensors (weights quantised before .to(device)); on GPU tensors it
    is the eager chain that tools/mse_bench.py times the kernel against.  16-bit data is widened to fp32, as the kernel widens it."""
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    c = cand.to(x.device)
    out = []
    for k in range(c.shape[0]):
        scale, lo, hi = c[k, 0], c[k, 1], c[k, 2]
        y = scale * torch.clamp(torch.round(x / scale), lo, hi)
        out.append(float(((x - y) ** 2).sum(dtype=torch.float64)))
    return torch.tensor(out, dtype=torch.float64, device=x.device)


class MSE_Estimator(RangeEstimatorBase):
    """The range that minimises the squared quantisation error (range_estimators.py:114-382; validate_clm.py --ranges_weights mse,
    --ranges_acts MSE): a 1-D grid of clipping thresholds for symmetric quantisers and one-sided data, a 2-D grid (threshold x integer
    skew of the zero point) for asymmetric quantisers on two-sided data, or scipy's bounded golden-section search over the same
    spaces.  Losses are accumulated over the batches without momentum; the search space is fixed by the first batch.

    Every candidate's grid (scale, zero point, integer limits) is derived on the host by the float32 tensor arithmetic of the
    quantiser's set_quant_range, vectorised over the candidates, once; the table then stays on the device and `ops.quant_mse` adds
    the losses of ALL candidates to a float64 device array from one read of the data per 256 candidates.  argmin and the chosen range
    follow by torch ops: after the first batch's one read of (min, max) the grid searches never synchronise.  Golden section is
    sequential: one K = 1 call and one host read per evaluation.  CPU tensors take `quant_mse_eager`.
    Deviation: fp16 / bf16 data is widened to fp32 for the error terms (the reference squares and sums in the storage type)."""

    def __init__(self, *args, num_candidates=100, opt_method=OptMethod.grid, range_margin=0.5, **kwargs):
        super().__init__(*args, **kwargs)
        assert opt_method in OptMethod
        self.opt_method = opt_method
        self.num_candidates = num_candidates
        self.loss_array = None        # float64 (1, N + 1) or (1, N + 1, max_int_skew, 2) on the data's device; index 0 stays +inf
        self.max_pos_thr = None
        self.max_neg_thr = None
        self.max_search_range = None
        self.one_sided_dist = None
        self.range_margin = range_margin
        self._cand = None             # (K, 4) fp32 candidate table of the grid searches, on the data's device
        self._range_table = None      # (loss_array.numel(), 2) fp32: the (x_min, x_max) that each entry of loss_array stands for
        if self.quantizer is None:
            raise NotImplementedError("A Quantizer must be given as an argument to the MSE RangeEstimator")
        self.max_int_skew = (2 ** self.quantizer.n_bits) // 4  # for asymmetric quantisation

    # ---- candidate grids: the arithmetic of _tensorize_min_max / set_quant_range, vectorised over the candidates
    def _current_grid(self):
        q = self.quantizer
        if not q.is_initialized:
            raise QuantizerNotInitializedError()
        zp = float(q.zero_point)
        return float(q.scale), float(q.int_min) - zp, float(q.int_max) - zp

    def candidate_rows(self, neg_thr, pos_thr) -> torch.Tensor:
        """(K, 4) fp32 rows (scale, int_min - zero_point, int_max - zero_point, 0) of the grids that the quantiser's set_quant_range
        would take from the thresholds (float64 values, as the reference's Python arithmetic produces them)."""
        q = self.quantizer
        neg, pos = np.broadcast_arrays(np.atleast_1d(np.asarray(neg_thr, dtype=np.float64)), np.atleast_1d(np.asarray(pos_thr, dtype=np.float64)))
        x_min, x_max = torch.from_numpy(neg.copy()).float(), torch.from_numpy(pos.copy()).float()
        x_min = torch.min(x_min, torch.zeros_like(x_min))
        x_max = torch.max(x_max, torch.ones_like(x_max) * q.eps)
        if q.symmetric:
            signed = x_min < 0
            int_min = torch.where(signed, torch.full_like(x_min, -(2.0 ** (q.n_bits - 1))), torch.zeros_like(x_min))
            int_max = torch.where(signed, torch.full_like(x_min, 2.0 ** (q.n_bits - 1) - 1), torch.full_like(x_min, 2.0 ** q.n_bits - 1))
            delta = torch.max(x_min.abs(), x_max) / int_max
            zero_point = torch.zeros_like(x_min)
        else:
            int_min, int_max = torch.zeros_like(x_min), torch.full_like(x_min, 2.0 ** q.n_bits - 1)
            delta = (x_max - x_min) / (2.0 ** q.n_bits - 1)
            zero_point = torch.clamp(torch.round(-x_min / delta), 0.0, 2.0 ** q.n_bits - 1)
        scale = torch.clamp(delta, min=q.eps)
        rows = torch.stack([scale, int_min - zero_point, int_max - zero_point, torch.zeros_like(scale)], dim=1)
        # `if x_min or x_max` (range_estimators.py:178): two thresholds of exactly 0 leave the copy of the quantiser on its CURRENT range
        same = torch.from_numpy((neg == 0) & (pos == 0))
        if bool(same.any()):
            rows[same] = torch.tensor(self._current_grid() + (0.0,), dtype=torch.float32)
        return rows.contiguous()

    def _losses(self, data, cand, loss=None):
        """The candidates' losses on `data`: added to `loss` (float64, on the device) when given, else returned."""
        if data.is_cuda:
            return ops.quant_mse(data, cand.to(data.device), loss, accumulate=loss is not None)
        got = quant_mse_eager(data, cand)
        if loss is None:
            return got
        loss += got
        return loss

    def loss_fx(self, data, neg_thr, pos_thr):
        return float(self._losses(self._prepare(data), self.candidate_rows(neg_thr, pos_thr))[0])

    @staticmethod
    def _prepare(data):
        data = data.detach()
        return data if data.dtype in (torch.float16, torch.bfloat16, torch.float32) else data.float()

    @property
    def step_size(self):
        if self.one_sided_dist is None:
            raise NoDataPassedError()
        return self.max_search_range / self.num_candidates

    @property
    def optimization_method(self):
        if self.one_sided_dist is None:
            raise NoDataPassedError()
        one_d = self.one_sided_dist or self.quantizer.symmetric
        if self.opt_method == OptMethod.grid:
            return self._perform_1D_search if one_d else self._perform_2D_search
        if self.opt_method == OptMethod.golden_section:
            return self._golden_section_symmetric if one_d else self._golden_section_asymmetric
        raise NotImplementedError("Optimization Method not Implemented")

    def _define_search_range(self, data, d_min: float, d_max: float):
        self.channel_groups = 1
        dev = data.device
        self.current_xmax = torch.zeros(1, device=dev)
        self.current_xmin = torch.zeros(1, device=dev)
        N, S = self.num_candidates, self.max_int_skew
        one_d = self.one_sided_dist or self.quantizer.symmetric
        if one_d:
            self.loss_array = torch.zeros((1, N + 1), dtype=torch.float64, device=dev)
            self.loss_array[:, 0] = float("inf")  # exclude interval_start = interval_finish
            self.max_pos_thr = max(abs(d_min), d_max) + self.range_margin
            self.max_neg_thr = -self.max_pos_thr
            self.max_search_range = self.max_pos_thr
        else:
            self.loss_array = torch.zeros((1, N + 1, S, 2), dtype=torch.float64, device=dev)
            self.loss_array[:, 0] = float("inf")
            self.max_pos_thr = d_max + self.range_margin
            self.max_neg_thr = d_min - self.range_margin
            self.max_search_range = max(abs(self.max_pos_thr), abs(self.max_neg_thr))
        self._cand = self._range_table = None
        if self.opt_method != OptMethod.grid:
            return
        # the thresholds of every entry of loss_array, in its own (flattened) order, by the reference's float64 arithmetic
        step = self.step_size
        if one_d:
            idx = np.arange(N + 1)
            pos = step * idx
            neg = np.zeros(N + 1) if self.one_sided_dist else -step * idx
        else:
            idx = np.arange(N + 1).reshape(-1, 1, 1)
            start, finish = -step * idx, step * idx
            delta = (finish - start) / (2 ** self.quantizer.n_bits - 1)
            skew = (np.array([1, -1]).reshape(1, 1, 2) * np.arange(S).reshape(1, -1, 1)) * delta
            neg = np.maximum(start + skew, self.max_neg_thr).reshape(-1)
            pos = np.minimum(finish + skew, self.max_pos_thr).reshape(-1)
        first = neg.size // (N + 1)  # entries of candidate index 0: never evaluated
        self._cand = self.candidate_rows(neg[first:], pos[first:]).to(dev)
        self._range_table = torch.from_numpy(np.stack([neg, pos], axis=1).astype(np.single)).to(dev)

    def _grid_search(self, data):
        """Add this batch's losses of all candidates, then take the range of the smallest accumulated loss (torch ops on the data's
        device: no host read)."""
        if self.loss_array.device != data.device:
            self.loss_array, self._cand, self._range_table = (t.to(data.device) for t in (self.loss_array, self._cand, self._range_table))
        flat = self.loss_array.view(-1)
        self._losses(data, self._cand, flat[flat.numel() - self._cand.shape[0]:])
        best = self._range_table.index_select(0, torch.argmin(flat).reshape(1))[0]  # (a tensor index, not a host integer: no synchronisation)
        self.current_xmin, self.current_xmax = best[0:1].clone(), best[1:2].clone()

    def _perform_1D_search(self, data):
        self._grid_search(data)

    def _perform_2D_search(self, data):
        self._grid_search(data)

    @staticmethod
    def _minimize_scalar():
        try:
            from scipy.optimize import minimize_scalar
        except ImportError as e:
            raise ImportError("MSE_Estimator with OptMethod.golden_section needs scipy (scipy.optimize.minimize_scalar); "
                              "OptMethod.grid does not") from e
        return minimize_scalar

    def golden_sym_loss(self, range, data):
        return self.loss_fx(data, 0 if self.one_sided_dist else -range, range)

    def golden_asym_shift_loss(self, shift, range, data):
        return self.loss_fx(data, -range + shift, range + shift)

    def golden_asym_range_loss(self, range, data):
        max_shift = 2 * range / (2 ** self.quantizer.n_bits - 1) * self.max_int_skew
        return self._minimize_scalar()(self.golden_asym_shift_loss, args=(range, data), bounds=(-max_shift, max_shift), method="Bounded").fun

    def _golden_section_symmetric(self, data):
        self.result = self._minimize_scalar()(self.golden_sym_loss, args=data, bounds=(0.01 * self.max_search_range, self.max_search_range),
                                              method="Bounded")
        self.current_xmax = torch.tensor([self.result.x], dtype=torch.float32).to(data.device)
        self.current_xmin = torch.zeros(1, device=data.device) if self.one_sided_dist else -self.current_xmax

    def _golden_section_asymmetric(self, data):
        minimize_scalar = self._minimize_scalar()
        self.result = minimize_scalar(self.golden_asym_range_loss, args=data, bounds=(0.01 * self.max_search_range, self.max_search_range),
                                      method="Bounded")
        self.final_range = self.result.x
        max_shift = 2 * self.final_range / (2 ** self.quantizer.n_bits - 1) * self.max_int_skew
        self.subresult = minimize_scalar(self.golden_asym_shift_loss, args=(self.final_range, data), bounds=(-max_shift, max_shift), method="Bounded")
        self.final_shift = self.subresult.x
        self.current_xmax = torch.tensor([self.final_range + self.final_shift], dtype=torch.float32).to(data.device)
        self.current_xmin = torch.tensor([-self.final_range + self.final_shift], dtype=torch.float32).to(data.device)

    def forward(self, data):
        data = self._prepare(data)
        if self.loss_array is None:
            # the search space is set by the first batch: one host read of (min, max)
            mm = ops.minmax(data) if data.is_cuda else torch.stack([data.min(), data.max()]).float()
            d_min, d_max = (float(v) for v in mm.tolist())
            if self.one_sided_dist is None:
                self.one_sided_dist = bool(d_min >= 0)
            self._define_search_range(data, d_min, d_max)
        self.optimization_method(data)
        return self.current_xmin, self.current_xmax

    def reset(self):
        super().reset()
        self.loss_array = None
        self._cand = self._range_table = None

    def extra_repr(self):
        repr = "opt_method={}".format(self.opt_method.name)
        if self.opt_method == OptMethod.grid:
            repr += " ,num_candidates={}".format(self.num_candidates)
        return repr


class _ClsEnum(Enum):
    @property
    def cls(self):
        return self.value

    def __call__(self, *a, **k):
        return self.value(*a, **k)

    def __str__(self):
        return self.name

    @classmethod
    def list_names(cls):
        return [m.name for m in cls]


class QMethods(_ClsEnum):
    symmetric_uniform = SymmetricUniformQuantizer
    asymmetric_uniform = AsymmetricUniformQuantizer


class RangeEstimators(_ClsEnum):
    current_minmax = CurrentMinMaxEstimator
    running_minmax = RunningMinMaxEstimator
    MSE = MSE_Estimator


# ------------------------------------------------------------------------------------------------------------
# manager + module wrappers
# ------------------------------------------------------------------------------------------------------------
def _count(mod: nn.Module, name: str) -> None:  # (the counters that tests and tools read to see which kernels ran)
    mod.__dict__[name] = mod.__dict__.get(name, 0) + 1


class QuantizationManager(nn.Module):
    """estimate_ranges: every forward updates the range, then quantises; fix_ranges: quantise with frozen buffers."""

    def __init__(self, qmethod=SymmetricUniformQuantizer, init=CurrentMinMaxEstimator, per_channel=False, x_min=None, x_max=None,
                 qparams=None, init_params=None):
        super().__init__()
        self.state = Qstates.estimate_ranges
        self.qmethod, self.init, self.per_channel = qmethod, init, per_channel
        self.qparams = qparams if qparams else {}
        self.init_params = init_params if init_params else {}
        self.range_estimator = None
        self.quantizer = self.qmethod(per_channel=self.per_channel, **self.qparams)
        self.quantizer.state = self.state
        if x_min is not None and x_max is not None:
            self.set_quant_range(x_min, x_max)
            self.fix_ranges()
        else:
            self.range_estimator = self.init(per_channel=self.per_channel, quantizer=self.quantizer, **self.init_params)

    @property
    def n_bits(self):
        return self.quantizer.n_bits

    def estimate_ranges(self):
        self.state = self.quantizer.state = Qstates.estimate_ranges

    def fix_ranges(self):
        if not self.quantizer.is_initialized:
            raise QuantizerNotInitializedError()
        self.state = self.quantizer.state = Qstates.fix_ranges
        self.quantizer.fix_ranges()

    def estimate_ranges_train(self):
        self.state = self.quantizer.state = Qstates.estimate_ranges_train

    def reset_ranges(self):
        self.range_estimator.reset()
        self.quantizer.reset()
        self.estimate_ranges()

    def set_quant_range(self, x_min, x_max):
        self.quantizer.set_quant_range(x_min, x_max)

    @property
    def is_fixed(self) -> bool:
        return self.state == Qstates.fix_ranges or (self.state == Qstates.estimate_ranges_train and not self.training)

    def forward(self, x):
        if not self.is_fixed:
            self.set_quant_range(*self.range_estimator(x))
            st = getattr(self.range_estimator, "device_state", None)
            if st is not None and x.is_cuda and type(self.quantizer) is AsymmetricUniformQuantizer:
                # the range is still moving: quantise with the grid derived on the device from the estimator's float64 pair
                # (the same arithmetic as set_quant_range above) instead of reading it back for a host-side descriptor
                return ops.fake_quant_range(x, st, self.quantizer.n_bits, self.quantizer.eps)
        return self.quantizer(x)

    def extra_repr(self):
        return f"state={self.state.name}"


def _apply_qm(root: nn.Module, fn):
    for m in root.modules():
        if isinstance(m, QuantizationManager):
            fn(m)


class QuantizedModule(nn.Module):
    """Switches a module between quantised and full-precision mode (`_quant_a` / `_quant_w` buffers)."""

    def __init__(self, *args, method=AsymmetricUniformQuantizer, act_method=None, weight_range_method=CurrentMinMaxEstimator,
                 act_range_method=RunningMinMaxEstimator, n_bits=8, n_bits_act=None, per_channel_weights=False, percentile=None,
                 weight_range_options=None, act_range_options=None, scale_domain="linear", **kwargs):
        for junk in ("act_quant_dict", "quant_dict", "quant_setup", "bayesian_bits_kwargs", "prune_method", "prune_kwargs"):
            kwargs.pop(junk, None)
        super().__init__(*args, **kwargs)
        self.method = method
        self.act_method = act_method or method
        self.n_bits = n_bits
        self.n_bits_act = n_bits_act or n_bits
        self.per_channel_weights = per_channel_weights
        self.percentile = percentile
        self.weight_range_method = weight_range_method
        self.weight_range_options = weight_range_options if weight_range_options else {}
        self.act_range_method = act_range_method
        self.act_range_options = act_range_options if act_range_options else {}
        self.scale_domain = scale_domain
        self.cached_params = None
        self._caching = True
        self.register_buffer("_quant_w", torch.BoolTensor([False]))
        self.register_buffer("_quant_a", torch.BoolTensor([False]))
        self._qa = self._qw = False  # host copies of the flags (no device read per forward)
        self.act_qparams = dict(n_bits=self.n_bits_act, scale_domain=self.scale_domain, act_quant=True)
        self.weight_qparams = dict(n_bits=self.n_bits, scale_domain=self.scale_domain, act_quant=False)

    def quantized_weights(self):
        self.cached_params = None
        self._quant_w = torch.BoolTensor([True]).to(self._quant_w.device)
        self._qw = True

    def full_precision_weights(self):
        self.cached_params = None
        self._quant_w = torch.BoolTensor([False]).to(self._quant_w.device)
        self._qw = False

    def quantized_acts(self):
        self._quant_a = torch.BoolTensor([True]).to(self._quant_a.device)
        self._qa = True

    def full_precision_acts(self):
        self._quant_a = torch.BoolTensor([False]).to(self._quant_a.device)
        self._qa = False

    def quantized(self):
        self.quantized_weights()
        self.quantized_acts()

    def full_precision(self):
        self.full_precision_weights()
        self.full_precision_acts()

    def get_quantizer_status(self):
        return dict(quant_a=self._qa, quant_w=self._qw)

    def fix_ranges(self):
        _apply_qm(self, lambda m: m.fix_ranges() if m.quantizer.is_initialized else None)

    def estimate_ranges(self):
        _apply_qm(self, lambda m: m.estimate_ranges())

    def estimate_ranges_train(self):
        _apply_qm(self, lambda m: m.estimate_ranges_train() if m.quantizer.is_initialized else None)

    def train(self, mode=True):
        super().train(mode)
        if mode:
            self.cached_params = None
        return self

    def _apply(self, *args, **kwargs):
        self.cached_params = None
        return super()._apply(*args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        # a quantised checkpoint carries `_quant_a` / `_quant_w` = True: the host copies must follow the loaded buffers,
        # or the module would silently run in full precision (one device read per load, none per forward)
        super()._load_from_state_dict(*args, **kwargs)
        self.cached_params = None
        self._qa, self._qw = bool(self._quant_a.item()), bool(self._quant_w.item())

    def extra_repr(self):
        return f"weight_quant={self._qw}, act_quant={self._qa}"


class QuantizedActivation(QuantizedModule):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.activation_quantizer = QuantizationManager(qmethod=self.act_method, qparams=self.act_qparams, init=self.act_range_method,
                                                        init_params=self.act_range_options)

    def quantize_activations(self, x):
        return self.activation_quantizer(x) if self._qa else x

    def forward(self, x):
        return self.quantize_activations(x)

    def fixed_spec(self) -> Optional[FakeQuantSpec]:
        """FakeQuantSpec if this quantiser is active with frozen ranges (fusable), None if inactive."""
        return self.activation_quantizer.quantizer.spec() if self._qa else None

    @property
    def fusable(self) -> bool:
        return (not self._qa) or self.activation_quantizer.is_fixed


class QuantLinear(QuantizedModule, nn.Linear):
    """nn.Linear with fake-quantised weights (cached in eval) and fake-quantised output activations."""

    def __init__(self, *args, activation=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.activation_function = copy.deepcopy(activation) if activation else None
        self.activation_quantizer = QuantizationManager(qmethod=self.act_method, init=self.act_range_method, qparams=self.act_qparams,
                                                        init_params=self.act_range_options)
        w_init = dict(percentile=self.percentile) if self.weight_range_method is CurrentMinMaxEstimator else self.weight_range_options
        self.weight_quantizer = QuantizationManager(qmethod=self.method, init=self.weight_range_method,
                                                    per_channel=self.per_channel_weights, qparams=self.weight_qparams, init_params=w_init)

    def get_params(self):
        if not self.training and self.cached_params:
            return self.cached_params
        weight, bias = self.weight, getattr(self, "bias", None)
        if self._qw:
            weight = self.weight_quantizer(weight)
        if self._caching and not self.training and self.cached_params is None:
            self.cached_params = (weight.detach().clone(), None if bias is None else bias.detach().clone())
        return weight, bias

    def _form(self, name, build, arg=None):
        """(the weight-derived form `name`, the fp32 weight scale).  All forms live in ONE dict behind ONE watch over the weight and the weight
        quantiser's buffers (`_delta`, `_signed`: assigned afresh by every set_quant_range), plus the quantiser itself and its bit width: emptied
        when any of them changed.  A form is `build(Iw)`, Iw (N, K) fp32 the weight's integers, when first asked for or kept for another `arg`."""
        qz = self.weight_quantizer.quantizer
        forms = cached(self.__dict__, "_form_cache", (qz, getattr(qz, "n_bits", None)),
                       lambda: [(self._parameters, "weight")] + [(qz._buffers, n_) for n_ in qz._buffers], dict)
        hit = forms.get(name)
        if hit is None or hit[0] != arg:
            with torch.no_grad():
                forms.setdefault("s32", float(np.float32(float(qz.scale))))
                hit = forms[name] = (arg, build(qz.to_integer_forward(self.weight.detach())))
        return hit[1], forms["s32"]

    def _pair_weights(self):
        """[Iw ; Iw * 2^-11] (2K, N) fp16 and the fp32 weight scale, cached: the quantised weight is scale * Iw with Iw an
        8-bit integer matrix - exact in fp16 - so `ops.split_pairs(x) @ this` is the fp32 linear at fp16 matrix-core speed."""
        return self._form("pair", lambda iw: torch.cat([iw.t(), iw.t() * (1.0 / 2048.0)], dim=0).to(torch.float16).contiguous())

    def _int_weights(self):
        """The quantised weight's integers Iw (N, K) as fp16 (exact) and the fp32 weight scale, cached - the weight operand of
        `ops.proj_quant_i8`, which forms Iw * 2^-11 for the lo half of the operand pairs in registers."""
        return self._form("int", lambda iw: iw.to(torch.float16).contiguous())

    def pair_gemm_ok(self, x) -> bool:
        """fp32 inference on the GPU with per-tensor symmetric <= 8-bit weights: the operand-pair GEMM applies."""
        qz = self.weight_quantizer.quantizer
        return (PAIR_GEMM and not self.training and self._qw and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()
                and type(qz) is SymmetricUniformQuantizer and qz.is_initialized and qz.n_bits <= 8 and self.in_features % 8 == 0)

    def linear_pairs(self, x, pairs=None, raw: bool = False):
        """x @ W_q^T + b through one fp16 GEMM on operand pairs (`pairs` = ops.split_pairs(x 2-D), shared by projections of the
        same input): fp32-accurate (the weight side exactly), ~3x faster than the fp32 library GEMM at these sizes.
        raw: return (accumulator, weight scale, bias) instead - the caller folds scale and bias into its next pass."""
        ww, s32 = self._pair_weights()
        if pairs is None:
            pairs = ops.split_pairs(x.reshape(-1, x.shape[-1]))
        acc = torch.mm(pairs, ww, out_dtype=torch.float32).view(*x.shape[:-1], self.out_features)
        if raw:
            return acc, s32, self.bias
        return torch.add(self.bias.detach(), acc, alpha=s32) if self.bias is not None else acc * s32

    def _pair_gemm_quantised(self, x):
        """The pair GEMM with its epilogue in ONE pass over the accumulator (`oeh_quantize_heads_i8`, values only): weight scale,
        bias and the frozen 8-bit output quantiser.  None when that does not apply (the caller then runs the separate ops)."""
        if not self.out_fixed8 or self.activation_function is not None or self.bias is None or self.out_features % 64 != 0 or x.dim() < 2:
            return None
        acc, s32, bias = self.linear_pairs(x, raw=True)
        sp = self.activation_quantizer.quantizer.spec()
        y = ops.quantize_heads_i8(acc.reshape(1, -1, self.out_features), sp, self.out_features // 64, want_values=True, alpha=s32,
                                  bias=bias.detach(), want_indices=False)
        return y.view(*x.shape[:-1], self.out_features)

    @property
    def out_fixed8(self) -> bool:
        """The output quantiser is active, frozen, 8-bit and asymmetric: what the kernels with a quantiser epilogue take.  Call sites add
        their own conditions (whole 64-column heads, a bias, no activation function, FUSED_PROJ ...)."""
        aq = self.activation_quantizer
        return self._qa and aq.is_fixed and type(aq.quantizer) is AsymmetricUniformQuantizer and aq.quantizer.n_bits == 8

    def index_gemm_ok(self, like) -> bool:
        """`linear_index` applies: what `pair_gemm_ok` asks of the weights, for an fp32 model on the GPU."""
        return self.pair_gemm_ok(like) and self.bias is not None and self.activation_function is None

    def int8_index_ok(self, rows: int) -> bool:
        """`linear_index` on int8 centred indices applies: frozen 8-bit asymmetric output quantiser, K % 64 == 0, whole 16-row groups."""
        return (FUSED_PROJ and self.out_fixed8 and self.out_features % 64 == 0 and self.in_features % 64 == 0 and rows % 16 == 0
                and self.bias is not None and self._int8_weights_fit())

    def _int8_weights_fit(self) -> bool:
        """The weight's integers fit a SIGNED byte.  A SymmetricUniformQuantizer whose weights are all >= 0 is unsigned: its integers
        run to 255, exact in fp16 (the fp16-integer form of `linear_index` serves them) but not as int8 - 128 ... 255 would wrap
        (ADVICE r4).  One host read per state of the weight forms' watch (the signed / unsigned switch and the bit width are in it: ADVICE r5, r6)."""
        return self._form("fit", lambda iw: bool(((iw >= -128) & (iw <= 127)).all()))[0]

    def _int8_weights(self, xzero: float):
        """The weight's integers as int8 (N, K), (128 - xzero) * their row sums as int32 (N) and the fp32 weight scale, cached."""
        def build(iw):
            if not self._int8_weights_fit():
                raise ValueError("the weight's integers do not fit int8 (an unsigned grid): use the fp16 integer form (int8_index_ok)")
            return iw.to(torch.int8).contiguous(), (int(128 - int(xzero)) * iw.to(torch.int64).sum(dim=1)).to(torch.int32).contiguous()
        (iw8, add), s32 = self._form("int8", build, float(xzero))
        return iw8, add, s32

    def linear_index(self, rel, xscale: float, out_dtype=torch.float32, xzero: float = 0.0):
        """This projection of x = xscale * rel, `rel` the INTEGERS idx - zp of the producer's 8-bit quantiser as a 16-bit float
        tensor (`ops.attn_fwd_i8(..., fq.ctx_emit_index)`): x W_q^T = (xscale * w_scale) * (rel . Iw), ONE fp16 GEMM of integers
        with exact products and fp32 accumulation - half the operand-pair GEMM and no split pass - then scale, bias and the
        frozen output quantiser in one pass over the accumulator (the reference: a float GEMM of the dequantised values,
        quantized_opt.py:271; the two agree to fp32 rounding of the sum)."""
        K = self.in_features
        shape = (*rel.shape[:-1], self.out_features)
        aq = self.activation_quantizer
        fixed8 = self.out_fixed8 and self.out_features % 64 == 0
        rel2 = rel.reshape(-1, K)
        if rel2.dtype == torch.int8:
            # the producer's CENTRED indices idx - 128 (`ops.attn_fwd_i8(..., out_dtype=torch.int8)`): both sides int8 on the integer matrix
            # cores, exact int32 sums; the per-column integer (128 - zp) * sum_k Iw turns them into the sums over idx - zp
            iw8, add, s32 = self._int8_weights(xzero)
            _count(self, "_int8_index_calls")  # (tests: which form ran)
            y = ops.proj_quant_values(rel2, iw8, self._bias32(), float(np.float32(xscale) * np.float32(s32)), aq.quantizer.spec(), pairs=False, acc_add=add)
            return y.view(shape).to(out_dtype)
        if (FUSED_PROJ and fixed8 and K % 32 == 0 and rel2.shape[0] % 16 == 0 and rel2.dtype == torch.float16 and rel2.stride(1) == 1
                and self.bias is not None):
            # ONE kernel: the GEMM of integers, scale, bias and the output quantiser in its epilogue (`oeh_proj_quant_i8`, values only)
            iw, s32 = self._int_weights()
            y = ops.proj_quant_values(rel2, iw, self.bias.detach(), float(np.float32(xscale) * np.float32(s32)), aq.quantizer.spec(), pairs=False)
            return y.view(shape).to(out_dtype)
        ww, s32 = self._pair_weights()
        acc = torch.mm(rel2, ww[:K], out_dtype=torch.float32)
        alpha = float(np.float32(xscale) * np.float32(s32))
        if fixed8:
            y = ops.quantize_heads_i8(acc.view(1, -1, self.out_features), aq.quantizer.spec(), self.out_features // 64, want_values=True,
                                      alpha=alpha, bias=self.bias.detach(), want_indices=False)
            return y.view(shape).to(out_dtype)
        res = torch.add(self.bias.detach(), acc, alpha=alpha).view(shape).to(out_dtype)
        return aq(res) if self._qa else res

    def _bias32(self):
        """The bias as the kernels' epilogues read it: fp32.  An fp32 module's own tensor; a 16-bit module's converted once per bias."""
        b = self.bias.detach()
        if b.dtype == torch.float32:
            return b
        return cached(self.__dict__, "_bias32_cache", (), lambda: [(self._parameters, "bias")], lambda: self.bias.detach().to(torch.float32).contiguous())

    def _own_modules(self):
        hit = self.__dict__.get("_own_modules_cache")
        if hit is None:
            hit = self.__dict__["_own_modules_cache"] = list(self.modules())
        return hit

    def fused_act(self) -> Optional[str]:
        """The activation name `ops.act_quant` takes ("none" | "relu" | "gelu") when this module's elementwise tail - scale, bias, activation
        function, output quantiser - may run as ONE pass, else None: FUSED_FFN on, a frozen 8-bit asymmetric output quantiser, eval, no
        forward hook on the module or on a member (a hook must see its module's own output), whole 16-column chunks, and an activation the
        kernel has (the tanh GELU is not one).  Host only; `forward_index` and `forward` add what they ask of the input."""
        if not FUSED_FFN or self.training or not self.out_fixed8 or self.out_features % 16 != 0 or has_hooks(*self._own_modules()):
            return None
        f = self.activation_function
        if f is None:
            return "none"
        if type(f) is nn.ReLU:
            return "relu"
        if type(f) is nn.GELU and getattr(f, "approximate", "none") == "none":
            return "gelu"
        return None

    def _tail_input_ok(self, x) -> bool:
        return x.is_cuda and x.dtype in ops._DT and x.dim() >= 2 and x.shape[-1] == self.in_features and not ops.grad_recording(x, self.weight, self.bias)

    def _gemm_quant_index(self, x, sp):
        """Route (a) of `forward_index`: the whole module as ONE launch of `ops.proj_quant_i8` - fp32 activations, one segment, int8 out - so that
        the accumulator never reaches memory.  Only for ReLU into a grid whose zero point is 0 (`_tensorize_min_max` clamps x_min to <= 0, so a
        post-ReLU range always gives one): the quantiser's clamp at index 0 then IS the ReLU, fq(relu(v)) == fq(v) index for index, and no
        activation is computed anywhere.  A NaN value takes index 0 in the epilogue (the saturating quotient's median drops it) - what
        fq(relu(NaN)) = fq(NaN) gives in the separate ops as well.  None where the kernel does not apply."""
        K, N = self.in_features, self.out_features
        if not (FUSED_PROJ and sp.zero_point == 0.0 and self.bias is not None and self.pair_gemm_ok(x) and K % 32 == 0 and N % 64 == 0):
            return None
        x2 = x.reshape(-1, K)
        rows = x2.shape[0]
        if rows == 0 or rows % 16 != 0:
            return None
        if x2.stride(1) != 1 or (x2.stride(0) * 4) % 16 != 0:
            x2 = x2.contiguous()
        if x2.data_ptr() % 16 != 0:
            x2 = x2.clone(memory_format=torch.contiguous_format)
        iw, s32 = self._int_weights()
        try:
            idx = ops.proj_quant_i8(x2, iw, self.bias.detach(), rows // 16, 16, [(s32, sp, False, False)], pairs=True)[0]
        except _OehError as e:  # a size / alignment the kernel refuses: the GEMM + the one-pass tail
            if e.code not in (-95, -14):
                raise
            return None
        _count(self, "_gemm_quant_calls")
        return idx.permute(0, 2, 1, 3).reshape(*x.shape[:-1], N)  # (a view: the kernel wrote (rows, N))

    def _fused_tail(self, x, act: str, sp: FakeQuantSpec, want_values: bool, want_index: bool):
        """Route (b): the GEMM as the unfused forward runs it, then ONE `ops.act_quant` launch for scale, bias, activation and quantiser."""
        weight, bias = self.get_params()
        _count(self, "_act_quant_calls")
        if self.pair_gemm_ok(x):
            acc, s32, b = self.linear_pairs(x, raw=True)
            if b is not None:
                return ops.act_quant(acc, sp, act=act, alpha=s32, bias=b.detach(), want_values=want_values, want_index=want_index)
            res = acc * s32
        else:
            res = nn.functional.linear(x.contiguous(), weight.contiguous(), bias=bias)
        return ops.act_quant(res, sp, act=act, want_values=want_values, want_index=want_index)

    def forward_index(self, x):
        """This module's output as (the centred int8 indices idx - 128 of its output quantiser, that quantiser's FakeQuantSpec) - what the next
        QuantLinear's `linear_index` takes on the integer matrix cores - or None when the fused tail does not apply (`fused_act`, a GPU
        tensor outside a recorded autograd graph).  Route (a), `_gemm_quant_index`, where it applies; else route (b), `_fused_tail`."""
        act = self.fused_act()
        if act is None or not self._tail_input_ok(x):
            return None
        sp = self.activation_quantizer.quantizer.spec()
        _count(self, "_fused_ffn_calls")
        idx = self._gemm_quant_index(x, sp) if act == "relu" else None
        if idx is None:
            idx = self._fused_tail(x, act, sp, False, True)
        return idx, sp

    def int8_consumer_ok(self, rows: int) -> bool:
        """`linear_index` on a producer's int8 indices computes this module's forward: `int8_index_ok`, and what `pair_gemm_ok` asks of the
        weights and the mode - for a model of any of the three dtypes (the integer GEMM reads no float activations)."""
        qz = self.weight_quantizer.quantizer
        return (not self.training and self._qw and self.activation_function is None and type(qz) is SymmetricUniformQuantizer and qz.is_initialized
                and qz.n_bits <= 8 and self.weight.is_cuda and not ops.grad_recording(self.weight, self.bias) and not has_hooks(*self._own_modules())
                and self.int8_index_ok(rows))

    def forward(self, x, offsets=None):
        if self.activation_function is not None and FUSED_FFN:
            act = self.fused_act()
            if act is not None and self._tail_input_ok(x):
                _count(self, "_fused_ffn_calls")
                return self._fused_tail(x, act, self.activation_quantizer.quantizer.spec(), True, False)
        weight, bias = self.get_params()
        if self.pair_gemm_ok(x):
            fused = self._pair_gemm_quantised(x)
            if fused is not None:
                return fused
            res = self.linear_pairs(x)
        else:
            res = nn.functional.linear(x.contiguous(), weight.contiguous(), bias=bias)
        if self.activation_function is not None:
            res = self.activation_function(res)
        if self._qa:
            res = self.activation_quantizer(res)
        return res


class QuantLayerNorm(QuantizedModule, nn.LayerNorm):
    """nn.LayerNorm with fake-quantised gamma (cached in eval) and fake-quantised output activations (autoquant_utils.py:64-72,
    hijacker.py:78-134).  On the GPU, without autograd and with an output quantiser the kernel can apply (`fusable_out`), the forward is ONE
    launch of `ops.resid_ln_quant`; otherwise the torch ops the reference runs - F.layer_norm, then the manager (range estimation included)."""

    def __init__(self, *args, activation=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.activation_function = copy.deepcopy(activation) if activation else None
        self.activation_quantizer = QuantizationManager(qmethod=self.act_method, init=self.act_range_method, qparams=self.act_qparams,
                                                        init_params=self.act_range_options)
        w_init = dict(percentile=self.percentile) if self.weight_range_method is CurrentMinMaxEstimator else self.weight_range_options
        self.weight_quantizer = QuantizationManager(qmethod=self.method, init=self.weight_range_method,
                                                    per_channel=self.per_channel_weights, qparams=self.weight_qparams, init_params=w_init)
        self._fused_ln_calls = 0  # launches of the fused kernel from this module's own forward (tests)

    get_params = QuantLinear.get_params  # the same rule: quantise the weight when asked to, keep the pair in eval

    @property
    def fusable_out(self) -> bool:
        """The output quantiser is inactive, or frozen and asymmetric: what the kernel's epilogue takes."""
        aq = self.activation_quantizer
        return (not self._qa) or (aq.is_fixed and type(aq.quantizer) is AsymmetricUniformQuantizer)

    def out_spec(self) -> Optional[FakeQuantSpec]:
        return self.activation_quantizer.quantizer.spec() if self._qa else None

    def kernel_ok(self, x, weight, bias) -> bool:
        """`ops.resid_ln_quant` computes this module's forward on `x` (the callers that fuse a residual in front add their own conditions)."""
        return (FUSED_LN and x.is_cuda and x.dtype in ops._DT and weight is not None and self.activation_function is None
                and len(self.normalized_shape) == 1 and 1 <= self.normalized_shape[0] <= ops.LN_MAX_COLS and x.dim() >= 1
                and x.shape[-1] == self.normalized_shape[0] and self.fusable_out and not ops.grad_recording(x, weight, bias))

    def kernel_params(self, weight, bias):
        """(gamma, beta) as the kernel reads them - fp32, dense - for the pair `get_params` returned, under one watch over that pair: an
        fp32 module's cached pair is passed through as it is, a 16-bit module's is converted once."""
        src = self.__dict__.setdefault("_ln_src", {})
        src["weight"], src["bias"] = weight, bias
        f32 = lambda t: None if t is None else t.detach().reshape(-1).to(torch.float32).contiguous()  # noqa: E731
        return cached(self.__dict__, "_ln_cache", (), lambda: [(src, "weight"), (src, "bias")], lambda: (f32(weight), f32(bias)))

    def forward(self, x, offsets=None):
        weight, bias = self.get_params()
        if self.kernel_ok(x, weight, bias):
            _count(self, "_fused_ln_calls")
            g, b = self.kernel_params(weight, bias)
            return ops.resid_ln_quant(x, None, g, b, self.eps, fq_out=self.out_spec())
        res = nn.functional.layer_norm(x.contiguous(), self.normalized_shape, None if weight is None else weight.contiguous(),
                                       None if bias is None else bias.contiguous(), self.eps)
        if self.activation_function is not None:
            res = self.activation_function(res)
        if self._qa:
            res = self.activation_quantizer(res)
        return res


def resid_ln_tail(owner: nn.Module, x, residual, res_quantizer: Optional["QuantizedActivation"], ln: nn.Module, want_sum: bool = False):
    """ln(res_quantizer(x + residual)) - the tail of a quantised block (quantized_bert.py:565-571, quantized_opt.py:341-349,365-374) - as ONE
    launch where the kernel applies: both quantisers inactive or frozen and asymmetric, inference on the GPU, no forward hooks on the two
    members (a hook must see its module's own output).  `owner`._fused_ln_calls counts those launches.  residual / res_quantizer may be None.
    Returns y, or (the quantised sum, y) with want_sum."""
    if isinstance(ln, QuantLayerNorm) and not owner.training and (residual is None or (residual.shape == x.shape and residual.dtype == x.dtype)):
        rq_ok = res_quantizer is None or (res_quantizer.fusable and (not res_quantizer._qa or type(res_quantizer.activation_quantizer.quantizer) is AsymmetricUniformQuantizer))
        mods = (ln,) if res_quantizer is None else (ln, res_quantizer)
        if rq_ok and not has_hooks(*mods):
            weight, bias = ln.get_params()
            if ln.kernel_ok(x, weight, bias) and not ops.grad_recording(residual):
                _count(owner, "_fused_ln_calls")
                g, b = ln.kernel_params(weight, bias)
                return ops.resid_ln_quant(x, residual, g, b, ln.eps, fq_sum=None if res_quantizer is None else res_quantizer.fixed_spec(),
                                          fq_out=ln.out_spec(), want_sum=want_sum)
    s = x if residual is None else x + residual
    if res_quantizer is not None:
        s = res_quantizer(s)
    y = ln(s)
    return (s, y) if want_sum else y


class FP32Acts(nn.Module):
    """The reference's pass-through in the place of an activation quantiser (base_quantized_classes.py:202-207): no ranges, no state."""

    def forward(self, x):
        return x

    def reset_ranges(self):
        pass


class QuantEmbedding(QuantizedModule, nn.Embedding):
    """nn.Embedding with a fake-quantised table (autoquant_utils.py:75-95).  Its output is NOT quantised again - a looked-up row of a quantised
    table is already on the grid - so the activation quantiser is the pass-through.  forward: F.embedding on the (in eval: cached)
    fake-quantised table.  The fused front (`embed_front`) does not read that fp32 copy: `kernel_table` hands the kernel the int8 indices of
    the frozen grid, or the raw table with the grid to apply on the fly."""

    def __init__(self, *args, activation=None, **kwargs):
        super().__init__(*args, **kwargs)
        if self.max_norm is not None:
            raise NotImplementedError("QuantEmbedding: max_norm renormalises the table in place during the forward; not implemented")
        self.activation_function = None
        w_init = dict(percentile=self.percentile) if self.weight_range_method is CurrentMinMaxEstimator else self.weight_range_options
        self.weight_quantizer = QuantizationManager(qmethod=self.method, init=self.weight_range_method,
                                                    per_channel=self.per_channel_weights, qparams=self.weight_qparams, init_params=w_init)
        self.activation_quantizer = FP32Acts()

    get_params = QuantLinear.get_params  # the same rule: quantise the table when asked to, keep it in eval (there is no bias)

    def _index_table(self):
        """(int8 indices of the table or None where the grid's integers do not fit a signed byte, fp32 scale, int_min, int_max) of the weight
        quantiser's current grid, built once per (table, range) under one watch - the table, the quantiser's buffers, the quantiser, its bits."""
        qz = self.weight_quantizer.quantizer

        def build():
            with torch.no_grad():
                lo, hi = float(qz.int_min), float(qz.int_max)
                fits = lo >= -128.0 and hi <= 127.0
                idx = qz.to_integer_forward(self.weight.detach()).to(torch.int8).contiguous() if fits else None
                return idx, float(np.float32(float(qz.scale))), lo, hi
        return cached(self.__dict__, "_i8_table", (qz, getattr(qz, "n_bits", None)),
                      lambda: [(self._parameters, "weight")] + [(qz._buffers, n_) for n_ in qz._buffers], build)

    def kernel_table(self):
        """This table as `ops.embed_sum_quant` gathers from it: (tensor, scale or None, int_min, int_max).  Full-precision weights: the table as
        it is.  Quantised weights on a frozen per-tensor symmetric grid: its int8 indices with the scale - or, where the integers do not fit a
        signed byte, the raw table with the grid to apply to the gathered rows.  Anything else (a range still being estimated, another weight
        quantiser): the fake-quantised table of `get_params`, range estimation included, as it is."""
        if not self._qw:
            return self.weight.detach(), None, 0.0, 0.0
        mgr = self.weight_quantizer
        if mgr.is_fixed and type(mgr.quantizer) is SymmetricUniformQuantizer and mgr.quantizer.is_initialized:
            idx, scale, lo, hi = self._index_table()
            return (idx if idx is not None else self.weight.detach()), scale, lo, hi
        return self.get_params()[0].detach(), None, 0.0, 0.0

    def forward(self, x, offsets=None):
        weight, _ = self.get_params()
        res = nn.functional.embedding(x.contiguous(), weight.contiguous(), self.padding_idx, None, self.norm_type, self.scale_grad_by_freq, self.sparse)
        if self._qa:
            res = self.activation_quantizer(res)
        return res


def _sum_quantizer_ok(q: "QuantizedActivation") -> bool:
    return q.fusable and (not q._qa or type(q.activation_quantizer.quantizer) is AsymmetricUniformQuantizer)


def embed_front(owner: nn.Module, lookups, sum_quantizers, ln: Optional[nn.Module] = None):
    """ln(q_k(... q_1(E_0[ids_0] + E_1[ids_1]) ... + E_k[ids_k])) - the front of a quantised model - as ONE launch of `ops.embed_sum_quant`
    where the kernel applies, else None (the caller then runs the torch ops the reference runs).  lookups: (QuantEmbedding, ids) pairs, the
    first possibly (None, inputs_embeds); sum_quantizers: one QuantizedActivation per lookup after the first; ln: a QuantLayerNorm or None.
    The kernel applies to GPU tensors of a supported dtype, outside training, with no autograd recording on the tables or inputs_embeds, every
    active sum / output quantiser frozen and asymmetric, no forward hooks on the members, rows of at most 8192 elements.
    `owner`._fused_embed_calls counts the launches."""
    if not FUSED_EMBED or owner.training:
        return None
    mods = [m for m, _ in lookups if m is not None] + list(sum_quantizers) + ([ln] if ln is not None else [])
    if has_hooks(*mods) or not all(_sum_quantizer_ok(q) for q in sum_quantizers):
        return None
    if any(m is not None and (not isinstance(m, QuantEmbedding) or m.training) for m, _ in lookups):
        return None
    if ln is not None and not (isinstance(ln, QuantLayerNorm) and ln.activation_function is None and len(ln.normalized_shape) == 1 and ln.fusable_out
                               and ln.weight is not None):
        return None
    first = lookups[0][1] if lookups[0][0] is None else lookups[0][0].weight
    dtype, cols = first.dtype, first.shape[-1]
    if dtype not in ops._DT or not 1 <= cols <= ops.LN_MAX_COLS or (ln is not None and ln.normalized_shape[0] != cols):
        return None
    args, watched = [], []
    for m, ids in lookups:
        if m is None:
            if not ids.is_cuda or ids.dim() != 3:
                return None
            watched.append(ids)
            continue
        if not (m.weight.is_cuda and ids.is_cuda and ids.dim() == 2 and ids.dtype in (torch.int32, torch.int64) and m.weight.dtype == dtype
                and m.weight.shape[-1] == cols):
            return None
        watched.append(m.weight)
    gamma = beta = None
    if ln is not None:
        weight, bias = ln.get_params()
        if not weight.is_cuda or ops.grad_recording(weight, bias):
            return None
        gamma, beta = ln.kernel_params(weight, bias)
    if ops.grad_recording(*watched):
        return None
    for m, ids in lookups:
        if m is None:
            args.append(ops.EmbedLookup(ids))
        else:
            table, scale, lo, hi = m.kernel_table()
            args.append(ops.EmbedLookup(table, ids, scale, lo, hi))
    _count(owner, "_fused_embed_calls")
    return ops.embed_sum_quant(args, gamma, beta, ln.eps if ln is not None else 0.0, fq_sums=[q.fixed_spec() for q in sum_quantizers],
                               fq_out=ln.out_spec() if ln is not None else None, dtype=dtype)


def quantize_model(model: nn.Module, **quant_params) -> nn.Module:
    """The cases of the reference's recursive rewriter (autoquant_utils.py:236-270) that the attention classes and the block tails need:
    nn.Linear (query/key/value, q_proj/k_proj/v_proj/out_proj, dense, fc2), nn.LayerNorm, nn.Embedding (the model fronts), and
    Sequential(Linear, ReLU | GELU) - OPT's fc1 (quantized_opt.py:292-294) and BERT's intermediate (quantized_bert.py:609-617) with the
    activation folded into the QuantLinear."""
    def copy_params(q, src, clone):
        q.weight.data = src.weight.data.clone() if clone else src.weight.data
        if getattr(src, "bias", None) is not None:
            q.bias.data = src.bias.data.clone() if clone else src.bias.data
        return q.to(src.weight.device)

    if type(model) is nn.Linear:
        return copy_params(QuantLinear(model.in_features, model.out_features, bias=model.bias is not None, **quant_params), model, False)
    if type(model) is nn.Embedding:
        q = QuantEmbedding(model.num_embeddings, model.embedding_dim, padding_idx=model.padding_idx, max_norm=model.max_norm, norm_type=model.norm_type,
                           scale_grad_by_freq=model.scale_grad_by_freq, sparse=model.sparse, **quant_params)
        return copy_params(q, model, False)
    if type(model) is nn.LayerNorm and model.elementwise_affine:
        return copy_params(QuantLayerNorm(model.normalized_shape, eps=model.eps, **quant_params), model, False)
    if type(model) is nn.Sequential and len(model) == 2 and type(model[0]) is nn.Linear and isinstance(model[1], (nn.ReLU, nn.GELU)):
        lin = model[0]
        q = QuantLinear(lin.in_features, lin.out_features, bias=lin.bias is not None, activation=model[1], **quant_params)
        return nn.Sequential(copy_params(q, lin, True))
    raise NotImplementedError(f"quantize_model: {type(model).__name__} is outside the attention path, the block tails and the embeddings")


class QuantizedModel(nn.Module):
    """Convenience switches over every QuantizedModule inside (base_quantized_model.py:18-162)."""

    def _each(self, fn):
        for m in self.modules():
            if isinstance(m, QuantizedModule):
                fn(m)

    def quantized_weights(self):
        self._each(lambda m: m.quantized_weights())

    def full_precision_weights(self):
        self._each(lambda m: m.full_precision_weights())

    def quantized_acts(self):
        self._each(lambda m: m.quantized_acts())

    def full_precision_acts(self):
        self._each(lambda m: m.full_precision_acts())

    def quantized(self):
        self._each(lambda m: m.quantized())

    def full_precision(self):
        self._each(lambda m: m.full_precision())

    def fix_ranges(self):
        _apply_qm(self, lambda m: m.fix_ranges() if m.quantizer.is_initialized else None)

    def estimate_ranges(self):
        _apply_qm(self, lambda m: m.estimate_ranges())

    def estimate_ranges_train(self):
        _apply_qm(self, lambda m: m.estimate_ranges_train() if m.quantizer.is_initialized else None)

    def set_quant_state(self, weight_quant, act_quant):
        (self.quantized_acts if act_quant else self.full_precision_acts)()
        (self.quantized_weights if weight_quant else self.full_precision_weights)()


# ------------------------------------------------------------------------------------------------------------
# the two quantised attention classes; before them, the frozen-range INT8 layer as a PLAN (round 5; VERDICT r4 weak #9: the eager quantised modules were host-bound - 97 us per BERT-base layer for
# 46 us of GPU work, 132 us per OPT-125m layer for 107).  `_int8_storage_core` is ~80 Python statements of eligibility checks, cache look-ups,
# descriptor filling and allocations around three launches; once the ranges are frozen nothing of that changes from one forward to the next except
# the input's address.  After a successful run the three C calls are kept PREBUILT (ops: `_prepared` forms): the int8 q / k / v^T index buffers and
# (OPT) the int8 context are the plan's own - stream-ordered reuse, keyed by stream -, a forward then allocates only what it returns, patches four or
# five pointers and launches.  A plan is valid for ONE input geometry and ONE state of the module: every tensor whose value was baked in (weights,
# biases, every quantiser's range buffers) is watched (_watch.TensorWatch: object, version counter, address), the quantisation state flags, training mode, forward hooks and
# this file's feature switches are re-checked on every call; anything else rebuilds it through the full path.
# ------------------------------------------------------------------------------------------------------------
I8_PLAN = True


class _I8LayerPlan:
    __slots__ = ("xkey", "flags", "watch", "hookmods", "mods", "stream", "padkey", "proj", "attn", "outp", "bufs", "B", "T", "E", "H", "want_values", "hdtype", "as_index")

    @staticmethod
    def survey(owner, lins, consumer, slots=None):
        """ONE pass over what a plan bakes in - the projections, the consumer, their two managers each, the three activation quantisers:
        returns the state flags (a tuple, only ever compared for equality) and appends every tensor slot to `slots` (for the watch) when given."""
        flags = [owner.training, INT8_STORAGE, INDEX_GEMM, FUSED_PROJ, PAIR_GEMM, I8_PLAN]
        managers = []
        for m in (*lins, consumer):
            if m is not None:
                flags += [m.training, m._qa, m._qw]
                managers += [m.weight_quantizer, m.activation_quantizer]
                if slots is not None:
                    slots += [(m._parameters, "weight"), (m._parameters, "bias")]
        for aq in (owner.attn_scores_act_quantizer, owner.attn_probs_act_quantizer, owner.context_act_quantizer):
            flags.append(aq._qa)
            managers.append(aq.activation_quantizer)
        for mg in managers:   # (type, n_bits, eps: Python attributes baked into the plan's specs - no buffers, the watch cannot see them)
            qz = mg.quantizer
            flags += [mg.state, type(qz).__name__, getattr(qz, "n_bits", None), getattr(qz, "eps", None)]
            if slots is not None:
                slots += [(qz._buffers, n_) for n_ in qz._buffers]
        return tuple(flags)

    def valid(self, owner, x, lins, consumer, padvec, stream) -> bool:
        if self.xkey != (x.shape, x.stride(), x.dtype, x.device) or self.stream != stream or (x.data_ptr() & 15) or x.device.index != torch.cuda.current_device():
            return False
        if self.mods != (*lins, consumer) or self.padkey != (None if padvec is None else (padvec.dtype, padvec.shape, padvec.stride())):   # (modules compare by identity: a projection swapped for another)
            return False
        if self.flags != self.survey(owner, lins, consumer):
            return False
        # The plan replays forward-only kernels: when autograd is recording and the input or a watched parameter requires grad, the full
        # path must run - it raises / takes the differentiable route as before (a plan built under no_grad used to be
        # replayed here and returned tensors without grad_fn - gradients dropped silently).  The predicate of ops.grad_recording.
        if torch.is_grad_enabled() and (x.requires_grad or any(t_.requires_grad for t_ in self.watch.tensors())):
            return False
        return self.watch.unchanged() and not has_hooks(*self.hookmods)

    @staticmethod
    def replay(owner, ckey, x, lins, consumer, padvec):
        """The owner's plan run on `x` when it was built for this call (`ckey`) and is still valid, else None -> the full path.  Never under
        stream capture: the full path's intermediates then live in the graph's own pool, not in buffers a later plan rebuild would free."""
        kept = owner.__dict__.get("_oeh_i8_plan")
        if kept is None or kept[0] != ckey or torch.cuda.is_current_stream_capturing():
            return None
        stream = ops._stream()
        if not kept[1].valid(owner, x, lins, consumer, padvec, stream.value):
            return None
        for name in ("_i8_plan_runs", "_i8_calls", "_fused_proj_calls"):
            _count(owner, name)
        if kept[1].as_index:
            _count(owner, "_index_gemm_calls")
            _count(consumer, "_int8_index_calls")
        return kept[1].run(x, padvec, stream)

    @staticmethod
    def _launch(prepared, stream, what):
        rc = prepared[0](*prepared[1], stream)
        if rc != 0:
            ops._lib.check(rc, what)

    def run(self, x, padvec, stream):
        B, T, E = self.B, self.T, self.E
        self.proj[1][0] = ops._ptr(x)
        yk = yv = None
        if self.want_values:
            yk, yv = torch.empty((B, T, E), dtype=torch.float32, device=x.device), torch.empty((B, T, E), dtype=torch.float32, device=x.device)
            self.proj[2][1].y, self.proj[2][2].y = yk.data_ptr(), yv.data_ptr()
        self._launch(self.proj, stream, "oeh_proj_quant_i8 (plan)")
        if padvec is not None:
            self.attn[2][0].key_pad_mask = padvec.data_ptr()
        if self.as_index:   # OPT: int8 context (the plan's buffer) -> out_proj on the integer matrix cores -> a fresh fp32 output
            self._launch(self.attn, stream, "oeh_attn_fwd (plan)")
            y = torch.empty((B * T, E), dtype=torch.float32, device=x.device)
            self.outp[2][0].y = y.data_ptr()
            self._launch(self.outp, stream, "oeh_proj_quant_i8 (plan, out_proj)")
            return y.view(B, T, E).to(self.hdtype), (yk, yv), True
        out = torch.empty((B, T, E), dtype=self.hdtype, device=x.device)   # (B, Sq, H, D)-contiguous: the merged context
        self.attn[1][4] = ops._ptr(out)
        self._launch(self.attn, stream, "oeh_attn_fwd (plan)")
        return out, (yk, yv), False

    @classmethod
    def build(cls, owner, x, lins, consumer, H, consts, grids, attn_kw, want_values, as_index, hookmods):
        """The three launches of the run that has just succeeded, prebuilt: same operands (`consts`: the fused projection's weights, biases and
        segments), same descriptors (`attn_kw`: the core's keywords as called) - only where the outputs go differs (the int8 intermediates into the plan's own buffers).
        Each of `proj`, `attn`, `outp` is ops' `_prepared` form: [fn, mutable argument list, what is patched per call (segment array / descriptors), ...]."""
        B, T, K = x.shape
        E, dev = H * 64, x.device
        padvec, fq_call = attn_kw["key_pad_mask"], attn_kw["fq"]
        pl = cls()
        pl.B, pl.T, pl.E, pl.H, pl.want_values, pl.hdtype, pl.as_index = B, T, E, H, bool(want_values), x.dtype, bool(as_index)
        qi, ki = torch.empty((B, T, E), dtype=torch.int8, device=dev), torch.empty((B, T, E), dtype=torch.int8, device=dev)
        vt = torch.empty((B, H, 64, T), dtype=torch.int8, device=dev)
        ytmp = torch.empty((B, T, E), dtype=torch.float32, device=dev) if want_values else None   # (pointer patched per call)
        pl.proj = []
        ops.proj_quant_i8(x.view(B * T, K), *consts, pairs=True, _outs=[(qi, None), (ki, ytmp), (vt, ytmp)], _prepared=pl.proj)
        heads = lambda t: t.view(B, T, H, 64).permute(0, 2, 1, 3)  # noqa: E731
        # as_index: the int8 context is the plan's own buffer; else the output's pointer is patched per call
        ctx8 = torch.empty((B, T, H, 64), dtype=torch.int8, device=dev) if as_index else None
        out_t = (ctx8 if as_index else torch.empty((B, T, H, 64), dtype=x.dtype, device=dev)).permute(0, 2, 1, 3)
        pl.attn = []
        ops.attn_fwd_i8(heads(qi), heads(ki), vt, grids, out=out_t, _prepared=pl.attn, **attn_kw)
        pl.attn[1] = list(pl.attn[1])   # (the argument tuple, made patchable)
        pl.outp = None
        if as_index:
            iw8, add, s32 = consumer._int8_weights(fq_call.ctx.zero_point)
            pl.outp = []
            ops.proj_quant_values(ctx8.view(B * T, E), iw8, consumer.bias.detach(), float(np.float32(fq_call.ctx.scale) * np.float32(s32)),
                                  consumer.activation_quantizer.quantizer.spec(), pairs=False, acc_add=add, _prepared=pl.outp)
        pl.bufs = (qi, ki, vt, ctx8)
        pl.xkey, pl.stream = (x.shape, x.stride(), x.dtype, x.device), ops._stream().value
        pl.padkey = None if padvec is None else (padvec.dtype, padvec.shape, padvec.stride())
        slots = []
        pl.flags = cls.survey(owner, lins, consumer, slots)
        pl.watch = TensorWatch(slots)
        pl.hookmods = hookmods
        pl.mods = (*lins, consumer)
        return pl


class _QuantAttnBase(GateBookkeeping, QuantizedModel):
    def _init_common(self, org_model, quant_params):
        self.attn_scores_act_quantizer = QuantizedActivation(**quant_params)
        self.attn_probs_act_quantizer = QuantizedActivation(**quant_params)
        self.context_act_quantizer = QuantizedActivation(**quant_params)
        self.softmax_fn = org_model.softmax_fn
        for name in GATE_ATTRS:  # the gate is not quantised (quantized_bert.py:256)
            setattr(self, name, getattr(org_model, name))
        self.last_gate_avg_prob = None
        self.last_gate_all_probs = None

    def _fq(self, ctx_before_gate: bool) -> Optional[AttnFakeQuant]:
        trio = (self.attn_scores_act_quantizer, self.attn_probs_act_quantizer, self.context_act_quantizer)
        if not all(t.fusable for t in trio):
            return None  # still estimating ranges: the tensors must be materialised
        return AttnFakeQuant(trio[0].fixed_spec(), trio[1].fixed_spec(), trio[2].fixed_spec(), ctx_before_gate=ctx_before_gate)

    def _calibrate_fused(self, q, k, v, *, scale=1.0, scale_div=0.0, attention_mask=None, clamp_min=False, detect_causal=False):
        """Qstates.estimate_ranges without the (B,H,Sq,Sk) tensors (VERDICT r2 missing #3; range_estimators.py:83-106 as driven by
        transformers_language/utils.py:50-71): the score quantiser's percentile range, then - with the scores quantised on that
        fresh range - the probability quantiser's, from `ops.attn_calibrate`, which recomputes the values tile by tile for every pass
        of the exact selection; then the context with both quantisers applied.  The recomputed values are fp32 from the stored
        (16-bit or fp32) q / k - what the fused eval kernels quantise; the observable path hands the estimators scores and
        probabilities ROUNDED to a 16-bit storage dtype, so for fp16 / bf16 modules the two paths' ranges differ by up to one storage
        ulp of the percentile value (2^-11 / 2^-8 relative; the context quantiser, which sees the rounded probabilities' product, up to 1 %
        in bf16 - tests/test_modules_gpu.py::test_fused_calibration_vs_observable_16bit).
        Returns the context (B,H,Sq,D) in q's dtype, or None when this does not apply (a quantiser that is off or already fixed, min-max estimators, host-side estimator state,
        an unregistered softmax, ...): the caller then runs the observable path."""
        if not FUSED_CALIBRATION or not q.is_cuda or q.dtype not in (torch.float16, torch.bfloat16, torch.float32) or q.shape[-1] not in (32, 64, 128):
            return None
        spec = spec_of(self.softmax_fn)
        mgrs = [m.activation_quantizer for m in (self.attn_scores_act_quantizer, self.attn_probs_act_quantizer)]
        if spec is None or not (self.attn_scores_act_quantizer._qa and self.attn_probs_act_quantizer._qa):
            return None
        for mg in mgrs:
            est = mg.range_estimator
            if (mg.is_fixed or type(mg.quantizer) is not AsymmetricUniformQuantizer or not isinstance(est, RunningMinMaxEstimator) or not est.percentile
                    or est.momentum is None or (est.current_xmin is not None and est.device_state is None)):
                return None
        # forward hooks on the quantiser modules (attach_act_hooks registers one on every named module) see the score / probability
        # tensors only on the observable path
        hooked = [m for aq in (self.attn_scores_act_quantizer, self.attn_probs_act_quantizer) for m in aq.modules()]
        if has_hooks(*hooked):
            return None
        B, H, Sq, D = q.shape
        Sk = k.shape[2]
        if B * H * Sq * Sk >= 2 ** 32:
            return None
        pad, full, causal, mask_min = resolve_mask(attention_mask, B, Sq, Sk, q.dtype, detect_causal)
        kw = dict(softmax=spec, scale=scale, scale_div=scale_div, key_pad_mask=pad, full_mask=full, causal=causal, clamp_min=clamp_min, mask_min=mask_min)
        states = []
        for which, mg in enumerate(mgrs):
            est, qz = mg.range_estimator, mg.quantizer
            first = est.device_state is None or est.device_state.device != q.device
            if first:
                est.device_state = torch.empty(2, dtype=torch.float64, device=q.device)
            ops.attn_calibrate(q, k, None, which, scores_range=states[0] if which == 1 else None, n_bits=qz.n_bits, eps=qz.eps,
                               q_lo=100 - est.percentile, q_hi=est.percentile, momentum=est.momentum, first=first, state=est.device_state, **kw)
            est.current_xmin, est.current_xmax = est.device_state[0].clone(), est.device_state[1].clone()
            mg.set_quant_range(est.current_xmin, est.current_xmax)  # the buffers the state dict / fix_ranges read (device arithmetic, no sync)
            states.append(est.device_state)
        qz = mgrs[0].quantizer
        ctx = ops.attn_calibrate(q, k, v, ops.CALIB_CONTEXT, scores_range=states[0], probs_range=states[1], n_bits=qz.n_bits, eps=qz.eps, **kw)
        _count(self, "_fused_calib_calls")  # (tests: which path ran)
        return ctx.to(q.dtype)

    def _qkv_pair_weights(self, lins):
        """The three projections' operand-pair weights (`QuantLinear._pair_weights`) side by side, (2K, 3E) fp16, and their fp32
        weight scales; rebuilt when any of the three was (a changed weight or weight range rebuilds that projection's own cache)."""
        parts = [m._pair_weights() for m in lins]
        hit = self.__dict__.get("_qkv_pair_cache")
        if hit is None or any(a is not b for a, (b, _) in zip(hit[0], parts)):
            hit = (tuple(p[0] for p in parts), torch.cat([p[0] for p in parts], dim=1).contiguous())
            self.__dict__["_qkv_pair_cache"] = hit
        return hit[1], [p[1] for p in parts]

    def _qkv_int_weights(self, lins):
        """The three projections' integer weights one after the other, (3E, K) fp16, their biases (3E) fp32 and their fp32 weight
        scales (`ops.proj_quant_i8`); rebuilt when a weight, a weight range or a bias changed."""
        parts = [m._int_weights() for m in lins]
        hit = self.__dict__.get("_qkv_int_cache")
        if hit is None or not hit[1].unchanged() or any(a is not b for a, (b, _) in zip(hit[0], parts)):
            with torch.no_grad():
                hit = (tuple(p[0] for p in parts), TensorWatch([(m._parameters, "bias") for m in lins]), torch.cat([p[0] for p in parts], dim=0).contiguous(),
                       torch.cat([m.bias.detach().float() for m in lins]).contiguous())
            self.__dict__["_qkv_int_cache"] = hit
        return hit[2], hit[3], [p[1] for p in parts]

    def _int8_storage_core(self, hidden_states, lins, H, head_dim, *, scale, scale_div, causal, padvec, mask_min, gate, fq, want_values,
                           consumer=None):
        """the q/k/v projections are QuantLinear - their outputs ARE 8-bit indices on calibrated grids
        (hijacker.py:78-127; quantized_opt.py:67-75, quantized_bert.py:236-238) - so the attention core takes the indices
        themselves and runs both products on the integer matrix cores (`ops.attn_fwd_i8`, include/oeh.h dtype OEH_I8).  Applies
        when the three output quantisers are 8-bit with frozen ranges, head_dim = 64, the softmax is unclipped or clipped with gamma <= 0 and the mask is
        none / causal / a key-padding vector of 0 / finfo.min entries (`padvec`, vouched for by the caller); returns the
        merged context (B, T, E) and the (k, v) float values (`want_values`: a decoder's cache), or None -> the caller runs the
        fake-quant path on floats.  `consumer`: the QuantLinear that takes the context next (OPT's out_proj); when the context
        quantiser is the core's last op the core hands it the quantiser's integers (`ctx_emit_index`) and the returned tensor is
        the consumer's OUTPUT (`QuantLinear.linear_index`), marked by the third element of the result.
        In steps: a plan of an earlier identical call replayed (_I8LayerPlan) | does the route apply | project | core and consumer | keep a plan."""
        if not INT8_STORAGE or not hidden_states.is_cuda or head_dim != 64:
            return None
        ckey = (H, float(scale), float(scale_div), bool(causal), float(mask_min), bool(want_values), fq.ctx_before_gate, id(consumer), self.softmax_fn)
        if I8_PLAN and gate is None:
            done = _I8LayerPlan.replay(self, ckey, hidden_states, lins, consumer, padvec)
            if done is not None:
                return done
        applies = self._int8_route_applies(hidden_states, lins, consumer, fq)
        if applies is None:
            return None
        bypassed, spec = applies
        outs, grids, consts = self._int8_project(hidden_states, lins, H, want_values)
        as_index = (INDEX_GEMM and consumer is not None and fq.ctx is not None and fq.ctx.qmax == 255.0 and (gate is None or not fq.ctx_before_gate)
                    and isinstance(consumer, QuantLinear) and consumer.in_features == H * head_dim and consumer.index_gemm_ok(hidden_states))
        # ... as int8 centred indices when the consumer takes them on the integer matrix cores (K % 64 == 0, a whole zero point), else as
        # the integers idx - zp in fp16
        as_int8 = as_index and consumer.int8_index_ok(hidden_states.shape[0] * hidden_states.shape[1]) and float(fq.ctx.zero_point) == float(int(fq.ctx.zero_point))
        attn_kw = dict(fq=dataclasses.replace(fq, ctx_emit_index=True) if as_index else fq,
                       out_dtype=(torch.int8 if as_int8 else torch.float16) if as_index else hidden_states.dtype, softmax=spec,
                       scale=scale, scale_div=scale_div, causal=causal, clamp_min=causal or padvec is not None, mask_min=mask_min, gate=gate, key_pad_mask=padvec)
        result = self._int8_core_and_consumer(hidden_states, outs, grids, consumer if as_index else None, fq, want_values, attn_kw)
        if (result is not None and I8_PLAN and gate is None and consts is not None and (as_int8 if as_index else consumer is None)
                and hidden_states.is_contiguous() and hidden_states.dtype == torch.float32 and not torch.cuda.is_current_stream_capturing()
                and hidden_states.device.index == torch.cuda.current_device()
                and (padvec is None or (padvec.dtype in (torch.float16, torch.float32) and padvec.shape == hidden_states.shape[:2] and padvec.stride(1) == 1))):
            try:
                self.__dict__["_oeh_i8_plan"] = (ckey, _I8LayerPlan.build(self, hidden_states, lins, consumer, H, consts, grids, attn_kw, want_values, as_index, bypassed))
            except _OehError as e:   # (a geometry one of the prepared calls refuses: every forward keeps taking the full path)
                self.__dict__["_oeh_i8_plan"] = None
                self.__dict__["_oeh_i8_plan_error"] = str(e)
        return result

    def _int8_route_applies(self, x, lins, consumer, fq):
        """Step 1 (after the switches, the device and the head dim): None when the route does not apply, else (the flattened list of the modules
        it bypasses, the softmax spec).  This path reads the QuantLinear weights and quantiser grids directly: the forwards of the projections, of the consumer and
        of the three activation quantisers never run, so forward hooks on any of them (attach_act_hooks registers one on every
        named module) would be bypassed silently - the module path then (as bert_attention.py / opt_attention.py do).
        (The flattened module list is remembered per set of top modules: walking `.modules()` of seven modules was a sixth of this
        path's host time, and the eager forward is host-bound; hooks registered later on any of them are still seen - the hook
        dictionaries are read on every call - only a submodule swapped in afterwards under the same top module would not be.)"""
        tops = (*lins, consumer, self.attn_scores_act_quantizer, self.attn_probs_act_quantizer, self.context_act_quantizer)
        bkey = tuple(id(t) for t in tops)
        bhit = self.__dict__.get("_bypassed_cache")
        if bhit is None or bhit[0] != bkey:
            bhit = (bkey, [m for top in tops if top is not None for m in top.modules()])
            self.__dict__["_bypassed_cache"] = bhit
        if has_hooks(*bhit[1]):
            return None
        spec, tgt_len = spec_of(self.softmax_fn), x.shape[1]
        if spec is None or (spec.clip and spec.gamma > 0.0) or tgt_len % 16 != 0 or tgt_len > 512 or fq.probs is None or fq.probs.qmax != 255.0 or fq.scores is None:
            return None
        # (`out_fixed8` asks for the asymmetric quantiser too - what every route below needs for its `spec()`)
        if not all(isinstance(m, QuantLinear) and m.out_fixed8 and m.activation_function is None for m in lins):
            return None
        return bhit[1], spec

    def _int8_project_fused(self, x, lins, specs, want_values):
        """fp32 model, ONE kernel: the pair GEMM against the three integer weight matrices with weight scale, bias and the three output
        quantisers in its epilogue (`oeh_proj_quant_i8`) - the (B*T, 3E) accumulator never reaches memory.  The fp32 activations go in as
        they are: the (hi, lo) operand split happens when a wave reads its fragments - the same values as `ops.split_pairs` would write,
        without the pass.  Returns (outs, the call's constant arguments for a plan - only for an input used as it is), or (None, None) when the kernel refuses."""
        bsz, tgt_len, K_in = x.shape
        x2 = x.reshape(-1, K_in)
        if x2.stride(1) != 1 or (x2.stride(0) * 4) % 16 != 0:
            x2 = x2.contiguous()
        if x2.data_ptr() % 16 != 0:   # (a view at an odd storage offset: the kernel's 16-byte row loads need an aligned copy)
            x2 = x2.clone(memory_format=torch.contiguous_format)
        w3, b3, scales3 = self._qkv_int_weights(lins)
        # per projection: (weight scale, output grid, transposed - v for the core -, float values too - k, v of a decoder's cache)
        consts = (w3, b3, bsz, tgt_len, [(scales3[n_], specs[n_], n_ == 2, n_ > 0 and want_values) for n_ in range(3)])
        try:
            outs = ops.proj_quant_i8(x2, *consts, pairs=True)
        except _OehError as e:  # a size / alignment the fused kernel refuses (32-bit lane offsets ...): the library pair GEMM
            if e.code not in (-95, -14):
                raise
            return None, None
        _count(self, "_fused_proj_calls")  # (tests: which path ran; counted even when the core refuses afterwards)
        return outs, (consts if x2.data_ptr() == x.data_ptr() else None)

    def _int8_project(self, x, lins, H, want_values):
        """Step 2: q, k, v^T as centred int8 indices in the core's layout [+ the k, v floats of a decoder's cache], by the first route that
        applies: the fused kernel | one pair GEMM for all three projections | projection by projection - GEMM, then ONE kernel
        (`oeh_quantize_heads_i8`).  Returns (outs, the three grids, the plan's constants or None)."""
        bsz, tgt_len, K_in, E = *x.shape, H * 64
        specs = [m.activation_quantizer.quantizer.spec() for m in lins]
        grids = [ops.QuantGrid.of(sp) for sp in specs]
        all_pairs = all(m.pair_gemm_ok(x) and m.bias is not None for m in lins)
        if FUSED_PROJ and all_pairs and K_in % 32 == 0 and all(m.in_features == K_in and m.out_features == E for m in lins):
            outs, consts = self._int8_project_fused(x, lins, specs, want_values)
            if outs:
                return outs, grids, consts
        pairs = acc3 = None
        if all_pairs:
            # fp32 model: the input as fp16 operand pairs, split once, and ONE fp16 GEMM against the three integer weight
            # matrices side by side; each projection's weight scale and bias are folded into its quantiser pass
            pairs = ops.split_pairs(x.reshape(-1, K_in))
            ww3, scales3 = self._qkv_pair_weights(lins)
            acc3 = torch.mm(pairs, ww3, out_dtype=torch.float32).view(bsz, tgt_len, 3 * E)
        outs = []
        for n_, m in enumerate(lins):
            alpha, qbias = 1.0, None
            if acc3 is not None:
                res, alpha, qbias = acc3[..., n_ * E:(n_ + 1) * E], scales3[n_], m.bias.detach()
            elif m.pair_gemm_ok(x) and m.bias is not None:
                if pairs is None:
                    pairs = ops.split_pairs(x.reshape(-1, K_in))
                res, alpha, qbias = m.linear_pairs(x, pairs, raw=True)
                qbias = qbias.detach()
            else:
                w, b = m.get_params()
                res = nn.functional.linear(x.contiguous(), w.contiguous(), bias=b)
            outs.append(ops.quantize_heads_i8(res, specs[n_], H, transpose=(n_ == 2), want_values=(n_ > 0 and want_values), alpha=alpha, bias=qbias))
        return outs, grids, None

    def _int8_core_and_consumer(self, x, outs, grids, index_consumer, fq, want_values, attn_kw):
        """Step 3: the core on the indices (None when it refuses the problem: -95) and, with `index_consumer`, that projection on the context
        quantiser's integers.  Returns (merged context or the consumer's output, (k, v) values, consumer applied?)."""
        qc = outs[0]
        kc, yk = outs[1] if want_values else (outs[1], None)
        vt, yv = outs[2] if want_values else (outs[2], None)
        try:
            out = ops.attn_fwd_i8(qc, kc, vt, grids, **attn_kw)
        except _OehError as e:
            if e.code != -95:
                raise
            return None
        _count(self, "_i8_calls")  # (tests: which core ran)
        merged = out.permute(0, 2, 1, 3).reshape(x.shape[0], x.shape[1], -1)
        if index_consumer is None:
            return merged, (yk, yv), False
        _count(self, "_index_gemm_calls")
        return index_consumer.linear_index(merged, fq.ctx.scale, out_dtype=x.dtype, xzero=fq.ctx.zero_point), (yk, yv), True


class QuantizedBertSelfAttentionWithExtras(_QuantAttnBase):
    """quantized_bert.py:221-440: fake-quant on scores (after /sqrt(d), before the mask), on probs, and on the context
    AFTER gating and head merge; the gate is applied without gate_scaling_factor (:422)."""

    def __init__(self, org_model, **quant_params):
        super().__init__()
        self.num_attention_heads = org_model.num_attention_heads
        self.attention_head_size = org_model.attention_head_size
        self.all_head_size = org_model.all_head_size
        self.position_embedding_type = getattr(org_model, "position_embedding_type", None)
        self.is_decoder = org_model.is_decoder
        self.query = quantize_model(org_model.query, **quant_params)
        self.key = quantize_model(org_model.key, **quant_params)
        self.value = quantize_model(org_model.value, **quant_params)
        self.dropout = org_model.dropout
        self._init_common(org_model, quant_params)

    def transpose_for_scores(self, x):
        return x.view(x.size()[:-1] + (self.num_attention_heads, self.attention_head_size)).permute(0, 2, 1, 3)

    def forward(self, hidden_states, attention_mask=None, head_mask=None, encoder_hidden_states=None, encoder_attention_mask=None,
                past_key_value=None, output_attentions=False):
        if self.position_embedding_type in ("relative_key", "relative_key_query"):
            raise NotImplementedError("relative position embeddings are not on the quantised MI355X path")
        H, div = self.num_attention_heads, float(np.sqrt(self.attention_head_size))
        # nothing observable is asked for: what every route but unfused_core needs
        plain = head_mask is None and not output_attentions and not (self.training and self.dropout.p > 0.0)
        fq = self._fq(ctx_before_gate=False)
        gate, gated = None, False
        if plain and fq is not None and encoder_hidden_states is None and past_key_value is None:
            # self-attention in inference: query / key / value are QuantLinear (quantized_bert.py:236-238) - their outputs are 8-bit
            # indices, and the whole core (scores / sqrt(d) -> fq -> + mask -> softmax -> fq -> P V -> gate -> fq) runs on them
            T = hidden_states.shape[1]
            pad8, full8, _, floor = resolve_mask(attention_mask, hidden_states.shape[0], T, T, hidden_states.dtype)
            if full8 is None and (pad8 is None or pad_is_boolean(attention_mask)):
                gate, gated = GateState.evaluate(self, hidden_states, H), True
                done = self._int8_storage_core(hidden_states, (self.query, self.key, self.value), H, self.attention_head_size, scale=1.0, scale_div=div,
                                               causal=False, padvec=pad8, mask_min=floor, gate=gate, fq=fq, want_values=self.is_decoder)
                if done is not None:
                    context, (yk, yv), _ = done
                    outputs = (context,)
                    if self.is_decoder:
                        outputs = outputs + ((self.transpose_for_scores(yk), self.transpose_for_scores(yv)),)
                    return outputs
        q = self.transpose_for_scores(self.query(hidden_states))
        if encoder_hidden_states is not None:
            attention_mask = encoder_attention_mask
        k, v = kv_source(self.key, self.value, self.transpose_for_scores, hidden_states, encoder_hidden_states, past_key_value)
        new_past = (k, v) if self.is_decoder else None
        if not gated:  # (else: the INT8 route declined after the gate was evaluated)
            gate = GateState.evaluate(self, hidden_states, H)
        kw = dict(softmax_fn=self.softmax_fn, scale_div=div, attention_mask=attention_mask)
        probs = None
        if plain and fq is not None and spec_of(self.softmax_fn) is not None:
            context = attention_core(q, k, v, gate=gate, fq=fq, **kw)
        else:
            ctx = self._calibrate_fused(q, k, v, scale_div=div, attention_mask=attention_mask) if plain and fq is None else None  # ranges without the (B,H,S,S) tensors
            if ctx is None:
                ctx, _, probs = unfused_core(q, k, v, dropout=self.dropout, head_mask=head_mask, fq_scores=self.attn_scores_act_quantizer,
                                             fq_probs=self.attn_probs_act_quantizer, **kw)
            context = self.context_act_quantizer(gated_merge(ctx, gate))
        outputs = (context, probs) if output_attentions else (context,)
        if self.is_decoder:
            outputs = outputs + (new_past,)
        return outputs


class QuantizedOPTAttentionWithExtras(_QuantAttnBase):
    """quantized_opt.py:54-274: fake-quant on the bmm output (before mask), on probs, and on P@V BEFORE gating; gate without
    scaling (:257); q/k/v/out projections are QuantLinear."""

    def __init__(self, org_model, **quant_params):
        super().__init__()
        self.embed_dim = org_model.embed_dim
        self.num_heads = org_model.num_heads
        self.dropout = org_model.dropout
        self.head_dim = org_model.head_dim
        self.scaling = org_model.scaling
        self.is_decoder = org_model.is_decoder
        self.k_proj = quantize_model(org_model.k_proj, **quant_params)
        self.v_proj = quantize_model(org_model.v_proj, **quant_params)
        self.q_proj = quantize_model(org_model.q_proj, **quant_params)
        self.out_proj = quantize_model(org_model.out_proj, **quant_params)
        self._init_common(org_model, quant_params)

    def _heads(self, t, bsz):
        return t.view(bsz, -1, self.num_heads, self.head_dim).permute(0, 2, 1, 3)

    def _shape(self, tensor, seq_len, bsz):
        return tensor.view(bsz, seq_len, self.num_heads, self.head_dim).transpose(1, 2).contiguous()

    def forward(self, hidden_states, key_value_states=None, past_key_value=None, attention_mask=None, layer_head_mask=None,
                output_attentions=False):
        bsz, tgt_len, _ = hidden_states.size()
        H, self_attn, cached = self.num_heads, key_value_states is None, past_key_value is not None
        # nothing observable is asked for: what every route but unfused_core needs
        plain = layer_head_mask is None and not output_attentions and not (self.training and self.dropout > 0.0)
        fq = self._fq(ctx_before_gate=True)
        gate, gated = None, False
        if plain and not self.training and fq is not None and self_attn and not cached:
            if attention_mask is not None and attention_mask.size() != (bsz, 1, tgt_len, tgt_len):  # (before any projection runs)
                raise ValueError(f"Attention mask should be of size {(bsz, 1, tgt_len, tgt_len)}, but is {attention_mask.size()}")
            # HF's decoder mask: causal, plus finfo.min columns for padded keys (checked once per tensor; the size-checked mask itself, not
            # through resolve_mask: no split, and a mask that is not causal ends the route here)
            causal8, pad8 = classify_causal(attention_mask) if attention_mask is not None else (False, None)
            if causal8 or attention_mask is None:
                gate, gated = GateState.evaluate(self, hidden_states, H), True
                done = self._int8_storage_core(hidden_states, (self.q_proj, self.k_proj, self.v_proj), H, self.head_dim, scale=self.scaling, scale_div=0.0,
                                               causal=causal8, padvec=pad8, mask_min=mask_min_of(attention_mask, hidden_states.dtype),
                                               gate=gate, fq=fq, want_values=self.is_decoder, consumer=self.out_proj)
                if done is not None:
                    merged, (yk, yv), projected = done
                    kv = (self._heads(yk, bsz), self._heads(yv, bsz)) if self.is_decoder else past_key_value
                    return (merged if projected else self.out_proj(merged)), None, kv
        q = self._heads(self.q_proj(hidden_states) * self.scaling, bsz)
        k, v = kv_source(self.k_proj, self.v_proj, lambda t: self._heads(t, bsz), hidden_states, key_value_states, past_key_value)
        new_past = (k, v) if self.is_decoder else past_key_value
        src_len = k.size(2)
        if attention_mask is not None and attention_mask.size() != (bsz, 1, tgt_len, src_len):
            raise ValueError(f"Attention mask should be of size {(bsz, 1, tgt_len, src_len)}, but is {attention_mask.size()}")
        if not gated:  # (else: the INT8 route declined after the gate was evaluated)
            gate = GateState.evaluate(self, hidden_states, H)
        kw = dict(attention_mask=attention_mask, clamp_min=attention_mask is not None)
        weights = None
        if plain and fq is not None and spec_of(self.softmax_fn) is not None:
            merged = attention_core(q, k, v, softmax_fn=self.softmax_fn, detect_causal=True, gate=gate, fq=fq, decode=self_attn and cached, **kw)
        else:
            ctx = self._calibrate_fused(q, k, v, detect_causal=True, **kw) if plain and fq is None else None  # ranges without the (B,H,S,S) tensors
            if ctx is None:
                hm = None if layer_head_mask is None else layer_head_mask.view(1, -1, 1, 1)
                drop = (lambda p: nn.functional.dropout(p, p=self.dropout, training=self.training))
                ctx, _, used = unfused_core(q, k, v, softmax_fn=self.softmax_fn, dropout=drop, head_mask=hm, fq_scores=self.attn_scores_act_quantizer,
                                            fq_probs=self.attn_probs_act_quantizer, **kw)
                weights = used if output_attentions else None
            merged = gated_merge(self.context_act_quantizer(ctx), gate)
        return self.out_proj(merged), weights, new_past


# ------------------------------------------------------------------------------------------------------------
# the block tails: what follows the attention module's out_proj in a quantised layer
# ------------------------------------------------------------------------------------------------------------
_LN_DECOMPOSED_KEYS = {"QuantizedBertSelfOutput": "layer_norm_res_self_output", "QuantizedBertOutput": "layer_norm_res_output"}


class _QuantizedBertTail(QuantizedModel):
    """dense -> dropout -> + input -> res_act_quantizer -> LayerNorm (quantized_bert.py:541-606).  Dropout is the identity in eval; in
    training the torch ops run.  The decomposed integer LayerNorm (quantized_bert.py:78-143) and the logarithmic sum quantiser are refused."""

    def __init__(self, org_model, **quant_params):
        super().__init__()
        self.quant_dict = DotDict(quant_params.get("quant_dict") or {})
        key = _LN_DECOMPOSED_KEYS[type(self).__name__]
        if self.quant_dict.get(key, False):
            raise NotImplementedError(f"quant_dict['{key}']: the decomposed LayerNorm is not implemented (only the fake-quantised nn.LayerNorm is)")
        if self.quant_dict.get("y", None) == "log":
            raise NotImplementedError("quant_dict['y'] == 'log': the logarithmic residual quantiser is not implemented")
        self.dense = quantize_model(org_model.dense, **quant_params)
        self.dropout = org_model.dropout
        self.res_act_quantizer = QuantizedActivation(**quant_params)
        self.LayerNorm = quantize_model(org_model.LayerNorm, **quant_params)
        self._fused_ln_calls = 0

    def finish(self, dense_out, input_tensor):
        """Everything after `dense`."""
        hidden_states = self.dropout(dense_out)
        return resid_ln_tail(self, hidden_states, input_tensor, self.res_act_quantizer, self.LayerNorm)

    def forward(self, hidden_states, input_tensor):
        return self.finish(self.dense(hidden_states), input_tensor)


class QuantizedBertSelfOutput(_QuantizedBertTail):
    """quantized_bert.py:541-571."""


class QuantizedBertOutput(_QuantizedBertTail):
    """quantized_bert.py:574-606."""


def feed_forward(fc1_act: nn.Module, fc2: nn.Module, x2d: torch.Tensor):
    """fc2(fc1_act(x2d)) for the two QuantLinears of a block's feed-forward, x2d (rows, E).  With FUSED_FFN, where fc1_act's fused tail applies
    (`QuantLinear.forward_index`) and fc2 can take its int8 indices (`QuantLinear.int8_consumer_ok`: weights that fit a signed byte,
    K % 64 == 0, rows % 16 == 0, a frozen 8-bit output quantiser, no hooks): fc1's quantiser writes the indices and fc2 runs on the integer
    matrix cores with its own quantiser in the epilogue - the (rows, FFN) float tensor between them is never written.  Anything else: the two
    modules' own forwards.  fc1_act counts `_fused_ffn_calls` (and `_gemm_quant_calls` | `_act_quant_calls`: which route), fc2 `_int8_index_calls`."""
    if (FUSED_FFN and isinstance(fc1_act, QuantLinear) and isinstance(fc2, QuantLinear) and x2d.dim() == 2 and fc2.in_features == fc1_act.out_features
            and fc1_act.fused_act() is not None and fc2.int8_consumer_ok(x2d.shape[0])):
        got = fc1_act.forward_index(x2d)
        if got is not None:
            idx8, sp = got
            return fc2.linear_index(idx8, sp.scale, out_dtype=x2d.dtype, xzero=sp.zero_point)
    return fc2(fc1_act(x2d))


def quantize_intermediate(org_module, **quant_params) -> nn.Module:
    """BERT's intermediate (dense + intermediate_act_fn) as one QuantLinear with the activation under its output quantiser
    (quantized_bert.py:609-617): a Sequential of that one module.  The activation may be a module or the function F.gelu; another plain
    callable is refused."""
    act = org_module.intermediate_act_fn
    if not isinstance(act, nn.Module):
        if act is not nn.functional.gelu:
            raise NotImplementedError(f"quantize_intermediate: the activation {act!r} is neither a module nor F.gelu")
        act = nn.GELU()
    return quantize_model(nn.Sequential(org_module.dense, act), **quant_params)


class QuantizedBertFeedForward(QuantizedModel):
    """The feed_forward_chunk of a quantised BERT layer (quantized_bert.py:620-700): intermediate (dense + GELU, one QuantLinear) ->
    QuantizedBertOutput.  `org_layer` has `.intermediate` (dense, intermediate_act_fn) and `.output` (dense, dropout, LayerNorm), as a
    BertLayer does; the members keep those names."""

    def __init__(self, org_layer, **quant_params):
        super().__init__()
        self.intermediate = quantize_intermediate(org_layer.intermediate, **quant_params)
        self.output = QuantizedBertOutput(org_layer.output, **quant_params)

    def forward(self, attention_output):
        out = self.output
        if FUSED_FFN and not has_hooks(out, self.intermediate):  # (`finish` bypasses the forward of `output`, feed_forward that of the Sequential)
            shape = attention_output.shape
            h = feed_forward(self.intermediate[0], out.dense, attention_output.reshape(-1, shape[-1]))
            return out.finish(h.view(*shape[:-1], h.shape[-1]), attention_output)
        return out(self.intermediate(attention_output), attention_output)


class QuantizedOPTDecoderLayer(QuantizedModel):
    """quantized_opt.py:277-384.  In eval with frozen ranges the residual sums, their quantisers and the LayerNorms are three launches:
    pre-LN (do_layer_norm_before) - the first LayerNorm alone, the attention residual with final_layer_norm (its quantised sum is the
    FFN's residual), and the FFN residual's quantiser on the torch add (its LayerNorm belongs to the next layer); post-LN - each
    residual with the LayerNorm that follows it, and nothing else."""

    def __init__(self, org_model, **quant_params):
        super().__init__()
        self.embed_dim = org_model.embed_dim
        self.do_layer_norm_before = org_model.do_layer_norm_before
        self.dropout = org_model.dropout
        self.activation_fn = org_model.activation_fn
        assert isinstance(self.activation_fn, nn.ReLU)
        self.self_attn = QuantizedOPTAttentionWithExtras(org_model.self_attn, **quant_params)
        self.self_attn_layer_norm = quantize_model(org_model.self_attn_layer_norm, **quant_params)
        self.fc1_act = quantize_model(nn.Sequential(org_model.fc1, org_model.activation_fn), **quant_params)[0]
        self.fc2 = quantize_model(org_model.fc2, **quant_params)
        self.final_layer_norm = quantize_model(org_model.final_layer_norm, **quant_params)
        self.self_attn_res_act_quantizer = QuantizedActivation(**quant_params)
        self.ffn_res_act_quantizer = QuantizedActivation(**quant_params)
        self._fused_ln_calls = 0

    def tail(self, attn_output, residual):
        """Everything after the attention module: (B, S, E) attention output and the layer's input -> the layer's output."""
        hidden_states = nn.functional.dropout(attn_output, p=self.dropout, training=self.training)
        shape = hidden_states.shape
        if self.do_layer_norm_before:
            residual, hidden_states = resid_ln_tail(self, hidden_states, residual, self.self_attn_res_act_quantizer, self.final_layer_norm, want_sum=True)
        else:
            hidden_states = residual = resid_ln_tail(self, hidden_states, residual, self.self_attn_res_act_quantizer, self.self_attn_layer_norm)
        residual = residual.reshape(-1, shape[-1])
        hidden_states = feed_forward(self.fc1_act, self.fc2, hidden_states.reshape(-1, shape[-1]))
        hidden_states = nn.functional.dropout(hidden_states, p=self.dropout, training=self.training)
        if self.do_layer_norm_before:
            return self.ffn_res_act_quantizer(residual + hidden_states).view(shape)
        return resid_ln_tail(self, hidden_states, residual, self.ffn_res_act_quantizer, self.final_layer_norm).view(shape)

    def forward(self, hidden_states, attention_mask=None, layer_head_mask=None, output_attentions=False, use_cache=False, past_key_value=None):
        residual = hidden_states
        if self.do_layer_norm_before:
            hidden_states = resid_ln_tail(self, hidden_states, None, None, self.self_attn_layer_norm)
        hidden_states, self_attn_weights, present_key_value = self.self_attn(hidden_states=hidden_states, past_key_value=past_key_value,
                                                                             attention_mask=attention_mask, layer_head_mask=layer_head_mask,
                                                                             output_attentions=output_attentions)
        outputs = (self.tail(hidden_states, residual),)
        if output_attentions:
            outputs += (self_attn_weights,)
        if use_cache:
            outputs += (present_key_value,)
        return outputs


# ------------------------------------------------------------------------------------------------------------
# the model fronts: embeddings -> sums -> (LayerNorm)
# ------------------------------------------------------------------------------------------------------------
class QuantizedBertEmbeddings(QuantizedModel):
    """quantized_bert.py:146-218: word + token type -> sum_input_token_type_embd_act_quantizer, += position ->
    sum_pos_embd_act_quantizer, LayerNorm, dropout.  In eval with frozen ranges on the GPU: one launch (`embed_front`).  quant_dict["Et"]
    selects the MSE golden-section range for the word table; the decomposed integer LayerNorm (quant_dict["layer_norm_embd"]) is refused."""

    def __init__(self, org_model, **quant_params):
        super().__init__()
        self.quant_dict = DotDict(quant_params.get("quant_dict") or {})
        if self.quant_dict.get("layer_norm_embd", False):
            raise NotImplementedError("quant_dict['layer_norm_embd']: the decomposed LayerNorm is not implemented (only the fake-quantised nn.LayerNorm is)")
        quant_params_ = dict(quant_params)
        if "Et" in self.quant_dict:
            quant_params_["weight_range_method"] = MSE_Estimator
            quant_params_["weight_range_options"] = dict(opt_method=OptMethod.golden_section)
        self.word_embeddings = quantize_model(org_model.word_embeddings, **quant_params_)
        self.position_embeddings = quantize_model(org_model.position_embeddings, **quant_params)
        self.token_type_embeddings = quantize_model(org_model.token_type_embeddings, **quant_params)
        self.dropout = org_model.dropout
        position_ids = org_model.position_ids
        if position_ids is not None:
            self.register_buffer("position_ids", position_ids)
        else:
            self.position_ids = position_ids
        self.position_embedding_type = getattr(org_model, "position_embedding_type", "absolute")
        self.sum_input_token_type_embd_act_quantizer = QuantizedActivation(**quant_params)
        self.sum_pos_embd_act_quantizer = QuantizedActivation(**quant_params)
        self.LayerNorm = quantize_model(org_model.LayerNorm, **quant_params)
        self._fused_embed_calls = 0

    def forward(self, input_ids=None, token_type_ids=None, position_ids=None, inputs_embeds=None):
        input_shape = input_ids.size() if input_ids is not None else inputs_embeds.size()[:-1]
        seq_length = input_shape[1]
        if position_ids is None:
            position_ids = self.position_ids[:, :seq_length]
        if token_type_ids is None:
            token_type_ids = torch.zeros(input_shape, dtype=torch.long, device=self.position_ids.device)
        absolute = self.position_embedding_type == "absolute"
        lookups = [(self.word_embeddings, input_ids) if inputs_embeds is None else (None, inputs_embeds), (self.token_type_embeddings, token_type_ids)]
        quantizers = [self.sum_input_token_type_embd_act_quantizer]
        if absolute:
            lookups.append((self.position_embeddings, position_ids))
            quantizers.append(self.sum_pos_embd_act_quantizer)
        fused = embed_front(self, lookups, quantizers, self.LayerNorm)
        if fused is not None:
            return self.dropout(fused)
        if inputs_embeds is None:
            inputs_embeds = self.word_embeddings(input_ids)
        embeddings = inputs_embeds + self.token_type_embeddings(token_type_ids)
        embeddings = self.sum_input_token_type_embd_act_quantizer(embeddings)
        if absolute:
            embeddings = embeddings + self.position_embeddings(position_ids)
            embeddings = self.sum_pos_embd_act_quantizer(embeddings)
        embeddings = self.LayerNorm(embeddings)
        return self.dropout(embeddings)


class QuantizedOPTLearnedPositionalEmbedding(QuantizedModel):
    """quantized_opt.py:27-51: the position table behind `offset`, positions counted along the attention mask."""

    def __init__(self, org_model, **quant_params):
        super().__init__()
        self.offset = org_model.offset
        self.quant_embedding = QuantEmbedding(org_model.num_embeddings, org_model.embedding_dim, padding_idx=org_model.padding_idx,
                                              max_norm=org_model.max_norm, norm_type=org_model.norm_type,
                                              scale_grad_by_freq=org_model.scale_grad_by_freq, sparse=org_model.sparse, **quant_params)
        self.quant_embedding.weight.data = org_model.weight.data.clone()
        self.quant_embedding.to(org_model.weight.device)
        self._fused_embed_calls = 0

    def position_ids(self, attention_mask, past_key_values_length: int = 0):
        """The table rows of a (B, S_total) mask: cumsum(mask) * mask - 1 cut to the new tokens, + offset (a padded position reads row offset - 1)."""
        attention_mask = attention_mask.long()
        positions = (torch.cumsum(attention_mask, dim=1).type_as(attention_mask) * attention_mask).long() - 1
        return positions[:, past_key_values_length:] + self.offset

    def forward(self, attention_mask, past_key_values_length: int = 0):
        return self.quant_embedding(self.position_ids(attention_mask, past_key_values_length))


def opt_embed_front(embed_tokens, embed_positions, embed_sum_act_quantizer, input_ids, attention_mask, past_key_values_length=0, inputs_embeds=None,
                    project_in=None):
    """quantized_opt.py:549-569: embed_sum_act_quantizer(embed_tokens(input_ids) + embed_positions(attention_mask, past_key_values_length)),
    the decoder's hidden states in front of its first layer.  One launch where `embed_front` applies (`embed_positions`._fused_embed_calls
    counts them); the position ids come from the reference's cumsum rule in torch - the id tensor is tiny.  attention_mask None: all ones.
    project_in (OPT-350m) sits between the lookup and the sum: the torch ops run."""
    if inputs_embeds is None:
        shape = input_ids.shape
        input_ids = input_ids.view(-1, shape[-1])
        B, S, dev = input_ids.shape[0], input_ids.shape[1], input_ids.device
    else:
        B, S, dev = inputs_embeds.shape[0], inputs_embeds.shape[1], inputs_embeds.device
    if attention_mask is None:
        attention_mask = torch.ones((B, S + past_key_values_length), dtype=torch.bool, device=dev)
    if project_in is None:
        pos = embed_positions.position_ids(attention_mask, past_key_values_length)
        first = (embed_tokens, input_ids) if inputs_embeds is None else (None, inputs_embeds)
        if not embed_positions.training and not has_hooks(embed_positions):
            fused = embed_front(embed_positions, [first, (embed_positions.quant_embedding, pos)], [embed_sum_act_quantizer], None)
            if fused is not None:
                return fused
    if inputs_embeds is None:
        inputs_embeds = embed_tokens(input_ids)
    pos_embeds = embed_positions(attention_mask, past_key_values_length)
    if project_in is not None:
        inputs_embeds = project_in(inputs_embeds)
    return embed_sum_act_quantizer(inputs_embeds + pos_embeds)


# The model fronts (QuantizedBertEmbeddings, opt_embed_front) as ONE launch of ops.embed_sum_quant where it applies; False: the separate ops
# (F.embedding on the fake-quantised tables, torch add, ops.fake_quant, the LayerNorm) - tests compare the two.
FUSED_EMBED = True
# The block tails (QuantLayerNorm, QuantizedBert[Self]Output, QuantizedOPTDecoderLayer) as ONE launch of ops.resid_ln_quant where it
# applies; False: the separate ops (torch add, ops.fake_quant, F.layer_norm, ops.fake_quant) - tests compare the two.
FUSED_LN = True
# estimate_ranges state: the score and probability quantisers' percentile ranges from `ops.attn_calibrate` (the (B,H,Sq,Sk)
# tensors are recomputed tile by tile inside the kernel, never stored); False: the observable path materialises them.
FUSED_CALIBRATION = True
# OPT's out_proj on the context quantiser's INTEGERS (ops ... ctx_emit_index + QuantLinear.linear_index): one 16-bit GEMM of
# integers instead of the split pass + the operand-pair GEMM.  False: the core writes float values, out_proj runs as any QuantLinear.
INDEX_GEMM = True
# The q / k / v projections of the INT8-storage path as ONE GEMM with the output quantisers in its epilogue (ops.proj_quant_i8;
# include/oeh.h: oeh_proj_quant_i8).  False: the library pair GEMM + three `oeh_quantize_heads_i8` passes (tests compare the two).
FUSED_PROJ = True
# The INT8-storage attention core (integer matrix cores) is used by QuantizedOPTAttentionWithExtras whenever it applies;
# False: always the fake-quant kernels on float values (tests compare the two).
INT8_STORAGE = True
# QuantLinear on fp32 inputs with quantised (8-bit integer x scale) weights: one fp16 GEMM on operand pairs instead of the fp32
# library GEMM (ops.split_pairs; include/oeh.h: oeh_split_pairs).  False: torch's fp32 linear (tests compare the two).
PAIR_GEMM = True
# The feed-forward of a quantised block (`feed_forward`: OPT's fc1 + ReLU -> fc2, BERT's intermediate + GELU -> output.dense): fc1's scale,
# bias, activation function and output quantiser as ONE pass (ops.act_quant; for ReLU into a zero-point-0 grid the whole fc1 as one
# ops.proj_quant_i8 launch) that hands fc2 the quantiser's int8 indices for the integer matrix cores (QuantLinear.linear_index).  False -
# the default until the measurements of DESIGN.md section 19 argue otherwise: the separate ops (tests compare the two).
FUSED_FFN = False


def set_fused_ffn(on: bool) -> bool:
    """Switch FUSED_FFN; returns the previous setting (tests and tools restore it)."""
    global FUSED_FFN
    prev, FUSED_FFN = FUSED_FFN, bool(on)
    return prev


# ------------------------------------------------------------------------------------------------------------
# config helpers (flag names / defaults of transformers_language/quant_configs.py:7-33, utils.py:27-47)
# ------------------------------------------------------------------------------------------------------------
class DotDict(dict):
    __setattr__ = dict.__setitem__
    __delattr__ = dict.__delitem__

    def __getattr__(self, key):
        if key in self:
            return self[key]
        raise AttributeError(f"DotDict instance has no key '{key}' ({self.keys()})")


def get_quant_config() -> DotDict:
    cfg = DotDict()
    cfg.act_quant = DotDict(cross_entropy_layer=None, num_batches=16, options={}, quant_method=RangeEstimators.running_minmax, std_dev=None)
    cfg.quant = DotDict(act_quant=True, n_bits=8, n_bits_act=8, num_candidates=None, per_channel=False, percentile=None, quant_setup="all",
                        qmethod=QMethods.symmetric_uniform, qmethod_act=QMethods.asymmetric_uniform, weight_quant=True,
                        weight_quant_method=RangeEstimators.current_minmax)
    return cfg


def val_qparams(config) -> dict:
    weight_range_options = {}
    if config.quant.weight_quant_method == RangeEstimators.MSE:
        weight_range_options = dict(opt_method=config.quant.weight_opt_method)
    if config.quant.num_candidates is not None:
        weight_range_options["num_candidates"] = config.quant.num_candidates
    return {
        "method": config.quant.qmethod.cls,
        "n_bits": config.quant.n_bits,
        "n_bits_act": config.quant.n_bits_act,
        "act_method": config.quant.qmethod_act.cls,
        "per_channel_weights": config.quant.per_channel,
        "percentile": config.quant.percentile,
        "quant_setup": config.quant.quant_setup,
        "weight_range_method": config.quant.weight_quant_method.cls,
        "weight_range_options": weight_range_options,
        "act_range_method": config.act_quant.quant_method.cls,
        "act_range_options": config.act_quant.options,
    }
