"""The loss both language models end in, on the HIP kernels of oeh_xent.hip: cross-entropy over the vocabulary with the logits read once
forward, and read once and written once backward - no shifted copy, no fp32 upcast, no log-probability tensor.

    cross_entropy(logits, labels, ...)          F.cross_entropy for class-last logits of any leading shape, any view
    FusedCrossEntropyLoss                       nn.CrossEntropyLoss's constructor and forward
    causal_lm_loss(logits, labels)              quantized_opt.py:872-877, the shift done by views
    masked_lm_loss(prediction_scores, labels)   quantized_bert.py:910-915
    PerplexityMeter                             validate_clm.py:556-594 with one device-to-host copy at the end

What the kernel does not cover - class weights, probability targets, float64 logits, CPU tensors, class-second logits of more than three
dimensions - runs F.cross_entropy on the same device, the way the attention modules take their torch-op path.  One deviation: the kernel
path returns the loss (and the per-row losses of reduction="none") in fp32 whatever the logits' type, as the reference gets it under
autocast; F.cross_entropy on fp16 logits outside autocast rounds it to fp16.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops

# Module switch like quantization.FUSED_LN: False runs the torch ops everywhere below.  True by rule: forward + backward is faster than the
# reference's chain at both the OPT and the BERT shape (profiles/xent_bench.txt).
FUSED_XENT = True


def _xent_forward(logits, labels, ignore_index, label_smoothing, reduction, shift):
    x, y = (logits[..., :-1, :], labels[..., 1:]) if shift else (logits, labels)
    # (the row losses are always stored: 4 bytes per row, and the reduce launch then has no load that waits for a label)
    mean, out2, lse, rows = ops.xent_fwd(x, y, ignore_index=ignore_index, label_smoothing=label_smoothing, want_rows=True)
    res = mean if reduction == "mean" else out2[0].to(torch.float32) if reduction == "sum" else rows.view(y.shape)
    return res, lse, out2


class _Xent(torch.autograd.Function):
    """Saves the logits (the backward reads them; the caller owns them anyway), the labels, lse and out2: no tensor of the logits' size is
    made for the backward.  Differentiable once: the gradient is a kernel's output and carries no graph."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index, label_smoothing, reduction, shift):
        res, lse, out2 = _xent_forward(logits, labels, ignore_index, label_smoothing, reduction, shift)
        ctx.save_for_backward(logits, labels, lse, out2)
        ctx.cfg = (ignore_index, label_smoothing, reduction, shift)
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        logits, labels, lse, out2 = ctx.saved_tensors
        ignore_index, label_smoothing, reduction, shift = ctx.cfg
        g = grad.to(torch.float32).contiguous()  # (the upstream gradient stays on the device: the kernel reads it there)
        dlogits = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
        x, y, dx = (logits[..., :-1, :], labels[..., 1:], dlogits[..., :-1, :]) if shift else (logits, labels, dlogits)
        if shift:
            dlogits[..., -1, :].zero_()  # the last position predicts nothing
        ops.xent_bwd(x, y, lse, out2, g, ignore_index=ignore_index, label_smoothing=label_smoothing, mean_reduction=reduction == "mean", out=dx)
        return dlogits, None, None, None, None, None


def _kernel_covers(logits, labels) -> bool:
    return (FUSED_XENT and isinstance(labels, torch.Tensor) and logits.is_cuda and labels.is_cuda and logits.dtype in ops._DT
            and labels.dtype in ops._ID_DT and logits.dim() >= 1 and tuple(labels.shape) == tuple(logits.shape[:-1]))


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100, label_smoothing: float = 0.0, reduction: str = "mean",
                  _shift: bool = False) -> torch.Tensor:
    """F.cross_entropy(logits.view(-1, V), labels.view(-1), ...) for logits (..., V) and integer labels (...): the classes are the LAST
    dimension, the leading ones are rows.  Views are read in place, by their strides.  Differentiable in the logits."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"{reduction} is not a valid value for reduction")
    if not _kernel_covers(logits, labels):
        x, y = (logits[..., :-1, :].contiguous(), labels[..., 1:].contiguous()) if _shift else (logits, labels)
        out = F.cross_entropy(x.reshape(-1, x.shape[-1]), y.reshape(-1), ignore_index=ignore_index, label_smoothing=label_smoothing, reduction=reduction)
        return out.view(y.shape) if reduction == "none" else out
    if ops.grad_recording(logits):
        return _Xent.apply(logits, labels, int(ignore_index), float(label_smoothing), reduction, _shift)
    with torch.no_grad():
        return _xent_forward(logits, labels, int(ignore_index), float(label_smoothing), reduction, _shift)[0]


class FusedCrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss with the kernel behind it: input (N, C) or (C,) with class indices, or (N, C, d1) - whose classes the kernel
    needs contiguous, so that layout costs ONE copy of the logits to (N, d1, C) forward and the transposition of the gradient backward
    (class-last logits through `cross_entropy` cost none).  Anything else nn.CrossEntropyLoss takes (class weights, probability targets, float64, CPU tensors, (N, C, d1, d2, ...))
    runs F.cross_entropy on the same device."""

    def __init__(self, weight: Optional[torch.Tensor] = None, size_average=None, ignore_index: int = -100, reduce=None, reduction: str = "mean",
                 label_smoothing: float = 0.0) -> None:
        super().__init__()
        if size_average is not None or reduce is not None:
            reduction = nn.CrossEntropyLoss(size_average=size_average, reduce=reduce).reduction  # (torch's own legacy mapping)
        self.register_buffer("weight", weight)
        self.ignore_index = ignore_index
        self.reduction = reduction
        self.label_smoothing = label_smoothing
        self._fused_xent_calls = 0  # launches of the kernel from this module's forward (tests)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        x = input.permute(0, 2, 1).contiguous() if input.dim() == 3 else input  # classes last: one copy, made here and not behind the op
        if not (self.weight is None and input.dim() in (1, 2, 3) and _kernel_covers(x, target)):
            return F.cross_entropy(input, target, weight=self.weight, ignore_index=self.ignore_index, reduction=self.reduction,
                                   label_smoothing=self.label_smoothing)
        self._fused_xent_calls += 1
        return cross_entropy(x, target, self.ignore_index, self.label_smoothing, self.reduction)


def causal_lm_loss(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """quantized_opt.py:872-877: CrossEntropyLoss()(logits[..., :-1, :].contiguous().view(-1, V), labels[..., 1:].contiguous().view(-1)),
    with the two shifts as views (pointer offsets) instead of copies.  The gradient comes back for the whole logits tensor, the last position's
    rows zero."""
    return cross_entropy(logits, labels, _shift=True)


def masked_lm_loss(prediction_scores: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """quantized_bert.py:910-915: CrossEntropyLoss()(prediction_scores.view(-1, V), labels.view(-1)); rows labelled -100 are not read."""
    return cross_entropy(prediction_scores, labels)


class PerplexityMeter:
    """validate_clm.py:556-594 without one .item() per batch: `update` adds a batch's mean loss to a float64 pair on the device (inside
    the loss kernel's own reduce launch), `perplexity` makes the one device-to-host copy and returns exp(mean of the batch means), inf
    where that overflows.  shift=True: the causal LM's loss (`causal_lm_loss`); False: rows as they are (`masked_lm_loss`)."""

    def __init__(self, shift: bool = True, ignore_index: int = -100) -> None:
        self.shift, self.ignore_index = shift, ignore_index
        self._meter = None  # float64 {sum of the batch means, batches} on the logits' GPU
        self._host = [0.0, 0.0]  # the same pair for batches that took the torch path

    def update(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """Adds this batch; returns its mean loss (a device scalar, not synchronised)."""
        if not _kernel_covers(logits, labels):
            loss = cross_entropy(logits.detach(), labels, self.ignore_index, _shift=self.shift)
            self.add_mean(float(loss))
            return loss
        if self._meter is None:
            self._meter = torch.zeros(2, dtype=torch.float64, device=logits.device)
        x, y = (logits[..., :-1, :], labels[..., 1:]) if self.shift else (logits, labels)
        return ops.xent_fwd(x.detach(), y, ignore_index=self.ignore_index, want_rows=True, meter=self._meter)[0]

    def add_mean(self, mean_loss: float) -> None:
        """One batch's mean loss from the host (the reference's own loop body)."""
        self._host[0] += float(mean_loss)
        self._host[1] += 1.0

    def state(self):
        """(sum of the batch means, batches): the one device-to-host copy."""
        s, n = self._host
        if self._meter is not None:
            ds, dn = self._meter.cpu().tolist()
            s, n = s + ds, n + dn
        return s, n

    def perplexity(self) -> float:
        s, n = self.state()
        try:
            return math.exp(s / n) if n else float("nan")
        except OverflowError:
            return float("inf")

    def reset(self) -> None:
        self._host = [0.0, 0.0]
        if self._meter is not None:
            self._meter.zero_()
