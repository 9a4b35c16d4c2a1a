"""The tail of a transformer block in training on the HIP kernels (include/oeh.h: oeh_drop_resid_ln_fwd / oeh_drop_resid_ln_bwd).

`dropout_add_layer_norm(x, residual, weight, bias, p, eps)` is LayerNorm(dropout(x) + residual) as ONE torch.autograd.Function: the
forward is one kernel that writes the sum, its LayerNorm and the two fp32 row statistics; the backward is a row kernel and a column
reduction that regenerate the dropout mask from the saved seed - nothing of the mask is stored.  With `want_sum` the sum is a second
output that carries its own gradient: the pre-LN (OPT) shape residual + dropout(h) in front of the next LayerNorm.  The post-LN (BERT)
shape dense -> dropout -> + input -> LayerNorm is `FusedBertSelfOutput` / `FusedBertOutput`; `fuse_block_tails(model)` swaps them into a
Hugging Face BERT in place.

The keep mask comes from the counter-based generator of the attention dropout (Philox4x32-10) on a stream of its own; without a
dropout_seed one is drawn from torch's default CPU generator, so torch.manual_seed reproduces a run.  It is a different random stream
from nn.Dropout's.

`FUSED_LN_TRAIN` switches the fused call on; off - and for whatever the kernels do not cover (`_kernel_covers`) - the same function runs
the torch chain F.dropout -> add -> F.layer_norm.  The default follows tools/ln_train_bench.py.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops
from .autograd_attention import draw_seed

FUSED_LN_TRAIN = True

# calls of the fused path since import (tests read it to see which path a call took)
CALLS = {"forward": 0, "backward": 0, "torch": 0}


def set_fused_ln_train(on: bool) -> bool:
    """Switch the fused training block tail on or off; returns the previous setting."""
    global FUSED_LN_TRAIN
    prev, FUSED_LN_TRAIN = FUSED_LN_TRAIN, bool(on)
    return prev


def _kernel_covers(x: torch.Tensor, residual: Optional[torch.Tensor], weight: Optional[torch.Tensor], p: float, capturing: Optional[bool] = None) -> bool:
    """True when the HIP kernels take this call: GPU tensors, x (and residual) of one of fp16 / bf16 / fp32, 1 <= cols <= 8192, a contiguous
    last dimension, a LayerNorm weight - and no dropout while a stream is being captured: the seed is a host value baked into the captured
    launch, so every replay of the graph would repeat the same mask."""
    if weight is None or not x.is_cuda or x.dim() == 0:
        return False
    if x.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        return False
    if residual is not None and (residual.dtype != x.dtype or residual.shape != x.shape or (x.shape[-1] > 1 and residual.stride(-1) != 1)):
        return False
    cols = x.shape[-1]
    if cols < 1 or cols > ops.LN_MAX_COLS or (cols > 1 and x.stride(-1) != 1):
        return False
    if p > 0.0:
        if capturing is None:
            capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            return False
    return True


class _DropoutAddLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, p, eps, seed, want_sum):
        s, y, mean, rstd = ops.drop_resid_ln_fwd(x, residual, weight, bias, eps, p=p, seed=seed)
        ctx.save_for_backward(s, mean, rstd, weight)
        ctx.p, ctx.seed, ctx.eps = p, seed, eps
        ctx.has_residual, ctx.has_bias = residual is not None, bias is not None
        ctx.bias_dtype = None if bias is None else bias.dtype
        ctx.want_sum = want_sum
        CALLS["forward"] += 1
        if not want_sum:
            ctx.mark_non_differentiable(s)
        return s, y

    @staticmethod
    @once_differentiable
    def backward(ctx, dsum, dy):
        s, mean, rstd, weight = ctx.saved_tensors
        if dy is None:
            dy = torch.zeros_like(s)
        if not ctx.want_sum:
            dsum = None
        want_dr = ctx.has_residual and ctx.needs_input_grad[1]
        dx, dr, dgamma, dbeta = ops.drop_resid_ln_bwd(dy.to(s.dtype), s, weight, mean, rstd, ctx.eps, dsum=None if dsum is None else dsum.to(s.dtype),
                                                      p=ctx.p, seed=ctx.seed, want_dr=want_dr, want_dbeta=ctx.has_bias)
        CALLS["backward"] += 1
        return (dx, dr, dgamma.to(weight.dtype).view(weight.shape), None if dbeta is None else dbeta.to(ctx.bias_dtype).view(weight.shape),
                None, None, None, None)


def _torch_chain(x, residual, weight, bias, p, eps, training, want_sum):
    s = F.dropout(x, p, training) if p > 0.0 else x
    if residual is not None:
        s = s + residual
    y = F.layer_norm(s, (x.shape[-1],), weight, bias, eps)
    CALLS["torch"] += 1
    return (s, y) if want_sum else y


def dropout_add_layer_norm(x: torch.Tensor, residual: Optional[torch.Tensor], weight: Optional[torch.Tensor], bias: Optional[torch.Tensor] = None,
                           p: float = 0.0, eps: float = 1e-5, training: bool = True, want_sum: bool = False, dropout_seed: Optional[int] = None):
    """LayerNorm(dropout(x, p) + residual) over the last dimension: y, or (sum, y) with want_sum - sum = dropout(x) + residual in x's dtype,
    the residual stream of a pre-LN block; a gradient that arrives on it joins the LayerNorm's.  x, residual (..., N); weight, bias (N).
    training=False (or p == 0): no dropout.  dropout_seed: the uint64 seed of the keep mask (default: autograd_attention.draw_seed(), from
    torch's default CPU generator).  Differentiable in x, residual, weight and bias; the parameters' gradients are accumulated in float64, rounded
    once to fp32 and cast to the parameters' dtype.

    The HIP kernels run when `FUSED_LN_TRAIN` is on and `_kernel_covers` the call; otherwise the torch chain F.dropout -> add ->
    F.layer_norm does: residual of another dtype, float64, more than 8192 columns, a last dimension that is not contiguous, no weight -
    and p > 0 while a stream is being captured, because the seed is a host value recorded with the launch and a replayed graph would
    repeat the mask (nn.Dropout's generator state advances inside a graph; this one's does not)."""
    p = float(p) if training else 0.0
    if not (FUSED_LN_TRAIN and _kernel_covers(x, residual, weight, p)):
        return _torch_chain(x, residual, weight, bias, p, eps, training, want_sum)
    seed = None
    if p > 0.0:
        seed = draw_seed() if dropout_seed is None else int(dropout_seed)
    if not ops.grad_recording(x, residual, weight, bias):
        s, y, _, _ = ops.drop_resid_ln_fwd(x, residual, weight, bias, eps, p=p, seed=seed)
        CALLS["forward"] += 1
        return (s, y) if want_sum else y
    s, y = _DropoutAddLayerNorm.apply(x, residual, weight, bias, p, float(eps), seed, bool(want_sum))
    return (s, y) if want_sum else y


class FusedDropoutAddLayerNorm(nn.Module):
    """LayerNorm(dropout(x) + residual) with the LayerNorm's parameters `weight` and `bias` (`dropout_add_layer_norm`)."""

    def __init__(self, hidden_size: int, eps: float = 1e-5, p: float = 0.0):
        super().__init__()
        self.hidden_size, self.eps, self.p = int(hidden_size), float(eps), float(p)
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.bias = nn.Parameter(torch.zeros(hidden_size))

    def forward(self, x, residual=None, want_sum: bool = False):
        return dropout_add_layer_norm(x, residual, self.weight, self.bias, self.p, self.eps, self.training, want_sum)

    def extra_repr(self):
        return f"{self.hidden_size}, eps={self.eps}, p={self.p}"


class _FusedBertTail(nn.Module):
    """dense -> dropout -> + input_tensor -> LayerNorm with Hugging Face's submodule names (dense, LayerNorm, dropout): a BERT state dict
    loads strictly.  The last three steps are one `dropout_add_layer_norm` call."""

    def __init__(self, in_features: int, hidden_size: int, eps: float, p: float):
        super().__init__()
        self.dense = nn.Linear(in_features, hidden_size)
        self.LayerNorm = nn.LayerNorm(hidden_size, eps=eps)
        self.dropout = nn.Dropout(p)

    @classmethod
    def from_module(cls, org: nn.Module):
        """The fused form of a module with dense / LayerNorm / dropout submodules, sharing them (and so their parameters)."""
        new = cls.__new__(cls)
        nn.Module.__init__(new)
        new.dense, new.LayerNorm, new.dropout = org.dense, org.LayerNorm, org.dropout
        new.train(org.training)
        return new

    def forward(self, hidden_states: torch.Tensor, input_tensor: torch.Tensor) -> torch.Tensor:
        ln = self.LayerNorm
        return dropout_add_layer_norm(self.dense(hidden_states), input_tensor, ln.weight, ln.bias, self.dropout.p, ln.eps, self.training)


class FusedBertSelfOutput(_FusedBertTail):
    """BertSelfOutput: hidden_size -> hidden_size."""

    def __init__(self, config):
        super().__init__(config.hidden_size, config.hidden_size, config.layer_norm_eps, config.hidden_dropout_prob)


class FusedBertOutput(_FusedBertTail):
    """BertOutput: intermediate_size -> hidden_size."""

    def __init__(self, config):
        super().__init__(config.intermediate_size, config.hidden_size, config.layer_norm_eps, config.hidden_dropout_prob)


_FUSED_TAILS = {"BertSelfOutput": FusedBertSelfOutput, "BertOutput": FusedBertOutput}


def fuse_block_tails(model: nn.Module) -> int:
    """Swap every submodule whose class is named BertSelfOutput / BertOutput for its fused form, in place; the new modules share the old
    ones' dense, LayerNorm and dropout (state dicts and optimisers keep working).  Matches by class name - `transformers` is not
    imported.  Returns the number of modules swapped."""
    n = 0
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            fused = _FUSED_TAILS.get(type(child).__name__)
            if fused is not None and all(hasattr(child, a) for a in ("dense", "LayerNorm", "dropout")):
                setattr(parent, name, fused.from_module(child))
                n += 1
    return n
