"""The differentiable attention core on the HIP training kernels (include/oeh.h: oeh_attn_fwd_train / oeh_attn_bwd).

`fused_attention(q, k, v, ...)` is the op chain matmul -> scale -> mask -> clamp -> softmax / softmax_1 [-> clip] -> matmul of
opt_attention.py:204-263 / bert_attention.py:222-292 as ONE torch.autograd.Function: it saves q, k, v, o and the fp32 row statistic
lse - nothing of size Sq x Sk - and its backward is two HIP kernels.  Masks receive no gradient.  What the kernels do not take
(fp32 storage, head dim != 64, a softmax callable outside the registry) raises OehError with code -95: the caller decides, there is
no quiet reroute.  The attention modules call it when `attention.FUSED_BACKWARD` is on (attention.set_fused_backward).

Attention dropout (dropout_p > 0) runs inside the kernels: the keep mask of element (b, h, i, j) comes from a counter-based generator
(Philox4x32-10, include/oeh.h: oeh_dropout) keyed by a 64-bit seed, so the backward regenerates it from the seed saved in ctx and
nothing of size Sq x Sk is stored.  Without a dropout_seed one is drawn from torch's default CPU generator: torch.manual_seed
reproduces a run.  The mask is a different random stream from nn.Dropout's (attention.set_fused_dropout).
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops
from .ops import SoftmaxSpec

# calls of the fused training path since import (tests read it to see which path a module took)
CALLS = {"forward": 0, "backward": 0}


def _spec(softmax) -> Optional[SoftmaxSpec]:
    if isinstance(softmax, SoftmaxSpec):
        return softmax
    from .softmax import spec_of

    return spec_of(softmax)


def _unsupported(msg: str) -> _lib.OehError:
    err = _lib.OehError(f"fused_attention: {msg} (include/oeh.h: oeh_attn_fwd_train)")
    err.code = -95
    return err


class _FusedAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, spec, scale, scale_div, key_pad_mask, full_mask, causal, clamp_min, mask_min, dropout_p, dropout_seed):
        kw = dict(softmax=spec, scale=scale, scale_div=scale_div, key_pad_mask=key_pad_mask, full_mask=full_mask, causal=causal,
                  clamp_min=clamp_min, mask_min=mask_min, dropout_p=dropout_p, dropout_seed=dropout_seed)
        o, lse = ops.attn_fwd_train(q, k, v, **kw)
        ctx.save_for_backward(q, k, v, o, lse, key_pad_mask, full_mask)
        ctx.kw = {n: kw[n] for n in ("softmax", "scale", "scale_div", "causal", "clamp_min", "mask_min", "dropout_p", "dropout_seed")}
        ctx.mark_non_differentiable(lse)
        CALLS["forward"] += 1
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, key_pad_mask, full_mask = ctx.saved_tensors
        dq, dk, dv = ops.attn_bwd(q, k, v, o, do, lse, key_pad_mask=key_pad_mask, full_mask=full_mask, **ctx.kw)
        CALLS["backward"] += 1
        return dq, dk, dv, None, None, None, None, None, None, None, None, None, None


def draw_seed() -> int:
    """A uint64 dropout seed from torch's default CPU generator (a host op: no device sync; torch.manual_seed reproduces it)."""
    lo, hi = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64).tolist()
    return lo | (hi << 32)


def fused_supported(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, softmax) -> bool:
    """True when `fused_attention` takes this problem: GPU fp16 / bf16 q, k, v of one dtype, head dim 64, a registry softmax."""
    spec = _spec(softmax)
    return (spec is not None and q.is_cuda and q.dim() == 4 and k.dim() == 4 and v.dim() == 4 and q.dtype == k.dtype == v.dtype
            and ops.train_supported(q, spec))


def fused_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, softmax=SoftmaxSpec(), scale: float = 1.0, scale_div: float = 0.0,
                    key_pad_mask: Optional[torch.Tensor] = None, full_mask: Optional[torch.Tensor] = None, causal: bool = False,
                    clamp_min: bool = False, mask_min: Optional[float] = None, dropout_p: float = 0.0,
                    dropout_seed: Optional[int] = None) -> torch.Tensor:
    """Differentiable attention core.  q, k, v: logical (B,H,S,64) fp16 / bf16 views on one GPU; softmax: a SoftmaxSpec or a
    SOFTMAX_MAPPING entry; scale (multiply) or scale_div (divide, BERT); key_pad_mask additive (B,Sk) (or HF's (B,1,1,Sk));
    full_mask additive (B,1,Sq,Sk); causal: analytic mask (mask_min above the shifted diagonal); clamp_min: max(scores, mask_min);
    mask_min defaults to finfo(q.dtype).min; dropout_p: attention dropout on the (clipped) probabilities, 0 <= p < 1 (ignored when 0),
    its mask drawn from dropout_seed (uint64; default: draw_seed()).  Returns the logical (B,H,Sq,64) context, (B,Sq,H,64)-contiguous
    like ops.attn_fwd."""
    spec = _spec(softmax)
    if spec is None:
        raise _unsupported(f"softmax {softmax!r} is not a registry entry")
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError("q, k, v must be 4-D (B,H,S,D) views")
    if not (q.dtype == k.dtype == v.dtype):
        raise ValueError(f"q/k/v dtypes must match, got {q.dtype}, {k.dtype}, {v.dtype}")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise _unsupported(f"storage {q.dtype} (fp16 / bf16 only)")
    if q.shape[3] != 64:
        raise _unsupported(f"head dim {q.shape[3]} (64 only)")
    ops._need_gpu(q, k, v, key_pad_mask, full_mask, allow_grad=True)
    if key_pad_mask is not None and key_pad_mask.requires_grad or full_mask is not None and full_mask.requires_grad:
        key_pad_mask = None if key_pad_mask is None else key_pad_mask.detach()
        full_mask = None if full_mask is None else full_mask.detach()
    dropout_p = float(dropout_p)
    if dropout_p == 0.0:
        dropout_seed = None
    elif dropout_seed is None:
        dropout_seed = draw_seed()
    return _FusedAttention.apply(q, k, v, spec, float(scale), float(scale_div), key_pad_mask, full_mask, bool(causal), bool(clamp_min),
                                 None if mask_min is None else float(mask_min), dropout_p, dropout_seed)
