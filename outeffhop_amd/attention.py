"""Shared host-side pieces of the drop-in attention modules: the gate-type enum, gate construction /
evaluation, and the dispatch between the fused HIP kernel and the unfused (observable) path.

Reference anchors: AttentionGateType / logit  OutEffHop/transformers_language/models/bert_attention.py:16-25
                   gate definitions            bert_attention.py:119-162 (= opt_attention.py:105-144, vit_attention.py:152-195)
                   gate evaluation             bert_attention.py:294-331
"""
from __future__ import annotations

import math
import weakref
from enum import Flag
from functools import partial
from typing import Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib, ops
from . import softmax as _softmax
from ._watch import cached
from .ops import AttnFakeQuant, SoftmaxSpec
from .softmax import spec_of


class BaseEnumOptions(Flag):
    """Enum whose str() is the member name and that can list its names (quantization/utils.py:35-41)."""

    def __str__(self):
        return self.name

    @classmethod
    def list_names(cls):
        return [m.name for m in cls]


class AttentionGateType(BaseEnumOptions):
    none = 0
    unconditional_per_head = 1
    conditional_per_head = 2
    conditional_per_token = 3


def logit(p, eps=1e-16):
    p = np.clip(p, eps, 1 - eps)
    return -np.log(1 / p - 1)


_CONDITIONAL = (AttentionGateType.conditional_per_head, AttentionGateType.conditional_per_token)


def build_gate(num_heads: int, head_dim: int, model_dim: int, gate_type, gate_init, use_mlp: bool, use_mlp2: bool,
               all_features: bool, fine_tuning: bool, ft_std: float):
    """Create the `alpha` member exactly as the reference names/initialises it:
    Parameter[H] | Linear(E,H) | ModuleList of per-head Linear(d,1) / Sequential(Linear,ReLU,Linear) | None."""
    if gate_type == AttentionGateType.unconditional_per_head:
        return nn.Parameter(torch.zeros(num_heads), requires_grad=True)
    if gate_type not in _CONDITIONAL:
        return None
    if all_features:
        return nn.Linear(model_dim, num_heads, bias=True)
    heads = []
    for _ in range(num_heads):
        if use_mlp or use_mlp2:
            width = head_dim // 4 if use_mlp else head_dim
            heads.append(nn.Sequential(nn.Linear(head_dim, width, bias=True), nn.ReLU(), nn.Linear(width, 1, bias=True)))
            continue
        fc = nn.Linear(head_dim, 1, bias=True)
        if gate_init is not None:
            nn.init.constant_(fc.bias, float(logit(gate_init)))
        if fine_tuning:
            nn.init.normal_(fc.weight, mean=0.0, std=ft_std)
        heads.append(fc)
    return nn.ModuleList(heads)


# what a quantised module takes over from the module it wraps (quantization._QuantAttnBase._init_common)
GATE_ATTRS = ("attn_gate_type", "attn_gate_init", "attn_gate_mlp", "attn_gate_mlp2", "attn_gate_linear_all_features", "alpha", "gate_fn", "pooling_fn")


def init_gate(mod: nn.Module, num_heads: int, head_dim: int, model_dim: int, gate_type, gate_init, use_mlp: bool, use_mlp2: bool,
              all_features: bool, fine_tuning: bool, ft_std: float) -> None:
    """The gate attributes of a module's constructor as the reference sets them, `alpha` (`build_gate`) last: call it where the
    reference builds `alpha`, so that parameter order and the draws from the RNG are the reference's."""
    mod.last_gate_avg_prob = None
    mod.last_gate_all_probs = None
    mod.attn_gate_type = gate_type
    mod.attn_gate_init = gate_init
    mod.attn_gate_mlp = use_mlp
    mod.attn_gate_mlp2 = use_mlp2
    mod.attn_gate_linear_all_features = all_features
    mod.gate_fn = torch.sigmoid
    mod.pooling_fn = partial(torch.mean, dim=1, keepdims=True)
    mod.fine_tuning = fine_tuning
    mod.gate_scaling_factor = 1.0 / gate_init if (fine_tuning and gate_init is not None) else 1.0
    mod.alpha = build_gate(num_heads, head_dim, model_dim, gate_type, gate_init, use_mlp, use_mlp2, all_features, fine_tuning, ft_std)


class GateBookkeeping:
    """`last_gate_avg_prob` (bert_attention.py:329-331: the per-head mean of the gate probabilities, read by the training scripts'
    logging) as a LAZY attribute: the forward pass records the gate tensor, the two reductions run when somebody reads the
    value - not as two extra launches in every layer of every forward.  Assignment (None, a tensor) works as before."""

    @property
    def last_gate_avg_prob(self):
        src = self.__dict__.get("_oeh_gate_avg_src")
        if src is not None:
            gate, num_heads = src
            self.__dict__["_oeh_gate_avg"] = gate.mean(dim=0).view(num_heads, -1).mean(dim=1)
            self.__dict__["_oeh_gate_avg_src"] = None
        return self.__dict__.get("_oeh_gate_avg")

    @last_gate_avg_prob.setter
    def last_gate_avg_prob(self, value):
        self.__dict__["_oeh_gate_avg"] = value
        self.__dict__["_oeh_gate_avg_src"] = None


def _note_gate(mod: nn.Module, gate: torch.Tensor, num_heads: int) -> None:
    mod.last_gate_all_probs = gate
    if isinstance(mod, GateBookkeeping):
        mod.__dict__["_oeh_gate_avg_src"] = (gate, num_heads)
    else:
        mod.last_gate_avg_prob = gate.mean(dim=0).view(num_heads, -1).mean(dim=1)


_warned_autograd = []


def autograd_needed(mod: nn.Module, *ts) -> bool:
    """True when this forward has to be differentiable: autograd is recording and an input or a parameter of the module requires
    grad (training under the reference's swap-in: run_clm.py:214-233, run_mlm.py:200-219).  The modules then take the observable
    torch-op path (`unfused_core`, `softmax.softmax_autograd`, `gate_autograd`) - slower, on the GPU - because the HIP kernels are
    forward-only; under torch.no_grad() / inference_mode() nothing changes.  Says so once."""
    if not torch.is_grad_enabled():
        return False
    if not (any(t is not None and t.requires_grad for t in ts) or any(p.requires_grad for p in mod.parameters())):
        return False
    if not _warned_autograd:
        import warnings

        _warned_autograd.append(True)
        warnings.warn("outeffhop_amd: autograd is recording - this forward runs the differentiable torch-op path, not the fused HIP "
                      "kernels (forward-only); wrap inference in torch.no_grad()", RuntimeWarning, stacklevel=3)
    return True


def gate_autograd(mod: nn.Module, hidden_states: torch.Tensor, num_heads: int) -> Optional[torch.Tensor]:
    """The gate as the reference's torch ops (bert_attention.py:294-331 = opt_attention.py:265-304, vit_attention.py:241-262), so
    that gradients reach `alpha`: probabilities broadcastable to (B,H,T,1) WITHOUT the scaling factor, bookkeeping attributes set."""
    gt = mod.attn_gate_type
    if gt == AttentionGateType.unconditional_per_head:
        GATE_TRAIN_CALLS["torch"] += 1
        gate = torch.sigmoid(mod.alpha)
        mod.last_gate_avg_prob = gate.view(-1)
        return gate.view(1, -1, 1, 1)
    if gt not in _CONDITIONAL:
        return None
    GATE_TRAIN_CALLS["torch"] += 1
    if mod.attn_gate_linear_all_features:
        gate = torch.sigmoid(mod.alpha(hidden_states)).permute(0, 2, 1).contiguous().unsqueeze(3)
    else:
        x = hidden_states.view(hidden_states.shape[:-1] + (num_heads, -1)).permute(0, 2, 1, 3)  # (B,H,T,d)
        logits = []
        for h in range(num_heads):
            a = mod.alpha[h](x[:, h, ...])  # (B,T,1)
            if gt == AttentionGateType.conditional_per_head:
                a = a.mean(dim=1, keepdim=True)  # (B,1,1)
            logits.append(a)
        gate = torch.sigmoid(torch.stack(logits, dim=1))  # (B,H,*,1)
    mod.last_gate_all_probs = gate
    mod.last_gate_avg_prob = gate.mean(dim=0).view(num_heads, -1).mean(dim=1)
    return gate


class GateState:
    """Evaluates the gate with HIP kernels and keeps the reference's bookkeeping attributes."""

    @staticmethod
    def packed_weights(mod: nn.Module):
        """Per-head predictor weights stacked as (H,d)/(H) or (H,m,d)/(H,m)/(H,m)/(H); cached until a parameter (or a head module) changes."""
        heads = mod.alpha
        layers = tuple(heads.modules())

        def pack():
            with torch.no_grad():
                if isinstance(heads[0], nn.Linear):
                    return (torch.stack([h.weight[0] for h in heads]).float().contiguous(),
                            torch.stack([h.bias[0] for h in heads]).float().contiguous(), None, None)
                return (torch.stack([h[0].weight for h in heads]).float().contiguous(),
                        torch.stack([h[0].bias for h in heads]).float().contiguous(),
                        torch.stack([h[2].weight[0] for h in heads]).float().contiguous(),
                        torch.stack([h[2].bias[0] for h in heads]).float().contiguous())
        return cached(mod.__dict__, "_oeh_gate_cache", layers, lambda: [(m._parameters, n_) for m in layers for n_ in m._parameters], pack)

    @staticmethod
    def predictor(mod: nn.Module, hidden_states: torch.Tensor, num_heads: int, scaling: float):
        """The conditional per-token gate as an `ops.GatePredictor` for evaluation INSIDE the attention kernel, or None
        when the module's gate is of another kind (then `evaluate`).  Bookkeeping attributes are set from the
        predictor's `out` tensor by `finish_predictor` after the launch."""
        if mod.attn_gate_type != AttentionGateType.conditional_per_token or mod.attn_gate_linear_all_features:
            return None
        if hidden_states.dtype not in (torch.float16, torch.bfloat16, torch.float32) or hidden_states.dim() != 3 or hidden_states.stride(2) != 1:
            return None
        w1, b1, w2, b2 = GateState.packed_weights(mod)
        B, T, _ = hidden_states.shape
        out = torch.empty((B, num_heads, T), dtype=torch.float32, device=hidden_states.device)
        return ops.GatePredictor(hidden_states, w1, b1, w2, b2, scaling=float(scaling), out=out)

    @staticmethod
    def finish_predictor(mod: nn.Module, gp, num_heads: int) -> None:
        _note_gate(mod, gp.out.unsqueeze(3), num_heads)

    @staticmethod
    def evaluate(mod: nn.Module, hidden_states: torch.Tensor, num_heads: int) -> Optional[torch.Tensor]:
        """Gate probabilities, broadcastable to (B,H,T,1), fp32, WITHOUT the scaling factor; sets
        last_gate_avg_prob / last_gate_all_probs like bert_attention.py:299,329-331."""
        gt = mod.attn_gate_type
        if gt != AttentionGateType.none and ops.grad_recording(hidden_states, *(mod.alpha.parameters() if isinstance(mod.alpha, nn.Module) else (mod.alpha,))):
            ops._need_gpu(hidden_states, allow_grad=True)
            return gate_autograd(mod, hidden_states, num_heads)
        if gt == AttentionGateType.unconditional_per_head:
            gate = torch.sigmoid(mod.alpha.float())
            mod.last_gate_avg_prob = gate.view(-1)
            return gate.view(1, -1, 1, 1)
        if gt not in _CONDITIONAL:
            return None
        if mod.attn_gate_linear_all_features:
            gate = torch.sigmoid(mod.alpha(hidden_states).float()).permute(0, 2, 1).contiguous().unsqueeze(3)
        else:
            w1, b1, w2, b2 = GateState.packed_weights(mod)
            gate = ops.gate_fwd(hidden_states, num_heads, w1, b1, w2, b2,
                                per_head_pool=(gt == AttentionGateType.conditional_per_head), scaling=1.0)
        _note_gate(mod, gate, num_heads)
        return gate


def module_gate(mod: nn.Module, hidden_states: torch.Tensor, num_heads: int, in_kernel: bool):
    """The gate of one forward of a float module: (gate values | None, ops.GatePredictor | None).  `in_kernel`: this forward may
    evaluate a conditional per-token gate inside the attention kernel (it fuses, and the predictor's input is the query side's) -
    then the predictor, scaling inside, and `GateState.finish_predictor` after the launch.  Otherwise the values, times
    gate_scaling_factor unless the gate is unconditional (context *= gate * scaling, bert_attention.py:327) - or, with FUSED_GATE_TRAIN on
    in a differentiable forward the training kernels take (`gate_train_units`), a `DeferredGate` in their place: `gated_merge` runs it."""
    gp = GateState.predictor(mod, hidden_states, num_heads, mod.gate_scaling_factor) if in_kernel else None
    if gp is not None:
        return None, gp
    if FUSED_GATE_TRAIN and not in_kernel:  # (a differentiable forward is never fusable: its gate goes to gated_merge)
        units = gate_train_units(mod, hidden_states, num_heads)
        if units is not None:
            return DeferredGate(mod, hidden_states, num_heads, float(mod.gate_scaling_factor), units), None
    gate = GateState.evaluate(mod, hidden_states, num_heads)
    if gate is not None and mod.attn_gate_type != AttentionGateType.unconditional_per_head:
        gate = gate * mod.gate_scaling_factor
    return gate, None


# ---- the conditional per-token gate in training on the fused kernels (opt-in): with FUSED_GATE_TRAIN on, a differentiable forward of a module
# whose gate is conditional_per_token with separate per-head predictors (Linear(d,1) or Linear-ReLU-Linear, not attn_gate_linear_all_features),
# head dim 32 or 64, at most 64 hidden units, fp16 / bf16 / fp32 layer input with a contiguous last dimension runs predictors + sigmoid + context *
# gate as ops.gate_apply_fwd and its backward as ops.gate_apply_bwd (`GateApply`) instead of `gate_autograd`'s per-head loop and a
# torch multiply.  Everything else - the switch off, conditional_per_head, all-features and unconditional gates, another head dim, wider
# predictors, float64, the quantised modules (quantization.py calls GateState.evaluate itself) - keeps `gate_autograd`.  GATE_TRAIN_CALLS counts
# the launches of each kind.  Off by default: the gate enters the product as gate_out * scaling in fp32, where the torch path rounds the gate to a
# 16-bit context's dtype first.
FUSED_GATE_TRAIN = False
GATE_TRAIN_CALLS = {"forward": 0, "backward": 0, "torch": 0}


def set_fused_gate_train(on: bool = True) -> bool:
    """Run the per-token gate of differentiable forwards on the fused HIP kernels (True) or keep the torch-op path (False, the default).
    Returns the previous setting."""
    global FUSED_GATE_TRAIN
    prev, FUSED_GATE_TRAIN = FUSED_GATE_TRAIN, bool(on)
    return prev


def _predictor_units(alpha) -> Optional[int]:
    """Hidden units of the per-head predictors of `build_gate` (0: Linear(d, 1)), or None when `alpha` is anything else."""
    if not isinstance(alpha, nn.ModuleList) or len(alpha) == 0:
        return None
    first = alpha[0]
    if type(first) is nn.Linear:
        ok = all(type(f) is nn.Linear and f.out_features == 1 and f.bias is not None and f.in_features == first.in_features for f in alpha)
        return 0 if ok else None
    if type(first) is nn.Sequential and len(first) == 3 and type(first[0]) is nn.Linear:
        m, d = first[0].out_features, first[0].in_features
        for f in alpha:
            if not (type(f) is nn.Sequential and len(f) == 3 and type(f[0]) is nn.Linear and type(f[1]) is nn.ReLU and type(f[2]) is nn.Linear):
                return None
            if (f[0].out_features, f[0].in_features, f[2].in_features, f[2].out_features) != (m, d, m, 1) or f[0].bias is None or f[2].bias is None:
                return None
        return m
    return None


def gate_train_scope(mod: nn.Module, hidden_states: torch.Tensor, num_heads: int) -> Optional[int]:
    """The part of the route predicate that does not depend on where the tensors live: the predictors' hidden units (0: Linear) when the
    gate is conditional_per_token with separate predictors inside the kernels' scope and autograd is recording for the layer input or a
    predictor parameter, else None."""
    if mod.attn_gate_type != AttentionGateType.conditional_per_token or mod.attn_gate_linear_all_features:
        return None
    units = _predictor_units(mod.alpha)
    if units is None or units > ops.GATE_TRAIN_MAX_UNITS or has_hooks(*mod.alpha):
        return None
    if hidden_states.dim() != 3 or hidden_states.dtype not in (torch.float16, torch.bfloat16, torch.float32) or hidden_states.stride(2) != 1:
        return None
    if hidden_states.shape[2] % num_heads or hidden_states.shape[2] // num_heads not in ops.GATE_TRAIN_DIMS:
        return None
    first = mod.alpha[0] if units == 0 else mod.alpha[0][0]
    if first.in_features != hidden_states.shape[2] // num_heads or not all(p.is_floating_point() and p.dtype != torch.float64 for p in mod.alpha.parameters()):
        return None
    if not ops.grad_recording(hidden_states, *mod.alpha.parameters()):
        return None
    return units


def gate_train_units(mod: nn.Module, hidden_states: torch.Tensor, num_heads: int) -> Optional[int]:
    """The route predicate of the fused gate training path: `gate_train_scope`, and the layer input and every predictor parameter on one
    GPU (like `fused_supported`: anything else keeps `gate_autograd`, which says what it needs).  Does not look at the switch."""
    if not hidden_states.is_cuda:
        return None
    units = gate_train_scope(mod, hidden_states, num_heads)
    if units is None or any(p.device != hidden_states.device for p in mod.alpha.parameters()):
        return None
    return units


def _or_all(values) -> int:
    out = 0
    for v in values:
        out |= int(v)
    return out


class DeferredGate:
    """What `module_gate` returns in place of gate values when the fused training path takes the gate: `gated_merge` evaluates it together
    with the product, once the context exists."""
    __slots__ = ("mod", "hidden", "num_heads", "scaling", "units")

    def __init__(self, mod, hidden, num_heads, scaling, units):
        self.mod, self.hidden, self.num_heads, self.scaling, self.units = mod, hidden, num_heads, scaling, units

    def params(self):
        out = []
        for f in self.mod.alpha:
            out += [f.weight, f.bias] if self.units == 0 else [f[0].weight, f[0].bias, f[2].weight, f[2].bias]
        return out

    def takes(self, ctx: torch.Tensor) -> bool:
        """The context is one the kernels take: the layer input's dtype and device, (B,H,T,d), last dimension contiguous, and the rows of
        both tensors 16-byte aligned (pointer and strides) - what the entry point would refuse with OEH_EALIGN."""
        B, T, E = self.hidden.shape
        if ctx.dtype != self.hidden.dtype or ctx.device != self.hidden.device or tuple(ctx.shape) != (B, self.num_heads, T, E // self.num_heads) or ctx.stride(3) != 1:
            return False
        eb = ctx.element_size()
        return all((t.data_ptr() | _or_all(st * eb for st in t.stride()[:-1])) % 16 == 0 for t in (ctx, self.hidden))


class GateApply(torch.autograd.Function):
    """(merged, gate_out) = (ctx (B,H,T,d) * sigmoid(predictors(hidden_states)) * scaling as (B,T,H*d), the probabilities (B,H,T) fp32) on the
    fused training kernels (ops.gate_apply_fwd / ops.gate_apply_bwd).  params: per head (weight, bias) of a Linear(d,1) predictor (units == 0)
    or (fc1.weight, fc1.bias, fc2.weight, fc2.bias).  gate_out is not differentiable (bookkeeping only)."""

    @staticmethod
    def forward(fctx, ctx, hidden_states, scaling, units, *params):
        f32 = lambda ts: torch.stack([t.detach() for t in ts]).float().contiguous()  # noqa: E731
        if units == 0:
            w1, b1, w2, b2 = f32([p[0] for p in params[0::2]]), f32([p[0] for p in params[1::2]]), None, None
        else:
            w1, b1 = f32(params[0::4]), f32(params[1::4])
            w2, b2 = f32([p[0] for p in params[2::4]]), f32([p[0] for p in params[3::4]])
        out, gate_out = ops.gate_apply_fwd(ctx, hidden_states, w1, b1, w2, b2, scaling)
        GATE_TRAIN_CALLS["forward"] += 1
        fctx.save_for_backward(ctx, hidden_states, gate_out, w1, b1, w2, b2)
        fctx.scaling, fctx.units, fctx.param_dtypes = scaling, units, [p.dtype for p in params]
        fctx.mark_non_differentiable(gate_out)
        return out, gate_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(fctx, dout, _dgate):
        ctx, hidden_states, gate_out, w1, b1, w2, b2 = fctx.saved_tensors
        dctx, dhidden, dw1, db1, dw2, db2 = ops.gate_apply_bwd(dout, ctx, hidden_states, gate_out, w1, b1, w2, b2, fctx.scaling,
                                                               want_dhidden=fctx.needs_input_grad[1])
        GATE_TRAIN_CALLS["backward"] += 1
        grads = []
        for h in range(w1.shape[0]):
            if fctx.units == 0:
                grads += [dw1[h:h + 1], db1[h:h + 1]]
            else:
                grads += [dw1[h], db1[h], dw2[h:h + 1], db2[h:h + 1]]
        grads = [g if g.dtype == dt else g.to(dt) for g, dt in zip(grads, fctx.param_dtypes)]
        return (dctx, dhidden, None, None, *grads)


def gated_merge(ctx: torch.Tensor, gate) -> torch.Tensor:
    """The tail of the differentiable cores (fused_train_core, unfused_core): (B,H,S,d) context * gate -> (B,S,H*d).  gate: the values, None,
    or a `DeferredGate` (FUSED_GATE_TRAIN): then `GateApply` - or, for a context the kernels do not take after all, `gate_autograd` now."""
    if isinstance(gate, DeferredGate):
        if gate.takes(ctx):
            merged, gate_out = GateApply.apply(ctx, gate.hidden, gate.scaling, gate.units, *gate.params())
            _note_gate(gate.mod, gate_out.unsqueeze(3), gate.num_heads)  # (fp32 and detached here; the torch path's is in the model's dtype, in the graph)
            return merged
        gate = gate_autograd(gate.mod, gate.hidden, gate.num_heads) * gate.scaling
    if gate is not None:
        ctx = ctx * gate.to(ctx.dtype)
    return ctx.transpose(1, 2).reshape(ctx.shape[0], ctx.shape[2], -1)


# ---- fused q/k/v projection: the three E->E Linears of a self-attention layer as ONE library GEMM with the
# concatenated weight, returning strided (B,S,E) views of its (B,S,3E) output (the attention kernel takes strides, so there is
# no copy either side).  Inference only: parameters keep the reference's names (query/key/value, q_proj/k_proj/v_proj) and the
# concatenation is cached per module and rebuilt when a weight changes (tensor version counters / storage pointers).
FUSE_QKV = True


def fused_qkv(owner: nn.Module, x: torch.Tensor, lq: nn.Linear, lk: nn.Linear, lv: nn.Linear, q_scale: float = 1.0):
    """(q, k, v) = (lq(x) * q_scale, lk(x), lv(x)) from one GEMM, or None when the fused form does not apply (autograd on,
    QuantLinear / hooked / unequal layers, q_scale not a power of two - folding it into the weights is exact only then)."""
    if not FUSE_QKV or torch.is_grad_enabled() or not x.is_cuda:
        return None
    if not (type(lq) is nn.Linear and type(lk) is nn.Linear and type(lv) is nn.Linear) or has_hooks(lq, lk, lv):
        return None
    ws = (lq.weight, lk.weight, lv.weight)
    bs = (lq.bias, lk.bias, lv.bias)
    if not (ws[0].shape == ws[1].shape == ws[2].shape) or ws[0].dtype != x.dtype or any((b is None) != (bs[0] is None) for b in bs):
        return None
    mant, _ = math.frexp(q_scale)
    if mant != 0.5:
        return None
    triple = triple_gemm_ok(x, lq, lk, lv)

    def concat():  # (the two layouts: the triple GEMM's operand with the bias inside | weight and bias)
        w = torch.cat([ws[0].detach() * q_scale, ws[1].detach(), ws[2].detach()], dim=0).contiguous()
        b = None if bs[0] is None else torch.cat([bs[0].detach() * q_scale, bs[1].detach(), bs[2].detach()], dim=0).contiguous()
        return (triple_weights(w, b), None) if triple else (w, b)
    w, b = cached(owner.__dict__, "_oeh_qkv_cache", (lq, lk, lv, q_scale, x.dtype, triple),
                  lambda: [(m._parameters, n_) for m in (lq, lk, lv) for n_ in ("weight", "bias")], concat)
    if triple:  # fp32 model: one fp16 GEMM on operand triples (bias inside), fp32-accurate
        y = torch.mm(ops.split_triples(x.reshape(-1, x.shape[-1])), w, out_dtype=torch.float32).view(*x.shape[:-1], w.shape[1])
    else:
        y = torch.nn.functional.linear(x, w, b)
    e = ws[0].shape[0]
    return y[..., :e], y[..., e:2 * e], y[..., 2 * e:]


# ---- fp32 Linears as ONE fp16 GEMM on operand triples (include/oeh.h: oeh_split_triples): x W^T + b to ~2^-22 relative - measured
# closer to the float64 result than the fp32 library GEMM - at about twice its speed.  Inference only (no autograd).
TRIPLE_GEMM = True


def triple_weights(weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """[Wh ; Wl 2^-6 ; Wh 2^-6 ; bh ; bl 2^-6 ; 0 x6] (3K + 8, N) fp16 for a (N, K) fp32 weight: W = Wh + Wl 2^-11, b = bh + bl 2^-11."""
    with torch.no_grad():
        w = weight.detach().float()
        wh = w.clamp(-65504.0, 65504.0).half()
        wl = ((w - wh.float()) * 2048.0).clamp(-65504.0, 65504.0).half()
        n, k = w.shape
        out = torch.zeros((3 * k + 8, n), dtype=torch.float16, device=w.device)
        out[:k] = wh.t()
        out[k:2 * k] = (wl.float() * 0.015625).half().t()
        out[2 * k:3 * k] = (wh.float() * 0.015625).half().t()
        if bias is not None:
            b = bias.detach().float()
            bh = b.clamp(-65504.0, 65504.0).half()
            out[3 * k] = bh
            out[3 * k + 1] = ((b - bh.float()) * 2048.0 * 0.015625).clamp(-65504.0, 65504.0).half()
    return out


def triple_gemm_ok(x: torch.Tensor, *lins: nn.Linear) -> bool:
    return (TRIPLE_GEMM and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()
            and all(type(m) is nn.Linear and m.weight.dtype == torch.float32 and m.in_features % 8 == 0 for m in lins) and not has_hooks(*lins))


def linear_fp32(lin: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    """`lin(x)` for an fp32 nn.Linear in inference: the triple GEMM when it applies (weights cached per module, rebuilt when a
    parameter changes), the module's own forward otherwise."""
    if not triple_gemm_ok(x, lin):
        return lin(x)
    w3 = cached(lin.__dict__, "_oeh_triple_cache", None, lambda: [(lin._parameters, "weight"), (lin._parameters, "bias")],
                lambda: triple_weights(lin.weight, lin.bias))
    a = ops.split_triples(x.reshape(-1, x.shape[-1]))
    return torch.mm(a, w3, out_dtype=torch.float32).view(*x.shape[:-1], lin.out_features)


def has_hooks(*mods: nn.Module) -> bool:
    for m in mods:  # (a plain loop, not any() over a generator: every eager forward asks)
        if m._forward_hooks or m._forward_pre_hooks:
            return True
    return False


def mask_min_of(attention_mask: Optional[torch.Tensor], fallback_dtype: torch.dtype) -> float:
    """The floor of a masked score: finfo.min of a floating mask's dtype, else of `fallback_dtype` (the activations')."""
    mdt = attention_mask.dtype if attention_mask is not None and attention_mask.is_floating_point() else fallback_dtype
    return float(torch.finfo(mdt).min)


def split_mask(mask: Optional[torch.Tensor], B: int, Sq: int, Sk: int):
    """Classify an additive HF mask: (B,1,1,Sk) -> key padding vector; (B,1,Sq,Sk) -> full mask."""
    if mask is None:
        return None, None
    if mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[2] == 1 and mask.shape[0] in (1, B) and mask.shape[3] == Sk:
        return mask.expand(B, 1, 1, Sk).reshape(B, Sk), None
    if mask.dim() == 4 and tuple(mask.shape) == (B, 1, Sq, Sk):
        return None, mask
    return None, mask.expand(B, 1, Sq, Sk)


class _TensorMemo(dict):
    """A result per LIVE tensor object: id(tensor) -> (weak reference to the tensor, its version counter, result).  An entry answers only
    while its weak reference still points at the asking tensor and the version counter is unchanged, never by address alone: the
    caching allocator gives the next batch's mask the same address (and Python the same id), and a result remembered by address
    would apply the previous batch's padding to it.  Entries die with their tensors; 64 at the most."""

    def lookup(self, t: torch.Tensor, compute):
        key = id(t)
        hit = self.get(key)
        if hit is not None:
            if hit[0]() is t and hit[1] == t._version:
                return hit[2]
            del self[key]
        res = compute(t)

        def _forget(dead, _k=key):  # the tensor object is gone: its id may be reused by any other object
            ent = self.get(_k)
            if ent is not None and ent[0] is dead:
                del self[_k]

        if len(self) > 64:
            self.clear()
        self[key] = (weakref.ref(t, _forget), t._version, res)
        return res


_causal_cache = _TensorMemo()
_padbool_cache = _TensorMemo()


def _classify_causal(mask: torch.Tensor):
    B, _, T, S = mask.shape
    fmin = torch.finfo(mask.dtype).min
    causal = torch.full((T, S), fmin, dtype=mask.dtype, device=mask.device).triu(1 + S - T)
    pad = mask[:, 0, -1, :].clamp(min=fmin)  # the last query row sees every key: what is left is padding
    recon = (causal[None, None] + pad[:, None, None, :]).clamp(min=fmin)
    ok = bool(torch.equal(mask.clamp(min=fmin), recon)) and bool(((pad == 0) | (pad == fmin)).all())
    return (True, (pad.contiguous() if bool((pad != 0).any()) else None)) if ok else (False, None)


def classify_causal(mask: torch.Tensor):
    """Recognise HF's decoder mask: a (B,1,T,S) additive tensor that equals causal(finfo.min above the shifted
    diagonal) + key-padding(finfo.min columns), up to the clamp at finfo.min the attention applies anyway
    (opt_attention.py:220-223).  Returns (True, pad_vector_or_None) or (False, None).
    One pass over the mask per distinct tensor OBJECT (_TensorMemo): HF hands the same tensor to every layer of a forward."""
    return _causal_cache.lookup(mask, _classify_causal)


def pad_is_boolean(mask: torch.Tensor) -> bool:
    """True when an additive mask holds only 0 (visible) and values <= -1e4 (hidden) - HF's extended masks hold 0 / finfo.min.
    The integer-matrix-core attention (`ops.attn_fwd_i8`) DROPS a padded key instead of adding the mask value to its score, which
    is the reference's result exactly for such masks.  One pass (and one host read) per distinct mask tensor object (_TensorMemo)."""
    return _padbool_cache.lookup(mask, lambda m: bool(((m == 0) | (m <= -1.0e4)).all()))


def resolve_mask(attention_mask: Optional[torch.Tensor], B: int, Sq: int, Sk: int, dtype: torch.dtype, detect_causal: bool = False):
    """An additive HF mask as the kernels take it: (key-padding vector (B,Sk) | None, full (B,1,Sq,Sk) mask | None, causal, mask_min).
    With `detect_causal` a full mask that is HF's decoder mask becomes the analytic causal mask plus its padding vector
    (`classify_causal`: one device pass per mask tensor object); `dtype`: the activations', the floor's fallback (`mask_min_of`)."""
    pad, full = split_mask(attention_mask, B, Sq, Sk)
    causal = False
    if full is not None and detect_causal and Sq <= Sk:
        causal, padvec = classify_causal(full)
        if causal:
            full, pad = None, padvec
    return pad, full, causal, mask_min_of(attention_mask, dtype)


def kv_source(k_proj, v_proj, to_heads, hidden_states, cross_states, past_key_value, fused_kv=None):
    """HF's rule for where a forward's keys and values come from, as logical (B,H,S,d) tensors: projected from the layer input; those
    appended to a cached pair on dim 2; projected from `cross_states`; or, for cross-attention with a cache, the cached pair as it
    is.  `fused_kv`: the k / v parts of an already fused QKV result of the layer input (`fused_qkv`), used instead of the projections."""
    if cross_states is not None and past_key_value is not None:
        return past_key_value[0], past_key_value[1]
    if fused_kv is not None:
        k, v = to_heads(fused_kv[0]), to_heads(fused_kv[1])
    else:
        src = hidden_states if cross_states is None else cross_states
        k, v = to_heads(k_proj(src)), to_heads(v_proj(src))
    if cross_states is None and past_key_value is not None:
        k, v = torch.cat([past_key_value[0], k], dim=2), torch.cat([past_key_value[1], v], dim=2)
    return k, v


# ---- fp32-accurate context for fp32 models (opt-in): with COMPENSATED_PV on, every fused inference call on fp32 storage without fake-quant
# passes pv_pairs=True (include/oeh.h: oeh_attn_opts) - the probabilities enter the product with V as fp16 pairs, so the context is as accurate
# as the scores (the reference's validate runs measure outliers on fp32 models).  The in-kernel gate predictor is not available then (the gate
# runs as oeh_gate_fwd + gate values).  Off by default: it changes the fp32 outputs (in the last bits) and costs time.  The observable
# (torch-op) path and the training path do not change.
COMPENSATED_PV = False


def set_compensated_pv(on: bool = True) -> None:
    """Compute the fused fp32 attention's context from probability pairs (True) or with the fp16 probability operand (False, the default)."""
    global COMPENSATED_PV
    COMPENSATED_PV = bool(on)


def pv_pairs_for(q: torch.Tensor, fq=None) -> bool:
    """What attention calls on q pass as ops.attn_fwd(..., pv_pairs=): COMPENSATED_PV on fp32 storage without fake-quant."""
    return COMPENSATED_PV and q.dtype == torch.float32 and fq is None


# ---- generation steps on the split-key decode kernels: with SPLIT_DECODE on, a fused call that says `decode=True` (OPT's self-attention with
# a past_key_value, and the quantised decoder QuantizedOPTAttentionWithExtras with its three fake-quantisers: oeh_attn_decode_fq) and has at
# most 16 query rows, 16-bit storage, head dim 64, no gate predictor and no (B,1,Sq,Sk) mask left after
# split_mask / classify_causal runs ops.attn_decode - the keys of a head over many workgroups plus a combine pass - instead of ops.attn_fwd's
# one serial workgroup per (batch, head).  Outputs agree within the contract, not bit for bit (another summation order).  What the entry point
# refuses (OehError -95 / -14) falls back to ops.attn_fwd.
# OFF by default: against ops.attn_fwd (tools/decode_bench.py, profiles/decode_bench.txt; OPT-125m heads, one query row, fp16) the decode path
# measured 1.8-2.1x faster at B H = 12, Sk = 2048, but 0.55-0.9x at Sk = 512 and at B H = 192, and the crossover between those points is not
# measured - this rule routes every problem in scope, so it stays opt-in until a measured "B H <= x and Sk >= y" replaces it.
# With the fused INT8 chain (a quantised decoder's step: oeh_attn_decode_fq against oeh_attn_fwd's fq forms; tools/decode_bench.py --fq,
# profiles/decode_bench_fq.txt, the second table of DESIGN.md 10): 2.25-2.3x at B H = 12, Sk = 2048, 1.1x at B H = 192, Sk = 2048, 0.55-0.67x at Sk = 512.
SPLIT_DECODE = False


def set_split_decode(on: bool = True) -> None:
    """Route the modules' generation steps to the split-key decode kernels (True) or keep them on ops.attn_fwd (False, the default)."""
    global SPLIT_DECODE
    SPLIT_DECODE = bool(on)


def attention_core(
    q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, softmax_fn, scale: float = 1.0, scale_div: float = 0.0,
    attention_mask: Optional[torch.Tensor] = None, clamp_min: bool = False, detect_causal: bool = False,
    gate: Optional[torch.Tensor] = None, fq: Optional[AttnFakeQuant] = None, mask_min: Optional[float] = None,
    gate_mlp=None, decode: bool = False,
) -> torch.Tensor:
    """Fused path: logical (B,H,S,d) views in, (B,Sq,H*d) context out (head merge is free).  `gate_mlp`
    (ops.GatePredictor): the per-token gate is evaluated inside the attention kernel where the library supports that
    (full-row 16-bit kernel, <= 16 hidden units), else by `ops.gate_fwd` first.  `decode`: a generation step against a key / value
    cache - the split-key decode kernels where they apply (SPLIT_DECODE above)."""
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    spec = spec_of(softmax_fn)
    pad, full, causal, floor = resolve_mask(attention_mask, B, Sq, Sk, q.dtype, detect_causal)
    if mask_min is None:  # (a caller may set the floor itself)
        mask_min = floor
    # the fused INT8 chain stays on the quantiser grid with padded keys when the mask is a mask (0 / finfo.min entries - what
    # classify_causal has verified for a decoder mask; else one look per mask tensor object): include/oeh.h key_pad_boolean
    pad_bool = pad is not None and fq is not None and (causal or pad_is_boolean(attention_mask))
    pv = pv_pairs_for(q, fq)
    kw = dict(softmax=spec, scale=scale, scale_div=scale_div, key_pad_mask=pad, full_mask=full, key_pad_boolean=pad_bool, causal=causal,
              clamp_min=clamp_min, mask_min=mask_min, fq=fq, pv_pairs=pv)
    out = None
    if (decode and SPLIT_DECODE and gate_mlp is None and full is None and Sq <= 16 and D == 64
            and q.dtype in (torch.float16, torch.bfloat16)):
        try:
            out = ops.attn_decode(q, k, v, softmax=spec, scale=scale, scale_div=scale_div, key_pad_mask=pad, causal=causal, clamp_min=clamp_min,
                                  mask_min=mask_min, gate=gate, fq=fq)
        except _lib.OehError as e:  # outside the decode entry point's scope after all (gamma > 0, ctx_emit_index, alignment ...): the general forward
            if e.code not in (-95, -14):
                raise
    if gate_mlp is not None:
        units = 0 if gate_mlp.w1.dim() == 2 else gate_mlp.w1.shape[1]
        if full is None and ops.fused_gate_ok(B, H, Sq, Sk, D, q.dtype, clip=bool(spec.clip), fq=fq is not None, units=units,
                                              base=spec.base, gamma=spec.gamma, key_pad=pad is not None, causal=causal,
                                              scale=scale, scale_div=scale_div, mask_min=mask_min, pv_pairs=pv):
            try:
                out = ops.attn_fwd(q, k, v, gate_mlp=gate_mlp, **kw)
            except _lib.OehError as e:  # an option combination the 16-bit MFMA kernels do not take after all (alignment ...)
                if e.code not in (-95, -14):
                    raise
        if out is None:
            gp = gate_mlp
            g = ops.gate_fwd(gp.hidden, H, gp.w1, gp.b1, gp.w2, gp.b2, scaling=1.0)
            if gp.out is not None:
                gp.out.copy_(g[..., 0])
            gate = g * gp.scaling
    if out is None:
        out = ops.attn_fwd(q, k, v, gate=gate, **kw)
    return out.permute(0, 2, 1, 3).reshape(B, Sq, H * D)


# ---- training on the fused kernels (opt-in): with FUSED_BACKWARD on, a module whose forward has to be differentiable and needs none of
# the observable path's features (dropout > 0 in training unless FUSED_DROPOUT, output_attentions, hooks on the taps, head_mask,
# fake-quant, user callables) runs its core through autograd_attention.fused_attention - the HIP training forward and backward, nothing of size Sq x Sk saved -
# instead of unfused_core.  fp16 / bf16, head dim 64; anything else keeps the torch-op path.  Off by default.
FUSED_BACKWARD = False


def set_fused_backward(on: bool = True) -> None:
    """Switch the modules' differentiable path to the fused HIP backward (True) or back to the torch-op path (False, the default)."""
    global FUSED_BACKWARD
    FUSED_BACKWARD = bool(on)


# ---- attention dropout on the fused kernels (opt-in on top of FUSED_BACKWARD): with FUSED_DROPOUT on as well, a module training with
# attention dropout 0 < p < 1 (and none of the other observable-path features) runs it inside the kernels - a counter-based mask from
# a seed (autograd_attention), nothing of size Sq x Sk stored.  Off by default: the fused mask is a different random stream from
# nn.Dropout's, so turning it on changes which probabilities a seeded run drops.
FUSED_DROPOUT = False


def set_fused_dropout(on: bool = True) -> None:
    """Run the modules' attention dropout inside the fused training kernels (True; needs set_fused_backward(True) too) or keep it on the
    torch-op path (False, the default)."""
    global FUSED_DROPOUT
    FUSED_DROPOUT = bool(on)


def fused_train_core(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *, softmax_fn, scale: float = 1.0, scale_div: float = 0.0,
                     attention_mask: Optional[torch.Tensor] = None, clamp_min: bool = False, detect_causal: bool = False,
                     dropout_p: float = 0.0) -> Optional[torch.Tensor]:
    """The differentiable core on the fused training kernels: logical (B,H,Sq,d) context, or None when FUSED_BACKWARD is off or the
    problem is not one the kernels take (the caller then runs unfused_core).  Same score chain as unfused_core: the clamp floor is
    finfo of the scores' dtype; a decoder mask becomes the analytic causal mask plus a key-padding vector.  dropout_p: the attention
    dropout the module applies now (0 in eval); p > 0 needs FUSED_DROPOUT and p < 1, else None."""
    from .autograd_attention import fused_attention, fused_supported

    if not FUSED_BACKWARD or not fused_supported(q, k, v, softmax_fn):
        return None
    dropout_p = float(dropout_p)
    if dropout_p != 0.0 and not (FUSED_DROPOUT and 0.0 < dropout_p < 1.0):
        return None
    B, H, Sq, _ = q.shape
    Sk = k.shape[2]
    pad, full, causal, _ = resolve_mask(attention_mask, B, Sq, Sk, q.dtype, detect_causal)
    # as unfused_core: the floor is finfo.min of the scores' dtype (not the mask's), and there is a clamp only where a mask was added
    return fused_attention(q, k, v, softmax=spec_of(softmax_fn), scale=scale, scale_div=scale_div, key_pad_mask=pad, full_mask=full,
                           causal=causal, clamp_min=clamp_min and attention_mask is not None, mask_min=float(torch.finfo(q.dtype).min),
                           dropout_p=dropout_p)


def _dropout_p(dropout) -> Optional[float]:
    """The probability a module's attention dropout applies NOW (0 in eval) where it is nn.Dropout or a partial of F.dropout, else None."""
    if isinstance(dropout, nn.Dropout):
        return float(dropout.p) if dropout.training else 0.0
    if isinstance(dropout, partial) and dropout.func is nn.functional.dropout and not dropout.args and set(dropout.keywords) <= {"p", "training"}:
        return float(dropout.keywords.get("p", 0.5)) if dropout.keywords.get("training", True) else 0.0
    return None


def unfused_core(
    q, k, v, *, softmax_fn, scale: float = 1.0, scale_div: float = 0.0, attention_mask=None, clamp_min: bool = False,
    scores_tap=None, probs_tap=None, dropout=None, probs_after_tap=None, head_mask=None, extra_scores=None,
    fq_scores=None, fq_probs=None, need_probs: bool = True,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Observable path (output_attentions, forward hooks on the Identity taps, head_mask, training dropout,
    relative position scores, user-supplied softmax callables): the (B,H,Sq,Sk) tensors exist, the two
    contractions are rocBLAS batched GEMMs and the softmax is the HIP row kernel behind SOFTMAX_MAPPING.
    Op order of bert_attention.py:222-292 / opt_attention.py:204-263.
    Returns (context (B,H,Sq,d), probs before dropout/head-mask, probs actually multiplied with V).

    With softmax.FUSED_SOFTMAX_TRAIN on, the span from the scale to the dropout is ONE differentiable HIP kernel (softmax.masked_softmax)
    when there is no score or probability quantiser, no hook on scores_tap and the softmax callable has a spec.  Its own dropout - the
    fused attention kernels' stream, not nn.Dropout's - runs only with FUSED_DROPOUT on as well and no hook on probs_tap; a caller that
    drops `probs` passes need_probs=False and then gets None for it."""
    ops._need_gpu(q, k, v, allow_grad=True)  # GPU only, like the fused path: this package has no CPU implementation; differentiable
    scores = torch.matmul(q, k.transpose(-1, -2))
    if extra_scores is not None:
        scores = scores + extra_scores
    spec = spec_of(softmax_fn) if _softmax.FUSED_SOFTMAX_TRAIN else None
    if spec is not None and fq_scores is None and fq_probs is None and (scores_tap is None or not has_hooks(scores_tap)):
        p = _dropout_p(dropout) if FUSED_DROPOUT and (probs_tap is None or not has_hooks(probs_tap)) else None
        in_kernel = p is not None and 0.0 < p < 1.0
        probs, used = _softmax.masked_softmax(scores, spec, scale=scale, scale_div=scale_div or 0.0, mask=attention_mask,
                                              clamp_min=clamp_min and attention_mask is not None, dropout_p=p if in_kernel else 0.0,
                                              want_probs=need_probs or not in_kernel)
        out_dtype = getattr(softmax_fn, "out_dtype", None)  # (softmax.UpcastSoftmax: the dtype its callable form returns)
        if out_dtype is not None:
            probs = probs if probs is None or probs.dtype == out_dtype else probs.to(out_dtype)
            used = used if used.dtype == out_dtype else used.to(out_dtype)
        if not in_kernel:
            if probs_tap is not None:
                probs = probs_tap(probs)
            used = probs
            if dropout is not None:
                used = dropout(used)
        if probs_after_tap is not None:
            used = probs_after_tap(used)
        if head_mask is not None:
            used = used * head_mask
        return torch.matmul(used, v), probs, used
    if scale_div:
        scores = scores / scale_div
    elif scale != 1.0:
        scores = scores * scale
    if fq_scores is not None:
        scores = fq_scores(scores)
    if scores_tap is not None:
        scores = scores_tap(scores)
    if attention_mask is not None:
        scores = scores + attention_mask
        if clamp_min:
            scores = torch.max(scores, torch.tensor(torch.finfo(scores.dtype).min, device=scores.device))
    probs = softmax_fn(scores, dim=-1)
    if fq_probs is not None:
        probs = fq_probs(probs)
    if probs_tap is not None:
        probs = probs_tap(probs)
    used = probs
    if dropout is not None:
        used = dropout(used)
    if probs_after_tap is not None:
        used = probs_after_tap(used)
    if head_mask is not None:
        used = used * head_mask
    return torch.matmul(used, v), probs, used
