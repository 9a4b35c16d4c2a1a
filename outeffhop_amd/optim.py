"""The optimizer phase of a training step on the HIP kernels: `FusedAdamW`, a torch.optim.Optimizer whose step() is one launch over all
parameters (two more with gradient clipping folded in), and `clip_grad_norm_`, the drop-in for torch.nn.utils.clip_grad_norm_ /
accelerator.clip_grad_norm_ for callers who keep their own optimizer.

The reference's loops build torch.optim.AdamW over a decay and a no-decay group (run_clm.py:440-462), clip the global gradient norm and step
(run_clm.py:589-601).  Here

    optimizer = FusedAdamW(grouped_parameters, lr=lr, betas=(0.9, 0.95), max_grad_norm=max_grad_norm)
    ...
    optimizer.step()            # norm, clip and update; optimizer.grad_norm is the norm, on the device

The update is include/oeh.h's (oeh_adamw_step): fp32, every operation rounded on its own; DESIGN.md section 17 bounds it against float64.
It is not bit-equal to torch.optim.AdamW, whose lerp and addcmul contract.  State has torch's key names (step, exp_avg, exp_avg_sq; step a
CPU fp32 scalar), so a state_dict() loads into torch.optim.AdamW and back.  Under a GradScaler the class takes no part in the fused
found-inf protocol: the scaler unscales, synchronises and skips the call as for any optimizer (run_clm.py:603-606)."""
from __future__ import annotations

import math
from typing import Iterable, Optional, Union

import torch

from . import _lib, ops

__all__ = ["FusedAdamW", "clip_grad_norm_"]


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's arguments (amsgrad must stay False, lr a float) and max_grad_norm: the global 2-norm the gradients are clipped
    to inside the step, without writing them - None: no clipping and no norm.  Parameters and state are fp32 and contiguous; gradients
    fp32, fp16 or bf16; everything on one GPU.  Parameters without a gradient sit a step out, as in torch.  At most `ops.MT_MAX_GROUPS`
    distinct (hyper-parameters, step count) combinations per step.  step() synchronises nothing and cannot be captured into a graph: the
    step number and lr are host values recorded with the launch."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, amsgrad: bool = False, *,
                 max_grad_norm: Optional[float] = None):
        if amsgrad:
            raise ValueError("FusedAdamW has no amsgrad form")
        _check_hyper(lr, betas, eps, weight_decay)
        if max_grad_norm is not None and (isinstance(max_grad_norm, torch.Tensor) or math.isnan(float(max_grad_norm))):
            raise ValueError("max_grad_norm must be a number or None")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        # 0-dim float64 on the device: the norm of the last step's gradients before clipping, and what they were scaled by.  Both are views
        # of one buffer that the next step() writes again: .clone() what is to be kept.
        self.grad_norm: Optional[torch.Tensor] = None
        self.clip_coef: Optional[torch.Tensor] = None
        self._out4 = None
        self._plan, self._plan_key = None, None
        self.plan_builds = 0  # how often step() had to plan anew: once, then only when a tensor has moved
        # (the keys torch.optim.AdamW keeps in a group, with its defaults: a state_dict travels both ways)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None, capturable=False,
                        differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        for group in self.param_groups:
            self._check_group(group)

    def __setstate__(self, state) -> None:
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", None)
        self.grad_norm = self.clip_coef = self._plan = self._plan_key = self._out4 = None
        self.__dict__.setdefault("plan_builds", 0)

    @staticmethod
    def _check_hyper_group(group) -> None:
        if group.get("amsgrad") or group.get("maximize") or group.get("capturable") or group.get("differentiable"):
            raise ValueError("FusedAdamW has no amsgrad, maximize, capturable or differentiable form")
        _check_hyper(group["lr"], group["betas"], group["eps"], group["weight_decay"])

    @classmethod
    def _check_group(cls, group) -> None:
        cls._check_hyper_group(group)
        for p in group["params"]:
            if p.dtype != torch.float32:
                raise TypeError(f"FusedAdamW steps fp32 parameters, got {p.dtype}")
            if p.is_sparse or not p.is_contiguous():
                raise ValueError("FusedAdamW needs dense contiguous parameters")

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])
        self._plan_key = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ps, gs, ms, vs, keys = [], [], [], [], []
        for group in self.param_groups:
            self._check_hyper_group(group)  # (a scheduler or the caller may have written into the group since)
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse:
                    raise ValueError("FusedAdamW does not take sparse gradients")
                if not g.is_contiguous():
                    raise ValueError("FusedAdamW needs contiguous gradients")
                if g.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                    raise TypeError(f"FusedAdamW takes fp32, fp16 or bf16 gradients, got {g.dtype}")
                if not p.is_cuda:
                    raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
                if not ps and torch.cuda.is_current_stream_capturing():  # (seen before any state is made)
                    raise RuntimeError("FusedAdamW.step() cannot be captured into a graph: the step number and lr are host values recorded with the launch")
                if ps and p.device != ps[0].device:
                    raise ValueError(f"FusedAdamW steps parameters on one device, got {ps[0].device} and {p.device}")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif st["step"].is_cuda:  # (a state loaded from a capturable or fused torch optimizer: brought to the host once)
                    st["step"] = st["step"].detach().to("cpu", torch.float32)
                ps.append(p)
                gs.append(g)
                ms.append(st["exp_avg"])
                vs.append(st["exp_avg_sq"])
                keys.append((float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), int(st["step"].item()) + 1))
        if not ps:
            return loss
        kernel_groups = {}
        for k in keys:
            kernel_groups.setdefault(k, len(kernel_groups))
        if len(kernel_groups) > ops.MT_MAX_GROUPS:
            raise ValueError(f"FusedAdamW steps at most {ops.MT_MAX_GROUPS} distinct (hyper-parameters, step count) combinations at once, got {len(kernel_groups)}")
        index = [kernel_groups[k] for k in keys]
        key = tuple((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), g.dtype, i) for p, g, m, v, i in zip(ps, gs, ms, vs, index))
        # The cached plan does not own the gradients: zero_grad(set_to_none=True) must free them, and the next backward then usually gets
        # the same addresses back from the caching allocator - the key is equal and nothing is planned.  Every address is compared here
        # before the table is used again, so a stale table is never launched.
        if key != self._plan_key:
            self._plan = ops.mt_plan(ps, gs, ms, vs, index, hold_grads=False, replace=self._plan)
            self._plan_key = key
            self.plan_builds += 1
        descs = [ops.AdamWGroup(*k) for k in kernel_groups]
        if self.max_grad_norm is not None:
            # (one buffer for every step's norm: a steady loop's step() allocates nothing on the device)
            if self._out4 is None or self._out4.device != ps[0].device:
                self._out4 = torch.empty(4, dtype=torch.float64, device=ps[0].device)
                self.grad_norm, self.clip_coef = self._out4[1], self._out4[2]
            ops.grad_norm(self._plan, self.max_grad_norm, out=self._out4)
            ops.adamw_step(self._plan, descs, clip=self._out4)
        else:
            ops.adamw_step(self._plan, descs)
        for p in ps:
            self.state[p]["step"] += 1
        return loss


def _check_hyper(lr, betas, eps, weight_decay) -> None:
    if isinstance(lr, torch.Tensor):
        raise TypeError("FusedAdamW takes lr as a float: a tensor lr is for capturable steps, which are not here")
    if not lr >= 0.0:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not eps >= 0.0:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if len(betas) != 2 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
        raise ValueError(f"Invalid beta parameters: {betas}")
    if not weight_decay >= 0.0:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")


def clip_grad_norm_(parameters: Union[torch.Tensor, Iterable[torch.Tensor]], max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False,
                    foreach: Optional[bool] = None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ on the HIP kernels: the global 2-norm of the parameters' gradients in one pass (exact squares summed in
    float64, a fixed order) and one in-place pass that scales them by min(1, max_norm / (norm + 1e-6)).  Returns the norm before clipping, a
    0-dim float64 tensor on the device; nothing synchronises.  Another norm_type, CPU gradients, gradients that are not dense contiguous
    fp32 / fp16 / bf16 tensors on one GPU, a max_norm that is not positive, and error_if_nonfinite go to torch's function."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    # (max_norm <= 0: torch scales by a coefficient that is not positive, the kernels' rule is "no clipping")
    ours = float(norm_type) == 2.0 and not error_if_nonfinite and len(grads) > 0 and float(max_norm) > 0.0
    ours = ours and all(g.is_cuda and g.device == grads[0].device and not g.is_sparse and g.is_contiguous()
                        and g.dtype in (torch.float32, torch.float16, torch.bfloat16) for g in grads)
    if not ours:
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type, error_if_nonfinite, foreach)
    with torch.no_grad():
        plan = ops.mt_plan(None, grads)
        out4 = ops.grad_norm(plan, float(max_norm))
        ops.grad_scale_(plan, out4)
    return out4[1]
