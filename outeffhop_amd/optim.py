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
CPU fp32 scalar), so a state_dict() loads into torch.optim.AdamW and back.

fp16 mixed precision (the reference's regime, run_clm.py:587-606) is `FusedAdamW(..., amp=True)` with `LossScaler` or torch's GradScaler:

    optimizer = FusedAdamW(grouped_parameters, lr=lr, max_grad_norm=max_grad_norm, amp=True)
    scaler = LossScaler()
    ...
    scaler.scale(loss).backward()
    scaler.step(optimizer)      # norm = overflow check, 1/scale folded into the clip coefficient, the skip decided on the device
    scaler.update()             # one launch

No pass unscales the gradients and nothing waits for the device: include/oeh.h (oeh_grad_norm_amp, oeh_adamw_step_amp,
oeh_loss_scale_update), DESIGN.md section 17.1.  Without amp=True the class takes no part in the fused found-inf protocol: a GradScaler
unscales, synchronises and skips the call as for any optimizer (run_clm.py:603-606)."""
from __future__ import annotations

import math
from typing import Iterable, Optional, Union

import torch

from . import _lib, ops

__all__ = ["FusedAdamW", "LossScaler", "clip_grad_norm_"]


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's arguments (amsgrad must stay False, lr a float) and max_grad_norm: the global 2-norm the gradients are clipped
    to inside the step, without writing them - None: no clipping and no norm.  Parameters and state are fp32 and contiguous; gradients
    fp32, fp16 or bf16; everything on one GPU.  Parameters without a gradient sit a step out, as in torch.  At most `ops.MT_MAX_GROUPS`
    distinct (hyper-parameters, step count) combinations per step.  step() synchronises nothing and cannot be captured into a graph: the
    step number and lr are host values recorded with the launch.

    amp=True is the form for fp16 loss scaling.  The step counters then live in one fp32 device array of the optimizer's, one slot per
    parameter; state[p]["step"] is the 0-dim view of its slot (a step tensor that is not - after load_state_dict, or state made by a plain
    FusedAdamW or by torch - is copied into its slot once, which may wait for the device; the steady loop does not).  Kernel groups are
    the distinct hyper-parameters alone, at most `ops.MT_MAX_GROUPS`.  step() always runs the norm - it is the overflow check - so
    `grad_norm` (of the unscaled gradients) and `clip_coef` (with 1 / scale folded in) are always there, and max_grad_norm=None means a
    coefficient of 1 / scale.  The scale and the flag are `self.grad_scale` and `self.found_inf`, one-element fp32 device tensors, where a
    scaler has set them for the call (torch's protocol for optimizers with `_step_supports_amp_scaling`, which this instance then sets):
    grad_scale None means the gradients are already unscaled; with neither, the scale is 1 and the flag is the norm's own.  On an overflow
    nothing is read or written: parameters, moments and counters stay, and `step_skipped`, a 0-dim float64 view on the device, reads 1.
    A parameter without a gradient sits out, counter included; an empty parameter has no plan record, so its counter is not advanced
    either.  Capture into a graph still raises: lr stays a host value."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, amsgrad: bool = False, *,
                 max_grad_norm: Optional[float] = None, amp: bool = False):
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
        self.amp = bool(amp)
        self.step_skipped: Optional[torch.Tensor] = None  # amp: 0-dim float64 on the device, 1 when the last step() found an overflow
        self._steps, self._slots = None, None  # amp: the device step counters, one slot per parameter in group order, and the plan's slot table
        if self.amp:
            self._step_supports_amp_scaling = True  # (on the instance: a plain FusedAdamW must stay on the scaler's generic path)
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
        self.__dict__.setdefault("amp", False)
        self.__dict__.setdefault("_steps", None)
        self.step_skipped = self._slots = None

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

    def _counters(self, dev) -> torch.Tensor:
        """The device array of step counters, one slot per parameter in group order; grown (device to device) when a group was added."""
        n = sum(len(g["params"]) for g in self.param_groups)
        if self._steps is None or self._steps.numel() < n or self._steps.device != dev:
            new = torch.zeros(n, dtype=torch.float32, device=dev)
            old = self._steps
            if old is not None:
                new[:old.numel()].copy_(old)
                for st in self.state.values():  # the views follow their array
                    t = st.get("step")
                    if t is not None and t.is_cuda and t.untyped_storage().data_ptr() == old.untyped_storage().data_ptr():
                        st["step"] = new[t.storage_offset()]
            self._steps = new
        return self._steps

    def _step_amp(self, loss):
        ps, gs, ms, vs, keys, slots = [], [], [], [], [], []
        slot = -1
        for group in self.param_groups:
            self._check_hyper_group(group)
            b1, b2 = group["betas"]
            hyper = (float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]))
            for p in group["params"]:
                slot += 1
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
                    raise RuntimeError("FusedAdamW.step() cannot be captured into a graph: lr is a host value recorded with the launch")
                if ps and p.device != ps[0].device:
                    raise ValueError(f"FusedAdamW steps parameters on one device, got {ps[0].device} and {p.device}")
                steps = self._counters(p.device) if not ps else self._steps
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = steps[slot]  # (the array starts at zero)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                else:
                    t = st["step"]
                    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 0 and t.data_ptr() == steps.data_ptr() + 4 * slot):
                        steps[slot].copy_(t.detach().reshape(()))  # a loaded or foreign counter: into its slot, once
                        st["step"] = steps[slot]
                ps.append(p)
                gs.append(g)
                ms.append(st["exp_avg"])
                vs.append(st["exp_avg_sq"])
                keys.append(hyper)
                if p.numel():
                    slots.append(slot)
        if not ps:
            return loss
        kernel_groups = {}
        for k in keys:
            kernel_groups.setdefault(k, len(kernel_groups))
        if len(kernel_groups) > ops.MT_MAX_GROUPS:
            raise ValueError(f"FusedAdamW steps at most {ops.MT_MAX_GROUPS} distinct hyper-parameter combinations at once, got {len(kernel_groups)}")
        index = [kernel_groups[k] for k in keys]
        key = (self._steps.data_ptr(), tuple(slots),
               tuple((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), g.dtype, i) for p, g, m, v, i in zip(ps, gs, ms, vs, index)))
        if key != self._plan_key:
            self._plan = ops.mt_plan(ps, gs, ms, vs, index, hold_grads=False, replace=self._plan)
            self._slots = ops.mt_slots(self._plan, slots, replace=self._slots)
            self._plan_key = key
            self.plan_builds += 1
        if self._out4 is None or self._out4.device != ps[0].device:
            self._out4 = torch.empty(4, dtype=torch.float64, device=ps[0].device)
            self.grad_norm, self.clip_coef, self.step_skipped = self._out4[1], self._out4[2], self._out4[3]
        ops.grad_norm_amp(self._plan, self.max_grad_norm, grad_scale=getattr(self, "grad_scale", None), found_inf=getattr(self, "found_inf", None),
                          found_acc=getattr(self, "found_acc", None), out=self._out4)
        ops.adamw_step_amp(self._plan, [ops.AdamWGroup(*k, 0) for k in kernel_groups], self._out4, self._steps, self._slots)
        return loss

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.amp:
            return self._step_amp(loss)
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


class LossScaler:
    """torch.amp.GradScaler's loop for `FusedAdamW(amp=True)` with the state on the device: four fp32 {scale, growth tracker, found, skipped}.

        scaler.scale(loss).backward();  scaler.step(optimizer);  scaler.update()

    scale() multiplies by the device scale.  step() hands the optimizer the scale and the `found` accumulator and calls optimizer.step():
    the norm kernel is the overflow check, the unscale is folded into the step's coefficient, a step that found an overflow returns
    before it reads anything.  update() is one launch of torch's _amp_update_scale_ rule (include/oeh.h: oeh_loss_scale_update).  None of
    the three waits for the device; `get_scale()` and `steps_skipped()` do.  Several optimizers may share one scaler: each skips on its
    own gradients, update() sees the OR of their flags.  state_dict() has GradScaler's keys, so a checkpoint moves both ways.  An lr
    schedule that holds still on skipped steps (run_clm.py:603-606) is the loop's: `steps_skipped()` says by how much to correct it."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000, enabled: bool = True):
        if not (growth_factor > 0.0 and math.isfinite(growth_factor)) or not (backoff_factor > 0.0 and math.isfinite(backoff_factor)):
            raise ValueError("growth_factor and backoff_factor must be positive and finite")
        if int(growth_interval) < 1:
            raise ValueError("growth_interval must be at least 1")
        self._enabled = bool(enabled)
        self._growth_factor, self._backoff_factor, self._growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._init = (float(init_scale), 0.0, 0.0, 0.0)  # until the first call names the device
        self._state: Optional[torch.Tensor] = None

    def is_enabled(self) -> bool:
        return self._enabled

    def _on(self, dev) -> torch.Tensor:
        if not torch.device(dev).type == "cuda":
            raise _lib.OehError("outeffhop_amd ops need GPU tensors: the HIP library is the only implementation")
        if self._state is None:
            # (from pinned memory, in stream order: the first call waits for nothing either)
            self._state = torch.tensor(self._init, dtype=torch.float32).pin_memory().to(dev, non_blocking=True)
        elif self._state.device != torch.device(dev):
            raise ValueError(f"this LossScaler lives on {self._state.device}, got a tensor on {dev}")
        return self._state

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        """loss times the device scale (differentiable); the loss itself when not enabled."""
        if not self._enabled:
            return loss
        return loss * self._on(loss.device)[0]

    def step(self, optimizer, *args, **kwargs):
        """optimizer.step() with the scale and the found accumulator handed over; the optimizer skips on the device when its gradients
        overflowed.  Only a FusedAdamW(amp=True) can do that: anything else raises TypeError."""
        if not (isinstance(optimizer, FusedAdamW) and optimizer.amp):
            raise TypeError("LossScaler steps a FusedAdamW(amp=True); use torch.amp.GradScaler for other optimizers")
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        dev = next((p.device for g in optimizer.param_groups for p in g["params"] if p.grad is not None), None)
        if dev is None:
            return optimizer.step(*args, **kwargs)
        st = self._on(dev)
        optimizer.grad_scale, optimizer.found_inf, optimizer.found_acc = st[0:1], None, st[2:3]
        try:
            return optimizer.step(*args, **kwargs)
        finally:
            del optimizer.grad_scale, optimizer.found_inf, optimizer.found_acc

    def update(self) -> None:
        """Back off after a step that found an overflow, grow after growth_interval clean ones, clear the flag: one launch."""
        if self._enabled and self._state is not None:
            ops.loss_scale_update(self._state, self._growth_factor, self._backoff_factor, self._growth_interval)

    def _read(self):
        return self._init if self._state is None else tuple(self._state.tolist())

    def get_scale(self) -> float:
        """The scale as a float.  Synchronises."""
        return float(self._read()[0]) if self._enabled else 1.0

    def steps_skipped(self) -> int:
        """How many steps update() has seen skipped since the scaler was made.  Synchronises."""
        return int(self._read()[3])

    def get_growth_factor(self) -> float:
        return self._growth_factor

    def get_backoff_factor(self) -> float:
        return self._backoff_factor

    def get_growth_interval(self) -> int:
        return self._growth_interval

    def state_dict(self) -> dict:
        """torch.amp.GradScaler's five entries ({} when not enabled).  Synchronises."""
        if not self._enabled:
            return {}
        scale, tracker, _, _ = self._read()
        return {"scale": float(scale), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": int(tracker)}

    def load_state_dict(self, state_dict: dict) -> None:
        """Take a state_dict() of this class or of torch.amp.GradScaler.  The skip count is not part of it and stays."""
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        vals = (float(state_dict["scale"]), float(state_dict["_growth_tracker"]))
        if self._state is None:
            self._init = vals + self._init[2:]
        else:
            self._state[:2].copy_(torch.tensor(vals, dtype=torch.float32))


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
