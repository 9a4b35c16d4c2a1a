#!/usr/bin/env python3
"""Device time of the optimizer phase - global-norm clip + AdamW step over a whole model's parameters - fused against torch's two forms.

    python tools/adamw_bench.py [--out FILE] [--reps R] [--iters N] [--amp]

Parameter sets: the shape lists of BERT-base with its MLM head (BertForMaskedLM, decoder weight tied) and of OPT-125m (OPTForCausalLM, lm_head
tied), written out below - no model import.  fp32 parameters, gradients and moments; two groups as run_clm.py:443-458 splits them (matrices
with weight decay, biases and LayerNorm weights without); max_grad_norm 1.
Three candidates, each one step = clip + update:
  fused    ops.grad_norm + ops.adamw_step(clip=...)                     (3 launches; the gradients are not written)
  foreach  torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW's default update (its foreach form: what a user of the parent commit runs)
  tfused   torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(fused=True)'s update
torch's updates are called through torch.optim.adamw.adamw (imported by name), the function AdamW.step() itself calls per group - step() refuses graph capture
unless capturable=True, which would time a different kernel chain.
  device   graph replays timed by device events, as tools/ln_train_bench.py: `iters` steps per graph over `SETS` parameter sets in turn (one
           set alone is 16 bytes per parameter: 1.8 GB, seven times the last-level cache), the candidates' graphs replayed alternately `reps`
           times, median [min..max] per step.  A candidate that cannot be captured is timed as a plain loop between device events and marked.
  GB/s     32 bytes per parameter - g read for the norm; g, p, m, v read and p, m, v written - over the device time.  A whole-step rate
           from device events, not a kernel's share of peak from a trace.
  host     FusedAdamW.step() in a plain loop of 20 steps between two device events, host included, and torch.optim.AdamW's two forms behind
           clip_grad_norm_ the same way - twice: with the gradient tensors kept from step to step, and as the reference's loop runs it, with
           zero_grad() (set_to_none=True) and a stand-in backward that makes every gradient tensor anew (a clone per tensor: its own cost is
           the line "nothing").  The second says how many plans FusedAdamW built: none while the allocator hands the addresses back.
No ratio is promised: the three numbers are printed as measured.

--amp: the same phase under fp16 loss scaling (a GradScaler loop, run_clm.py:587-606), the same method, fp32 and fp16 gradients.  One step =
overflow check + unscale + clip + update (+ the scale's update where the candidate has one on the device):
  amp      ops.grad_norm_amp + ops.adamw_step_amp + ops.loss_scale_update       (5 launches; no pass over the gradients beside the norm's)
  plain    ops.grad_norm + ops.adamw_step: `fused` above, no loss scaling at all - the floor, measured in the same run
  parent   torch._amp_foreach_non_finite_check_and_unscale_ over the gradients, then `plain`: the device work of GradScaler + FusedAdamW()
  torch    the unscale, clip_grad_norm_, then torch's adamw(fused=True, grad_scale=..., found_inf=...)   (fp32 gradients only: it wants one dtype)
The unscale multiplies by 1.0 here, so that replay after replay finds the same gradients.  The host lines compare GradScaler + FusedAdamW()
with LossScaler + FusedAdamW(amp=True) in the loop with zero_grad() and the stand-in backward; the first reads found_inf back every step."""
import argparse
import os
import statistics
import sys

import torch
from torch.optim.adamw import adamw as torch_adamw  # (the function AdamW.step() calls per group)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import outeffhop_amd as oa  # noqa: E402
from outeffhop_amd import _lib, ops  # noqa: E402

SETS = 2
LR, BETAS, EPS, WD, MAX_NORM = 5e-5, (0.9, 0.95), 1e-8, 0.01, 1.0


def _encoder_layer(h, ffn):
    """q, k, v, out projections, a LayerNorm, the two feed-forward matrices, a LayerNorm"""
    return [(h, h), (h,)] * 4 + [(h,), (h,)] + [(ffn, h), (ffn,), (h, ffn), (h,)] + [(h,), (h,)]


def bert_base_mlm():
    h, ffn, vocab = 768, 3072, 30522
    shapes = [(vocab, h), (512, h), (2, h), (h,), (h,)]           # word, position, token-type embeddings, their LayerNorm
    for _ in range(12):
        shapes += _encoder_layer(h, ffn)
    return shapes + [(h, h), (h,), (h,), (h,), (vocab,)]          # MLM head: transform dense, LayerNorm, the decoder's bias (its weight is tied)


def opt_125m():
    h, ffn, vocab = 768, 3072, 50272
    shapes = [(vocab, h), (2050, h)]                              # token and learned position embeddings
    for _ in range(12):
        shapes += _encoder_layer(h, ffn)
    return shapes + [(h,), (h,)]                                  # final LayerNorm (lm_head is tied)


MODELS = (("BERT-base+MLM", bert_base_mlm), ("OPT-125m", opt_125m))


class ParamSet:
    def __init__(self, shapes, dev, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        self.params = [torch.nn.Parameter(0.02 * torch.randn(s, device=dev, generator=g)) for s in shapes]
        for p in self.params:
            p.grad = 0.01 * torch.randn(p.shape, device=dev, generator=g)
        self.m = [0.001 * torch.randn(p.shape, device=dev, generator=g) for p in self.params]
        self.v = [1e-4 * torch.rand(p.shape, device=dev, generator=g) + 1e-8 for p in self.params]
        self.group = [0 if p.dim() > 1 else 1 for p in self.params]
        self.steps_cpu = [torch.tensor(10.0) for _ in self.params]
        self.steps_dev = [torch.tensor(10.0, device=dev) for _ in self.params]
        self.plan = ops.mt_plan(self.params, [p.grad for p in self.params], self.m, self.v, self.group)
        self.numel = sum(p.numel() for p in self.params)

    def fused(self):
        out4 = ops.grad_norm(self.plan, MAX_NORM)
        ops.adamw_step(self.plan, [ops.AdamWGroup(LR, *BETAS, EPS, WD, 11), ops.AdamWGroup(LR, *BETAS, EPS, 0.0, 11)], clip=out4)

    def _torch(self, fused):
        torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
        for grp, wd in ((0, WD), (1, 0.0)):
            idx = [i for i, gi in enumerate(self.group) if gi == grp]
            steps = self.steps_dev if fused else self.steps_cpu
            torch_adamw([self.params[i] for i in idx], [self.params[i].grad for i in idx], [self.m[i] for i in idx], [self.v[i] for i in idx], [],
                        [steps[i] for i in idx], foreach=None if fused else True, fused=True if fused else None, capturable=False,
                        differentiable=False, amsgrad=False, beta1=BETAS[0], beta2=BETAS[1], lr=LR, weight_decay=wd, eps=EPS, maximize=False)

    def foreach(self):
        with torch.no_grad():
            self._torch(False)

    def tfused(self):
        with torch.no_grad():
            self._torch(True)


class AmpSet(ParamSet):
    """A parameter set whose gradients carry a loss scale, in `gdtype`; the gradients are `grads` (a 16-bit one cannot be a fp32 parameter's .grad)"""

    def __init__(self, shapes, dev, seed, gdtype):
        super().__init__(shapes, dev, seed)
        self.grads = [p.grad.to(gdtype) for p in self.params]
        if gdtype != torch.float32:
            for p in self.params:
                p.grad = None
            self.plan = ops.mt_plan(self.params, self.grads, self.m, self.v, self.group)
        n = len(self.params)
        self.counters = torch.full((n,), 10.0, device=dev)
        self.slots = ops.mt_slots(self.plan, range(n))
        self.state = torch.tensor([65536.0, 0.0, 0.0, 0.0], device=dev)  # the scaler: scale, tracker, found, skipped
        self.inv_scale, self.found = torch.ones((), device=dev), torch.zeros((), device=dev)  # (0-dim, as GradScaler's own)
        self.hyper = [ops.AdamWGroup(LR, *BETAS, EPS, WD, 11), ops.AdamWGroup(LR, *BETAS, EPS, 0.0, 11)]

    def amp(self):
        out4 = ops.grad_norm_amp(self.plan, MAX_NORM, grad_scale=self.state[0:1], found_acc=self.state[2:3])
        ops.adamw_step_amp(self.plan, self.hyper, out4, self.counters, self.slots)
        ops.loss_scale_update(self.state, 2.0, 0.5, 2000)

    def plain(self):
        ops.adamw_step(self.plan, self.hyper, clip=ops.grad_norm(self.plan, MAX_NORM))

    def parent(self):
        torch._amp_foreach_non_finite_check_and_unscale_(self.grads, self.found, self.inv_scale)
        self.plain()

    def torch_fused(self):
        with torch.no_grad():
            torch._amp_foreach_non_finite_check_and_unscale_(self.grads, self.found, self.inv_scale)
            torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
            for grp, wd in ((0, WD), (1, 0.0)):
                idx = [i for i, gi in enumerate(self.group) if gi == grp]
                torch_adamw([self.params[i] for i in idx], [self.grads[i] for i in idx], [self.m[i] for i in idx], [self.v[i] for i in idx], [],
                            [self.steps_dev[i] for i in idx], foreach=None, fused=True, capturable=False, differentiable=False, amsgrad=False,
                            beta1=BETAS[0], beta2=BETAS[1], lr=LR, weight_decay=wd, eps=EPS, maximize=False, grad_scale=self.inv_scale, found_inf=self.found)


def replay_ms(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


class Loop:
    """The stand-in for a graph where a candidate cannot be captured: the same steps in a plain loop"""

    def __init__(self, steps):
        self.steps = steps

    def replay(self):
        for s in self.steps:
            s()


def timed_graph(steps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s in steps[:SETS]:
            s()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for s in steps:
                s()
        return g, ""
    except (RuntimeError, AssertionError) as e:
        torch.cuda.synchronize()
        return Loop(steps), f" (plain loop, not a graph: {str(e).splitlines()[0][:100]})"


def loop_us(step, iters):
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main_amp(a, lib, dev):
    lines = [f"# adamw_bench --amp: {lib.oeh_build_info().decode()}",
             f"# one step = overflow check + unscale + global-norm clip + AdamW update over every parameter.  device: event times of graph replays ({a.iters} steps per"
             f" graph over {SETS} parameter sets in turn), median of {a.reps} alternating replays [min..max]; host: a plain loop, host included; no tracer",
             "# amp: ops.grad_norm_amp + ops.adamw_step_amp + ops.loss_scale_update; plain: ops.grad_norm + ops.adamw_step (no loss scaling);"
             " parent: torch's non-finite check and unscale, then plain; torch: unscale + clip_grad_norm_ + adamw(fused=True, grad_scale, found_inf)"]
    for name, shapes_of in MODELS:
        shapes = shapes_of()
        for gdtype in (torch.float32, torch.float16):
            sets = [AmpSet(shapes, dev, 100 + i, gdtype) for i in range(SETS)]
            n = sets[0].numel
            cands = ("amp", "plain", "parent") + (("torch",) if gdtype == torch.float32 else ())
            graphs, notes = {}, {}
            for cand in cands:
                graphs[cand], notes[cand] = timed_graph([getattr(sets[i % SETS], "torch_fused" if cand == "torch" else cand) for i in range(a.iters)])
            times = {c: [] for c in graphs}
            for _ in range(a.reps):
                for c, g in graphs.items():
                    times[c].append(replay_ms(g) * 1e3 / a.iters)
            del graphs
            med = {c: statistics.median(t) for c, t in times.items()}
            gb = 4 if gdtype == torch.float32 else 2
            first = len(lines)
            lines.append(f"{name}, {str(gdtype).split('.')[-1]} gradients: {len(shapes)} tensors, {n / 1e6:.1f} M parameters; amp and plain move {24 + 2 * gb} B/parameter,"
                         f" parent {24 + 4 * gb}")
            for c in cands:
                lines.append(f"  device {c:8s} {med[c]:9.1f} us [{min(times[c]):.1f}..{max(times[c]):.1f}]  amp / this {med['amp'] / med[c]:5.3f}{notes[c]}")
            if gdtype == torch.float32:
                # the loop a user runs, host included: zero_grad(), a stand-in backward that makes every gradient anew (scaled), step, update
                s0 = sets[0]
                src = [g * 65536.0 for g in s0.grads]
                groups = lambda: [{"params": [p for p, g in zip(s0.params, s0.group) if g == 0], "weight_decay": WD},  # noqa: E731
                                  {"params": [p for p, g in zip(s0.params, s0.group) if g == 1], "weight_decay": 0.0}]

                def looped(o, scaler):
                    def go():
                        o.zero_grad()
                        for p, g in zip(s0.params, src):
                            p.grad = g.clone()
                        scaler.step(o)
                        scaler.update()
                    return go

                ts = torch.amp.GradScaler("cuda")
                ts.scale(torch.zeros((), device=dev))
                for label, o, sc in (("GradScaler + FusedAdamW(max_grad_norm)", oa.FusedAdamW(groups(), lr=LR, betas=BETAS, eps=EPS, max_grad_norm=MAX_NORM), ts),
                                     ("LossScaler + FusedAdamW(max_grad_norm, amp=True)",
                                      oa.FusedAdamW(groups(), lr=LR, betas=BETAS, eps=EPS, max_grad_norm=MAX_NORM, amp=True), oa.LossScaler())):
                    us = statistics.median(loop_us(looped(o, sc), 20) for _ in range(3))
                    lines.append(f"  host   {label:50s} {us:9.1f} us per step with zero_grad() and new gradient tensors; {o.plan_builds} plans built,"
                                 f" {int(sc.steps_skipped()) if hasattr(sc, 'steps_skipped') else 0} steps skipped")
                    del o
                del src, s0
            for ln in lines[first:]:
                print(ln, flush=True)
            del sets
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--amp", action="store_true", help="the phase under fp16 loss scaling: amp, plain, parent and torch")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw_bench needs a GPU: there is no CPU timing")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    if a.amp:
        return main_amp(a, lib, dev)
    lines = [f"# adamw_bench: {lib.oeh_build_info().decode()}",
             f"# one step = global-norm clip + AdamW update over every parameter, fp32 gradients.  device: event times of graph replays ({a.iters} steps per graph over"
             f" {SETS} parameter sets in turn), median of {a.reps} alternating replays [min..max]; host: a plain loop of optimizer.step(), host included; no tracer",
             "# fused: ops.grad_norm + ops.adamw_step; foreach: torch clip_grad_norm_ + torch.optim.AdamW's default update; tfused: the same with fused=True"]
    for name, shapes_of in MODELS:
        shapes = shapes_of()
        sets = [ParamSet(shapes, dev, 100 + i) for i in range(SETS)]
        n = sets[0].numel
        graphs, notes = {}, {}
        for cand in ("fused", "foreach", "tfused"):
            graphs[cand], notes[cand] = timed_graph([getattr(sets[i % SETS], cand) for i in range(a.iters)])
        times = {c: [] for c in graphs}
        for _ in range(a.reps):
            for c, g in graphs.items():
                times[c].append(replay_ms(g) * 1e3 / a.iters)
        del graphs
        med = {c: statistics.median(t) for c, t in times.items()}
        lines.append(f"{name}: {len(shapes)} tensors, {n / 1e6:.1f} M parameters, {32 * n / 1e9:.2f} GB at 32 B/parameter")
        for c in ("fused", "foreach", "tfused"):
            lines.append(f"  device {c:8s} {med[c]:9.1f} us [{min(times[c]):.1f}..{max(times[c]):.1f}]  {32 * n / (med[c] * 1e-6) / 1e9:7.1f} GB/s on 32 B/param"
                         f"  foreach / this {med['foreach'] / med[c]:5.2f}x{notes[c]}")
        # what a training loop sees: the optimizers' own step() in a plain loop - with the gradient tensors kept from step to step, and as the
        # reference's loop runs it: zero_grad() (set_to_none=True) and a stand-in backward that makes every gradient tensor anew
        s0 = sets[0]
        src = [p.grad.clone() for p in s0.params]
        groups = lambda: [{"params": [p for p, g in zip(s0.params, s0.group) if g == 0], "weight_decay": WD},  # noqa: E731
                          {"params": [p for p, g in zip(s0.params, s0.group) if g == 1], "weight_decay": 0.0}]

        def looped(o, step):
            def go():
                o.zero_grad()
                for p, g in zip(s0.params, src):
                    p.grad = g.clone()
                step()
            return go

        host = []
        opt = oa.FusedAdamW(groups(), lr=LR, betas=BETAS, eps=EPS, max_grad_norm=MAX_NORM)
        kept = statistics.median(loop_us(opt.step, 20) for _ in range(3))
        builds = opt.plan_builds
        host.append(("FusedAdamW(max_grad_norm).step()", kept, statistics.median(loop_us(looped(opt, opt.step), 20) for _ in range(3)),
                     f"; {opt.plan_builds - builds} plans built in the {3 * 23} steps with new gradient tensors"))
        host.insert(0, ("nothing (zero_grad + the stand-in backward alone)", 0.0, statistics.median(loop_us(looped(opt, lambda: None), 20) for _ in range(3)), ""))
        for label, kw in (("clip_grad_norm_ + AdamW().step()", {}), ("clip_grad_norm_ + AdamW(fused=True).step()", {"fused": True})):
            topt = torch.optim.AdamW(groups(), lr=LR, betas=BETAS, eps=EPS, **kw)

            def tstep():
                torch.nn.utils.clip_grad_norm_(s0.params, MAX_NORM)
                topt.step()
            host.append((label, statistics.median(loop_us(tstep, 20) for _ in range(3)), statistics.median(loop_us(looped(topt, tstep), 20) for _ in range(3)), ""))
            del topt
        for label, us, us_new, note in host:
            lines.append(f"  host   {label:50s} {us:9.1f} us per step, gradients kept | {us_new:9.1f} us with zero_grad() and new gradient tensors{note}")
        del src
        for ln in lines[-(4 + len(host)):]:
            print(ln, flush=True)
        del sets, s0, opt
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
