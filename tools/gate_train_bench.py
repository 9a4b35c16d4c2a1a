#!/usr/bin/env python3
"""Forward + backward times of the conditional per-token gate and its product with the context: attention.FUSED_GATE_TRAIN on (ops.gate_apply_fwd
/ ops.gate_apply_bwd behind attention.GateApply) against the switch off (attention.gate_autograd's per-head loop and the torch multiply of
attention.gated_merge - the parent path) in the same process.

    python tools/gate_train_bench.py [--out FILE] [--reps R] [--iters N]

Shapes: BERT B32 S128 H12 d64 with 0 (Linear), 16 (attn_gate_mlp) and 64 (attn_gate_mlp2) hidden units, OPT B16 S512 H12 d64 with 16; fp16 and
fp32.  One step = attention.module_gate + attention.gated_merge on a module that holds only the gate, and torch.autograd.grad of the merged
context for the context, the layer input and every predictor parameter.  Two kinds of number, named for what they are:
  step    (default mode) a plain loop of `iters` steps over a ring of inputs larger than the 256 MB last-level cache between two device events,
          ended by a synchronise, the two settings alternating `reps` times, median [min..max] per step.  The time a training loop sees for
          this part of a step, host included: where the launches are small it is the host's time to enqueue them, not the kernels'.
  kernel  summed kernel time per step from a kernel trace, each (shape, dtype, side) in a process of its own under the tracer:
              rocprofv3 --kernel-trace --stats --output-format csv -d DIR/<case>_<side> -- python tools/gate_train_bench.py --trace-case <case> --side on|off
              python tools/gate_train_bench.py --summarise DIR [--out FILE]     (no GPU: reads the *_kernel_stats.csv files, appends to FILE)
          --trace-case runs `--trace-steps` steps of one side and nothing else; the summary divides every kernel's total by the steps and
          names the fused side's four launches - gate forward, product, backward rows, backward reduce - and the rest (the stacking and
          casting of the per-head parameters, the layout copies of autograd) next to the switch-off side's sum and launch count.
The step is not captured into a graph here: run on the default stream first, a step leaves the predictor parameters' gradient nodes on that
stream, and inside a capture autograd then makes the default stream wait for an event of the capturing one - the case torch's warning about
the nodes' stream names.  The four launches themselves replay from a graph (tests/test_gate_train_gpu.py).
No speed-up is required of either side: the lines are the record, and say so when the fused path is slower."""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outeffhop_amd import _lib, attention as A  # noqa: E402

SHAPES = (("BERT", 32, 128, 12, 64, 0), ("BERT", 32, 128, 12, 64, 16), ("BERT", 32, 128, 12, 64, 64), ("OPT", 16, 512, 12, 64, 16))  # B, T, H, d, units
RING_BYTES = 600_000_000


class GateOnly(A.GateBookkeeping, nn.Module):
    """The gate members of an attention module (attention.init_gate) and nothing else."""

    def __init__(self, H, d, units):
        super().__init__()
        A.init_gate(self, H, d, H * d, A.AttentionGateType.conditional_per_token, 0.25 if units == 0 else None, units == d // 4, units == d, False, False, 0.0)


def loop_us(step, ring, iters):
    for i in range(5):
        step(*ring[i % len(ring)])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        step(*ring[i % len(ring)])
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


CASES = [(dtype,) + shape for dtype in (torch.float16, torch.float32) for shape in SHAPES]
FUSED_KERNELS = (("gate fwd", ("oeh_gate_mfma_kernel", "oeh_gate_logit")), ("product", ("oeh_gate_apply_fwd_kernel",)),
                 ("bwd rows", ("oeh_gate_train_bwd_kernel",)), ("bwd reduce", ("oeh_gate_train_reduce_kernel",)))


def case_name(i):
    dtype, name, B, T, H, d, units = CASES[i]
    return f"{name:4s} B{B} S{T} H{H} d{d} m{units:<2d} {str(dtype).split('.')[-1]:8s}"


def make_step(i, dev, sets):
    dtype, name, B, T, H, d, units = CASES[i]
    torch.manual_seed(1)
    mod = GateOnly(H, d, units).to(dev)
    if dtype != torch.float32:
        mod = mod.to(dtype)
    params = list(mod.alpha.parameters())
    t = lambda *s: torch.randn(*s, device=dev, dtype=dtype)  # noqa: E731  (no cast kernel of the set-up in the trace)
    ring = [(t(B, H, T, d).requires_grad_(), t(B, T, H * d).requires_grad_(), t(B, T, H * d)) for _ in range(sets)]

    def step(ctx, hidden, dout):
        gate, _ = A.module_gate(mod, hidden, H, in_kernel=False)
        merged = A.gated_merge(ctx, gate)
        return torch.autograd.grad(merged, (ctx, hidden, *params), dout)
    return step, ring


def trace_case(i, side, steps):
    """`steps` steps of one side of one case and nothing else on the device but the inputs' set-up: for a run under the kernel tracer."""
    dev = torch.device("cuda", 0)
    step, ring = make_step(i, dev, 4)
    torch.cuda.synchronize()
    A.set_fused_gate_train(side == "on")
    for k in range(steps):
        step(*ring[k % len(ring)])
    torch.cuda.synchronize()
    print(f"traced {steps} steps: {case_name(i)} {side}")
    return 0


def summarise(root, out, steps):
    import csv
    import glob

    lines = [f"# kernel: summed kernel time per step, us (rocprofv3 --kernel-trace --stats, {steps} steps of one side per process; the inputs' set-up kernels"
             " - randn, casts - are left out by name); launches = kernel launches per step",
             "# fused side: gate fwd = oeh_gate_fwd's launch, product = oeh_gate_apply_fwd_kernel, bwd rows = oeh_gate_train_bwd_kernel, bwd reduce ="
             " oeh_gate_train_reduce_kernel, rest = stacking / casting the per-head parameters and autograd's copies"]
    for i in range(len(CASES)):
        tot = {}
        for side in ("on", "off"):
            files = glob.glob(os.path.join(root, f"{i}_{side}", "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                tot[side] = None
                continue
            rows = [r for r in csv.DictReader(open(files[0])) if "distribution" not in r["Name"] and "copyBuffer" not in r["Name"] and "fillBuffer" not in r["Name"]]
            us = lambda rs: sum(float(r["TotalDurationNs"]) for r in rs) / steps / 1e3  # noqa: E731
            parts = {}
            if side == "on":
                for label, keys in FUSED_KERNELS:
                    parts[label] = us([r for r in rows if any(k in r["Name"] for k in keys)])
                parts["rest"] = us(rows) - sum(parts.values())
            tot[side] = (us(rows), sum(int(r["Calls"]) for r in rows) / steps, parts)
        if tot["on"] is None or tot["off"] is None:
            lines.append(f"{case_name(i)} kernel: not measured")
            continue
        (u_on, n_on, parts), (u_off, n_off, _) = tot["on"], tot["off"]
        slower = "  (fused SLOWER)" if u_on > u_off else ""
        lines.append(f"{case_name(i)} kernel: on {u_on:8.2f} us in {n_on:5.1f} launches (" + ", ".join(f"{k} {v:.2f}" for k, v in parts.items()) +
                     f")  off {u_off:8.2f} us in {n_off:5.1f} launches  off / on {u_off / u_on:6.2f}x{slower}")
    print("\n".join(lines))
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--trace-case", type=int, default=None, help="index into the (dtype, shape) list: run only --trace-steps steps of --side")
    ap.add_argument("--side", choices=("on", "off"), default="on")
    ap.add_argument("--trace-steps", type=int, default=50)
    ap.add_argument("--summarise", default=None, help="directory of the tracer's outputs, one <case>_<side> folder each")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.out, a.trace_steps)
    if not torch.cuda.is_available():
        raise SystemExit("gate_train_bench needs a GPU: there is no CPU timing")
    if a.trace_case is not None:
        return trace_case(a.trace_case, a.side, a.trace_steps)
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lines = [f"# gate_train_bench: {lib.oeh_build_info().decode()}",
             f"# one forward + backward of gate + product: a plain loop of {a.iters} steps over a ring of inputs of > {RING_BYTES // 1_000_000} MB between two device "
             f"events, host included; median of {a.reps} alternating runs [min..max] per step; no graph, no tracer",
             "# on: attention.FUSED_GATE_TRAIN (ops.gate_apply_fwd + ops.gate_apply_bwd); off: attention.gate_autograd + the torch multiply, the parent path"]
    for dtype in (torch.float16, torch.float32):
        esize = torch.empty(0, dtype=dtype).element_size()
        for name, B, T, H, d, units in SHAPES:
            torch.manual_seed(1)
            mod = GateOnly(H, d, units).to(dev)  # (a .half() model's predictors are 16-bit too; the kernels take fp32 copies of them)
            if dtype != torch.float32:
                mod = mod.to(dtype)
            params = list(mod.alpha.parameters())
            n = B * T * H * d
            sets = max(2, min(16, -(-RING_BYTES // (3 * n * esize))))
            ring = []
            for _ in range(sets):
                t = lambda *s: torch.randn(*s, device=dev).to(dtype)  # noqa: E731
                ring.append((t(B, H, T, d).requires_grad_(), t(B, T, H * d).requires_grad_(), t(B, T, H * d)))

            def step(ctx, hidden, dout):
                gate, _ = A.module_gate(mod, hidden, H, in_kernel=False)
                merged = A.gated_merge(ctx, gate)
                return torch.autograd.grad(merged, (ctx, hidden, *params), dout)

            for on in (True, False):  # each path once, with its counters
                prev = A.set_fused_gate_train(on)
                n0 = dict(A.GATE_TRAIN_CALLS)
                step(*ring[0])
                took = {k: A.GATE_TRAIN_CALLS[k] - n0[k] for k in n0}
                A.set_fused_gate_train(prev)
                assert took == ({"forward": 1, "backward": 1, "torch": 0} if on else {"forward": 0, "backward": 0, "torch": 1}), took
            t_on, t_off = [], []
            for _ in range(a.reps):
                prev = A.set_fused_gate_train(True)
                t_on.append(loop_us(step, ring, a.iters))
                A.set_fused_gate_train(False)
                t_off.append(loop_us(step, ring, a.iters))
                A.set_fused_gate_train(prev)
            u_on, u_off = statistics.median(t_on), statistics.median(t_off)
            slower = "  (fused SLOWER)" if u_on > u_off else ""
            line = (f"{name:4s} B{B} S{T} H{H} d{d} m{units:<2d} {str(dtype).split('.')[-1]:8s} on {u_on:8.1f} us [{min(t_on):.1f}..{max(t_on):.1f}]  "
                    f"off {u_off:8.1f} us [{min(t_off):.1f}..{max(t_off):.1f}]  off / on {u_off / u_on:6.2f}x{slower}  ({sets} input sets)")
            print(line, flush=True)
            lines.append(line)
            del ring
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
