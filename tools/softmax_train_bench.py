#!/usr/bin/env python3
"""Forward + backward of the span between the two products of the unfused attention path - scale, mask, clamp, softmax, clip, dropout -
on the differentiable HIP row softmax (softmax.masked_softmax: oeh_softmax_train_fwd / oeh_softmax_train_bwd) against the torch-op chain.

    python tools/softmax_train_bench.py [--out FILE] [--reps R] [--iters N]

Shapes: OPT-125m B16 H12 S512 with the (B,1,S,S) causal mask and the clamp; BERT-base B32 H12 S128 with the (B,1,1,S) mask, / sqrt(64) and
dropout 0.1 (fused arm: the kernel's own dropout, probs not written; chain arm: F.dropout); a STanHop shape, 32 * 7 * 4 * 24 rows of 24
segments, fp32.  Softmax: softmax1, vanilla, clippedsoftmax1(-.025:1); fp16 and fp32 scores (masks in the scores' dtype).
Arms: fused = softmax.masked_softmax; chain = attention.unfused_core's ops as the parent commit runs them (the fp16 OPT module upcasts
around its softmax) with softmax.softmax_autograd.  Both arms: torch.autograd.grad of the tensor that meets V with respect to the scores;
the two matmuls are not in the measurement.
Method: one process, the arms alternating, after a warm-up; median [min..max] of `reps` repetitions, per step.  Two measurements:
  device  graph replays timed by device events, as tools/ln_train_bench.py: `iters` steps per graph, the two graphs replayed alternately;
          fused = ops.softmax_train_fwd + ops.softmax_train_bwd (the calls behind masked_softmax: its dropout is refused under capture
          because the seed is a host value), chain = the torch ops and torch.autograd.grad through them.
  step    what a training loop sees, host included: `iters` steps of masked_softmax / the chain and torch.autograd.grad in a plain loop
          between two device events.
peak: torch.cuda.max_memory_allocated over one step above what was allocated before it
(scores, mask and the incoming gradient are allocated before).  bytes: what the fused calls have to move - forward x (+ mask) read, y or u
written; backward x, dy or du (+ mask) read, dx written - over the fused DEVICE time, against 8 TB/s.  A whole-call rate from device events, not a
kernel's share of peak from a trace.  No tracer."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outeffhop_amd import _lib, ops  # noqa: E402
from outeffhop_amd import softmax as S  # noqa: E402

PEAK_BW = 8.0e12
SOFTMAXES = ("softmax1", "vanilla", "clippedsoftmax1(-.025:1)")


def shapes(dtype, dev):
    fmin = torch.finfo(dtype).min
    causal = torch.triu(torch.full((512, 512), fmin, device=dev, dtype=dtype), 1)[None, None].expand(16, 1, 512, 512).contiguous()
    pad = torch.zeros(32, 1, 1, 128, device=dev, dtype=dtype)
    pad[::2, ..., 100:] = fmin
    yield "OPT B16 H12 S512 causal+clamp", (16, 12, 512, 512), dict(mask=causal, clamp_min=True), dtype == torch.float16
    yield "BERT B32 H12 S128 pad p0.1", (32, 12, 128, 128), dict(mask=pad, scale_div=8.0, dropout_p=0.1), False
    if dtype == torch.float32:
        yield "STanHop 21504 x 24", (32 * 7, 4, 24, 24), dict(scale=1.0 / 8.0), False


def chain(scores, spec, upcast, scale=1.0, scale_div=0.0, mask=None, clamp_min=False, dropout_p=0.0, floor=None):
    s = scores
    if scale_div:
        s = s / scale_div
    elif scale != 1.0:
        s = s * scale
    if mask is not None:
        s = s + mask
        if clamp_min:
            s = torch.max(s, floor)  # (the parent builds this scalar tensor per call: a host-to-device copy, which a capture does not take)
    probs = S.softmax_autograd(s.float(), spec, -1).to(s.dtype) if upcast else S.softmax_autograd(s, spec, -1)
    return F.dropout(probs, dropout_p, True) if dropout_p > 0.0 else probs


def replay_ms(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed_graph(step, iters):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream, as graph capture of a backward asks
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            step()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_train_bench needs a GPU: there is no CPU timing")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lines = [f"# softmax_train_bench: {lib.oeh_build_info().decode()}",
             f"# one forward + backward of the span.  device: event times of graph replays ({a.iters} steps per graph), step: a plain loop of {a.iters} steps, host"
             f" included; arms alternating, median of {a.reps} repetitions [min..max] per step; peak: allocated above the inputs over one step; bytes: the fused"
             " calls' algorithmic traffic over the fused device time, of 8 TB/s; no tracer",
             "# fused: softmax.masked_softmax (oeh_softmax_train_fwd + oeh_softmax_train_bwd); chain: the parent commit's torch ops (unfused_core + softmax_autograd + F.dropout)"]
    for dtype in (torch.float16, torch.float32):
        esize = torch.empty(0, dtype=dtype).element_size()
        for name, shape, kw, upcast in shapes(dtype, dev):
            scores = (3.0 * torch.randn(shape, device=dev)).to(dtype).requires_grad_()
            g = torch.randn(shape, device=dev).to(dtype)
            p = kw.get("dropout_p", 0.0)
            mask = kw.get("mask")
            n = scores.numel()
            floor_t = torch.tensor(torch.finfo(dtype).min, device=dev, dtype=dtype)
            nbytes = 5 * n * esize + (2 * mask.numel() * mask.element_size() if mask is not None else 0) + 16 * (n // shape[-1])
            for key in SOFTMAXES:
                spec = S.spec_of(S.SOFTMAX_MAPPING[key])

                def fused():
                    _, used = S.masked_softmax(scores, spec, seed=1234, want_probs=False, **kw)
                    return torch.autograd.grad(used, scores, g)[0]

                def torch_chain():
                    return torch.autograd.grad(chain(scores, spec, upcast, floor=floor_t, **kw), scores, g)[0]

                floor = float(torch.finfo(dtype).min) if kw.get("clamp_min") else None
                okw = dict(scale=kw.get("scale", 1.0), scale_div=kw.get("scale_div", 0.0), mask=mask, clamp_min=floor, p=p, seed=1234 if p else None)

                def fused_ops():
                    y, u, stats = ops.softmax_train_fwd(scores, spec, want_y=p == 0.0, **okw)
                    return ops.softmax_train_bwd(scores, stats, g if p == 0.0 else None, g if p > 0.0 else None, spec, **okw)

                df, dc = [], []
                try:
                    gf, gc = timed_graph(fused_ops, a.iters), timed_graph(torch_chain, a.iters)
                    for _ in range(a.reps):
                        df.append(replay_ms(gf) * 1e3 / a.iters)
                        dc.append(replay_ms(gc) * 1e3 / a.iters)
                    del gf, gc
                except RuntimeError as e:  # a backward that cannot be captured: the step times stand alone, and say so
                    lines.append(f"# device times not measured ({name} {dtype} {key}): {str(e).splitlines()[0][:160]}")
                    print(lines[-1], flush=True)
                    df, dc = [float("nan")], [float("nan")]
                    torch.cuda.synchronize()
                vf, vc = statistics.median(df), statistics.median(dc)
                n0 = dict(S.CALLS)
                arms = {"fused": fused, "chain": torch_chain}
                times = {k: [] for k in arms}
                peak = {}
                for k, fn in arms.items():
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    base = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    fn()
                    torch.cuda.synchronize()
                    peak[k] = (torch.cuda.max_memory_allocated() - base) / 1e6
                for _ in range(a.reps):
                    for k, fn in arms.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.iters):
                            fn()
                        e1.record()
                        e1.synchronize()
                        times[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
                assert S.CALLS["torch"] == n0["torch"] and S.CALLS["backward"] > n0["backward"]  # the fused arm ran the kernels
                uf, uc = statistics.median(times["fused"]), statistics.median(times["chain"])
                line = (f"{name:30s} {str(dtype).split('.')[-1]:8s} {key:25s} device: fused {vf:8.1f} us [{min(df):.1f}..{max(df):.1f}]  "
                        f"chain {vc:8.1f} us [{min(dc):.1f}..{max(dc):.1f}]  chain / fused {vc / vf:5.2f}x{'  FUSED LOSES' if vf > vc else ''}  |  "
                        f"step: fused {uf:8.1f} us [{min(times['fused']):.1f}..{max(times['fused']):.1f}]  "
                        f"chain {uc:8.1f} us [{min(times['chain']):.1f}..{max(times['chain']):.1f}]  chain / fused {uc / uf:5.2f}x{'  FUSED LOSES' if uf > uc else ''}  |  "
                        f"peak fused {peak['fused']:7.1f} MB  chain {peak['chain']:7.1f} MB  |  {nbytes / 1e6:6.1f} MB  {nbytes / (vf * 1e-6) / 1e9:7.1f} GB/s "
                        f"({100.0 * nbytes / (vf * 1e-6) / PEAK_BW:4.1f} % of 8 TB/s)  "
                        f"{ops.softmax_train_variant(*shape, dtype, spec=spec, mask_dtype=None if mask is None else dtype, clamp=bool(kw.get('clamp_min')), p=p)}")
                print(line, flush=True)
                lines.append(line)
            del scores, g
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
