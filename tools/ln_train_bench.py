#!/usr/bin/env python3
"""Forward + backward times of the fused training block tail (oeh_drop_resid_ln_fwd / oeh_drop_resid_ln_bwd) against the eager chain.

    python tools/ln_train_bench.py [--out FILE] [--reps R] [--iters N]

Shapes: 4096 x 768 (BERT-base, B = 32, S = 128: post-LN, y only) and 8192 x 768 (OPT-125m, B = 16, S = 512: pre-LN, the sum is a second
output with a gradient of its own); fp16 and fp32; p = 0.1 and p = 0.  Per line, two measurements of one forward + backward:
  device  graph replays timed by device events, as tools/ln_bench.py: `iters` steps per graph over a ring of inputs larger than the 256 MB
          last-level cache, the two graphs replayed alternately `reps` times, median [min..max] per step.  fused = ops.drop_resid_ln_fwd +
          ops.drop_resid_ln_bwd; chain = F.dropout -> add -> F.layer_norm and torch.autograd.grad through them.
  step    what a training loop sees, host included: layers.dropout_add_layer_norm and .backward() of a scalar loss in a plain loop of
          `iters` steps between two device events, the switch layers.FUSED_LN_TRAIN on / off (off = the parent commit's behaviour).
  bytes   what the fused calls have to move: x, r read and sum, y written; s, dy (and dsum) read and dx, dr written; and that over the
          fused device time.  A whole-call rate from device events, not a kernel's share of peak from a trace.
The rule for the default of layers.FUSED_LN_TRAIN: the fused forward + backward is faster than the chain at both model shapes in fp16
(device time, p = 0.1 and p = 0) - exit status 1 otherwise.  No tracer."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outeffhop_amd import _lib, layers, ops  # noqa: E402

MODEL_SHAPES = (("BERT-base", 4096, 768, False), ("OPT-125m", 8192, 768, True))  # name, rows, cols, want_sum
RING_BYTES = 600_000_000
EPS = 1e-5


def replay_ms(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed_graph(step, ring, iters):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the default stream, as graph capture of a backward asks
        for i in range(3):
            step(*ring[i % len(ring)])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(iters):
            step(*ring[i % len(ring)])
    return g


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ln_train_bench needs a GPU: there is no CPU timing")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lines = [f"# ln_train_bench: {lib.oeh_build_info().decode()}",
             f"# one forward + backward.  device: event times of graph replays ({a.iters} steps per graph) over a ring of inputs of > {RING_BYTES // 1_000_000} MB,"
             f" median of {a.reps} alternating replays [min..max]; step: a plain loop of {a.iters} steps with .backward(), host included, median of 3; no tracer",
             "# fused: ops.drop_resid_ln_fwd + ops.drop_resid_ln_bwd (step: layers.dropout_add_layer_norm); chain: F.dropout -> add -> F.layer_norm and their autograd"]
    ok = True
    for dtype in (torch.float16, torch.float32):
        esize = torch.empty(0, dtype=dtype).element_size()
        for name, rows, cols, want_sum in MODEL_SHAPES:
            n = rows * cols
            sets = max(2, min(16, -(-RING_BYTES // ((4 + int(want_sum)) * n * esize))))
            ring = []
            for _ in range(sets):
                x = torch.randn(rows, cols, device=dev)
                x[:, 7] *= 40.0
                x[:, cols - 3] *= -25.0
                t = lambda: torch.randn(rows, cols, device=dev).to(dtype)  # noqa: E731
                ring.append((x.to(dtype).requires_grad_(), t().requires_grad_(), t(), t() if want_sum else None))
            gamma = (1.0 + 0.2 * torch.randn(cols, device=dev)).to(dtype).requires_grad_()
            beta = (0.1 * torch.randn(cols, device=dev)).to(dtype).requires_grad_()
            for p in (0.1, 0.0):
                def fused(x, r, dy, dsum):
                    s, y, mean, rstd = ops.drop_resid_ln_fwd(x, r, gamma, beta, EPS, p=p, seed=12345)
                    return ops.drop_resid_ln_bwd(dy, s, gamma, mean, rstd, dsum=dsum, p=p, seed=12345)

                def chain(x, r, dy, dsum):
                    s = (F.dropout(x, p, True) if p > 0 else x) + r
                    y = F.layer_norm(s, (cols,), gamma, beta, EPS)
                    outs, grads = ((y, s), (dy, dsum)) if want_sum else ((y,), (dy,))
                    return torch.autograd.grad(outs, (x, r, gamma, beta), grads)

                def step(x, r, dy, dsum):  # a training loop's view: the public function, a scalar loss, .backward()
                    out = layers.dropout_add_layer_norm(x, r, gamma, beta, p=p, eps=EPS, want_sum=want_sum)
                    loss = (out[1].float() * dy).sum() + (out[0].float() * dsum).sum() if want_sum else (out.float() * dy).sum()
                    loss.backward()
                    for t_ in (x, r, gamma, beta):
                        t_.grad = None

                tf, tc = [], []
                try:
                    gf, gc = timed_graph(fused, ring, a.iters), timed_graph(chain, ring, a.iters)
                    for _ in range(a.reps):
                        tf.append(replay_ms(gf) * 1e3 / a.iters)
                        tc.append(replay_ms(gc) * 1e3 / a.iters)
                    del gf, gc
                except RuntimeError as e:  # a backward that cannot be captured: the step times below stand alone, and say so
                    lines.append(f"# device times not measured ({name} {dtype} p {p}): {str(e).splitlines()[0][:160]}")
                    print(lines[-1], flush=True)
                    tf, tc = [float("nan")], [float("nan")]
                    torch.cuda.synchronize()
                uf, uc = statistics.median(tf), statistics.median(tc)
                sf, sc = [], []
                for _ in range(3):
                    prev = layers.set_fused_ln_train(True)
                    sf.append(loop_us(step, ring, a.iters))
                    layers.set_fused_ln_train(False)
                    sc.append(loop_us(step, ring, a.iters))
                    layers.set_fused_ln_train(prev)
                nbytes = (8 + int(want_sum)) * n * esize + 6 * cols * 4
                line = (f"{name:9s} {str(dtype).split('.')[-1]:8s} {rows:5d} x {cols:4d} {'+ sum' if want_sum else '     '} p {p:3.1f}  "
                        f"device: fused {uf:7.2f} us [{min(tf):.2f}..{max(tf):.2f}]  chain {uc:7.2f} us [{min(tc):.2f}..{max(tc):.2f}]  chain / fused {uc / uf:5.2f}x  "
                        f"{nbytes / 1e6:6.1f} MB  {nbytes / (uf * 1e-6) / 1e9:7.1f} GB/s fused, {nbytes / (uc * 1e-6) / 1e9:7.1f} GB/s chain  |  "
                        f"step: fused {statistics.median(sf):7.1f} us  chain {statistics.median(sc):7.1f} us  ({sets} input sets)")
                print(line, flush=True)
                lines.append(line)
                if dtype == torch.float16 and not (uf < uc if uf == uf else statistics.median(sf) < statistics.median(sc)):
                    ok = False
            del ring
            torch.cuda.empty_cache()
    lines.append("# rule (fused forward + backward faster than the chain at both model shapes in fp16, device time): " + ("met" if ok else "NOT met"))
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
