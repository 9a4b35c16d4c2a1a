#!/usr/bin/env python3
"""Times of the fused block tail (oeh_resid_ln_quant) against the chain of ops a user had before it.

    python tools/ln_bench.py [--out FILE] [--reps R] [--iters N]

Shapes: 4096 x 768 (BERT-base, B = 32, S = 128), 8192 x 768 (OPT-125m, B = 16, S = 512), 8192 x 1024 and 8192 x 2048; fp32 and fp16;
with and without the quantised sum as a second output.  Per line:
  fused   ONE ops.resid_ln_quant call: residual add, sum quantiser, LayerNorm, output quantiser
  chain   torch.add -> ops.fake_quant -> F.layer_norm -> ops.fake_quant (the sum is an intermediate of the chain either way)
  bytes   what the fused call has to move: x and r read, y written (and the sum), gamma and beta; and that over the fused time as a
          fraction of 8 TB/s.  A whole-call rate from device events, not a kernel's share of peak from a trace.
Method (tools/mse_bench.py): both forms are captured into one graph of `iters` calls each that walk a ring of (x, r) pairs larger than
the 256 MB last-level cache; the two graphs are replayed alternately `reps` times, each replay timed by device events; the line reports
the median per-call time and the spread.  No tracer.  The one condition - the rule by which quantization.FUSED_LN defaults to True: the
fused call is not slower than the chain at the two model shapes, 4096 x 768 and 8192 x 768, in fp32 - exit status 1 otherwise."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outeffhop_amd import _lib, ops  # noqa: E402

SHAPES = ((4096, 768), (8192, 768), (8192, 1024), (8192, 2048))
MODEL_SHAPES = ((4096, 768), (8192, 768))
RING_BYTES = 600_000_000
PEAK_BYTES_PER_S = 8.0e12
EPS = 1e-5


def timed_graph(launch, ring, iters):
    launch(*ring[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(iters):
            launch(*ring[i % len(ring)])
    return g


def replay_ms(g):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=400)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ln_bench needs a GPU: there is no CPU timing")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lines = [f"# ln_bench: {lib.oeh_build_info().decode()}",
             f"# event times of graph replays ({a.iters} calls per graph) over a ring of (x, r) pairs of > {RING_BYTES // 1_000_000} MB, median of {a.reps} alternating"
             " replays [min..max]; no tracer",
             "# fused: ops.resid_ln_quant; chain: torch.add -> ops.fake_quant -> F.layer_norm -> ops.fake_quant; both 8-bit quantisers on"]
    ok = True
    for dtype in (torch.float32, torch.float16):
        esize = torch.empty(0, dtype=dtype).element_size()
        for rows, cols in SHAPES:
            n = rows * cols
            pairs = max(2, min(32, -(-RING_BYTES // (2 * n * esize))))
            ring = []
            for _ in range(pairs):
                x = torch.randn(rows, cols, device=dev)
                x[:, 7] *= 40.0
                x[:, cols - 3] *= -25.0
                ring.append((x.to(dtype), torch.randn(rows, cols, device=dev).to(dtype)))
            gamma = 1.0 + 0.2 * torch.randn(cols, device=dev)
            beta = 0.1 * torch.randn(cols, device=dev)
            gamma_t, beta_t = gamma.to(dtype), beta.to(dtype)
            fq_sum = ops.FakeQuantSpec.from_delta(260.0 / 255.0, 110.0)
            fq_out = ops.FakeQuantSpec.from_delta(60.0 / 255.0, 128.0)
            for with_sum in (False, True):
                def fused(x, r):
                    return ops.resid_ln_quant(x, r, gamma, beta, EPS, fq_sum=fq_sum, fq_out=fq_out, want_sum=with_sum)

                def chain(x, r):
                    s = ops.fake_quant(torch.add(x, r), fq_sum)
                    y = ops.fake_quant(torch.nn.functional.layer_norm(s, (cols,), gamma_t, beta_t, EPS), fq_out)
                    return (s, y) if with_sum else y

                gf, gc = timed_graph(fused, ring, a.iters), timed_graph(chain, ring, a.iters)
                tf, tc = [], []
                for _ in range(a.reps):
                    tf.append(replay_ms(gf) * 1e3 / a.iters)
                    tc.append(replay_ms(gc) * 1e3 / a.iters)
                uf, uc = statistics.median(tf), statistics.median(tc)
                nbytes = (3 + int(with_sum)) * n * esize + 2 * cols * 4
                line = (f"{str(dtype).split('.')[-1]:8s} {rows:5d} x {cols:4d} {'+ sum' if with_sum else '     '}  {ops.resid_ln_variant(rows, cols, dtype):18s} "
                        f"fused {uf:7.2f} us [{min(tf):.2f}..{max(tf):.2f}]  chain {uc:7.2f} us [{min(tc):.2f}..{max(tc):.2f}]  chain / fused {uc / uf:5.2f}x  "
                        f"{nbytes / 1e6:6.1f} MB  {nbytes / (uf * 1e-6) / 1e12:5.2f} TB/s = {nbytes / (uf * 1e-6) / PEAK_BYTES_PER_S:5.1%} of 8 TB/s  ({pairs} pairs)")
                print(line, flush=True)
                lines.append(line)
                if dtype == torch.float32 and (rows, cols) in MODEL_SHAPES and not uf <= uc:
                    ok = False
                del gf, gc
            del ring
            torch.cuda.empty_cache()
    lines.append("# condition (fused not slower than the chain at 4096 x 768 and 8192 x 768 in fp32, with and without the sum): " + ("met" if ok else "NOT met"))
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
