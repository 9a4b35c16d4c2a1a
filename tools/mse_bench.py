#!/usr/bin/env python3
"""Times of the fused quantisation-error search (oeh_quant_mse under MSE_Estimator) against the eager op chain.

    python tools/mse_bench.py [--out FILE] [--reps R]

Shapes, fp16 and fp32: (16, 12, 512, 512) - the score tensor of the cfg4 configuration - and (768, 3072), a weight.  Per shape:
  search  one batch of MSE_Estimator's 1-D grid search with 100 candidates on an initialised estimator: ops.quant_mse adding all
          candidates' losses to the float64 device array, argmin, the range looked up - no host synchronisation
  eager   the same batch by the estimator's CPU-tensor code path called on the GPU tensors (quantization.quant_mse_eager: per candidate
          divide, round, clamp, scale, subtract, square, float64 sum and one host read, as range_estimators.py:134-142), then the
          same accumulate / argmin
  K = 1   one ops.quant_mse call with a single candidate: a golden-section step (without its host read)
  minmax  oeh_minmax over the same bytes: a pure read pass, the floor of one pass
Method (tools/outlier_bench.py): search, K = 1 and minmax are captured into one graph of `iters` calls each that walk a ring of input
buffers larger than the 256 MB last-level cache; the graphs are replayed alternately `reps` times, each replay timed by device events;
the line reports the median per-call time.  The eager chain synchronises with the host per candidate and cannot be captured: it is timed
by events around a loop over the same ring.  No tracer.  The one condition: the fused search is faster than the eager chain at both
shapes, in both dtypes - exit status 1 otherwise."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outeffhop_amd import _lib, ops  # noqa: E402
from outeffhop_amd.quantization import MSE_Estimator, OptMethod, SymmetricUniformQuantizer, quant_mse_eager  # noqa: E402

SHAPES = (((16, 12, 512, 512), 6, 2), ((768, 3072), 64, 8))  # shape, calls per graph, eager calls per timing
RING_BYTES = 600_000_000


def timed_graph(launch, ring, iters):
    launch(ring[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(iters):
            launch(ring[i % len(ring)])
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
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mse_bench needs a GPU: there is no CPU timing")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lines = [f"# mse_bench: {lib.oeh_build_info().decode()}",
             f"# search / K = 1 / minmax: event times of graph replays over a ring of > {RING_BYTES // 1_000_000} MB, median of {a.reps} alternating replays;"
             " eager: events around a loop over the same ring; no tracer",
             f"# C = {ops.QMSE_CHUNK}, slice = {ops.QMSE_SLICE}, at most {ops.QMSE_MAX_BLOCKS} workgroups; 1-D grid search, 100 candidates, symmetric 8-bit quantiser"]
    ok = True
    for dtype in (torch.float16, torch.float32):
        for shape, iters, n_eager in SHAPES:
            n = 1
            for s in shape:
                n *= s
            nbytes = n * torch.empty(0, dtype=dtype).element_size()
            ring = [torch.randn(shape, device=dev, dtype=torch.float32).to(dtype) for _ in range(min(64, -(-RING_BYTES // nbytes)))]
            est = MSE_Estimator(num_candidates=100, opt_method=OptMethod.grid, quantizer=SymmetricUniformQuantizer(n_bits=8))
            est(ring[0])  # the first batch: one host read of (min, max), the candidate table goes to the device
            cand1 = est._cand[49:50].contiguous()
            loss1 = torch.empty(1, dtype=torch.float64, device=dev)
            mm = torch.empty(2, dtype=torch.float32, device=dev)

            def search(x):
                est(x)

            def single(x):
                ops.quant_mse(x, cand1, loss1)

            def minmax(x):
                _lib.check(lib.oeh_minmax(ops._ptr(x), x.numel(), ops._DT[x.dtype], ops._ptr(mm), ops._stream()), "oeh_minmax")

            def eager(x):
                flat = est.loss_array.view(-1)
                flat[1:] += quant_mse_eager(x, est._cand)
                best = est._range_table.index_select(0, torch.argmin(flat).reshape(1))[0]
                return best[0:1].clone(), best[1:2].clone()

            ga, gb, gc = timed_graph(search, ring, iters), timed_graph(single, ring, iters), timed_graph(minmax, ring, iters)
            ta, tb, tc = [], [], []
            for _ in range(a.reps):
                ta.append(replay_ms(ga) * 1e3 / iters)
                tb.append(replay_ms(gb) * 1e3 / iters)
                tc.append(replay_ms(gc) * 1e3 / iters)
            eager(ring[0])
            te = []
            for _ in range(min(a.reps, 3)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(n_eager):
                    eager(ring[i % len(ring)])
                e1.record()
                e1.synchronize()
                te.append(e0.elapsed_time(e1) * 1e3 / n_eager)
            ua, ub, uc, ue = (statistics.median(t) for t in (ta, tb, tc, te))
            line = (f"{str(dtype).split('.')[-1]:8s} {str(shape):20s} {nbytes / 1e6:6.1f} MB  search {ua:9.1f} us [{min(ta):.1f}..{max(ta):.1f}] "
                    f"({ua * 1e-6 / (n * 100) * 1e12:.2f} ps per element and candidate)  eager chain {ue:10.1f} us  eager / search {ue / ua:6.1f}x  "
                    f"K = 1 {ub:8.1f} us [{min(tb):.1f}..{max(tb):.1f}]  minmax {uc:8.1f} us  ({len(ring)} buffers)")
            print(line, flush=True)
            lines.append(line)
            if not ua < ue:
                ok = False
            del ga, gb, gc, ring, est
            torch.cuda.empty_cache()
    lines.append("# condition (the fused search is faster than the eager chain at every shape): " + ("met" if ok else "NOT met"))
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
