#!/usr/bin/env python3
"""Times of the fused outlier statistics (oeh_outlier_stats) against a pure read pass and against the reference's eager op chain.

    python tools/outlier_bench.py [--out FILE] [--iters N] [--reps R]

Shapes: fp16 and fp32, (16, 512 * 768) and (32, 128 * 768) - an OPT-125m / BERT-base layer output per batch, flattened per sample as
validate_clm.py:570 does - and (8192, 768), token rows.  Three times per shape:
  fused   ops.outlier_stats with a device meter, accumulate = 3 (everything the evaluation loop needs from the tensor); beside it the
          same call without the meter (stats only)
  minmax  oeh_minmax over the same bytes: a pure read pass, the floor
  eager   the reference's chain restated in torch on the GPU - x.norm(dim=1, p=inf), mean, std, ((x - mu) ** 4).mean, the quotient -
          with its two .item() calls per sample (validate_clm.py:575-586, transformers_language/utils.py:9-20)
Method (tools/decode_bench.py): fused and minmax are captured into one graph of `iters` calls each that walk a ring of input buffers larger
than the 256 MB last-level cache, the graphs are replayed alternately `reps` times, each replay timed by device events; the line reports
the median per-call time.  The eager chain cannot be captured (it synchronises with the host 2 * rows times per call): it is timed by
events around a loop over the same ring.  No tracer.  The one condition: fused is faster than eager at (16, 512 * 768) - exit status 1 otherwise."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outeffhop_amd import _lib, ops  # noqa: E402

SHAPES = ((16, 512 * 768), (32, 128 * 768), (8192, 768))
RING_BYTES = 600_000_000


def eager_chain(x, eps=1e-6):
    """the reference's per-batch measurement of one hooked tensor, sums kept as its AverageMeter keeps them"""
    s_inf = s_kurt = 0.0
    x = x.view(x.size(0), -1)
    for v in x.norm(dim=1, p=np.inf):
        s_inf += v.item()
    mu = x.mean(dim=1, keepdims=True)
    s = x.std(dim=1)
    mu4 = ((x - mu) ** 4.0).mean(dim=1)
    for v in mu4 / (s ** 4.0 + eps):
        s_kurt += v.item()
    return s_inf, s_kurt


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
    ap.add_argument("--iters", type=int, default=96)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("outlier_bench needs a GPU: there is no CPU timing")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lines = [f"# outlier_bench: {lib.oeh_build_info().decode()}",
             f"# fused / minmax: event times of graph replays ({a.iters} calls per graph over a ring of > {RING_BYTES // 1_000_000} MB, median of {a.reps} alternating replays);"
             " eager: events around a loop over the same ring; no tracer",
             f"# W = {ops.STATS_WAVE_COLS}, C = {ops.STATS_CHUNK}"]
    ok = True
    for dtype in (torch.float16, torch.float32):
        for rows, cols in SHAPES:
            nbytes = rows * cols * torch.empty(0, dtype=dtype).element_size()
            ring = [torch.randn(rows, cols, device=dev, dtype=torch.float32).to(dtype) for _ in range(min(64, -(-RING_BYTES // nbytes)))]
            meter = torch.zeros(4, dtype=torch.float64, device=dev)
            stats = torch.empty(rows, 4, dtype=torch.float32, device=dev)
            wb = lib.oeh_outlier_stats_work_bytes(rows, cols)
            work = torch.empty(wb // 8 + 1, dtype=torch.int64, device=dev)
            mm = torch.empty(2, dtype=torch.float32, device=dev)

            def fused(x):
                ops.outlier_stats(x, meter=meter, accumulate=3, out=stats, work=work)

            def minmax(x):
                _lib.check(lib.oeh_minmax(ops._ptr(x), x.numel(), ops._DT[x.dtype], ops._ptr(mm), ops._stream()), "oeh_minmax")

            def plain(x):
                ops.outlier_stats(x, out=stats, work=work)

            ga, gb, gp = timed_graph(fused, ring, a.iters), timed_graph(minmax, ring, a.iters), timed_graph(plain, ring, a.iters)
            ta, tb, tp = [], [], []
            for _ in range(a.reps):
                ta.append(replay_ms(ga) * 1e3 / a.iters)
                tb.append(replay_ms(gb) * 1e3 / a.iters)
                tp.append(replay_ms(gp) * 1e3 / a.iters)
            n_eager = max(2, min(len(ring), 20000 // (2 * rows)))
            eager_chain(ring[0])
            tc = []
            for _ in range(min(a.reps, 3)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(n_eager):
                    eager_chain(ring[i % len(ring)])
                e1.record()
                e1.synchronize()
                tc.append(e0.elapsed_time(e1) * 1e3 / n_eager)
            ua, ub, uc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
            line = (f"{str(dtype).split('.')[-1]:8s} ({rows:5d}, {cols:7d}) {nbytes / 1e6:6.1f} MB  fused {ua:8.2f} us [{min(ta):.2f}..{max(ta):.2f}] "
                    f"{nbytes / (ua * 1e-6) / 1e12:5.2f} TB/s  without meter {statistics.median(tp):8.2f} us  minmax {ub:8.2f} us [{min(tb):.2f}..{max(tb):.2f}]  fused / minmax {ua / ub:5.2f}  "
                    f"eager chain {uc:10.1f} us ({2 * rows} .item() calls)  eager / fused {uc / ua:7.1f}x  ({len(ring)} buffers)")
            print(line, flush=True)
            lines.append(line)
            if (rows, cols) == SHAPES[0] and not ua < uc:
                ok = False
            del ga, gb, gp, ring
            torch.cuda.empty_cache()
    lines.append("# condition (fused faster than the eager chain at (16, 393216)): " + ("met" if ok else "NOT met"))
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
