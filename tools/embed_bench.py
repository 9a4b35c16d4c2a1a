#!/usr/bin/env python3
"""Times of the fused model front (oeh_embed_sum_quant) against the chain of ops a user had before it.

    python tools/embed_bench.py [--out FILE] [--reps R] [--iters N]

Shapes: BERT-base B 32, S 128 (vocab 30522, 2 token types, 512 positions, E 768: three lookups, two sum quantisers, LayerNorm, output
quantiser) and OPT-125m B 16, S 512 (vocab 50272, 2050 positions, E 768: two lookups, one sum quantiser, no LayerNorm); fp32 and fp16.
Per line:
  float   ONE ops.embed_sum_quant call on the raw tables, the weight grid applied to the gathered rows
  int8    ONE ops.embed_sum_quant call on the int8 index tables (what the modules use once the weight ranges are frozen)
  chain   what the package offered before: cached fake-quantised tables -> F.embedding -> torch.add -> ops.fake_quant (-> add -> fake_quant)
          -> ops.resid_ln_quant (BERT)
  bytes   what a fused call has to move: the ids, one gathered row per lookup and position (4 / 2 / 1 bytes an element), y written,
          gamma and beta; and that over the fused time as a fraction of 8 TB/s.  A whole-call rate from device events.
Method (tools/ln_bench.py): every form is captured into one graph of `iters` calls that walk a ring of (ids, output) sets whose outputs
exceed the 256 MB last-level cache; the graphs are replayed alternately `reps` times, each replay timed by device events; a line reports the
median per-call time and the spread.  No tracer.  The tables themselves are shared by the ring's entries (a model has one set): how much
of a table the cache keeps is part of what a user sees.  The one condition - the rule by which quantization.FUSED_EMBED defaults to True: neither
fused call is slower than the chain at both model shapes in fp32 - exit status 1 otherwise."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outeffhop_amd import _lib, ops  # noqa: E402
from outeffhop_amd import quantization as Q  # noqa: E402

F = torch.nn.functional
MODELS = (("bert-base", 32, 128, 768, (30522, 2, 512)), ("opt-125m", 16, 512, 768, (50272, 2050)))
RING_BYTES = 600_000_000
PEAK_BYTES_PER_S = 8.0e12
EPS = 1e-12


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
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("embed_bench needs a GPU: there is no CPU timing")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lines = [f"# embed_bench: {lib.oeh_build_info().decode()}",
             f"# event times of graph replays ({a.iters} calls per graph) over a ring of (ids, output) sets with > {RING_BYTES // 1_000_000} MB of outputs, median of"
             f" {a.reps} alternating replays [min..max]; no tracer",
             "# float / int8: ops.embed_sum_quant; chain: F.embedding on cached fake-quantised tables -> torch.add -> ops.fake_quant ... -> ops.resid_ln_quant"]
    ok = True
    for dtype in (torch.float32, torch.float16):
        esize = torch.empty(0, dtype=dtype).element_size()
        for name, B, S, E, sizes in MODELS:
            bert = len(sizes) == 3
            tables, grids, wq, i8 = [], [], [], []
            for n in sizes:
                w = (0.05 * torch.randn(n, E, device=dev))
                w[:, 7] *= 40.0
                w = w.to(dtype)
                qz = Q.SymmetricUniformQuantizer(n_bits=8)
                qz.set_quant_range(w.min(), w.max())
                tables.append(w)
                grids.append((float(qz.scale), float(qz.int_min), float(qz.int_max)))
                wq.append(qz(w))
                i8.append(qz.to_integer_forward(w).to(torch.int8))
            n_out = B * S * E
            sets = max(2, min(64, -(-RING_BYTES // (n_out * esize))))
            ring = []
            for _ in range(sets):
                ids = [torch.randint(0, sizes[0], (B, S), device=dev)]
                if bert:
                    ids += [torch.randint(0, 2, (B, S), device=dev), torch.arange(S, device=dev).expand(1, -1)]
                else:
                    ids += [torch.arange(2, S + 2, device=dev).expand(B, -1).contiguous()]
                ring.append((ids, torch.empty(B, S, E, dtype=dtype, device=dev)))
            gamma = 1.0 + 0.2 * torch.randn(E, device=dev)
            beta = 0.1 * torch.randn(E, device=dev)
            fqs = [ops.FakeQuantSpec.from_delta(30.0 / 255.0, 110.0), ops.FakeQuantSpec.from_delta(31.0 / 255.0, 112.0)][:len(sizes) - 1]
            fq_out = ops.FakeQuantSpec.from_delta(60.0 / 255.0, 128.0) if bert else None
            g, b = (gamma, beta) if bert else (None, None)

            def fused_float(ids, out):
                lk = [ops.EmbedLookup(w, i, *gr) for w, i, gr in zip(tables, ids, grids)]
                return ops.embed_sum_quant(lk, g, b, EPS, fq_sums=fqs, fq_out=fq_out, dtype=dtype, out=out)

            def fused_int8(ids, out):
                lk = [ops.EmbedLookup(w, i, *gr) for w, i, gr in zip(i8, ids, grids)]
                return ops.embed_sum_quant(lk, g, b, EPS, fq_sums=fqs, fq_out=fq_out, dtype=dtype, out=out)

            def chain(ids, out):
                s = F.embedding(ids[0], wq[0])
                for t in range(1, len(sizes)):
                    s = ops.fake_quant(torch.add(s, F.embedding(ids[t], wq[t])), fqs[t - 1])
                return ops.resid_ln_quant(s, None, gamma, beta, EPS, fq_out=fq_out, out=out) if bert else s

            graphs = [timed_graph(f, ring, a.iters) for f in (fused_float, fused_int8, chain)]
            times = [[], [], []]
            for _ in range(a.reps):
                for k, gr in enumerate(graphs):
                    times[k].append(replay_ms(gr) * 1e3 / a.iters)
            med = [statistics.median(t) for t in times]
            rows = B * S
            id_bytes = sum(i.numel() * 8 for i in ring[0][0])
            par = 2 * E * 4 if bert else 0
            nb_float = rows * E * esize * (len(sizes) + 1) + id_bytes + par
            nb_int8 = rows * E * (len(sizes) + esize) + id_bytes + par
            rate = lambda nb, us: f"{nb / 1e6:6.1f} MB {nb / (us * 1e-6) / 1e12:5.2f} TB/s = {nb / (us * 1e-6) / PEAK_BYTES_PER_S:5.1%} of 8 TB/s"  # noqa: E731
            sp = lambda t: f"[{min(t):.2f}..{max(t):.2f}]"  # noqa: E731
            line = (f"{str(dtype).split('.')[-1]:8s} {name:9s} B {B:2d} S {S:3d}  {ops.embed_sum_variant(B, S, E, dtype, n_tab=len(sizes)):22s} "
                    f"float {med[0]:7.2f} us {sp(times[0])} {rate(nb_float, med[0])}  int8 {med[1]:7.2f} us {sp(times[1])} {rate(nb_int8, med[1])}  "
                    f"chain {med[2]:7.2f} us {sp(times[2])}  chain / float {med[2] / med[0]:5.2f}x  chain / int8 {med[2] / med[1]:5.2f}x  ({sets} sets)")
            print(line, flush=True)
            lines.append(line)
            if dtype == torch.float32 and not (med[0] <= med[2] and med[1] <= med[2]):
                ok = False
            del graphs, ring
            torch.cuda.empty_cache()
    lines.append("# condition (neither fused call slower than the chain at both model shapes in fp32): " + ("met" if ok else "NOT met"))
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
