#!/usr/bin/env python3
"""Times of one layer's quantised feed-forward: the fused route (quantization.FUSED_FFN) against the chain the same modules run with the
switch off - which is what they ran before the switch existed.

    python tools/ffn_bench.py [--out FILE] [--reps R] [--iters N]

Shapes: OPT-125m, 8192 x 768 -> 3072 -> 768 with ReLU (B = 16, S = 512); BERT-base, 4096 x 768 -> 3072 -> 768 with GELU (B = 32, S = 128);
each for an fp32 and an fp16 model.  Symmetric 8-bit weights, frozen 8-bit asymmetric activation quantisers whose ranges are the min / max of
the full-precision activations of the first input.  Per line:
  fused   quantization.feed_forward(fc1_act, fc2, x) with FUSED_FFN on: fc1 + activation + quantiser -> int8 indices -> fc2 on the integer
          matrix cores with its quantiser in the epilogue (the route's name: which form fc1 took)
  chain   the same call with FUSED_FFN off = fc2(fc1_act(x)): GEMM, scale + bias, activation, fake-quant, GEMM, scale + bias + fake-quant
Method (tools/ln_bench.py): both forms are captured into one graph of `iters` calls each that walk a ring of inputs larger than the 256 MB
last-level cache; the two graphs are replayed alternately `reps` times, each replay timed by device events; the line reports the median
per-call time and the spread.  No tracer.  The tool states ratios; it sets no condition (exit status 0)."""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outeffhop_amd import _lib  # noqa: E402
from outeffhop_amd import quantization as Q  # noqa: E402

CASES = (("OPT-125m", 8192, 768, 3072, "relu"), ("BERT-base", 4096, 768, 3072, "gelu"))
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


def build(E, F, act, dtype, x0):
    """(fc1_act, fc2) with every range frozen: the weights' min / max, the activations' from the full-precision chain on x0."""
    qp = Q.val_qparams(Q.get_quant_config())
    qp["quant_dict"] = {}
    g = torch.Generator().manual_seed(0)
    l1, l2 = nn.Linear(E, F), nn.Linear(F, E)
    with torch.no_grad():
        for lin in (l1, l2):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * 0.03)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    fc1 = Q.quantize_model(nn.Sequential(l1, nn.ReLU() if act == "relu" else nn.GELU()), **qp)[0].cuda().to(dtype)
    fc2 = Q.quantize_model(l2, **qp).cuda().to(dtype)
    with torch.no_grad():
        h = fc1.activation_function(nn.functional.linear(x0, fc1.weight, fc1.bias))
        o = nn.functional.linear(h, fc2.weight, fc2.bias)
        for m, t in ((fc1, h), (fc2, o)):
            m.weight_quantizer.set_quant_range(m.weight.min().float(), m.weight.max().float())
            m.activation_quantizer.set_quant_range(t.min().float(), t.max().float())
            m.quantized()
            m.fix_ranges()
            m.eval()
    return fc1, fc2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ffn_bench needs a GPU: there is no CPU timing")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lines = [f"# ffn_bench: {lib.oeh_build_info().decode()}",
             f"# event times of graph replays ({a.iters} calls per graph) over a ring of inputs of > {RING_BYTES // 1_000_000} MB, median of {a.reps} alternating"
             " replays [min..max]; no tracer",
             "# fused: quantization.feed_forward with FUSED_FFN on; chain: the same modules with FUSED_FFN off"]
    prev = Q.FUSED_FFN
    try:
        for name, rows, E, F, act in CASES:
            for dtype in (torch.float32, torch.float16):
                esize = torch.empty(0, dtype=dtype).element_size()
                n_in = max(2, min(48, -(-RING_BYTES // (rows * E * esize))))
                ring = [torch.randn(rows, E, device=dev).to(dtype) for _ in range(n_in)]
                fc1, fc2 = build(E, F, act, dtype, ring[0])

                def run(x):
                    return Q.feed_forward(fc1, fc2, x)

                with torch.no_grad():
                    Q.set_fused_ffn(True)
                    gf = timed_graph(run, ring, a.iters)
                    route = ("gemm+quant" if fc1.__dict__.get("_gemm_quant_calls", 0) else "gemm, act_quant" if fc1.__dict__.get("_act_quant_calls", 0) else "-") + \
                            (" -> int8 fc2" if fc2.__dict__.get("_int8_index_calls", 0) else " -> fc2 unfused")
                    Q.set_fused_ffn(False)
                    gc = timed_graph(run, ring, a.iters)
                    y_chain = run(ring[1])
                    Q.set_fused_ffn(True)
                    same = float((run(ring[1]) != y_chain).float().mean())
                    Q.set_fused_ffn(False)
                tf, tc = [], []
                for _ in range(a.reps):
                    tf.append(replay_ms(gf) * 1e3 / a.iters)
                    tc.append(replay_ms(gc) * 1e3 / a.iters)
                uf, uc = statistics.median(tf), statistics.median(tc)
                line = (f"{name:9s} {str(dtype).split('.')[-1]:8s} {rows:5d} x {E} -> {F} -> {E} {act:4s}  [{route}]  fused {uf:8.2f} us [{min(tf):.2f}..{max(tf):.2f}]  "
                        f"chain {uc:8.2f} us [{min(tc):.2f}..{max(tc):.2f}]  chain / fused {uc / uf:5.2f}x  outputs that differ {same:.1e}  ({n_in} inputs)")
                print(line, flush=True)
                lines.append(line)
                del gf, gc, ring, fc1, fc2
                torch.cuda.empty_cache()
    finally:
        Q.set_fused_ffn(prev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
