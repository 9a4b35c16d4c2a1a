#!/usr/bin/env python3
"""Same-process A/B of the split-key decode kernels (oeh_attn_decode, default split rule) against oeh_attn_fwd on the same buffers - what a
generation step of OPT-125m ran before the decode entry point existed.

    python tools/decode_bench.py [--out FILE] [--sweep] [--fq] [--iters N] [--reps R]

Shapes: H = 12, D = 64, fp16, causal, Sq = 1, B in {1, 16} x Sk in {512, 2048}, softmax1 and clippedsoftmax1(-.025:1).
Method: each side's launches are captured into one graph of `iters` calls that walk a ring of K / V buffer sets (so that a call does not find
the previous call's cache lines), the two graphs are replayed alternately `reps` times, each replay timed by device events; the line reports
the median per-call time of each side.  Times are event times of graph replays, not tracer kernel times.  --sweep adds the time of every
explicit split count (how the default rule was chosen).  At B = 16, Sk = 2048 the line also gives the achieved share of 8 TB/s on the
algorithmic bytes (K + V + q + o).
--fq: the same comparison with the fused INT8 chain - oeh_attn_decode_fq against oeh_attn_fwd with the same oeh_fq_desc (what a generation step of
the quantised OPT decoder runs without the decode route); the three ranges are calibrated once per shape and form from the first buffer set
(percentiles 0.001 / 99.999 of the float intermediates, as the tests do), the context quantised before the (absent) gate."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outeffhop_amd import _lib, ops  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
FORMS = {"softmax1": ops.SoftmaxSpec(1, False, 0.0, 1.0), "clippedsoftmax1(-.025:1)": ops.SoftmaxSpec(1, True, -0.025, 1.1)}


def make_desc(q, k, v, o, spec):
    """fp16, unscaled, causal with clamp_min at fp32's minimum (OPT's decoder step)"""
    return ops._attn_desc(q, k, v, o, _lib.OEH_F16, _lib.OEH_F16, spec, 1.0, 0.0, True, True, None, torch.float32)


def calibrated_fq(q, k, v, spec):
    """an oeh_fq_desc with all three quantisers on, ranges from the float intermediates of this buffer set"""
    from oracle import oeh_oracle as O

    qn, kn, vn = (t.float().cpu().numpy() for t in (q, k, v))
    kw = dict(base=spec.base, clip=bool(spec.clip), gamma=spec.gamma, eta=spec.eta, causal=True, clamp_min=True)
    ctx, fp = O.attn_core(qn, kn, vn, want=("scores", "probs"), **kw)
    fqd = _lib.oeh_fq_desc()
    for dst, x in ((fqd.scores, fp["scores"]), (fqd.probs, fp["probs"]), (fqd.ctx, ctx)):
        ops._fill_fq(dst, ops.FakeQuantSpec.from_delta(*O.quant_range_to_params(*np.percentile(x, (0.001, 99.999)))))
    fqd.ctx_quant_before_gate = 1
    return fqd


def timed_graph(launch, sets, iters):
    """one graph of `iters` launches walking the buffer ring"""
    launch(sets[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(iters):
            launch(sets[i % len(sets)])
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
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--fq", action="store_true", help="with the fused INT8 chain: oeh_attn_decode_fq against oeh_attn_fwd with the same quantisers")
    ap.add_argument("--boundary", action="store_true", help="the shapes around the modules' routing rule instead of the standard four")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench needs a GPU: there is no CPU timing")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    lines = [f"# decode_bench{' --fq' if a.fq else ''}: {lib.oeh_build_info().decode()}",
             f"# event times of graph replays ({a.iters} calls per graph, median of {a.reps} alternating replays); no tracer"]
    H, D, Sq = 12, 64, 1
    gen = torch.Generator().manual_seed(0)
    for B in ((1, 2, 4, 8) if a.boundary else (1, 16)):
        for Sk in ((1024, 2048, 4096) if a.boundary else (512, 2048)):
            kv_bytes = 2 * B * H * Sk * D * 2
            nsets = int(min(8, max(2, -(-600_000_000 // kv_bytes))))
            sets = []
            for _ in range(nsets):
                q = (torch.randn(B, H, Sq, D, generator=gen) * D ** -0.5).half().to(dev)
                k = torch.randn(B, H, Sk, D, generator=gen).half().to(dev)
                v = torch.randn(B, H, Sk, D, generator=gen).half().to(dev)
                o = torch.empty(B, Sq, H, D, dtype=torch.float16, device=dev).permute(0, 2, 1, 3)
                sets.append((q, k, v, o))
            algo_bytes = kv_bytes + 2 * B * H * Sq * D * 2
            for form, spec in FORMS.items():
                d = make_desc(*sets[0], spec)
                work = torch.empty(max(int(lib.oeh_attn_decode_work_bytes(C.byref(d), s)) for s in (0, 64)) // 8 + 2, dtype=torch.int64, device=dev)
                stream = lambda: ops._stream()  # noqa: E731
                fqd = calibrated_fq(*sets[0][:3], spec) if a.fq else None
                fqp = None if fqd is None else C.byref(fqd)

                def fwd(s, d=d, fqp=fqp):
                    _lib.check(lib.oeh_attn_fwd(C.byref(d), ops._ptr(s[0]), ops._ptr(s[1]), ops._ptr(s[2]), ops._ptr(s[3]), fqp, stream()), "oeh_attn_fwd")

                def dec(s, d=d, splits=0, fqp=fqp):
                    if fqp is not None:
                        _lib.check(lib.oeh_attn_decode_fq(C.byref(d), fqp, splits, ops._ptr(s[0]), ops._ptr(s[1]), ops._ptr(s[2]), ops._ptr(s[3]), ops._ptr(work), stream()), "oeh_attn_decode_fq")
                        return
                    _lib.check(lib.oeh_attn_decode(C.byref(d), splits, ops._ptr(s[0]), ops._ptr(s[1]), ops._ptr(s[2]), ops._ptr(s[3]), ops._ptr(work), stream()), "oeh_attn_decode")

                fwd(sets[0])
                want = sets[0][3].clone()
                dec(sets[0])
                torch.cuda.synchronize()
                diff = float((sets[0][3].float() - want.float()).abs().max())
                ga, gb = timed_graph(fwd, sets, a.iters), timed_graph(dec, sets, a.iters)
                ta, tb = [], []
                for _ in range(a.reps):
                    ta.append(replay_ms(ga) * 1e3 / a.iters)
                    tb.append(replay_ms(gb) * 1e3 / a.iters)
                ua, ub = statistics.median(ta), statistics.median(tb)
                fwd_name = lib.oeh_attn_variant(C.byref(d), fqp).decode()
                dec_name = lib.oeh_attn_decode_fq_variant(C.byref(d), fqp, 0).decode()
                wa, wb = (25, 27) if a.fq else (22, 24)  # (the "/fq" names are longer; the plain mode keeps the columns of profiles/decode_bench.txt)
                line = (f"B={B:2d} Sk={Sk:4d} {form:24s} {fwd_name:{wa}s} {ua:7.2f} us [{min(ta):.2f}..{max(ta):.2f}]  {dec_name:{wb}s} {ub:7.2f} us [{min(tb):.2f}..{max(tb):.2f}]  "
                        f"speed-up {ua / ub:5.2f}x  max |diff| {diff:.1e}  ({nsets} buffer sets)")
                if fqd is not None:
                    line += f"  context step {fqd.ctx.scale:.1e}"
                if B == 16 and Sk == 2048:
                    line += f"  {algo_bytes / 1e6:.1f} MB algorithmic: {algo_bytes / (ub * 1e-6) / 1e12:.2f} TB/s = {100.0 * algo_bytes / (ub * 1e-6) / PEAK_BYTES_PER_S:.1f} % of 8 TB/s"
                print(line, flush=True)
                lines.append(line)
                if a.sweep:
                    parts = []
                    seen = set()
                    for s in (1, 2, 4, 8, 16, 32, 64):
                        name = lib.oeh_attn_decode_fq_variant(C.byref(d), fqp, s).decode()
                        if name in seen:
                            continue
                        seen.add(name)
                        gs = timed_graph(lambda st, s=s: dec(st, splits=s), sets, a.iters)
                        ts = statistics.median(replay_ms(gs) * 1e3 / a.iters for _ in range(3))
                        parts.append(f"{name.split('/')[1]} {ts:.2f}")
                        del gs
                    line = f"    sweep (us): {'  '.join(parts)}"
                    print(line, flush=True)
                    lines.append(line)
                del ga, gb
            del sets
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
