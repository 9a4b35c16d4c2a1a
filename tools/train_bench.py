#!/usr/bin/env python3
"""fwd + bwd of ONE attention core at the reference's pre-training shapes (OutEffHop_script/submit_outlier_opt.sh / submit_outlier_bert.sh:
OPT-12L12H at block_size 512, BERT-6L12H at 128), in one process, three ways:
  fused    outeffhop_amd.fused_attention (oeh_attn_fwd_train + oeh_attn_bwd: three HIP kernels, nothing S x S stored)
  torchop  attention.unfused_core under autograd with the registry softmax - the modules' differentiable path without the switch
  sdpa     torch.nn.functional.scaled_dot_product_attention (vanilla softmax only; for reference)
One JSON line per (shape, softmax, path): median us of fwd + bwd over --iters timed calls (device events, after --warmup), peak memory
beyond the inputs (torch.cuda.max_memory_allocated), and the fused path's roofline fraction:
  FLOPs = 3.5 x 4 B H Sq Sk D (the forward's two products and the backward's five), x 1/2 for causal;
  bytes = (q, k, v, o, dO in + dq, dk, dv out) = 8 B H S D x 2 bytes;
  roofline = max(FLOPs / 2500 TFLOP/s, bytes / 8 TB/s) (MI355X fp16 / bf16 dense MFMA and HBM peaks), frac = roofline / measured.

With --attn-dropout P (0 < P < 1) two more paths run attention dropout at P, as the modules do in training:
  fused_drop    fused_attention(dropout_p=P): the mask drawn inside the kernels (a fresh seed per call), still nothing S x S stored
  torchop_drop  unfused_core with nn.functional.dropout on the probabilities (the observable path's dropout)
and every row carries "attn_dropout" (0 for the paths without it).

    python tools/train_bench.py [--iters 50] [--warmup 10] [--only opt|bert] [--attn-dropout 0.1]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

PEAK_TFLOPS, PEAK_TBS = 2500.0, 8.0

SHAPES = [  # (name, B, H, S, causal, key padding, softmaxes)
    ("opt", 16, 12, 512, True, False, ("softmax1", "vanilla", "clippedsoftmax1(-.025:1)")),
    ("opt", 48, 12, 512, True, False, ("softmax1", "vanilla", "clippedsoftmax1(-.025:1)")),
    ("bert", 32, 12, 128, False, True, ("softmax1", "vanilla", "clippedsoftmax1(-.025:1)")),
]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def peak_mem(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default=None)
    ap.add_argument("--paths", default=None, help="comma list (default: fused,torchop,sdpa and, with --attn-dropout, fused_drop,torchop_drop)")
    ap.add_argument("--attn-dropout", type=float, default=0.0)
    a = ap.parse_args()
    if not 0.0 <= a.attn_dropout < 1.0:
        raise SystemExit("--attn-dropout must be in [0, 1)")
    if not torch.cuda.is_available():
        raise SystemExit("train_bench needs a GPU (there is no CPU timing of HIP kernels)")
    from outeffhop_amd import SOFTMAX_MAPPING, fused_attention
    from outeffhop_amd.attention import unfused_core
    from outeffhop_amd.softmax import spec_of

    pd = a.attn_dropout
    paths = (a.paths or ("fused,torchop,sdpa" + (",fused_drop,torchop_drop" if pd > 0 else ""))).split(",")
    dt = torch.float16
    for name, B, H, S, causal, padded, sms in SHAPES:
        if a.only and name != a.only:
            continue
        g = torch.Generator(device="cuda").manual_seed(0)
        q = (torch.randn(B, H, S, 64, generator=g, device="cuda", dtype=dt) * 0.125).requires_grad_(True)
        k, v = (torch.randn(B, H, S, 64, generator=g, device="cuda", dtype=dt).requires_grad_(True) for _ in range(2))
        do = torch.randn(B, H, S, 64, generator=g, device="cuda", dtype=dt)
        fmin = torch.finfo(dt).min
        pad = None
        if padded:
            pad = torch.zeros(B, S, device="cuda", dtype=dt)
            for b in range(B):
                pad[b, S - (b * 37) % (S // 2):] = fmin
        # the torch-op path gets the masks as HF hands them: OPT's (B,1,S,S) decoder mask, BERT's (B,1,1,S) padding
        if causal:
            am = torch.triu(torch.full((S, S), fmin, device="cuda", dtype=dt), 1)[None, None].expand(B, 1, S, S).contiguous()
        else:
            am = pad[:, None, None, :]
        flops = 3.5 * 4.0 * B * H * S * S * 64 * (0.5 if causal else 1.0)
        nbytes = 8.0 * B * H * S * 64 * 2
        roof_us = max(flops / (PEAK_TFLOPS * 1e12), nbytes / (PEAK_TBS * 1e12)) * 1e6
        for smname in sms:
            fn = SOFTMAX_MAPPING[smname]
            spec = spec_of(fn)
            up = (lambda x, dim=-1, _f=fn: _f(x.float(), dim=dim).to(dt))  # OPT's upcast branch (opt_attention.py:227-230)
            runs = {
                "fused": lambda: torch.autograd.grad(
                    fused_attention(q, k, v, softmax=spec, key_pad_mask=pad, causal=causal, clamp_min=causal), (q, k, v), do),
                "torchop": lambda: torch.autograd.grad(
                    unfused_core(q, k, v, softmax_fn=up, attention_mask=am, clamp_min=causal)[0], (q, k, v), do),
            }
            if pd > 0:
                drop = (lambda t: torch.nn.functional.dropout(t, p=pd, training=True))
                runs["fused_drop"] = lambda: torch.autograd.grad(
                    fused_attention(q, k, v, softmax=spec, key_pad_mask=pad, causal=causal, clamp_min=causal, dropout_p=pd), (q, k, v), do)
                runs["torchop_drop"] = lambda: torch.autograd.grad(
                    unfused_core(q, k, v, softmax_fn=up, attention_mask=am, clamp_min=causal, dropout=drop)[0], (q, k, v), do)
            if spec.base == 0 and not spec.clip:
                runs["sdpa"] = lambda: torch.autograd.grad(
                    torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=None if causal else am, is_causal=causal, scale=1.0),
                    (q, k, v), do)
            for path, run in runs.items():
                if path not in paths:
                    continue
                med, lo, hi = timed(run, a.iters, a.warmup)
                mem = peak_mem(run)
                rec = {"shape": name, "B": B, "H": H, "S": S, "D": 64, "causal": causal, "key_pad": padded, "softmax": smname, "path": path,
                       "dtype": "f16", "us_fwd_bwd": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1), "iters": a.iters,
                       "peak_mem_mb": round(mem / 2 ** 20, 1)}
                if pd > 0:
                    rec["attn_dropout"] = pd if path.endswith("_drop") else 0.0
                if path in ("fused", "fused_drop"):
                    rec["roofline"] = {"flops": flops, "bytes": nbytes, "bound": "mfma" if flops / (PEAK_TFLOPS * 1e12) >= nbytes / (PEAK_TBS * 1e12)
                                       else "hbm", "roofline_us": round(roof_us, 2), "frac": round(roof_us / med, 4),
                                       "tflops": round(flops / med * 1e-6, 1)}
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
