#!/usr/bin/env python3
"""Times of the fused cross-entropy (losses.causal_lm_loss / masked_lm_loss / FusedCrossEntropyLoss on oeh_xent_fwd / oeh_xent_bwd) against
the chain of torch ops the reference runs, in the same process on the same tensors.

    python tools/xent_bench.py [--out FILE] [--reps R] [--iters N]

Shapes: OPT-125m 16 x 512 x 50272 fp16 (quantized_opt.py:872-877: the shifted .contiguous() copy + CrossEntropyLoss() under fp16 autocast),
BERT 32 x 128 x 30522 fp16 with 15 % of the rows labelled (quantized_bert.py:910-915, under fp16 autocast), ViT 1024 x 1000 fp32 with
label_smoothing = 0.1, and one short row set 2 x 16 x 50272 fp16.  Per shape two lines, forward alone (under no_grad) and forward + backward
(torch.autograd.grad of the loss in the logits):
  fused   the losses.* call
  chain   the reference's lines
  bytes   what the fused call has to move - the labelled rows read once forward; read once more and every row written backward - and that
          over the fused time, beside the 6.0-6.3 TB/s a streaming kernel reaches on this part.  A whole-call rate from device events
          (launches, the reduce launch and autograd's bookkeeping included), not a kernel's share of peak from a trace.
Method: eager calls, `iters` per window, each window between two device events; chain and fused windows alternate `reps` times; the line
reports the median per-call time and the spread.  The logits of a shape are a ring of tensors of more than 600 MB in all (the last-level
cache holds 256 MB), walked call by call.  The two small shapes are bound by the host's launches in either form; they are there for the ratio a
user sees.  No tracer.  The one condition - the rule by which losses.FUSED_XENT defaults to True: forward + backward is faster than the
chain at both the OPT and the BERT shape - exit status 1 otherwise."""
import argparse
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from outeffhop_amd import _lib, losses, ops  # noqa: E402

RING_BYTES = 600_000_000
STREAM_TB_S = (6.0, 6.3)


def shapes():
    # name, logits shape, dtype, share of labelled rows, kind
    return (("OPT-125m", (16, 512, 50272), torch.float16, 1.0, "clm"),
            ("BERT", (32, 128, 30522), torch.float16, 0.15, "mlm"),
            ("ViT", (1024, 1000), torch.float32, 1.0, "vit"),
            ("short rows", (2, 16, 50272), torch.float16, 1.0, "clm"))


def chain_loss(kind, logits, labels):
    V = logits.shape[-1]
    if kind == "vit":
        return nn.CrossEntropyLoss(label_smoothing=0.1)(logits, labels)
    with torch.autocast("cuda", dtype=torch.float16):
        if kind == "clm":
            shift_logits = logits[..., :-1, :].contiguous()
            shift_labels = labels[..., 1:].contiguous()
            return nn.CrossEntropyLoss()(shift_logits.view(-1, V), shift_labels.view(-1))
        return nn.CrossEntropyLoss()(logits.view(-1, V), labels.view(-1))


_vit = losses.FusedCrossEntropyLoss(label_smoothing=0.1)


def fused_loss(kind, logits, labels):
    if kind == "vit":
        return _vit(logits, labels)
    return losses.causal_lm_loss(logits, labels) if kind == "clm" else losses.masked_lm_loss(logits, labels)


def window_ms(fn, kind, ring, labels, iters, backward, start):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        x = ring[(start + i) % len(ring)]
        if backward:
            torch.autograd.grad(fn(kind, x, labels), x)
        else:
            with torch.no_grad():
                fn(kind, x, labels)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xent_bench needs a GPU: there is no CPU timing")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"# xent_bench: {lib.oeh_build_info().decode()}",
             f"# event times of windows of {a.iters} eager calls over a ring of logits of > {RING_BYTES // 1_000_000} MB, median of {a.reps} alternating windows"
             " [min..max]; no tracer",
             "# fused: losses.causal_lm_loss / masked_lm_loss / FusedCrossEntropyLoss; chain: the reference's shifted .contiguous() + CrossEntropyLoss()"
             " under fp16 autocast (ViT: fp32, label_smoothing 0.1)"]
    verdict = {}
    for name, shape, dtype, labelled, kind in shapes():
        V = shape[-1]
        esize = torch.empty(0, dtype=dtype).element_size()
        n = 1
        for s in shape:
            n *= s
        ring = [(2.0 * torch.randn(shape, device=dev, generator=gen)).to(dtype).requires_grad_() for _ in range(max(1, min(160, -(-RING_BYTES // (n * esize)))))]
        labels = torch.randint(0, V, shape[:-1], device=dev, generator=gen)
        if labelled < 1.0:
            labels[torch.rand(shape[:-1], device=dev, generator=gen) >= labelled] = -100
        rows_all = n // V
        view = labels[..., 1:] if kind == "clm" else labels
        rows_read = int((view != -100).sum())
        # the same loss from both forms before anything is timed
        with torch.no_grad():
            lf, lc = float(fused_loss(kind, ring[0], labels)), float(chain_loss(kind, ring[0], labels))
        if not abs(lf - lc) <= 2e-3 * abs(lc):
            raise SystemExit(f"{name}: fused loss {lf} != chain loss {lc}")
        variant = ops.xent_variant(1, rows_all, V, dtype, label_smoothing=0.1 if kind == "vit" else 0.0, dx_offset=0)
        for backward in (False, True):
            for fn in (fused_loss, chain_loss):  # warm-up
                window_ms(fn, kind, ring, labels, 2, backward, 0)
            tf, tc = [], []
            for r in range(a.reps):
                tf.append(window_ms(fused_loss, kind, ring, labels, a.iters, backward, r))
                tc.append(window_ms(chain_loss, kind, ring, labels, a.iters, backward, r))
            mf, mc = statistics.median(tf), statistics.median(tc)
            nbytes = rows_read * V * esize * (2 if backward else 1) + (rows_all * V * esize if backward else 0)
            rate = nbytes / (mf * 1e-3) / 1e12
            lines.append(f"{name:<10} {' x '.join(str(s) for s in shape):>18} {str(dtype).replace('torch.', ''):<8} {'fwd + bwd' if backward else 'fwd      '}  {variant:<22}"
                         f" fused {mf * 1e3:9.1f} us [{min(tf) * 1e3:.1f}..{max(tf) * 1e3:.1f}]  chain {mc * 1e3:9.1f} us [{min(tc) * 1e3:.1f}..{max(tc) * 1e3:.1f}]"
                         f"  chain / fused {mc / mf:6.2f}x  {nbytes / 1e6:8.1f} MB  {rate:5.2f} TB/s (streaming: {STREAM_TB_S[0]}-{STREAM_TB_S[1]} TB/s)  ({len(ring)} tensors)")
            print(lines[-1], flush=True)
            if backward and name in ("OPT-125m", "BERT"):
                verdict[name] = mf < mc
        del ring
        torch.cuda.empty_cache()
    ok = all(verdict.values()) and len(verdict) == 2
    lines.append(f"# condition (fused forward + backward faster than the chain at the OPT and the BERT shape): {'met' if ok else 'NOT met'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
