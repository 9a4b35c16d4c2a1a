#!/usr/bin/env python3
"""Same-process A/B (GPU box) of the fp32-storage attention with and without the probability pairs (include/oeh.h: oeh_attn_opts.pv_pairs):
blocks of launches alternate between the two forms on the same inputs (rotated over enough buffer sets to exceed the 256 MiB Infinity
Cache); the median of each form's block means is printed, one line per shape.
    python tools/pv_pairs_bench.py [--iters 200] [--blocks 12]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from outeffhop_amd import ops

FMIN = float(np.finfo(np.float32).min)
SHAPES = [  # name, B, H, S, options
    ("OPT-125m fp32 softmax1", 16, 12, 512, dict(softmax=ops.SoftmaxSpec(1, False, 0.0, 1.0), causal=True, clamp_min=True, mask_min=FMIN)),
    ("OPT-125m fp32 clippedsoftmax1", 16, 12, 512, dict(softmax=ops.SoftmaxSpec(1, True, -0.025, 1.1), causal=True, clamp_min=True, mask_min=FMIN)),
    ("BERT-base fp32 softmax1 key padding", 32, 12, 128, dict(softmax=ops.SoftmaxSpec(1, False, 0.0, 1.0), scale_div=8.0, mask_min=FMIN, pad=True)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=12)
    a = ap.parse_args()
    D = 64
    for name, B, H, S, kw in SHAPES:
        kw = dict(kw)
        g = torch.Generator(device="cuda").manual_seed(0)
        nsets = max(2, min(32, int(700e6 // (3 * B * H * S * D * 4)) + 1))
        if kw.pop("pad", False):
            pad = torch.zeros(B, S, device="cuda")
            for b, n in enumerate(torch.randint(S // 2, S + 1, (B,), generator=torch.Generator().manual_seed(1)).tolist()):
                pad[b, n:] = FMIN
            kw["key_pad_mask"] = pad
        calls = {False: [], True: []}
        for _ in range(nsets):
            q, k, v = (torch.randn(B, S, H, D, device="cuda", generator=g).permute(0, 2, 1, 3) for _ in range(3))
            for pv in (False, True):
                calls[pv].append(ops.PreparedAttn(q * D ** -0.5, k, v, pv_pairs=pv, **kw))
        var = {pv: ops.attn_variant(B, H, S, S, D, torch.float32, clip=kw["softmax"].clip, causal=kw.get("causal", False),
                                    key_pad="key_pad_mask" in kw, scale_div=kw.get("scale_div", 0.0), pv_pairs=pv) for pv in (False, True)}
        times = {False: [], True: []}
        for blk in range(a.blocks + 1):
            for pv in ((False, True) if blk % 2 == 0 else (True, False)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                cs = calls[pv]
                e0.record()
                for i in range(a.iters):
                    cs[i % len(cs)]()
                e1.record()
                torch.cuda.synchronize()
                if blk > 0:   # (block 0: warm-up)
                    times[pv].append(e0.elapsed_time(e1) * 1e3 / a.iters)
        t0, t1 = statistics.median(times[False]), statistics.median(times[True])
        print(f"{name:38s} B={B} H={H} S={S}: {var[False]} {t0:7.2f} us | {var[True]} {t1:7.2f} us | x{t1 / t0:.3f}", flush=True)


if __name__ == "__main__":
    main()
