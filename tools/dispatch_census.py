#!/usr/bin/env python3
"""Census of the attention dispatch: which kernel variant the library names (oeh_attn_variant / oeh_attn_variant_ex) and which
code oeh_attn_fwd / oeh_attn_fwd_ex return, over a fixed seeded grid of descriptors.  Host only - two builds of the library
(OEH_LIB=...) are compared by diffing their output; tests/test_dispatch_cpu.py replays tests/golden/dispatch_census.txt.

  dispatch_census.py [--cases N]            names: one line per case, at every diagnostic-hook setting
  dispatch_census.py --rc [--cases N]       return codes with fake pointers - ONLY on a machine without a GPU (every refusal is
                                            returned before any HIP call; a call that reaches a launcher returns -5 there)
  dispatch_census.py --golden N             N lines, hooks not enabled, names only (the committed fixture)

A line:  <case> | <results> [h<off_mask>.<mq>=<results> ...] [nohooks=<results>]
  case    = dt od B H Sq Sk D base clip causal pad full mask_min scale gate fq          (see AXES below)
  results = variant,variant_ex,variant_ex+pairs,variant_ex+reserved ("-" = no name)     names
          = per pointer layout (aligned;off by 2 bytes;stride off 16-byte rows) fwd,ex,ex+pairs,ex+reserved   --rc
  a hook setting is printed only where it differs from the defaults (0, 0).
The tool exits non-zero unless the census contains every kernel family (and, with --rc, every return code).
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 20260117
CHUNK = 5000
S_VALUES = (1, 28, 32, 33, 48, 64, 65, 111, 112, 128, 129, 192, 256, 257, 320, 384, 385, 448, 512, 513, 640, 2048)
# B, H: with ceil(Sq / 128) workgroups per head, both sides of 256 problems and of 384 / 416 / 768 workgroups
BH_VALUES = ((1, 1), (2, 4), (2, 12), (8, 12), (103, 1), (104, 1), (9, 12), (16, 12), (207, 1), (208, 1), (255, 1), (256, 1), (32, 12),
             (383, 1), (415, 1), (416, 1), (767, 1), (64, 12), (128, 12))
AXES = dict(
    dt=("f16", "bf16", "f32", "i8"),
    od=("=", "f32", "f16", "bf16", "i8"),            # o_dtype: "=" the storage type (f16 for i8)
    D=(16, 32, 64, 80, 128),
    base=(0, 1),
    clip=("0", "n", "p"),                            # off; gamma < 0; gamma > 0
    causal=(0, 1),
    pad=("0", "1", "b"),                             # key padding: none; a vector; a vector with key_pad_boolean
    full=(0, 1),
    mm=("min", "1e4"),                               # mask_min: finfo.min; exactly -1e4
    sc=("s", "d8", "d7", "s0", "dn"),                # scale 0.125; scale_div 8; 7; scale 0; scale_div -8
    gate=("0", "v", "h0", "h16", "h80", "hm", "hs"), # none; values; in-kernel with 0 / 16 / 80 units; misaligned hidden; hidden row stride 0
    fq=("0", "sp", "s", "p", "c", "sp4095", "spd", "spce", "spceb"),  # quantisers: scores / probs / ctx; probs qmax 4095; a dump pointer;
)                                                                      # ctx_emit_index after / before the gate
HOOKS = [(0, 0)] + [(1 << b, 0) for b in range(1, 12)] + [(0, 1), (0, 2)]
DT = dict(f16=0, bf16=1, f32=2, i8=3)
FIELDS = ("dt", "od", "B", "H", "Sq", "Sk", "D", "base", "clip", "causal", "pad", "full", "mm", "sc", "gate", "fq")
FAKE = 0x10000000  # fake device addresses: nothing on the host dereferences them


def draw(rng: random.Random) -> tuple:
    """One case.  The full product of the axes is ~10^12: a seeded sample, every axis drawn independently."""
    dt = rng.choice(AXES["dt"])
    od = rng.choice(("f16", "bf16", "f32", "i8") if dt == "i8" else ("=", "f32"))
    B, H = rng.choice(BH_VALUES)
    Sq = rng.choice(S_VALUES)
    Sk = Sq if rng.random() < 0.7 else rng.choice(S_VALUES)
    D = 64 if dt == "i8" and rng.random() < 0.6 else rng.choice(AXES["D"])
    pick = lambda k, p0: AXES[k][0] if rng.random() < p0 else rng.choice(AXES[k])  # noqa: E731  (the plain value more often than 1 / n)
    return (dt, od, B, H, Sq, Sk, D, rng.choice(AXES["base"]), pick("clip", 0.4), rng.choice(AXES["causal"]), pick("pad", 0.5),
            0 if rng.random() < 0.8 else 1, pick("mm", 0.7), pick("sc", 0.6), pick("gate", 0.5), pick("fq", 0.4))


def build(case: tuple, layout: int = 0):
    """(desc, fq or None, q, k, v, o) of a case; layout 0 aligned, 1 pointers off by 2 bytes, 2 a row stride that breaks 16-byte rows."""
    from outeffhop_amd._lib import oeh_attn_desc, oeh_fq_desc

    dt, od, B, H, Sq, Sk, D, base, clip, causal, pad, full, mm, sc, gate, fq = case
    d = oeh_attn_desc()
    d.B, d.H, d.Sq, d.Sk, d.D, d.dtype = B, H, Sq, Sk, D, DT[dt]
    d.o_dtype = DT["f16" if dt == "i8" else dt] if od == "=" else DT[od]
    row = D + 1 if layout == 2 else D
    for st, S in ((d.q_stride, Sq), (d.k_stride, Sk), (d.v_stride, Sk), (d.o_stride, Sq)):
        st[0], st[1], st[2] = H * S * row, S * row, row
    d.scale, d.scale_div = {"s": (0.125, 0.0), "d8": (1.0, 8.0), "d7": (1.0, 7.0), "s0": (0.0, 0.0), "dn": (1.0, -8.0)}[sc]
    d.softmax_base, d.causal = base, causal
    if clip != "0":
        d.clip, d.gamma, d.eta = 1, (-0.025 if clip == "n" else 0.01), 1.0
    d.mask_min = -3.4028234663852886e38 if mm == "min" else -1.0e4
    if pad != "0":
        d.key_pad_mask, d.key_pad_dtype, d.key_pad_stride, d.key_pad_boolean = FAKE, 2, Sk, int(pad == "b")
    if full:
        d.full_mask, d.full_mask_dtype = FAKE, 2
        d.full_mask_stride[0], d.full_mask_stride[1] = Sq * Sk, Sk
    if gate == "v":
        d.gate = FAKE
        d.gate_stride[0], d.gate_stride[1], d.gate_stride[2] = H * Sq, Sq, 1
    elif gate != "0":
        d.gate_hidden = FAKE + (2 if gate == "hm" else 0)
        d.gate_hidden_stride[0], d.gate_hidden_stride[1] = Sq * 768, (0 if gate == "hs" else 768)
        d.gate_units = {"h0": 0, "h80": 80}.get(gate, 16)
        d.gate_w1 = d.gate_b1 = FAKE
        if d.gate_units:
            d.gate_w2 = d.gate_b2 = FAKE
        d.gate_scaling = 1.0
    if dt == "i8":
        for g, zp in ((d.q_grid, 128.0), (d.k_grid, 117.0), (d.v_grid, 0.0)):
            g.scale, g.zero_point = 0.05, zp
    f = None
    if fq != "0":
        f = oeh_fq_desc()
        on = dict(s=fq.startswith("s"), p="p" in fq[:2], c=fq in ("c", "spce", "spceb"))
        for q_, key in ((f.scores, "s"), (f.probs, "p"), (f.ctx, "c")):
            if on[key]:
                q_.enable, q_.scale, q_.zero_point, q_.qmax = 1, 0.1, (3.0 if key != "p" else 0.0), 255.0
        if fq == "sp4095":
            f.probs.qmax = 4095.0
        if fq == "spd":
            f.scores.dump_idx = FAKE
        if fq in ("spce", "spceb"):
            f.ctx_emit_index, f.ctx_quant_before_gate = 1, int(fq == "spceb")
    p = FAKE + (2 if layout == 1 else 0)
    return d, f, p, p + 0x1000000, p + 0x2000000, p + 0x3000000


def fmt_case(case: tuple) -> str:
    return " ".join(str(x) for x in case)


def parse_case(text: str) -> tuple:
    w = text.split()
    return tuple(int(x) if k in ("B", "H", "Sq", "Sk", "D", "base", "causal", "full") else x for k, x in zip(FIELDS, w))


def _opts(pairs: int, reserved: int):
    from outeffhop_amd._lib import oeh_attn_opts

    o = oeh_attn_opts(pv_pairs=pairs)
    o.reserved[1] = reserved
    return C.byref(o)


def names(lib, case: tuple) -> str:
    d, f, *_ = build(case)
    dp, fp = C.byref(d), (None if f is None else C.byref(f))
    r = [lib.oeh_attn_variant(dp, fp), lib.oeh_attn_variant_ex(dp, _opts(0, 0), fp), lib.oeh_attn_variant_ex(dp, _opts(1, 0), fp),
         lib.oeh_attn_variant_ex(dp, _opts(0, 7), fp)]
    return ",".join("-" if x is None else x.decode() for x in r)


def codes(lib, case: tuple) -> str:
    out = []
    for layout in range(3):
        d, f, q, k, v, o = build(case, layout)
        dp, fp = C.byref(d), (None if f is None else C.byref(f))
        r = [lib.oeh_attn_fwd(dp, q, k, v, o, fp, None)]
        r += [lib.oeh_attn_fwd_ex(dp, _opts(pv, res), q, k, v, o, fp, None) for pv, res in ((0, 0), (1, 0), (0, 7))]
        out.append(",".join(str(x) for x in r))
    return ";".join(out)


def reset_hooks(lib) -> int:
    """The hooks at their defaults: 0, or -95 where they are not enabled (include/oeh_debug.h)."""
    lib.oeh_debug_set_variant.argtypes = [C.c_int, C.c_int]
    lib.oeh_debug_set_variant.restype = C.c_int
    return lib.oeh_debug_set_variant(0, 0)


def _load(hooks: bool):
    if hooks:
        os.environ["OEH_DEBUG_HOOKS"] = "1"
    else:
        os.environ.pop("OEH_DEBUG_HOOKS", None)
    from outeffhop_amd import _lib

    lib = _lib.load()
    if reset_hooks(lib) != (0 if hooks else -95):
        raise SystemExit("dispatch_census: the diagnostic hooks are not in the state this pass needs")
    return lib


def _chunk(job) -> tuple:
    """Worker: the lines of one chunk of cases, with the hooks enabled or not (one process serves one of the two)."""
    index, n, rc, hooks = job
    lib = _load(hooks)
    rng = random.Random(SEED * 1000003 + index)
    fn = codes if rc else names
    lines, seen = [], set()
    for _ in range(n):
        case = draw(rng)
        if hooks:
            base = fn(lib, case)
            parts = [base]
            seen.add(base)
            for off, mq in HOOKS[1:]:
                lib.oeh_debug_set_variant(off, mq)
                r = fn(lib, case)
                if r != base:
                    parts.append(f"h{off}.{mq}={r}")
                    seen.add(r)
            lib.oeh_debug_set_variant(0, 0)
            lines.append(f"{fmt_case(case)} | {' '.join(parts)}")
        else:
            r = fn(lib, case)
            seen.add(r)
            lines.append(f"{fmt_case(case)} | nohooks={r}")
    return "\n".join(lines), seen


def missing_families(results: set, rc: bool) -> list:
    """What the issue's coverage condition still lacks in a set of result strings."""
    if rc:
        have = {c for r in results for lay in r.split(";") for c in lay.split(",")}
        return [c for c in ("-22", "-95", "-14", "-5") if c not in have]
    have = {n for r in results for n in r.split(",")}
    want = {"no name": lambda n: n == "-", "generic": lambda n: n == "generic", "mfma16": lambda n: n.startswith("mfma16/") and "/fq" not in n,
            "mfma16/fq": lambda n: n.startswith("mfma16/") and n.endswith("/fq")}
    for st in (2, 4):
        want[f"small/ST{st}"] = lambda n, st=st: n.startswith(f"small/ST{st}/")
    for o in ("f16", "bf16", "f32", "i8"):
        want[f"i8mfma/{o}"] = lambda n, o=o: n.startswith("i8mfma/") and n.endswith("/" + o)
    for mq in (1, 2):
        p = f"flash16/MQ{mq}/"
        want[p + "plain"] = lambda n, p=p: n.startswith(p) and n.count("/") == 3 and "+" not in n
        for s in ("/fq2p", "/clip2p", "+pv2"):
            want[p + s] = lambda n, p=p, s=s: n.startswith(p) and s in n
    for nt in (8, 16, 32):
        p = f"fast16/NT{nt}/"
        want[p + "plain"] = lambda n, p=p: n.startswith(p) and n.count("/") == 3 and "+" not in n
        for s in ("/clip", "/fq", "+pv2"):
            want[p + s] = lambda n, p=p, s=s: n.startswith(p) and s in n
    return [k for k, ok in want.items() if not any(ok(n) for n in have)]


def golden_lines(n: int) -> list:
    """n lines with the hooks not enabled, spread evenly over the distinct results of the first chunks of the census."""
    lib = _load(False)
    groups = {}
    for index in range(40):
        rng = random.Random(SEED * 1000003 + index)
        for _ in range(CHUNK):
            case = draw(rng)
            groups.setdefault(names(lib, case), []).append(case)
    out = []
    depth = 0
    while len(out) < n:
        row = [(r, g[depth]) for r, g in sorted(groups.items()) if depth < len(g)]
        if not row:
            break
        out += [f"{fmt_case(c)} | {r}" for r, c in row[: n - len(out)]]
        depth += 1
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", type=int, default=2_000_000, help="cases per hook setting (seeded sample of the grid)")
    ap.add_argument("--rc", action="store_true", help="return codes of oeh_attn_fwd[_ex] with fake pointers (no GPU in the machine)")
    ap.add_argument("--golden", type=int, default=0, metavar="N", help="print N fixture lines (names, hooks not enabled)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    if a.rc:
        import torch

        if torch.cuda.device_count() > 0:
            raise SystemExit("dispatch_census --rc passes fake pointers to oeh_attn_fwd: only on a machine without a GPU")
    if a.golden:
        lines = golden_lines(a.golden)
        print("\n".join(lines))
        lack = missing_families({ln.split(" | ")[1] for ln in lines}, False)
        if lack:
            print("dispatch_census: the fixture lacks " + ", ".join(lack), file=sys.stderr)
        return 1 if lack else 0
    import multiprocessing as mp

    chunks = [(i, min(CHUNK, a.cases - i * CHUNK)) for i in range((a.cases + CHUNK - 1) // CHUNK)]
    seen = set()
    for hooks in (True, False):  # the hooks are read once per process: one pool of fresh processes each
        with mp.get_context("spawn").Pool(a.jobs) as pool:
            for text, s in pool.imap(_chunk, [(i, n, a.rc, hooks) for i, n in chunks]):
                print(text)
                seen |= s
    distinct = {n for r in seen for lay in r.split(";") for n in lay.split(",")}
    print(f"dispatch_census: {a.cases} cases x {len(HOOKS)} hook settings + 1 pass without hooks, {len(distinct)} distinct "
          f"{'codes' if a.rc else 'names'}", file=sys.stderr)
    lack = missing_families(seen, a.rc)
    if lack:
        print("dispatch_census: the grid lacks " + ", ".join(lack), file=sys.stderr)
    return 1 if lack else 0


if __name__ == "__main__":
    sys.exit(main())
