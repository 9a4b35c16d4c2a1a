"""The INT8-storage attention kernel (csrc/oeh_attn_i8.hip) instance by instance: the compiled instances, a staged model of what one launch
computes, and the registry of cases that launches every instance.  numpy and ctypes only; tests/test_attn_i8_instances_cpu.py checks the
registry and the model's power without a GPU, tests/test_attn_i8_instances_gpu.py runs it.

An instance key names one compiled kernel: ("i8", NT, OUT, DUMP, CQ2, PAD) of oeh_attn_i8_kernel<NT, OUT, DUMP, CQ2, PAD>, OUT 0 fp16,
1 bf16, 2 fp32, 3 int8 (the context quantiser's centred indices).  `instance_from` takes the variant name the library gives
(i8mfma/NT%d/D64/<out>) and restates only what launch_i8_nt / launch_i8_variant read beyond it: any dump pointer -> DUMP, a q grid with zero
point 0 -> CQ2, a padding vector -> PAD.

The model is written from include/oeh.h and the kernel's header comment, in three stages, each computed from the KERNEL'S dump of the stage
before, so that an error is pinned to the stage that made it:
  1. scores, exact: S = sum_d (iq - zq)(ik - zk) is an integer below 2^23; the index is clip(rint(S k1), -zs, 255 - zs) + zs on the exact
     product of the integer and the fp32 constant k1 (exact in float64), ties to even.  k1 as the host forms it (oeh_api.hip).
  2. probabilities, float64 with a tie band: x = scale_s rel, the softmax over the visible keys, the optional clip, the index
     clip(rint(p / scale_p + zp_p), 0, 255).  A kernel's index must equal the model's wherever p / scale_p + zp_p is further than
     4 ERR64 / scale_p from a half-integer, and be at most one step away inside that band.  ERR64 is the fp32 oracle's own largest distance
     from float64 on the probabilities of all cases (`err64`; tests/test_attn_i8_instances_cpu.py holds it to its range and to the per-case
     figures, the GPU test uses the same number).
  3. context, exact: O = sum_k (iv - zv)(ip - zp_p) is an integer; then single correctly rounded fp32 operations - int -> float, x so, the
     IEEE quotient by the context step, rint, clamp, the gate multiply, x scale - restated in numpy fp32.  Bit for bit, the sign of zero
     included: the reference's (idx - zp) * scale is never -0.
(S and O are formed by float64 matrix products: every partial sum is an integer below 2^53, so they are the exact integers.)"""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000000  # a fake device address: nothing on the host dereferences it
F32, F64 = np.float32, np.float64
FMIN32 = float(np.finfo(np.float32).min)
FMIN16 = float(np.finfo(np.float16).min)
OUTS = {"f16": 0, "bf16": 1, "f32": 2, "i8": 3}
FORMS = ("dump", "f32", "f16", "bf16", "i8")  # the five output forms every problem fans out over: oeh_attn_i8_kernel<., OUT, DUMP, ., .>
D = 64

# ERR64, the ruler of stage 2: `err64()` below - the fp32 oracle's largest distance from float64 on the probabilities of the registry's cases, computed
# once per process from the oracle itself (2.56e-7 where this was written), never from a kernel.
BAND = 4.0          # four times the reference's own rounding
BAND_SHARE = 1e-3   # at most this share of a case's probability indices may lie inside the band


# ---- what the library was built with --------------------------------------------------------------------------------------------------
def targs(name: str):
    """The integer template arguments of a mangled kernel name (tools/instantiations.py: targs)."""
    return [int(x) for x in re.findall(r"L[ib](-?\d+)E", name.replace("Ln", "L-"))]


_BUILT = None


def built_instances():
    """The instantiations of oeh_attn_i8_kernel in the built liboeh_hip.so, from the code object's kernel names (tools/kernel_resources.py)."""
    global _BUILT
    if _BUILT is None:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "oeh_attn_i8_kernel"], capture_output=True, text=True,
                             check=True).stdout
        found = set()
        for line in out.splitlines():
            if "oeh_attn_i8_kernelI" in line:
                a = targs(line.split()[0])
                assert len(a) == 5, line
                found.add(("i8",) + tuple(a))
        assert found, "no INT8-storage attention kernel in the built library"
        _BUILT = frozenset(found)
    return _BUILT


def instance_from(name: str, d, f):
    """The instance key of the launch the library names `name` for descriptor d / f."""
    fam, nt, dim, out = name.split("/")
    assert fam == "i8mfma" and dim == "D64", name
    dump = bool(f.scores.dump_idx) or bool(f.probs.dump_idx) or bool(f.ctx.dump_idx)  # launch_i8_nt
    return ("i8", int(nt[2:]), OUTS[out], int(dump), int(d.q_grid.zero_point == 0.0), int(bool(d.key_pad_mask)))  # launch_i8_variant


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        from outeffhop_amd import _lib as L

        _LIB = L.load()
    return _LIB


def form_case(c, form):
    """The case a form of problem c runs: the int8 form writes the context quantiser's integers, so it needs that quantiser, as the last
    operation (after the gate where there is one) - `emit_case`; the others run c itself."""
    return emit_case(c) if form == "i8" else c


def emit_case(c):
    return dict(c, emit=True, gc=c["gc"] or (0.03, 126.0), before=c["before"] and c["gate"] is None)


def descriptor(c, form):
    """(oeh_attn_desc, oeh_fq_desc) of a form of a case with fake pointers: what decides the kernel."""
    from outeffhop_amd._lib import OEH_F16, OEH_BF16, OEH_F32, OEH_I8, oeh_attn_desc, oeh_fq_desc

    c = form_case(c, form)
    g = grids(c)
    d = oeh_attn_desc()
    d.B, d.H, d.Sq, d.Sk, d.D, d.dtype = c["B"], c["H"], c["Sq"], c["Sk"], D, OEH_I8
    d.o_dtype = {"dump": OEH_F32, "f32": OEH_F32, "f16": OEH_F16, "bf16": OEH_BF16, "i8": OEH_I8}[form]
    H, Sq, Sk, cache = c["H"], c["Sq"], c["Sk"], c["cache"]
    if c["layout"] == "bshe":
        qs, ks = (Sq * H * D, D, H * D), ((Sk + cache) * H * D, D, H * D)
    else:
        qs, ks = (H * Sq * D, Sq * D, D), (H * (Sk + cache) * D, (Sk + cache) * D, D)
    vs = (H * D * (Sk + cache), D * (Sk + cache), Sk + cache)
    for st, s in zip((d.q_stride, d.k_stride, d.v_stride, d.o_stride), (qs, ks, vs, ((Sq + 2 * c["guard"]) * H * D, D, H * D))):
        st[0], st[1], st[2] = s
    d.scale, d.scale_div = c["scale"], c["scale_div"]
    d.softmax_base, d.causal, d.clamp_min, d.mask_min = c["base"], int(c["causal"]), 1, FMIN32
    if c["clip"] is not None:
        d.clip, d.gamma, d.eta = 1, c["clip"][0], c["clip"][1]
    if c["pad"] is not None:
        d.key_pad_mask, d.key_pad_dtype, d.key_pad_stride, d.key_pad_boolean = FAKE, (OEH_F16 if c["pad"][0] == "f16" else OEH_F32), Sk, 1
    if c["gate"] is not None:
        d.gate = FAKE
        d.gate_stride[0], d.gate_stride[1], d.gate_stride[2] = (H * Sq, Sq, 1) if c["gate"] == "token" else (0, 1, 0)
    for name in ("q", "k", "v"):
        getattr(d, name + "_grid").scale, getattr(d, name + "_grid").zero_point = g[name]
    f = oeh_fq_desc()
    for q_, key in ((f.scores, "s"), (f.probs, "p"), (f.ctx, "c")):
        if g[key] is not None:
            q_.enable, q_.scale, q_.zero_point, q_.qmax = 1, g[key][0], g[key][1], 255.0
            if form == "dump":
                q_.dump_idx = FAKE
    f.ctx_quant_before_gate, f.ctx_emit_index = int(c["before"]), int(c["emit"])
    return d, f


def variant_name(c, form):
    d, f = descriptor(c, form)
    n = _lib().oeh_attn_variant_ex(C.byref(d), None, C.byref(f))
    return None if n is None else n.decode()


def instance_of(c, form):
    name = variant_name(c, form)
    assert name is not None, (c["name"], form, "the library names no kernel")
    return instance_from(name, *descriptor(c, form))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _p(name, B, H, Sq, Sk, **kw):
    """One problem.  layout: "bshe" - q / k (B,H,S,64) views of (B,S,H*64) storage, "bhsd" - contiguous; cache: keys of random bytes behind
    the Sk keys of k and v_t (slices of longer caches); guard: a row of fill on either side of the output's rows; zq / zk / zv / zs / zpp:
    zero points of q, k, v, the scores and the probabilities; tie: k1 is exactly 2^-7 (all steps powers of two); pad: (dtype, [per sample
    (kind, n, value)]) with kind "none" | "right" (keys >= n hidden) | "left" (keys < n hidden) | "full"; gate: None | "token" | "head";
    gc: the context grid (step, zero point) or None; before: context quantiser before the gate; emit: ctx_emit_index."""
    c = dict(name=name, B=B, H=H, Sq=Sq, Sk=Sk, layout="bshe", cache=0, guard=0, zq=128.0, zk=128.0, zv=128.0, zs=128.0, zpp=0.0, tie=False, base=1,
             clip=None, scale=0.125, scale_div=0.0, causal=False, pad=None, gate=None, gc=(0.03, 126.0), before=True, emit=False)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    c["seed"] = 7000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    if c["pad"] is not None:
        assert len(c["pad"][1]) == B
    assert Sk % 16 == 0 and Sk <= 512 and (not c["causal"] or Sq <= Sk) and c["cache"] % 16 == 0
    return c


CLIP_A, CLIP_B = (-0.025, 1.0), (-0.003, 1.003)
DIV = 7.3   # a divisor that is no power of two


def _pad(dt, *rows):
    return (dt, list(rows))


def _problems():
    """Two or three problems per (NT, CQ2, PAD) group.  In every group: a case whose k1 is exactly 2^-7 (exact ties S k1 = n + 1/2), a causal
    one and a non-causal one, softmax_1 and vanilla, a clipped one, `scale` and `scale_div`, a gate with the context quantiser before it and
    one with the quantiser after it, a probability grid with zero point 7, k / v zero points off 128, a cache tail; in every PAD group a
    padding vector alone and on top of the causal mask, fp32 and fp16, finfo.min and exactly -1e4, right / left / whole-tile / full padding."""
    R, L, F, N = "right", "left", "full", "none"
    out = [
        # ---- NT 8: 16, 48, 80, 128 keys
        _p("nt8-a", 1, 6, 128, 128, tie=True, causal=True, gate="token", zq=255.0, zk=97.0, zv=0.0, cache=48),
        _p("nt8-b", 1, 1, 77, 16, base=0, clip=CLIP_B, scale_div=DIV, gate="head", before=False, zpp=7.0, zq=97.0, zk=140.0, zv=255.0, zs=100.0, layout="bhsd", guard=1),
        _p("nt8-c", 2, 3, 33, 80, causal=True, base=0, gc=None, zq=128.0, zk=0.0, zv=128.0, zs=140.0, cache=16, layout="bhsd"),
        _p("nt8-cq2-a", 1, 17, 100, 128, tie=True, causal=True, gate="token", zq=0.0, zk=131.0, zv=97.0, cache=16),
        _p("nt8-cq2-b", 2, 3, 77, 48, base=1, clip=CLIP_A, scale_div=8.0, gate="head", before=False, zpp=7.0, zq=0.0, zk=128.0, zv=255.0, zs=100.0, layout="bhsd", guard=1),
        _p("nt8-pad-a", 3, 2, 128, 128, tie=True, causal=True, gate="token", zq=97.0, zk=120.0, zv=0.0, cache=16,
           pad=_pad("f16", (R, 64, FMIN16), (L, 37, -1.0e4), (F, 0, FMIN16))),
        _p("nt8-pad-b", 3, 2, 77, 80, base=0, clip=CLIP_B, scale_div=DIV, gate="head", before=False, zpp=7.0, zq=255.0, zk=128.0, zv=160.0, zs=140.0, layout="bhsd",
           guard=1, pad=_pad("f32", (R, 51, -1.0e4), (F, 0, FMIN32), (N, 0, 0.0))),
        _p("nt8-cq2-pad-a", 2, 3, 90, 128, tie=True, causal=True, gate="token", zq=0.0, zk=97.0, zv=120.0, cache=32, pad=_pad("f16", (L, 50, FMIN16), (R, 100, -1.0e4))),
        _p("nt8-cq2-pad-b", 3, 1, 20, 48, base=0, clip=CLIP_A, scale_div=8.0, gate="head", before=False, zpp=7.0, zq=0.0, zk=140.0, zv=255.0, zs=100.0, layout="bhsd",
           guard=1, pad=_pad("f32", (R, 17, -1.0e4), (F, 0, FMIN32), (L, 5, FMIN32))),
        # ---- NT 16: 144, 208, 256 keys
        _p("nt16-a", 2, 3, 256, 256, tie=True, causal=True, gate="token", zq=97.0, zk=255.0, zv=120.0, cache=16),
        _p("nt16-b", 1, 6, 77, 144, base=0, clip=CLIP_A, scale_div=DIV, gate="head", before=False, zpp=7.0, zq=128.0, zk=97.0, zv=0.0, zs=140.0, layout="bhsd", guard=1),
        _p("nt16-cq2-a", 1, 6, 150, 208, tie=True, causal=True, gate="token", zq=0.0, zk=120.0, zv=255.0, cache=48, layout="bhsd"),
        _p("nt16-cq2-b", 1, 17, 77, 256, base=1, clip=CLIP_B, scale_div=8.0, gate="head", before=False, zpp=7.0, zq=0.0, zk=131.0, zv=97.0, zs=100.0, guard=1),
        _p("nt16-pad-a", 3, 2, 208, 208, tie=True, causal=True, gate="token", zq=255.0, zk=97.0, zv=131.0, cache=16,
           pad=_pad("f16", (R, 128, FMIN16), (L, 70, FMIN16), (F, 0, -1.0e4))),
        _p("nt16-pad-b", 3, 2, 77, 144, base=0, clip=CLIP_A, scale_div=DIV, gate="head", before=False, zpp=7.0, zq=97.0, zk=0.0, zv=255.0, zs=100.0, layout="bhsd", guard=1,
           pad=_pad("f32", (R, 101, -1.0e4), (F, 0, FMIN32), (L, 64, FMIN32))),
        _p("nt16-cq2-pad-a", 2, 3, 200, 256, tie=True, causal=True, gate="token", zq=0.0, zk=140.0, zv=0.0, cache=16, layout="bhsd",
           pad=_pad("f16", (R, 192, FMIN16), (L, 100, -1.0e4))),
        _p("nt16-cq2-pad-b", 3, 1, 77, 208, base=0, clip=CLIP_B, scale_div=8.0, gate="head", before=False, zpp=7.0, zq=0.0, zk=97.0, zv=120.0, zs=140.0, guard=1,
           pad=_pad("f32", (R, 150, -1.0e4), (F, 0, FMIN32), (N, 0, 0.0))),
        # ---- NT 32: 272, 384, 400, 464, 512 keys.  384: n_kt == R; 400, 464: n_kt > R with a ragged last tile; Sq = Sk = 512: n_kt 1 ... 8
        _p("nt32-a", 1, 2, 512, 512, tie=True, causal=True, gate="token", zq=255.0, zk=120.0, zv=97.0),
        _p("nt32-b", 1, 6, 77, 400, base=0, clip=CLIP_B, scale_div=DIV, gate="head", before=False, zpp=7.0, zq=97.0, zk=131.0, zv=255.0, zs=100.0, layout="bhsd", guard=1,
           cache=48),
        _p("nt32-c", 2, 1, 300, 464, causal=True, base=0, gc=None, zq=128.0, zk=255.0, zv=0.0, zs=140.0, cache=16),
        _p("nt32-cq2-a", 1, 3, 400, 464, tie=True, causal=True, gate="token", zq=0.0, zk=97.0, zv=131.0, cache=16, layout="bhsd"),
        _p("nt32-cq2-b", 1, 6, 77, 384, base=1, clip=CLIP_A, scale_div=8.0, gate="head", before=False, zpp=7.0, zq=0.0, zk=120.0, zv=0.0, zs=140.0, guard=1),
        _p("nt32-cq2-c", 1, 2, 130, 272, base=1, gc=None, zq=0.0, zk=140.0, zv=255.0, zs=100.0, cache=32),
        _p("nt32-pad-a", 3, 1, 400, 400, tie=True, causal=True, gate="token", zq=97.0, zk=255.0, zv=120.0, cache=16,
           pad=_pad("f16", (R, 320, FMIN16), (L, 129, -1.0e4), (F, 0, FMIN16))),
        _p("nt32-pad-b", 3, 2, 77, 512, base=0, clip=CLIP_B, scale_div=DIV, gate="head", before=False, zpp=7.0, zq=255.0, zk=97.0, zv=0.0, zs=140.0, layout="bhsd", guard=1,
           pad=_pad("f32", (R, 448, -1.0e4), (F, 0, FMIN32), (L, 64, FMIN32))),
        _p("nt32-pad-c", 2, 2, 140, 272, causal=True, base=0, gc=(0.03, 121.0), zq=128.0, zk=0.0, zv=255.0, zs=100.0, pad=_pad("f32", (R, 260, -1.0e4), (L, 140, FMIN32))),
        _p("nt32-cq2-pad-a", 2, 1, 512, 512, tie=True, causal=True, gate="token", zq=0.0, zk=131.0, zv=255.0, pad=_pad("f32", (R, 450, -1.0e4), (L, 64, FMIN32))),
        _p("nt32-cq2-pad-b", 3, 2, 77, 464, base=0, clip=CLIP_A, scale_div=8.0, gate="head", before=False, zpp=7.0, zq=0.0, zk=120.0, zv=97.0, zs=100.0, layout="bhsd", guard=1,
           cache=16, pad=_pad("f32", (R, 401, -1.0e4), (F, 0, FMIN32), (N, 0, 0.0))),
        _p("nt32-cq2-pad-c", 1, 3, 384, 384, causal=True, base=1, emit=True, zq=0.0, zk=128.0, zv=140.0, zs=128.0, pad=_pad("f16", (R, 300, FMIN16))),
    ]
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


CASES = _problems()
GROUPS = tuple((nt, cq2, pad) for nt in (8, 16, 32) for cq2 in (0, 1) for pad in (0, 1))
GROUP_IDS = tuple(f"NT{nt}{'-cq2' if cq2 else ''}{'-pad' if pad else ''}" for nt, cq2, pad in GROUPS)


def group_of(c):
    return (8 if c["Sk"] <= 128 else (16 if c["Sk"] <= 256 else 32), int(c["zq"] == 0.0), int(c["pad"] is not None))


_BY_INSTANCE = None


def by_instance():
    """{instance key: [(case, form)]} over CASES x FORMS."""
    global _BY_INSTANCE
    if _BY_INSTANCE is None:
        t = {}
        for c in CASES:
            for form in FORMS:
                t.setdefault(instance_of(c, form), []).append((c, form))
        _BY_INSTANCE = t
    return _BY_INSTANCE


# ---- a case's inputs and constants ----------------------------------------------------------------------------------------------------
def _indices(rng, shape, zp, amp):
    """uint8 indices around the zero point with per-row amplitude amp (rows, 1): two-sided, or one-sided where the zero point is an end of the
    range; 2 % of the entries anywhere in 0 ... 255 (the ends of the signed bytes included)."""
    n = rng.standard_normal(shape) * amp
    if zp == 0.0:
        n = np.abs(n)
    elif zp == 255.0:
        n = -np.abs(n)
    idx = np.clip(np.rint(zp + n), 0, 255)
    anywhere = rng.random(shape) < 0.02
    return np.where(anywhere, rng.integers(0, 256, shape), idx).astype(np.uint8)


def k1_of(sq, sk, ss, scale, scale_div):
    """oeh_api.hip: (float)((double)sq * (double)sk * mult / (double)ss), mult = scale or 1 / (double)scale_div, on the fp32 values."""
    mult = 1.0 / F64(F32(scale_div)) if scale_div != 0.0 else F64(F32(scale))
    return F32(F64(F32(sq)) * F64(F32(sk)) * mult / F64(F32(ss)))


def so_of(sp, sv):
    return F32(F64(F32(sp)) * F64(F32(sv)))


SAT_TARGET = 0.045


@functools.lru_cache(maxsize=None)
def _prep(name):
    c = next(c for c in CASES if c["name"] == name)
    rng = np.random.default_rng(c["seed"])
    B, H, Sq, Sk, cache = c["B"], c["H"], c["Sq"], c["Sk"], c["cache"]
    big = rng.random((B, H, Sq, 1)) < 0.25   # a quarter of the query rows with three times the amplitude: both ends of the score grid saturate
    qi = _indices(rng, (B, H, Sq, D), c["zq"], np.where(big, 36.0, 12.0))
    ki = _indices(rng, (B, H, Sk + cache, D), c["zk"], 34.0 if c["tie"] else 36.0)   # (k1 is given in a tie case: the amplitude sets the saturated share)
    vi = rng.integers(0, 256, (B, H, Sk + cache, D)).astype(np.uint8)
    S = np.matmul(qi.astype(F64) - c["zq"], np.swapaxes(ki[:, :, :Sk].astype(F64) - c["zk"], -1, -2))
    S_tail = None if not cache else np.matmul(qi.astype(F64) - c["zq"], np.swapaxes(ki[:, :, Sk:Sk + 1].astype(F64) - c["zk"], -1, -2))
    assert np.abs(S).max() < 2 ** 23
    zs = c["zs"]
    sv = 0.035
    if c["tie"]:
        sq, sk, ss = 2.0 ** -5, 2.0 ** -5, 2.0 ** -6
        assert c["scale"] == 0.125 and c["scale_div"] == 0.0
    else:
        lo_k, hi_k = 1e-6, 1.0   # the k1 at which SAT_TARGET of the scores saturate at the fuller end of the grid

        def sat(k1):
            return max(float((S * k1 < -zs - 0.5).mean()), float((S * k1 > 255.0 - zs + 0.5).mean()))
        for _ in range(40):
            mid = (lo_k * hi_k) ** 0.5
            lo_k, hi_k = (mid, hi_k) if sat(mid) < SAT_TARGET else (lo_k, mid)
        # q and k steps that are powers of two: the fp32 oracle's products and sums are then exact too, and it differs from the model in the scores by
        # the roundings of its two divisions alone; the score step carries k1's odd significand (0.06 or so: rows from flat to peaked)
        mult = 1.0 / c["scale_div"] if c["scale_div"] != 0.0 else c["scale"]
        sq, sk = 2.0 ** -4, 2.0 ** -4
        ss = float(F32(sq * sk * mult / hi_k))
    k1 = k1_of(sq, sk, ss, c["scale"], c["scale_div"])
    assert np.abs(S * F64(k1)).max() < 2 ** 22   # the magic-number rounding's range (oeh_common.h: grid_rel_m)
    sp = float(F32(1.0 / (255.0 - c["zpp"])))
    pad = None
    if c["pad"] is not None:
        pad = np.zeros((B, Sk), dtype=np.float16 if c["pad"][0] == "f16" else np.float32)
        for b, (kind, n, val) in enumerate(c["pad"][1]):
            if kind == "right":
                pad[b, n:] = val
            elif kind == "left":
                pad[b, :n] = val
            elif kind == "full":
                pad[b, :] = val
    gate = None
    if c["gate"] == "token":
        gate = rng.random((B, H, Sq, 1)).astype(F32)
    elif c["gate"] == "head":
        gate = rng.random((1, H, 1, 1)).astype(F32)
    return dict(qi=qi, ki=ki, vi=vi, S=S, S_tail=S_tail, k1=k1, pad=pad, gate=gate,
                grids=dict(q=(float(F32(sq)), c["zq"]), k=(float(F32(sk)), c["zk"]), v=(float(F32(sv)), c["zv"]), s=(float(F32(ss)), zs), p=(sp, c["zpp"])))


def prep(c):
    return _prep(c["name"])


def grids(c):
    """{"q", "k", "v", "s", "p", "c": (step, zero point)} of a case (c["gc"] may be a form's: `emit_case`)."""
    return dict(prep(c)["grids"], c=None if c["gc"] is None else (float(F32(c["gc"][0])), c["gc"][1]))


# ---- the staged model -----------------------------------------------------------------------------------------------------------------
def _rint_half_away(t):
    return np.sign(t) * np.floor(np.abs(t) + 0.5)


def stage1(c, mut=None):
    """Score indices (B,H,Sq,Sk) uint8 of every key < Sk of every query row: the reference quantises before the mask."""
    p = prep(c)
    g = grids(c)
    zq, zk, zs = g["q"][1], g["k"][1], g["s"][1]
    S, k1 = p["S"], F64(p["k1"])
    if mut in ("cq-dropped", "ck-dropped", "Dcqck-dropped", "cq2-64-added-once"):
        # the kernel's form: sum (a + cq)(b + ck) = sum a b + ck sum a + cq sum b + D cq ck on the centred indices a, b
        a, b = p["qi"].astype(F64) - 128.0, p["ki"][:, :, :c["Sk"]].astype(F64) - 128.0
        cq, ck = 128.0 - zq, 128.0 - zk
        asum, bsum = a.sum(-1)[..., :, None], b.sum(-1)[..., None, :]
        ab = np.matmul(a, np.swapaxes(b, -1, -2))
        if mut == "cq-dropped":
            S = ab + ck * asum
        elif mut == "ck-dropped":
            S = ab + cq * bsum
        elif mut == "Dcqck-dropped":
            S = ab + ck * asum + cq * bsum
        else:
            S = ab + ck * asum + (cq - 64.0) * bsum + D * cq * ck
    if mut == "scale_div-as-scale":
        k1 = F64(k1_of(g["q"][0], g["k"][0], g["s"][0], c["scale_div"], 0.0))
    t = S * k1   # exact: a 24-bit integer times a 24-bit significand
    r = _rint_half_away(t) if mut == "half-away" else np.rint(t)
    lo, hi = -zs + (mut == "clamp-lo-plus-1"), 255.0 - zs - (mut == "clamp-hi-minus-1")
    return (np.clip(r, lo, hi) + zs).astype(np.uint8)


def visible(c, mut=None):
    """(B,1,Sq,Sk) bool: the keys a row sees - causal: key <= row + Sk - Sq; padding: entries <= -1e4 are hidden."""
    p = prep(c)
    B, Sq, Sk = c["B"], c["Sq"], c["Sk"]
    vis = np.ones((B, 1, Sq, Sk), dtype=bool)
    if c["causal"]:
        lim = np.arange(Sq)[:, None] + (Sk - Sq) + (mut == "causal-limit-plus-1")
        vis &= (np.arange(Sk)[None, :] <= lim)[None, None]
    if p["pad"] is not None:
        pad = p["pad"].astype(F32)
        hid = pad < -1.0e4 if mut == "1e4-visible" else pad <= -1.0e4
        if mut == "pad-boundary-plus-1":
            hid = hid.copy()
            for b in range(B):
                first = np.nonzero(hid[b])[0]
                if first.size:
                    hid[b, first[0]] = False
        vis = vis & ~hid[:, None, None, :]
    return vis


def stage2(c, s_idx, mut=None):
    """(float64 probabilities after the clip, t = p / scale_p + zp_p, the index clip(rint(t), 0, 255)) from score indices."""
    p = prep(c)
    g = grids(c)
    ss, zs = g["s"]
    sp, zpp = g["p"]
    Sk = c["Sk"]
    x = F64(F32(ss)) * (s_idx.astype(F64) - zs)
    vis = np.broadcast_to(visible(c, mut), x.shape)
    if mut == "tail-key-kept":   # the first key behind the row, from the cache's bytes, seen by every query
        xt = F64(F32(ss)) * np.clip(np.rint(p["S_tail"] * F64(p["k1"])), -zs, 255.0 - zs)
        x, vis = np.concatenate([x, xt], axis=-1), np.concatenate([vis, np.ones_like(vis[..., :1])], axis=-1)
    none = ~vis.any(-1, keepdims=True)
    M = np.where(vis, x, -np.inf).max(-1, keepdims=True)
    M = np.where(none, 0.0, M)
    e = np.where(vis, np.exp(x - M), 0.0)
    plus = 0.0 if c["base"] != 1 else {"plus1-dropped": 0.0, "plus1-doubled": 2.0}.get(mut, 1.0)
    den = e.sum(-1, keepdims=True) + plus * np.exp(-M)
    if c["base"] == 1:   # a row without a visible key: exactly 0
        pr = np.where(none, 0.0, e / np.where(none, 1.0, den))
    else:                # ... uniform over all Sk keys under the vanilla softmax
        pr = np.where(none, 1.0 / Sk, e / np.where(none, 1.0, den))
    pr = pr[..., :Sk]
    if c["clip"] is not None:
        gam, eta = c["clip"]
        w, g0 = F64(F32(F64(eta) - F64(gam))), F64(F32(gam))   # fill_problem: eta - gamma formed in double, rounded once
        if mut == "eta-minus-gamma-is-1":
            w = 1.0
        if mut == "gamma-is-0":
            g0 = 0.0
        pr = np.clip(w * pr + g0, 0.0, 1.0)
    t = pr / F64(F32(sp)) + (0.0 if mut == "zpp-ignored" else zpp)
    return pr, t, np.clip(np.rint(t), 0.0, 255.0).astype(np.uint8)


def oracle_probs(c, s_idx):
    """O.attn_core's fp32 probabilities on dequantised score indices: the scores enter as q against an identity k (every product exact), the
    masks and the softmax are the oracle's own."""
    from oracle import oeh_oracle as O

    p, g = prep(c), grids(c)
    x = O.fq_dequant(s_idx.astype(F32), F32(g["s"][0]), F32(g["s"][1]))
    eye = np.eye(c["Sk"], dtype=F32)[None, None]
    kw = dict(base=c["base"], causal=c["causal"], clamp_min=True, mask_min=FMIN32, want=("probs",))
    if c["clip"] is not None:
        kw.update(clip=True, gamma=c["clip"][0], eta=c["clip"][1])
    if p["pad"] is not None:
        kw["pad_mask"] = p["pad"].astype(F32)
    return O.attn_core(x, eye, np.zeros((1, 1, c["Sk"], 1), dtype=F32), **kw)[1]["probs"]


def err64_of(c):
    """The largest distance of the oracle's fp32 probabilities from the model's float64 ones on case c's own (exact) score indices."""
    s_idx = stage1(c)
    return float(np.abs(oracle_probs(c, s_idx).astype(F64) - stage2(c, s_idx)[0]).max())


_ERR64 = None


def err64():
    """ONE number for all cases: the reference's own rounding, the ruler of the probability stage."""
    global _ERR64
    if _ERR64 is None:
        _ERR64 = max(err64_of(c) for c in CASES)
    return _ERR64


def band_of(c, t):
    """True where t is within BAND * ERR64 / scale_p of a half-integer: the kernel's index may be either neighbour there."""
    return np.abs(np.abs(t - np.floor(t)) - 0.5) <= BAND * err64() / F64(F32(grids(c)["p"][0]))


def prob_distance(c, t, p_idx):
    """The least distance of a kernel's probability from float64 that its index proves: t64 lies this far outside [idx - 1/2, idx + 1/2]
    (an index at an end of the range stands for everything beyond it)."""
    i = p_idx.astype(F64)
    lo = np.where(i == 0.0, -np.inf, i - 0.5)
    hi = np.where(i == 255.0, np.inf, i + 0.5)
    return np.maximum(np.maximum(lo - t, t - hi), 0.0) * F64(F32(grids(c)["p"][0]))


def _quant_rel(x, step, zp):
    """The reference's idx - zp = clamp(round(x / step) + zp, 0, 255) - zp in fp32: the IEEE quotient, ties to even; never -0."""
    with np.errstate(over="ignore"):
        r = np.rint((x / F32(step)).astype(F32))
    return (np.clip(r + F32(zp), F32(0.0), F32(255.0)) - F32(zp)).astype(F32)


def stage3(c, p_idx, mut=None):
    """(context indices (B,H,Sq,64) uint8 or None, the fp32 output) from probability indices."""
    p = prep(c)
    g = grids(c)
    zv, zpp = g["v"][1], g["p"][1]
    Sk = c["Sk"]
    v = p["vi"][:, :, :Sk].astype(F64)
    pc = p_idx.astype(F64)
    if mut in ("cv-dropped", "cp-dropped", "ncvcp-dropped"):   # sum (v + cv)(p + cp) = o + cp vsum + cv psum + n cv cp on the centred indices
        cv, cp = 128.0 - zv, 128.0 - zpp
        vc, pcc = v - 128.0, pc - 128.0
        n = 64 * ((Sk + 63) // 64)
        if mut == "cv-dropped":
            O = np.matmul(pcc + cp, vc)
        elif mut == "cp-dropped":
            O = np.matmul(pcc, vc + cv)
        else:
            O = np.matmul(pc - zpp, v - zv) - n * cv * cp
    else:
        O = np.matmul(pc - zpp, v - zv)
    so = so_of(g["p"][0], g["v"][0])
    x = (so * O.astype(F32)).astype(F32)
    gate = None if p["gate"] is None or mut == "gate-left-out" else p["gate"]
    gated = p["gate"] is not None
    before = c["before"] if mut != "ctx-quantiser-other-side" else not c["before"]
    rel = None
    if g["c"] is not None:
        step, zc = g["c"]
        oscale = F32(1.0) if c["emit"] else F32(step)
    if g["c"] is not None and (before or not gated):
        rel = _quant_rel(x, step, zc)
        x = (oscale * rel).astype(F32)
    if gate is not None:
        x = (x * gate).astype(F32)
    if g["c"] is not None and not before and gated:
        rel = _quant_rel(x, step, zc)
        x = (oscale * rel).astype(F32)
    return (None if rel is None else (rel + F32(zc)).astype(np.uint8)), x


# ---- acceptance: what tests/test_attn_i8_instances_gpu.py asks of a launch's dumps and output -----------------------------------------
def check_stages(c, s_idx, p_idx, c_idx, out):
    """Stages 1 - 3 on the dumps (B,H,Sq,Sk) / (B,H,Sq,Sk) / (B,H,Sq,64) uint8 and the fp32 output of a DUMP launch of case c; an AssertionError
    names the stage.  Returns (largest probability distance from float64 / ERR64, share of the probability indices inside the band)."""
    want_s = stage1(c)
    bad = s_idx != want_s
    assert not bad.any(), (c["name"], "stage 1: score indices", int(bad.sum()), [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:4]])
    _, t, want_p = stage2(c, s_idx)
    band = band_of(c, t)
    diff = np.abs(p_idx.astype(np.int32) - want_p.astype(np.int32))
    dist = float(prob_distance(c, t, p_idx).max()) / err64()
    assert not (diff[~band] != 0).any() and diff.max() <= 1, (c["name"], "stage 2: probability indices", int((diff[~band] != 0).sum()), int(diff.max()), f"distance / ERR64 {dist:.2f}",
                                                                [tuple(int(i) for i in ix) for ix in np.argwhere((diff != 0) & ~band)[:4]])
    assert dist <= BAND, (c["name"], "stage 2: probability distance / ERR64", dist)
    want_c, want_o = stage3(c, p_idx)
    if want_c is not None:
        bad = c_idx != want_c
        assert not bad.any(), (c["name"], "stage 3: context indices", int(bad.sum()), [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:4]])
    bad = np.ascontiguousarray(out, dtype=F32).view(np.int32) != want_o.view(np.int32)
    assert not bad.any(), (c["name"], "stage 3: output bits", int(bad.sum()), [(tuple(int(i) for i in ix), float(out[tuple(ix)]), float(want_o[tuple(ix)])) for ix in np.argwhere(bad)[:4]])
    return dist, float(band.mean())


MUTANTS1 = ("cq-dropped", "ck-dropped", "Dcqck-dropped", "cq2-64-added-once", "half-away", "clamp-lo-plus-1", "clamp-hi-minus-1", "scale_div-as-scale")
MUTANTS2 = ("plus1-dropped", "plus1-doubled", "tail-key-kept", "causal-limit-plus-1", "pad-boundary-plus-1", "1e4-visible", "eta-minus-gamma-is-1", "gamma-is-0",
            "zpp-ignored")
MUTANTS3 = ("cv-dropped", "cp-dropped", "ncvcp-dropped", "gate-left-out", "ctx-quantiser-other-side")
MUTANTS = MUTANTS1 + MUTANTS2 + MUTANTS3


def exercises(c, kind):
    """Whether case c can tell a kernel with `kind` wrong from a right one."""
    if kind in ("cq-dropped",):
        return c["zq"] != 128.0
    if kind == "ck-dropped":
        return c["zk"] != 128.0
    if kind == "Dcqck-dropped":
        return c["zq"] != 128.0 and c["zk"] != 128.0
    if kind == "cq2-64-added-once":
        return c["zq"] == 0.0
    if kind == "half-away":
        return c["tie"]
    if kind == "scale_div-as-scale":
        return c["scale_div"] != 0.0
    if kind in ("plus1-dropped", "plus1-doubled"):
        return c["base"] == 1
    if kind == "tail-key-kept":
        return c["cache"] > 0
    if kind == "causal-limit-plus-1":
        return c["causal"]
    if kind == "pad-boundary-plus-1":
        return c["pad"] is not None
    if kind == "1e4-visible":
        return c["pad"] is not None and any(r[0] != "none" and r[2] == -1.0e4 for r in c["pad"][1])
    if kind in ("eta-minus-gamma-is-1", "gamma-is-0"):
        return c["clip"] is not None
    if kind == "zpp-ignored":
        return c["zpp"] != 0.0
    if kind in ("cv-dropped", "ncvcp-dropped"):
        return c["zv"] != 128.0
    if kind == "gate-left-out":
        return c["gate"] is not None
    if kind == "ctx-quantiser-other-side":
        return c["gate"] is not None and c["gc"] is not None and not c["emit"]
    return True


def run_model(c, mut=None):
    """What a kernel with `mut` wrong would dump and write: every stage from its own stage before."""
    s_idx = stage1(c, mut if mut in MUTANTS1 else None)
    p_idx = stage2(c, s_idx, mut if mut in MUTANTS2 else None)[2]
    c_idx, out = stage3(c, p_idx, mut if mut in MUTANTS3 else None)
    return s_idx, p_idx, c_idx, out
