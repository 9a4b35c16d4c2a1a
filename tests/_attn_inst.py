"""The compiled instances of the three matrix-core attention families - the one-pass kernel (csrc/oeh_attn_flash*.inl), the full-row kernel
(csrc/oeh_attn_fast.inl) and the general kernel (csrc/oeh_attn_mfma.inl) - and the registry of cases that launches every one of them.
numpy and ctypes only; tests/test_attn_instances_cpu.py checks the registry without a GPU, tests/test_plan_instances_gpu.py runs it.

An instance key names one compiled kernel:
  ("fast",  NT, D, IN, CLIP, GATE, FQ, SRC32, O32, PV2)     oeh_attn_fast_kernel
  ("flash", D, IN, MQ, PAD, GATE, SRC32, TP, O32, PV2)      oeh_attn_flash_kernel
  ("hot",   D, IN, MQ)                                      oeh_attn_flash_hot_kernel
  ("mfma",  NT, D, IN, FQ)                                  oeh_attn_mfma_kernel
IN: 0 fp16, 1 bf16, 2 fp32 (the general kernel only: the other two read fp32 storage as SRC32 with IN 0).

`instance_of` asks the library for the variant name (oeh_attn_variant_ex under the case's hooks) - family, NT / MQ, D, storage, clip, fq and
pv2 - and restates only what the launch ladders read beyond the name (launch_fast_nt_d_in, launch_flash_d_mq_in, launch_nt_d of
oeh_attn_mfma.inl, fill_hot of oeh_api.hip): a padding vector or a full mask, the in-kernel gate predictor, fp32 output of 16-bit storage,
key_pad_boolean, and whether the hot argument prefix can be filled."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np

from tests import _attn_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000000  # a fake device address: nothing on the host dereferences it
DT = {"fp16": 0, "bf16": 1, "fp32": 2}
NO_FLASH, NO_FAST, NO_MFMA = 1 << 1, 1 << 2, 1 << 3
NO_FLASH_F32, NO_FAST_F32 = 1 << 6, 1 << 7
FORCE_FLASH, NO_D128_RULE, NO_HOT = 1 << 8, 1 << 11, 1 << 13
HOT_MAX_H, HOT_MAX_NQT, HOT_MAX_S = 0xFFFF, 0xFFF, 0xFFFF  # csrc/oeh_attn_params.h: kHotMax*


# ---- what the library was built with --------------------------------------------------------------------------------------------------
def targs(name: str):
    """The integer template arguments of a mangled kernel name (tools/instantiations.py: targs)."""
    return [int(x) for x in re.findall(r"L[ib](-?\d+)E", name.replace("Ln", "L-"))]


_BUILT = None


def built_instances():
    """The instantiations of the four templates in the built liboeh_hip.so, from the code object's kernel names (tools/kernel_resources.py)."""
    global _BUILT
    if _BUILT is None:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "oeh_attn_fast_kernel", "oeh_attn_flash_kernel",
                              "oeh_attn_flash_hot_kernel", "oeh_attn_mfma_kernel"], capture_output=True, text=True, check=True).stdout
        found = set()
        for line in out.splitlines():
            m = re.search(r"oeh_attn_(fast|flash_hot|flash|mfma)_kernelI", line)
            if not m:
                continue
            a = targs(line.split()[0])
            fam = {"fast": "fast", "flash": "flash", "flash_hot": "hot", "mfma": "mfma"}[m.group(1)]
            width = {"fast": 9, "flash": 9, "hot": 3, "mfma": 4}[fam]
            found.add((fam,) + tuple(a + [0] * (width - len(a)))[:width])
        assert found, "no attention kernel in the built library"
        _BUILT = frozenset(found)
    return _BUILT


# ---- a case's descriptor, host only ---------------------------------------------------------------------------------------------------
def strides(c):
    """(q, k, v) strides in elements (batch, head, row) as `_attn_ref.pose` lays the case out; the output is ops.attn_fwd's own
    (B,Sq,H,D) buffer, or rows of a float32 one."""
    B, H, Sq, Sk, D = c["B"], c["H"], c["Sq"], c["Sk"], c["D"]
    lay = c["layout"]

    def one(S, slot):
        if lay == "blhe":
            return (S * H * D, D, H * D)
        if lay == "fused":
            return (S * 3 * H * D, D, 3 * H * D)
        if lay == "longkv" and slot > 0:
            return (H * (S + 5) * D, (S + 5) * D, D)
        if lay == "qslice" and slot == 0:
            return (H * Sk * D, Sk * D, D)
        return (H * S * D, S * D, D)
    return one(Sq, 0), one(Sk, 1), one(Sk, 2)


def descriptor(c):
    """(oeh_attn_desc, oeh_fq_desc or None, oeh_attn_opts or None) of a case with fake pointers, as tools/dispatch_census.build does."""
    from outeffhop_amd._lib import oeh_attn_desc, oeh_attn_opts, oeh_fq_desc

    d = oeh_attn_desc()
    d.B, d.H, d.Sq, d.Sk, d.D, d.dtype = c["B"], c["H"], c["Sq"], c["Sk"], c["D"], DT[c["storage"]]
    d.o_dtype = DT["fp32"] if c["out32"] else d.dtype
    for st, s in zip((d.q_stride, d.k_stride, d.v_stride), strides(c)):
        st[0], st[1], st[2] = s
    d.o_stride[0], d.o_stride[1], d.o_stride[2] = c["Sq"] * c["H"] * c["D"], c["D"], c["H"] * c["D"]
    d.scale, d.scale_div = c["scale"], c["scale_div"]
    d.softmax_base, d.causal, d.clamp_min = c["base"], int(c["causal"]), int(c["clamp_min"])
    if c["clip"] is not None:
        d.clip, d.gamma, d.eta = 1, c["clip"][0], c["clip"][1]
    d.mask_min = c["mask_min"]
    if c["pad"] is not None:
        d.key_pad_mask, d.key_pad_dtype, d.key_pad_stride, d.key_pad_boolean = FAKE, DT["fp16" if c["pad"] == "f16" else "fp32"], c["Sk"], int(c["pad_bool"])
    if c["full"] is not None:
        d.full_mask, d.full_mask_dtype = FAKE, DT["fp16" if c["full"] == "f16" else "fp32"]
        d.full_mask_stride[0], d.full_mask_stride[1] = c["Sq"] * c["Sk"], c["Sk"]
    if c["gate"] is not None:
        d.gate = FAKE
        d.gate_stride[0], d.gate_stride[1], d.gate_stride[2] = (c["H"] * c["Sq"], c["Sq"], 1) if c["gate"] == "token" else (0, 1, 0)
    if c["gate_units"] is not None:
        d.gate_hidden = FAKE
        d.gate_hidden_stride[0], d.gate_hidden_stride[1] = c["Sq"] * c["H"] * c["D"], c["H"] * c["D"]
        d.gate_units = c["gate_units"]
        d.gate_w1 = d.gate_b1 = FAKE
        if c["gate_units"]:
            d.gate_w2 = d.gate_b2 = FAKE
        d.gate_scaling, d.gate_out = gate_scaling(c), FAKE
    f = None
    if c["gs"] or c["gp"] or c["gc"]:
        f = oeh_fq_desc()
        for q_, key in ((f.scores, "gs"), (f.probs, "gp"), (f.ctx, "gc")):
            g = A.grid(c, key)
            if g is not None:
                q_.enable, q_.scale, q_.zero_point, q_.qmax = 1, g[0], g[1], g[2]
                if c["dumps"]:
                    q_.dump_idx = FAKE
        f.ctx_quant_before_gate, f.ctx_emit_index = int(c["before"]), int(c["emit"])
    return d, f, (oeh_attn_opts(pv_pairs=1) if c["pv_pairs"] else None)


gate_scaling = A.gate_scaling


def variant_name(lib, c, d=None, f=None, o=None):
    """oeh_attn_variant_ex under the case's hook mask and flash_mq_force; d, f, o: the real descriptor where there is one."""
    if d is None:
        d, f, o = descriptor(c)
    assert lib.oeh_debug_set_variant(c["hook"], c["mq"]) == 0, "the diagnostic hooks are not enabled (OEH_DEBUG_HOOKS=1)"
    try:
        n = lib.oeh_attn_variant_ex(C.byref(d), None if o is None else C.byref(o), None if f is None else C.byref(f))
    finally:
        lib.oeh_debug_set_variant(0, 0)
    return None if n is None else n.decode()


def instance_from(name: str, d, f, hook: int):
    """The instance key of the launch the library names `name` for descriptor d / f under `hook`."""
    pv2 = name.endswith("+pv2")
    fam, n, dim, dt, *tags = name[:-4].split("/") if pv2 else name.split("/")
    n, dim = int(n[2:]), int(dim[1:])
    f32 = dt == "f32"
    inn = 1 if dt == "bf16" else 0
    pad, full = bool(d.key_pad_mask), bool(d.full_mask)
    gate = bool(d.gate_hidden) and not d.gate            # oeh_api.hip: gate_in_kernel
    o32 = not f32 and d.o_dtype == DT["fp32"]            # plan_attn: pl.out32
    fq = "fq" in tags or "fq2p" in tags
    if fam == "fast16":                                  # launch_fast_nt_d_in
        pad_bool = pad and bool(d.key_pad_boolean) and d.mask_min < -1.0e4  # fill_params: P.pad_bool
        FQ = 0 if not fq else (1 if not pad else (3 if pad_bool else 2))
        return ("fast", n, dim, inn, int("clip" in tags), int(gate), FQ, int(f32), int(o32), int(pv2))
    if fam == "flash16":                                 # launch_flash_d_mq_in
        TP = 2 if fq else (1 if "clip2p" in tags else 0)
        if TP == 0 and not (pad or full or gate or f32 or o32) and not hook & NO_HOT:  # fill_hot
            # (fill_hot's last condition, nBHpad == (nBH + 7) & ~7, is how oeh_attn_fwd_ex fills the one-pass kernel's block always)
            same = all(d.q_stride[i] == d.k_stride[i] == d.v_stride[i] for i in range(3))
            nqt = (d.Sq + 64 * n - 1) // (64 * n)
            if same and d.H <= HOT_MAX_H and nqt <= HOT_MAX_NQT and d.Sq <= HOT_MAX_S and d.Sk <= HOT_MAX_S:
                return ("hot", dim, inn, n)
        return ("flash", dim, inn, n, int(pad or full), int(gate), int(f32), TP, int(o32), int(pv2))
    assert fam == "mfma16", name                         # launch_nt_d
    chain = bool(f) and f.scores.enable and f.probs.enable and not pad and not full and d.scale_div == 0.0
    return ("mfma", n, dim, 2 if f32 else inn, 0 if not fq else (1 if chain else 2))


_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        os.environ.setdefault("OEH_DEBUG_HOOKS", "1")
        from outeffhop_amd import _lib as L

        _LIB = L.load()
    return _LIB


def instance_of(c):
    name = variant_name(_lib(), c)
    assert name is not None, (c["name"], "the library names no kernel")
    return instance_from(name, *descriptor(c)[:2], c["hook"])


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
S8, P8, C8 = A.S8, A.P8, A.C8
S6 = (-5.0, 5.0, 6)
S5 = (-5.0, 5.0, 5)
S_RAMP5 = (-64.0, 60.0, 5)
S_RAMP = (-64.0, 63.0, 7)        # the score grid of the causal cases' ramp
C4 = (-2.0, 2.0, 4)
S_LONG = (-256.0, 254.0, 8)      # the coarse score grid of the long peaked rows (_attn_ref.ROUTE_CASES)
# gamma > 0 gives every key a weight of at least gamma: the fp16 probability operand's rounding (2^-12 relative on average) then sums over all Sk
# keys, gamma Sk E|v| 2^-12 - inside the fp16 contract's 1e-3 at 100 keys (9.8e-4), not at 200 or 330: the general kernel's gamma > 0 case has 100 keys
GAMMA_POS = (0.05, 1.0)
CLIPS = ((-0.025, 1.1), (-0.05, 1.2))  # (eta - gamma far enough from 1 for the bf16 contract to see it)
LAYOUTS = ("contig", "blhe", "fused", "longkv")
SK_OF_NT = {8: 100, 16: 200, 32: 330}
DN = {"fp16": "f16", "bf16": "bf16", "fp32": "f32"}


def _shift(n_visible: int, spread: float) -> float:
    """The constant that puts the largest of n_visible scores of standard deviation `spread` near 0: rows on both sides of it, so that
    the "+1" of softmax_1 weighs in some rows and the largest key in others."""
    return -round(spread * float(np.sqrt(2.0 * np.log(max(n_visible, 2)))), 1)


def _mk(tag, n, Sq, Sk, D, st, *, kind, base, layout_i, **kw):
    """One case of the registry.  kind: "dense" - non-causal, no padding, peaked rows; "causal" - Sq < Sk; "pad" - non-causal, a padding
    vector that leaves sample 1 three visible keys; "cpad" - causal with a padding vector that hides sample 1's second half; "full" - a
    (B,1,Sq,Sk) mask."""
    lay = LAYOUTS[layout_i % 4]
    quant = any(kw.get(g) for g in ("gs", "gp", "gc"))
    kw = dict(kw)
    if kind in ("causal", "cpad"):
        kw.update(causal=True, clamp_min=True)
        if lay == "fused":
            lay = "blhe"
    elif lay == "fused":
        Sq = Sk
    if kind in ("pad", "cpad"):
        kw.update(pad="f16" if (st != "fp32" and layout_i % 2) else "f32", lens=(Sk, 3 if kind == "pad" else Sk // 2))
        if kw["pad"] == "f16":
            kw["mask_min"] = A.R.FMIN16
    if kind == "full":
        kw.update(full="f32")
    if kw.pop("samestride", False) and Sq != Sk:
        lay = "qslice"
    if quant:
        if kw.get("gc") and st == "bf16":  # a context grid whose step the bf16 contract (2e-2) can see
            kw["gc"] = C4
        if Sk > 512:  # long rows: peaked inputs on the coarse score grid
            kw.update(gs=S_LONG)
            spread = (8.0 if D < 128 else 5.0) if kw.get("gc") else 4.0  # (without a context grid: more keys of a row weigh enough to be missed)
        elif kind in ("causal", "cpad") and kw.get("gs"):
            kw["gs"] = S_RAMP if Sk <= 256 else S_RAMP5  # (330 keys: fewer bits, fewer rows with a score inside the tie band)
            spread = 1.0
        else:
            spread = (1.0 if base == 1 else 2.0) if kw.get("gs") else 6.0  # (softmax_1 cases are shifted: the scores stay on the grid)
            if kw.get("gs") and (Sk > 128 or D == 128):  # fewer bits from 200 keys and at head dim 128: fewer rows hold a score inside the tie band
                kw["gs"] = S5 if (Sk > 128 and D == 128) else S6
    elif st == "fp32" and not kw.get("pv_pairs"):
        # fp32 storage without the probability pairs: the probability operand is one fp16 number, so the kernel's error is up to 2^-11 sum |p| |v| -
        # inside the contract's 5e-4 (1 + |want|) on rows that spread their weight, not on peaked rows of large |v| with cancelling signs
        spread = 1.0
    else:
        spread = 6.0 if kind in ("causal", "cpad") else 4.0
    if kind == "pad":
        spread = min(spread, 2.0)
    if st == "fp32" and not kw.get("pv_pairs") and not quant and kind in ("pad", "cpad", "full"):
        base = int(kind == "pad")
        if kind == "pad":  # (the three visible keys share their weight with the "+1")
            kw["shift"] = -3.0
    if kind in ("causal", "cpad") and (Sk <= 512 or not quant):
        # causal rows see at least Sk - Sq + 1 keys: a ramp over the keys (0.15 per key, largest score near 0) gives the latest visible keys -
        # the diagonal's among them - most of every row's weight, so a causal limit that is off by one shows in every row
        kw.update(ramp=0.15, shift=None)
        spread = 1.0
    kw["qmul"] = spread
    if base == 1 and kind != "pad" and "shift" not in kw:  # (the ramp's cases need none: their largest score is near 0)
        kw["shift"] = _shift(Sk - Sq + 1 if kind in ("causal", "cpad") else Sk, spread)
    return A._c(f"{tag}-{n}-{kind}", Sq, Sk, D, B=2, H=3, storage=st, base=base, layout=lay, **kw)


def _quant_kinds(kinds, st, clip=None):
    """The cases of a form with all three quantisers: kinds[0] with the context quantiser before a per-token gate; the causal kind without
    context quantiser and gate (nothing then hides a key's weight below a grid step); kinds[0] with the context quantiser after a per-head
    gate; bf16, where the context grid has 4 bits: kinds[0] once more without it."""
    more = (kinds[1], kinds[1]) if clip else ()  # (the clip floors most keys to 0: more causal rows for the key on the diagonal to weigh in)
    return (kinds[0], kinds[1], kinds[0]) + ((kinds[0],) if st == "bf16" else ()) + more


def _quant_case(kw, ki, emit):
    """The ki-th case of `_quant_kinds`, set in kw; returns its softmax base."""
    if ki == 1 or ki >= 3:
        kw.update(gc=None, gate=None)
    if ki == 2:
        kw.update(before=False, gate="head", emit=emit)
    return (0, 1, 1)[ki] if ki < 3 else ki % 2


def _fast_cases():
    out = []
    for li, (st, D, nt) in enumerate(itertools.product(A.R.STORAGES, (32, 64, 128), (8, 16, 32))):
        Sk = SK_OF_NT[nt]
        f32 = st == "fp32"
        hook = NO_FLASH | NO_D128_RULE
        forms = []
        for clip in (None, CLIPS[li % 2]):
            forms.append(("plain", dict(clip=clip), ("dense", "causal", "pad")))
            forms.append(("gate", dict(clip=clip, gate_units=-1), ("dense", "causal", "pad")))
            forms.append(("fq1", dict(clip=clip, gs=S8, gp=P8, gc=C8, gate="token"), ("dense", "causal")))
            forms.append(("fq2", dict(clip=clip, gs=S8, gp=P8), ("pad", "cpad")))
            forms.append(("fq3", dict(clip=clip, gs=S8, gp=P8, gc=C8, gate="token", pad_bool=True), ("pad", "cpad")))
            if f32:
                forms.append(("pv2", dict(clip=clip, pv_pairs=True), ("dense", "causal", "pad")))
        if not f32 and D == 64:
            forms += [("o32", dict(out32=True), ("dense", "causal", "pad")), ("o32-clip", dict(out32=True, clip=CLIPS[li % 2]), ("dense", "causal", "pad")),
                      ("o32-gate", dict(out32=True, gate_units=-1), ("dense", "causal", "pad"))]
        if not f32 and D == 128:
            forms.append(("o32", dict(out32=True), ("dense", "causal", "pad")))
        for fi, (form, kw, kinds) in enumerate(forms):
            tag = f"fast-NT{nt}-D{D}-{DN[st]}-{form}" + ("-clip" if kw.get("clip") and "clip" not in form else "")
            if kw.get("gc"):
                kinds = _quant_kinds(kinds, st, kw.get("clip"))
            for ki, kind in enumerate(kinds):
                kw2 = dict(kw)
                if kw2.get("gate_units") == -1:
                    kw2["gate_units"] = (0, 48)[(ki + fi) % 2]
                base = (0, 1)[(ki + fi + li) % 2]
                if kw.get("gc"):
                    base = _quant_case(kw2, ki, emit=form == "fq3")
                if form == "fq2":      # arbitrary additive values: the second case pads with -3e4 where the first has finfo.min
                    base = ki
                    if ki:
                        kw2["mask_min"] = -3.0e4
                if not kw.get("gc") and kw2.get("gate_units") is None and ki == min(1, len(kinds) - 1):
                    kw2["gate"] = ("token", "head")[(li + fi) % 2]  # gate values: a run-time branch of every instance's epilogue
                kernel = f"fast16/NT{nt}/D{D}/{DN[st]}" + ("/clip" if kw.get("clip") else "") + ("/fq" if form.startswith("fq") else "") + ("+pv2" if form == "pv2" else "")
                out.append(_mk(tag, ki, 70, Sk, D, st, kind=kind, base=base, layout_i=li + fi + ki, hook=hook, kernel=kernel, **kw2))
    return out


def _flash_cases():
    out = []
    for li, (st, D, mq) in enumerate(itertools.product(A.R.STORAGES, (32, 64, 128), (1, 2))):
        f32 = st == "fp32"
        if f32 and D == 128 and mq == 2:
            continue  # oeh_api.hip: flash_mq - one block per wave there
        hook = FORCE_FLASH
        plain3 = ("dense", "causal")
        forms = [("plain", dict(hook=hook | NO_HOT), plain3), ("pad", dict(), ("pad", "cpad")), ("full", dict(), ("full",)),
                 ("clip2p", dict(clip=CLIPS[li % 2]), plain3 + ("dense",)), ("clip2p-pad", dict(clip=CLIPS[li % 2]), ("pad", "full", "cpad")),
                 ("fq2p", dict(gs=S_LONG, gp=P8, gc=C8, gate="token"), plain3), ("fq2p-pad", dict(gs=S_LONG, gp=P8, gc=C8, gate="token", pad_bool=True), ("pad", "cpad"))]
        if not f32:
            forms += [("hot", dict(samestride=True), plain3), ("gate", dict(gate_units=-1), plain3), ("pad-gate", dict(gate_units=-1), ("pad", "cpad"))]
            if D == 64:
                forms += [("o32", dict(out32=True, hook=hook | NO_HOT), plain3), ("o32-pad", dict(out32=True), ("pad", "cpad")),
                          ("o32-full", dict(out32=True), ("full",)), ("o32-gate", dict(out32=True, gate_units=-1), plain3)]
            if D == 128 and mq == 1:
                forms.append(("o32", dict(out32=True), plain3))
        else:
            forms += [("pv2", dict(pv_pairs=True), plain3), ("pv2-clip2p", dict(pv_pairs=True, clip=CLIPS[li % 2]), plain3)]
            if not (D == 64 and mq == 2):
                forms += [("pv2-pad", dict(pv_pairs=True), ("pad", "full", "cpad")), ("pv2-clip2p-pad", dict(pv_pairs=True, clip=CLIPS[li % 2]), ("pad", "full", "cpad"))]
        for fi, (form, kw, kinds) in enumerate(forms):
            two_pass = "2p" in form
            tag = f"flash-MQ{mq}-D{D}-{DN[st]}-{form}"
            if kw.get("gc"):
                kinds = _quant_kinds(kinds, st)
            for ki, kind in enumerate(kinds):
                kw2 = dict(kw)
                kw2.setdefault("hook", hook)
                if kw2.get("gate_units") == -1:
                    kw2["gate_units"] = (0, 48)[(ki + fi) % 2]
                base = (0, 1)[(ki + fi + li) % 2]
                if kw.get("gc"):
                    base = _quant_case(kw2, ki, emit="pad" in form)
                if "fq2p-pad" in form:  # oeh_api.hip: flash_two_pass_can - padded keys on the grid only with softmax_1
                    base = 1
                Sk = 530 if (two_pass or kind == "full") else 200
                if form.endswith("clip2p") and D == 128 and ki:
                    Sk = 385  # (head dim 128: the two-pass clip from 384 keys)
                if not kw.get("gc") and kw2.get("gate_units") is None and ki == min(1, len(kinds) - 1):
                    kw2["gate"] = ("token", "head")[(li + fi) % 2]  # gate values: a run-time branch of every instance's epilogue
                kernel = f"flash16/MQ{mq}/D{D}/{DN[st]}" + ("/fq2p" if "fq2p" in form else ("/clip2p" if "clip2p" in form else "")) + ("+pv2" if "pv2" in form else "")
                out.append(_mk(tag, ki, 150, Sk, D, st, kind=kind, base=base, layout_i=li + fi + ki, mq=mq, kernel=kernel, **kw2))
    return out


def _mfma_cases():
    out = []
    for li, (st, D, nt) in enumerate(itertools.product(A.R.STORAGES, (32, 64, 128), (8, 16, 32))):
        Sk = SK_OF_NT[nt]
        hook = NO_FLASH | NO_FAST
        clip = CLIPS[li % 2]
        forms = [("plain", dict(), (("full", dict()), ("causal", dict(clip=clip, hook=hook)), ("pad", dict(hook=hook, gate="token")), ("dense", dict(hook=hook, clip=GAMMA_POS if nt == 8 else None)))),
                 ("fq1", dict(gs=S8, gp=P8, gc=C8, gate="token", hook=hook), (("dense", dict()), ("causal", dict(clip=clip, gc=None, gate=None)), ("dense", dict(before=False, gate="head")))),
                 ("fq2", dict(hook=hook), (("pad", dict(gs=S8, gp=P8, gc=C8, gate="token")), ("causal", dict(gs=S8, clip=clip)), ("dense", dict(gp=P8, gc=C8, gate="head", before=False, emit=True, gs=None)),
                                           ("full", dict(gs=S8, gp=P8))))]
        for fi, (form, kw, kinds) in enumerate(forms):
            tag = f"mfma-NT{nt}-D{D}-{DN[st]}-{form}"
            for ki, (kind, extra) in enumerate(kinds):
                kw2 = dict(kw, **extra)
                base = (0, 1)[(ki + fi + li) % 2]
                kernel = f"mfma16/NT{nt}/D{D}/{DN[st]}" + ("" if form == "plain" else "/fq")
                out.append(_mk(tag, ki, 70, Sk, D, st, kind=kind, base=base, layout_i=li + fi + ki, kernel=kernel, **kw2))
    return out


CASES = tuple(_fast_cases() + _flash_cases() + _mfma_cases())

# Built instances that no descriptor can launch: {instance key: the ladder or plan line that excludes it}.
UNREACHABLE = {}


def group_of(inst):
    """(family, D, IN, NT or MQ): how tests/test_plan_instances_gpu.py is parametrised."""
    if inst[0] in ("fast", "mfma"):
        return (inst[0], inst[2], ("f16", "bf16", "f32")[2 if (inst[0] == "fast" and inst[7]) else inst[3]], inst[1])
    if inst[0] == "hot":
        return ("flash", inst[1], ("f16", "bf16")[inst[2]], inst[3])
    return ("flash", inst[1], "f32" if inst[6] else ("f16", "bf16")[inst[2]], inst[3])


# every (family, D, storage, NT or MQ) that has instances - written out, so that collecting the test files needs no built library
# (tests/test_attn_instances_cpu.py holds it against the built instances); fp32 storage at d = 128 has one block per wave only
GROUPS = tuple(sorted([(fam, D, dt, nt) for fam in ("fast", "mfma") for D in (32, 64, 128) for dt in ("f16", "bf16", "f32") for nt in (8, 16, 32)]
                      + [("flash", D, dt, mq) for D in (32, 64, 128) for dt in ("f16", "bf16", "f32") for mq in (1, 2) if not (D == 128 and dt == "f32" and mq == 2)]))
GROUP_IDS = tuple(f"{g[0]}-D{g[1]}-{g[2]}-{'MQ' if g[0] == 'flash' else 'NT'}{g[3]}" for g in GROUPS)

_BY_INSTANCE = None


def by_instance():
    """{instance key: [cases]} over CASES."""
    global _BY_INSTANCE
    if _BY_INSTANCE is None:
        t = {}
        for c in CASES:
            t.setdefault(instance_of(c), []).append(c)
        _BY_INSTANCE = t
    return _BY_INSTANCE
