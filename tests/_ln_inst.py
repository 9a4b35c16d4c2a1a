"""The compiled instances of the LayerNorm-row family - the block tail (csrc/oeh_ln.hip), the embedding front (csrc/oeh_embed.hip) and the
training tail's two row kernels (csrc/oeh_ln_train.hip), which share ln_plan, dispatch_ln_ch and launch_ln_rows of csrc/oeh_ln_row.h - and
the registry of cases that launches every one of them.  numpy and ctypes only; tests/test_ln_instances_cpu.py checks the registry without a
GPU, tests/test_ln_instances_gpu.py runs it.

An instance key names one compiled kernel:
  ("ln", IN, CH, FORM)                     oeh_resid_ln_kernel
  ("embed", IN, CH, FORM, NT)              oeh_embed_kernel
  ("ln_train_fwd", IN, CH, FORM, DROP)     oeh_ln_train_fwd_kernel
  ("ln_train_bwd", IN, CH, FORM, DROP)     oeh_ln_train_bwd_kernel
IN: 0 fp16, 1 bf16, 2 fp32.  FORM: 0 one wave per row, 1 one workgroup per row, 2 element accesses.  CH: accesses per thread.

`instance_of` asks the library's host-only names (oeh_resid_ln_variant, oeh_embed_sum_variant, oeh_drop_resid_ln_variant) with the row
stride the case's tensors have, and parses form, CH, Tn, dtype and /drop: ln_plan is not restated here.  The widths are not written down
either: `ranges` scans the name over every width up to 8192 and a case sits at the first and at the last width of each (form, CH) range.
At the first width only thread 0 of the last access has a chunk, so nearly every `ch < nchunk` predicate of that access is false; at the
last width every access of every thread is full.  The element form's last width is a multiple of the 16-byte vector: it is reached with
rows cols + 1 elements apart.

A case has 5 rows: the wave form's second workgroup has one row and three idle waves.  The run-time branches behind a template instance
rotate over the cases by index (`_flags`); the two widths of an instance take complementary values."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

from tests._attn_inst import ROOT, targs

KERNELS = ("ln", "embed", "ln_train_fwd", "ln_train_bwd")
DTN = ("f16", "bf16", "f32")             # IN -> the dtype of the variant names
FORMS = ("wave", "block", "scalar")      # FORM -> the form of the variant names
VEC = (8, 8, 4)                          # IN -> elements of a 16-byte access
ROWS, MAX_COLS = 5, 8192
P_DROP = 0.1
_TEMPLATES = {"oeh_resid_ln_kernel": ("ln", 3), "oeh_embed_kernel": ("embed", 4), "oeh_ln_train_fwd_kernel": ("ln_train_fwd", 4),
              "oeh_ln_train_bwd_kernel": ("ln_train_bwd", 4)}


# ---- what the library was built with --------------------------------------------------------------------------------------------------
_BUILT = None


def built_instances():
    """The instantiations of the four templates in the built liboeh_hip.so, from the code object's kernel names (tools/kernel_resources.py).
    The training kernels sit in an anonymous namespace: the match is on the kernel's name."""
    global _BUILT
    if _BUILT is None:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), *_TEMPLATES], capture_output=True, text=True, check=True).stdout
        found = set()
        for line in out.splitlines():
            m = re.search(r"\d+(oeh_resid_ln_kernel|oeh_embed_kernel|oeh_ln_train_fwd_kernel|oeh_ln_train_bwd_kernel)I", line)
            if not m:
                continue
            kernel, width = _TEMPLATES[m.group(1)]
            a = targs(line.split()[0])
            assert len(a) >= width, line
            found.add((kernel,) + tuple(a[:width]))
        assert found, "no LayerNorm-row kernel in the built library"
        _BUILT = frozenset(found)
    return _BUILT


# ---- the library's names, host only -----------------------------------------------------------------------------------------------------
_LIB = None


def _lib():
    global _LIB
    if _LIB is None:
        from outeffhop_amd import _lib as L

        _LIB = (L, L.load())
    return _LIB


def ln_name(IN, rows, cols, stride):
    """oeh_resid_ln_variant for (rows, cols) tensors of dtype IN whose rows are `stride` elements apart."""
    L, lib = _lib()
    d = L.oeh_ln_desc()
    d.rows, d.cols, d.dtype, d.eps = rows, cols, IN, 1e-5
    d.x_stride = d.r_stride = d.sum_stride = d.y_stride = stride
    n = lib.oeh_resid_ln_variant(C.byref(d))
    return None if n is None else n.decode()


def embed_name(IN, B, S, cols, nt, stride, int8=False):
    """oeh_embed_sum_variant for nt lookups into tables whose rows, like the outputs', are `stride` elements apart."""
    L, lib = _lib()
    d = L.oeh_embed_desc()
    d.B, d.S, d.cols, d.dtype, d.n_tab, d.eps = B, S, cols, IN, nt, 1e-5
    d.sum_stride = d.y_stride = stride
    for t in range(nt):
        l = d.tab[t]
        l.table, l.ids, l.n_rows, l.row_stride, l.id_stride_b, l.id_stride_s = 4096, 4096, 2, stride, S, 1  # (fake addresses: nothing reads them)
        if int8:
            l.form, l.scale, l.int_min, l.int_max = L.OEH_TAB_I8, 1.0, -128.0, 127.0
    n = lib.oeh_embed_sum_variant(C.byref(d))
    return None if n is None else n.decode()


def train_name(IN, rows, cols, stride, p, backward):
    """oeh_drop_resid_ln_variant; the backward's /G<workgroups>x<rows per slab> suffix stays on."""
    L, lib = _lib()
    d = L.oeh_ln_train_desc()
    d.rows, d.cols, d.dtype, d.eps = rows, cols, IN, 1e-5
    d.x_stride = d.r_stride = d.sum_stride = d.y_stride = d.dsum_stride = stride
    d.drop.p, d.drop.seed = p, 0
    n = lib.oeh_drop_resid_ln_variant(C.byref(d), int(backward))
    return None if n is None else n.decode()


def key_of(name):
    """The instance key a variant name stands for."""
    p = name.split("/")
    if p[0] == "ln":        # ln/wave/CH4/f32
        return ("ln", DTN.index(p[3]), int(p[2][2:]), FORMS.index(p[1]))
    if p[0] == "embed":     # embed/block/CH4/T2/f16
        return ("embed", DTN.index(p[4]), int(p[2][2:]), FORMS.index(p[1]), int(p[3][1:]))
    assert p[0] == "ln_train" and p[1] in ("fwd", "bwd"), name  # ln_train/bwd/block/CH8/f32[/drop]/G512x2
    return ("ln_train_" + p[1], DTN.index(p[4]), int(p[3][2:]), FORMS.index(p[2]), int(len(p) > 5 and p[5] == "drop"))


def variant_name(c, stride=None):
    """The library's name for case c, with rows `stride` (default: the case's) elements apart."""
    st = c["stride"] if stride is None else stride
    if c["kernel"] == "ln":
        return ln_name(c["IN"], ROWS, c["cols"], st)
    if c["kernel"] == "embed":
        return embed_name(c["IN"], c["B"], c["S"], c["cols"], c["nt"], st, c["tab"] == "int8")
    return train_name(c["IN"], ROWS, c["cols"], st, c["p"], c["kernel"] == "ln_train_bwd")


def instance_of(c):
    name = variant_name(c)
    assert name is not None, (c["name"], "the library names no kernel")
    return key_of(name)


# ---- the widths -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ranges(IN):
    """{(FORM, CH): (first width, last width)} of dtype IN, from oeh_resid_ln_variant over every multiple of VEC up to 8192 with dense rows
    (the 16-byte forms) and over every width with rows cols + 1 elements apart (element accesses)."""
    out = {}

    def note(cols, stride):
        k = key_of(ln_name(IN, ROWS, cols, stride))
        lo, hi = out.get((k[3], k[2]), (cols, cols))
        out[(k[3], k[2])] = (min(lo, cols), max(hi, cols))
    for cols in range(VEC[IN], MAX_COLS + 1, VEC[IN]):
        note(cols, cols)
    for cols in range(1, MAX_COLS + 1):
        note(cols, cols + 1)
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
# five on / off branches in complementary pairs: the two widths of an instance (an even index and the next) take opposite values of each
_MASKS5 = (0b11111, 0b00000, 0b10101, 0b01010, 0b11010, 0b00101, 0b01111, 0b10000)
_MASKS3 = (0b111, 0b000, 0b101, 0b010, 0b011, 0b100, 0b110, 0b001)
_MASKS2 = (0b11, 0b00, 0b01, 0b10)

# {case name: n}: the n-th next seed, where the first draw's tie band is over half the cap (tests/test_ln_instances_cpu.py says which)
RESEED = {}


def _flags(kernel, i, nt):
    """The run-time branches of the i-th case of a (kernel, form)."""
    if kernel == "ln":  # block tail: residual, beta, sum quantiser, output quantiser, sum output
        m = _MASKS5[i % 8]
        return dict(r=bool(m & 1), beta=bool(m & 2), sq=bool(m & 4), oq=bool(m & 8), sum=bool(m & 16))
    if kernel == "embed":  # table form, id dtype, LayerNorm or none, middle / last sum quantiser, beta, output quantiser
        m = _MASKS5[(i + i // 8) % 8]
        ln = i % 5 != 2
        return dict(tab=("plain", "grid", "int8")[i % 3], id64=bool(m & 1), ln=ln, mid=bool(m & 2) and nt == 3, last=bool(m & 4) and nt >= 2,
                    beta=bool(m & 8) and ln, oq=bool(m & 16) and ln, B=(5, 1)[i % 2], S=(1, 5)[i % 2])
    if kernel == "ln_train_fwd":  # residual, beta
        m = _MASKS2[i % 4]
        return dict(r=bool(m & 1), beta=bool(m & 2))
    m = _MASKS3[i % 8]  # backward: dsum, want_dr, want_dbeta
    return dict(dsum=bool(m & 1), dr=bool(m & 2), dbeta=bool(m & 4))


def _variants(kernel):
    return {"ln": (None,), "embed": (1, 2, 3)}.get(kernel, (0, 1))


@functools.lru_cache(maxsize=None)
def cases():
    """One case per instance and width (first and last of the instance's range), in a fixed order."""
    out, count = [], {}
    for kernel in KERNELS:
        for IN in range(3):
            for (form, ch), (lo, hi) in sorted(ranges(IN).items()):
                for v in _variants(kernel):
                    for which, cols in (("first", lo), ("last", hi)):
                        i = count[(kernel, form)] = count.get((kernel, form), -1) + 1
                        stride = cols + 1 if (form == 2 and cols % VEC[IN] == 0) else cols
                        tag = "" if kernel == "ln" else f"-T{v}" if kernel == "embed" else ("-nodrop", "-drop")[v]
                        c = dict(kernel=kernel, IN=IN, form=form, CH=ch, cols=cols, stride=stride, which=which, index=i,
                                 name=f"{kernel}-{DTN[IN]}-{FORMS[form]}-CH{ch}{tag}-{which}{cols}", **_flags(kernel, i, v))
                        if kernel == "embed":
                            c["nt"] = v
                        elif kernel != "ln":
                            c["p"] = P_DROP if v else 0.0
                        c["inst"] = (kernel, IN, ch, form) + (() if v is None else (v,))
                        c["seed"] = 20000 + 13 * len(out) + 7919 * RESEED.get(c["name"], 0)
                        out.append(c)
    return tuple(out)


# Built instances that no descriptor can launch: {instance key: the plan line that excludes it}.
UNREACHABLE = {}


def group_of(inst):
    """(kernel, dtype, form, CH): how tests/test_ln_instances_gpu.py is parametrised."""
    return (inst[0], DTN[inst[1]], FORMS[inst[3]], inst[2])


# every (kernel, dtype, form, CH) that has instances - written out, so that collecting the test files needs no built library
# (tests/test_ln_instances_cpu.py holds it against the built instances)
_CH = {("f32", "wave"): (1, 2, 4), ("f32", "block"): (2, 4, 8), ("f16", "wave"): (1, 2), ("f16", "block"): (1, 2, 4),
       ("bf16", "wave"): (1, 2), ("bf16", "block"): (1, 2, 4)}
GROUPS = tuple((k, dt, form, ch) for k in KERNELS for dt in DTN for form in FORMS for ch in _CH.get((dt, form), (1, 4, 16, 32)))
GROUP_IDS = tuple(f"{g[0]}-{g[1]}-{g[2]}-CH{g[3]}" for g in GROUPS)


@functools.lru_cache(maxsize=None)
def by_instance():
    """{instance key: [cases]} by the library's own names."""
    t = {}
    for c in cases():
        t.setdefault(instance_of(c), []).append(c)
    return t


def cases_of(group):
    return [c for c in cases() if group_of(c["inst"]) == tuple(group)]
