"""The refusal matrix of the attention entry points (include/oeh.h) - no GPU needed: one valid descriptor, one mutation (or an ordered pair
of mutations) at a time, through every entry point that judges a descriptor.  Every cell's value is written out below: a return code, or for
the host-only name / size functions the name, None or the byte count.  The entry points share their descriptor predicates
(outeffhop_amd/csrc/oeh_desc.h) but keep their own ORDER of refusals and their own codes: the pairs pin the order.

A cell marked X is not called: that entry point does not refuse the mutation and would go on to launch, and nothing here may reach a launch."""
import ctypes as C
import math

import pytest

E, N, A = -22, -95, -14  # OEH_EINVAL, OEH_ENOTSUP, OEH_EALIGN
X = "not refused: not called"
B, H, S, D = 2, 3, 80, 64

# the columns of TABLE (the decode family is called with Sq = 1)
ENTRIES = ("fwd_ex", "variant_ex", "decode", "decode_fq", "decode_work_bytes", "decode_variant", "decode_fq_variant", "fwd_train",
           "fwd_train_dropout", "bwd", "bwd_dropout", "bwd_work_bytes", "dropout_mask", "calibrate")
DECODE = ENTRIES[2:7]


def _L():
    from outeffhop_amd import _lib

    return _lib


class Case:
    """The valid call: B=2, H=3, Sq=Sk=80 (decode: Sq=1), D=64, fp16, contiguous strides, every pointer 256."""

    def __init__(self, Sq):
        L = _L()
        d = self.d = L.oeh_attn_desc()
        d.B, d.H, d.Sq, d.Sk, d.D, d.dtype, d.o_dtype = B, H, Sq, S, D, 0, 0
        d.q_stride[:] = d.o_stride[:] = [H * Sq * D, Sq * D, D]
        d.k_stride[:] = d.v_stride[:] = [H * S * D, S * D, D]
        d.scale, d.softmax_base, d.eta = 0.125, 1, 1.0
        d.mask_min = -3.4028234663852886e38
        self.null_desc = False
        self.p = dict.fromkeys(("q", "k", "v", "o", "work", "lse", "dout", "dq", "dk", "dv", "keep"), 256)
        self.fq = None
        self.opts = None
        self.drop = L.oeh_dropout(p=0.1, seed=7)

    def quantisers(self):
        if self.fq is None:
            self.fq = _L().oeh_fq_desc()
            for f in (self.fq.scores, self.fq.probs, self.fq.ctx):
                f.enable, f.scale, f.zero_point, f.qmax = 0, 0.05, 128.0, 255.0
            self.fq.scores.enable = 1
        return self.fq

    def options(self):
        if self.opts is None:
            self.opts = _L().oeh_attn_opts()
        return self.opts


def _set(**kw):
    def m(c):
        for name, val in kw.items():
            setattr(c.d, name, val)
    return m


def _ptr(name, val):
    def m(c):
        c.p[name] = val
    return m


def _stride(field, i, val):
    def m(c):
        getattr(c.d, field)[i] = val
    return m


def _fq(which, **kw):
    def m(c):
        fq = c.quantisers()
        if which is None:
            for name, val in kw.items():
                setattr(fq, name, val)
            return
        f = getattr(fq, which)
        f.enable = 1
        for name, val in kw.items():
            setattr(f, name, val)
    return m


def _null_desc(c):
    c.null_desc = True


def _reserved(c):
    c.options().reserved[1] = 1


def _pv_pairs(c):
    c.options().pv_pairs = 1


def _drop_p1(c):
    c.drop.p = 1.0


def _causal_long(c):
    c.d.causal, c.d.Sq = 1, c.d.Sk + 8


MUTATIONS = {
    "null descriptor": (_null_desc,),
    **{f"null {n}": (_ptr(n, None),) for n in ("q", "k", "v", "o", "work", "lse", "dout", "dq", "dk", "dv", "keep")},
    **{f"{n} = 0": (_set(**{n: 0}),) for n in ("B", "H", "Sq", "Sk", "D")},
    "dtype = 7": (_set(dtype=7),),
    "softmax_base = 5": (_set(softmax_base=5),),
    "key_pad_mask with dtype BF16": (_set(key_pad_mask=256, key_pad_dtype=1, key_pad_stride=S),),
    "full_mask with dtype BF16": (_set(full_mask=256, full_mask_dtype=1),),
    "q_stride[0] = -1": (_stride("q_stride", 0, -1),),
    "v_stride[1] = 2^32": (_stride("v_stride", 1, 1 << 32),),
    "k at 264": (_ptr("k", 264),),
    "k_stride[2] = 12": (_stride("k_stride", 2, 12),),
    "scale_div = 0, scale = inf": (_set(scale_div=0.0, scale=math.inf),),
    "scale_div = -4": (_set(scale_div=-4.0),),
    "scale_div = nan": (_set(scale_div=math.nan),),
    "scale_div = inf": (_set(scale_div=math.inf),),
    "clip with gamma = +0.01": (_set(clip=1, gamma=0.01),),
    "causal with Sq > Sk": (_causal_long,),
    "D = 48": (_set(D=48),),
    "fp32 storage": (_set(dtype=2, o_dtype=2),),
    "INT8 storage": (_set(dtype=3, o_dtype=0),),
    "o_dtype F32": (_set(o_dtype=2),),
    "gate set": (_set(gate=256),),
    "gate_hidden set": (_set(gate_hidden=256),),
    "fq: scale 0": (_fq("scores", scale=0.0),),
    "fq: scale = inf": (_fq("probs", scale=math.inf),),
    "fq: qmax = inf": (_fq("ctx", qmax=math.inf),),
    "fq: zero point > qmax": (_fq("probs", zero_point=300.0),),
    "fq: dump_idx with qmax 1023": (_fq("scores", dump_idx=256, qmax=1023.0),),
    "fq: ctx_emit_index without ctx": (_fq(None, ctx_emit_index=1),),
    "opts: a reserved word": (_reserved,),
    "opts: pv_pairs on fp16": (_pv_pairs,),
    # the pairs: which refusal comes first
    "stride 2^32 + misaligned pointer": (_stride("q_stride", 0, 1 << 32), _ptr("k", 264)),
    "null q + softmax_base = 5": (_ptr("q", None), _set(softmax_base=5)),
    "reserved opts word + null descriptor": (_reserved, _null_desc),
    "fp32 storage + D = 48": (_set(dtype=2, o_dtype=2), _set(D=48)),
    "dropout p = 1.0 + null descriptor": (_drop_p1, _null_desc),
}


def call(entry, muts):
    L = _L()
    lib = L.load()
    c = Case(1 if entry in DECODE else S)
    for m in muts:
        m(c)
    vp = lambda name: None if c.p[name] is None else C.c_void_p(c.p[name])  # noqa: E731
    d = None if c.null_desc else C.byref(c.d)
    fq = None if c.fq is None else C.byref(c.fq)
    opts = None if c.opts is None else C.byref(c.opts)
    drop = C.byref(c.drop)
    name = lambda r: None if r is None else r.decode()  # noqa: E731
    q, k, v, o = vp("q"), vp("k"), vp("v"), vp("o")
    st = lambda: (C.c_int64 * 3)(H * S * D, S * D, D)  # noqa: E731
    if entry == "fwd_ex":
        return lib.oeh_attn_fwd_ex(d, opts, q, k, v, o, fq, None)
    if entry == "variant_ex":
        return name(lib.oeh_attn_variant_ex(d, opts, fq))
    if entry == "decode":
        return lib.oeh_attn_decode(d, 0, q, k, v, o, vp("work"), None)
    if entry == "decode_fq":
        return lib.oeh_attn_decode_fq(d, fq, 0, q, k, v, o, vp("work"), None)
    if entry == "decode_work_bytes":
        return lib.oeh_attn_decode_work_bytes(d, 0)
    if entry == "decode_variant":
        return name(lib.oeh_attn_decode_variant(d, 0))
    if entry == "decode_fq_variant":
        return name(lib.oeh_attn_decode_fq_variant(d, fq, 0))
    if entry == "fwd_train":
        return lib.oeh_attn_fwd_train(d, q, k, v, o, vp("lse"), None)
    if entry == "fwd_train_dropout":
        return lib.oeh_attn_fwd_train_dropout(d, drop, q, k, v, o, vp("lse"), None)
    if entry == "bwd":
        return lib.oeh_attn_bwd(d, q, k, v, o, vp("dout"), st(), vp("lse"), vp("dq"), st(), vp("dk"), st(), vp("dv"), st(), vp("work"), None)
    if entry == "bwd_dropout":
        return lib.oeh_attn_bwd_dropout(d, drop, q, k, v, o, vp("dout"), st(), vp("lse"), vp("dq"), st(), vp("dk"), st(), vp("dv"), st(),
                                        vp("work"), None)
    if entry == "bwd_work_bytes":
        return lib.oeh_attn_bwd_work_bytes(d)
    if entry == "dropout_mask":
        return lib.oeh_attn_dropout_mask(d, drop, vp("keep"), None)
    assert entry == "calibrate"  # the context form: q, k, v and the fp32 context output are all judged
    return lib.oeh_attn_calibrate(d, q, k, v, o, 2, None, None, 8, 1e-8, 0.0, 100.0, 0.1, 1, None, None, None)


TABLE = {
    # fwd_ex, variant_ex, decode, decode_fq, decode_work_bytes, decode_variant, decode_fq_variant, fwd_train, fwd_train_dropout, bwd, bwd_dropout, bwd_work_bytes, dropout_mask, calibrate
    'null descriptor': (E, None, E, E, E, None, None, E, E, E, E, E, E, E),
    'null q': (E, 'fast16/NT8/D64/f16', E, E, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', E, E, E, E, 3840, X, E),
    'null k': (E, 'fast16/NT8/D64/f16', E, E, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', E, E, E, E, 3840, X, E),
    'null v': (E, 'fast16/NT8/D64/f16', E, E, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', E, E, E, E, 3840, X, E),
    'null o': (E, 'fast16/NT8/D64/f16', E, E, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', E, E, E, E, 3840, X, E),
    'null work': (X, 'fast16/NT8/D64/f16', E, E, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', X, X, E, E, 3840, X, X),
    'null lse': (X, 'fast16/NT8/D64/f16', X, X, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', E, E, E, E, 3840, X, X),
    'null dout': (X, 'fast16/NT8/D64/f16', X, X, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', X, X, E, E, 3840, X, X),
    'null dq': (X, 'fast16/NT8/D64/f16', X, X, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', X, X, E, E, 3840, X, X),
    'null dk': (X, 'fast16/NT8/D64/f16', X, X, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', X, X, E, E, 3840, X, X),
    'null dv': (X, 'fast16/NT8/D64/f16', X, X, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', X, X, E, E, 3840, X, X),
    'null keep': (X, 'fast16/NT8/D64/f16', X, X, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', X, X, X, X, 3840, E, X),
    'B = 0': (E, None, E, E, E, None, None, E, E, E, E, E, E, E),
    'H = 0': (E, None, E, E, E, None, None, E, E, E, E, E, E, E),
    'Sq = 0': (E, None, E, E, E, None, None, E, E, E, E, E, E, E),
    'Sk = 0': (E, None, E, E, E, None, None, E, E, E, E, E, E, E),
    'D = 0': (E, None, E, E, E, None, None, E, E, E, E, E, X, N),
    'dtype = 7': (E, None, E, E, E, None, None, E, E, E, E, E, X, E),
    'softmax_base = 5': (E, 'fast16/NT8/D64/f16', E, E, E, None, None, E, E, E, E, E, X, E),
    'key_pad_mask with dtype BF16': (E, 'fast16/NT8/D64/f16', E, E, E, None, None, E, E, E, E, E, X, E),
    'full_mask with dtype BF16': (E, 'mfma16/NT8/D64/f16', N, N, N, None, None, E, E, E, E, E, X, E),
    'q_stride[0] = -1': (N, 'fast16/NT8/D64/f16', N, N, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', N, N, N, N, N, X, A),
    'v_stride[1] = 2^32': (N, 'fast16/NT8/D64/f16', N, N, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', N, N, N, N, N, X, X),
    'k at 264': (X, 'fast16/NT8/D64/f16', A, A, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', A, A, A, A, 3840, X, A),
    'k_stride[2] = 12': (X, 'fast16/NT8/D64/f16', A, A, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', A, A, A, A, 3840, X, A),
    'scale_div = 0, scale = inf': (X, 'mfma16/NT8/D64/f16', N, N, N, None, None, E, E, E, E, E, X, X),
    'scale_div = -4': (X, 'mfma16/NT8/D64/f16', N, N, N, None, None, X, X, X, X, 3840, X, X),
    'scale_div = nan': (X, 'mfma16/NT8/D64/f16', N, N, N, None, None, E, E, E, E, E, X, X),
    'scale_div = inf': (X, 'mfma16/NT8/D64/f16', N, N, N, None, None, E, E, E, E, E, X, X),
    'clip with gamma = +0.01': (X, 'mfma16/NT8/D64/f16', N, N, N, None, None, X, X, X, X, 3840, X, X),
    'causal with Sq > Sk': (X, 'mfma16/NT8/D64/f16', N, N, N, None, None, X, X, X, X, 4224, X, X),
    'D = 48': (X, 'generic', N, N, N, None, None, N, N, N, N, N, X, N),
    'fp32 storage': (X, 'fast16/NT8/D64/f32', N, N, N, None, None, N, N, N, N, N, X, X),
    'INT8 storage': (E, None, N, N, N, None, None, N, N, N, N, N, X, E),
    'o_dtype F32': (X, 'fast16/NT8/D64/f16', X, X, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', N, N, N, N, N, X, X),
    'gate set': (X, 'fast16/NT8/D64/f16', X, X, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', N, N, N, N, N, X, X),
    'gate_hidden set': (E, 'fast16/NT8/D64/f16', N, N, N, None, None, N, N, N, N, N, X, X),
    'fq: scale 0': (E, 'mfma16/NT8/D64/f16/fq', X, E, 1584, 'decode16/SP1/D64/f16', None, X, X, X, X, 3840, X, X),
    'fq: scale = inf': (X, 'fast16/NT8/D64/f16/fq', X, E, 1584, 'decode16/SP1/D64/f16', None, X, X, X, X, 3840, X, X),
    'fq: qmax = inf': (X, 'mfma16/NT8/D64/f16/fq', X, E, 1584, 'decode16/SP1/D64/f16', None, X, X, X, X, 3840, X, X),
    'fq: zero point > qmax': (E, 'fast16/NT8/D64/f16/fq', X, E, 1584, 'decode16/SP1/D64/f16', None, X, X, X, X, 3840, X, X),
    'fq: dump_idx with qmax 1023': (N, 'mfma16/NT8/D64/f16/fq', X, N, 1584, 'decode16/SP1/D64/f16', None, X, X, X, X, 3840, X, X),
    'fq: ctx_emit_index without ctx': (E, 'mfma16/NT8/D64/f16/fq', X, N, 1584, 'decode16/SP1/D64/f16', None, X, X, X, X, 3840, X, X),
    'opts: a reserved word': (E, None, X, X, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', X, X, X, X, 3840, X, X),
    'opts: pv_pairs on fp16': (N, None, X, X, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', X, X, X, X, 3840, X, X),
    'stride 2^32 + misaligned pointer': (N, 'fast16/NT8/D64/f16', N, N, 1584, 'decode16/SP1/D64/f16', 'decode16/SP1/D64/f16', N, N, N, N, N, X, A),
    'null q + softmax_base = 5': (E, 'fast16/NT8/D64/f16', E, E, E, None, None, E, E, E, E, E, X, E),
    'reserved opts word + null descriptor': (E, None, E, E, E, None, None, E, E, E, E, E, E, E),
    'fp32 storage + D = 48': (X, 'generic', N, N, N, None, None, N, N, N, N, N, X, N),
    'dropout p = 1.0 + null descriptor': (E, None, E, E, E, None, None, E, E, E, E, E, E, E),
}


def test_the_table_covers_every_mutation_and_only_refusals_or_host_only_calls():
    assert set(TABLE) == set(MUTATIONS)
    host_only = {"variant_ex", "decode_work_bytes", "decode_variant", "decode_fq_variant", "bwd_work_bytes"}
    for mut, row in TABLE.items():
        assert len(row) == len(ENTRIES), mut
        for entry, want in zip(ENTRIES, row):
            assert want is X or entry in host_only or want in (E, N, A), (mut, entry, want)
        assert any(want is not X for want in row), mut


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_refusal(mut):
    for entry, want in zip(ENTRIES, TABLE[mut]):
        if want is not X:
            assert call(entry, MUTATIONS[mut]) == want, (mut, entry)
