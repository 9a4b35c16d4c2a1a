"""Host side of the quantised model fronts (QuantEmbedding, QuantizedBertEmbeddings, QuantizedOPTLearnedPositionalEmbedding, opt_embed_front
and the C entry point oeh_embed_sum_quant) without a GPU: class and key names against the reference's recorded ones, the torch path against
the composed torch ops, the refusals of the module layer, the int8 table cache, the ABI, every refusal code in its order, the launch-form
names, and the position ids of the OPT front."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import _embed_ref as ER
from tests.conftest import load_golden

torch = pytest.importorskip("torch")
nn = torch.nn
F = torch.nn.functional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "oeh.h")
EINVAL, ENOTSUP, EALIGN = -22, -95, -14


def _qp(**quant_dict):
    from outeffhop_amd import quantization as Q

    qp = Q.val_qparams(Q.get_quant_config())
    qp["quant_dict"] = dict(quant_dict)
    return qp


def _bert_org(E=768, vocab=512, positions=512, pos_type="absolute"):
    return types.SimpleNamespace(word_embeddings=nn.Embedding(vocab, E, padding_idx=0), position_embeddings=nn.Embedding(positions, E),
                                 token_type_embeddings=nn.Embedding(2, E), LayerNorm=nn.LayerNorm(E, eps=1e-12), dropout=nn.Dropout(0.1),
                                 position_ids=torch.arange(positions).expand((1, -1)), position_embedding_type=pos_type)


class _OPTPositions(nn.Embedding):
    """transformers' OPTLearnedPositionalEmbedding as far as the constructor of the quantised class reads it."""

    def __init__(self, num_embeddings, embedding_dim):
        self.offset = 2
        super().__init__(num_embeddings + self.offset, embedding_dim)


def _strict_load(mod, keys):
    own = mod.state_dict()
    assert set(own) <= set(keys), sorted(set(own) - set(keys))
    res = mod.load_state_dict({k: own[k] if k in own else torch.tensor(0.5) for k in keys}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert sorted(mod.state_dict()) == sorted(k for k in keys if ".range_estimator.quantizer." not in k)


def test_quantize_model_rewrites_embedding():
    from outeffhop_amd import quantization as Q

    emb = nn.Embedding(50, 16, padding_idx=3)
    q = Q.quantize_model(emb, **_qp())
    assert type(q) is Q.QuantEmbedding and isinstance(q, nn.Embedding) and isinstance(q, Q.QuantizedModule)
    assert (q.num_embeddings, q.embedding_dim, q.padding_idx) == (50, 16, 3)
    assert q.weight.data_ptr() == emb.weight.data_ptr()  # shared, as for Linear
    assert isinstance(q.weight_quantizer, Q.QuantizationManager) and type(q.weight_quantizer.quantizer) is Q.SymmetricUniformQuantizer
    assert not isinstance(q.activation_quantizer, Q.QuantizationManager) and sum(1 for _ in q.activation_quantizer.parameters()) == 0
    x = torch.randn(2, 3)
    assert q.activation_quantizer(x) is x  # the reference's pass-through: a looked-up row is not quantised again
    import outeffhop_amd as P

    for name in ("QuantEmbedding", "QuantizedBertEmbeddings", "QuantizedOPTLearnedPositionalEmbedding", "opt_embed_front"):
        assert getattr(P, name) is getattr(Q, name)
    assert Q.FUSED_EMBED in (True, False)


def test_recorded_reference_state_dict_keys_load_strictly():
    from outeffhop_amd import quantization as Q

    g = load_golden("embed_front.npz")
    keys = lambda p: json.loads(str(g[p]))  # noqa: E731
    fresh = Q.quantize_model(nn.Embedding(7, 8, padding_idx=0), **_qp())
    assert sorted(fresh.state_dict()) == keys("qemb.keys")
    _strict_load(fresh, keys("qemb.keys_calibrated"))
    bert = Q.QuantizedBertEmbeddings(_bert_org(), **_qp())
    _strict_load(bert, keys("bert.keys"))
    for name in ("word_embeddings", "position_embeddings", "token_type_embeddings"):
        assert type(getattr(bert, name)) is Q.QuantEmbedding
    assert type(bert.LayerNorm) is Q.QuantLayerNorm and isinstance(bert.dropout, nn.Dropout) and bert.position_embedding_type == "absolute"
    assert type(bert.sum_input_token_type_embd_act_quantizer) is Q.QuantizedActivation and type(bert.sum_pos_embd_act_quantizer) is Q.QuantizedActivation
    pos = Q.QuantizedOPTLearnedPositionalEmbedding(_OPTPositions(64, 32), **_qp())
    assert sorted(pos.state_dict()) == keys("optpos.keys") and pos.offset == 2 and type(pos.quant_embedding) is Q.QuantEmbedding
    assert pos.quant_embedding.num_embeddings == 66
    _strict_load(pos, keys("opt.optpos_keys_calibrated"))
    # without position ids on the original the attribute is a plain None, and a relative position type skips the position table
    org = _bert_org(16, 20, 12, "relative_key")
    org.position_ids = None
    m = Q.QuantizedBertEmbeddings(org, **_qp())
    assert m.position_ids is None and "position_ids" not in m.state_dict() and m.position_embedding_type == "relative_key"


def test_torch_path_on_cpu_equals_the_composed_ops():
    from outeffhop_amd import quantization as Q

    torch.manual_seed(3)
    org = _bert_org(16, 50, 12)
    m = Q.QuantizedBertEmbeddings(org, **_qp()).eval()
    ids, tt = torch.randint(0, 50, (2, 5)), torch.randint(0, 2, (2, 5))
    ln = lambda s, w: F.layer_norm(s, (16,), w, org.LayerNorm.bias, 1e-12)  # noqa: E731
    want = ln(org.word_embeddings.weight[ids] + org.token_type_embeddings.weight[tt] + org.position_embeddings.weight[:5][None], org.LayerNorm.weight)
    assert torch.equal(m(ids, tt), want)
    assert torch.equal(m(ids), ln(org.word_embeddings.weight[ids] + org.token_type_embeddings.weight[0] + org.position_embeddings.weight[:5][None], org.LayerNorm.weight))
    dense = torch.randn(2, 5, 16)
    pid = torch.tensor([[4, 3, 2, 1, 0]])
    assert torch.equal(m(None, tt, pid, dense), ln(dense + org.token_type_embeddings.weight[tt] + org.position_embeddings.weight[pid], org.LayerNorm.weight))
    # quantised weights (the activation quantisers have no CPU path): F.embedding on the fake-quantised tables
    m.quantized_weights()
    wq = lambda e: e.weight_quantizer(e.weight.detach())  # noqa: E731
    want = ln(F.embedding(ids, wq(m.word_embeddings)) + F.embedding(tt, wq(m.token_type_embeddings)) + F.embedding(pid, wq(m.position_embeddings)),
              wq(m.LayerNorm))
    got = m(ids, tt, pid)
    assert torch.equal(got, want) and not torch.equal(wq(m.word_embeddings), org.word_embeddings.weight)
    assert m._fused_embed_calls == 0
    # a relative position type: two lookups
    m2 = Q.QuantizedBertEmbeddings(_bert_org(16, 50, 12, "relative_key"), **_qp()).eval()
    o2 = m2.word_embeddings.weight[ids] + m2.token_type_embeddings.weight[tt]
    assert torch.equal(m2(ids, tt), F.layer_norm(o2, (16,), m2.LayerNorm.weight, m2.LayerNorm.bias, 1e-12))
    # training mode: dropout is live, the torch ops run
    m.train()
    assert m(ids, tt).shape == (2, 5, 16) and m._fused_embed_calls == 0
    # the OPT front
    et = Q.quantize_model(nn.Embedding(50, 16, padding_idx=1), **_qp()).eval()
    pe = Q.QuantizedOPTLearnedPositionalEmbedding(_OPTPositions(20, 16), **_qp()).eval()
    qa = Q.QuantizedActivation(**_qp())
    mask = torch.tensor([[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]])
    rows = torch.tensor([[1, 1, 2, 3, 4], [2, 3, 4, 5, 6]])
    h = Q.opt_embed_front(et, pe, qa, ids, mask)
    assert torch.equal(h, et.weight[ids] + pe.quant_embedding.weight[rows]) and pe._fused_embed_calls == 0
    assert torch.equal(Q.opt_embed_front(et, pe, qa, None, mask, inputs_embeds=dense), dense + pe.quant_embedding.weight[rows])
    assert torch.equal(Q.opt_embed_front(et, pe, qa, ids, None), et.weight[ids] + pe.quant_embedding.weight[2:7][None])
    proj = nn.Linear(16, 16, bias=False)
    pe16 = Q.QuantizedOPTLearnedPositionalEmbedding(_OPTPositions(20, 16), **_qp()).eval()
    assert torch.equal(Q.opt_embed_front(et, pe16, qa, ids, mask, project_in=proj), proj(et.weight[ids]) + pe16.quant_embedding.weight[rows])


def test_layer_norm_embd_and_max_norm_are_refused():
    from outeffhop_amd import quantization as Q

    with pytest.raises(NotImplementedError, match="layer_norm_embd"):
        Q.QuantizedBertEmbeddings(_bert_org(16, 20, 12), **_qp(layer_norm_embd=True))
    Q.QuantizedBertEmbeddings(_bert_org(16, 20, 12), **_qp(layer_norm_embd=False, layer_norm_res_output=True))  # another class's key
    with pytest.raises(NotImplementedError, match="max_norm"):
        Q.quantize_model(nn.Embedding(20, 16, max_norm=1.0), **_qp())
    with pytest.raises(NotImplementedError, match="max_norm"):
        Q.QuantEmbedding(20, 16, max_norm=2.0, **_qp())
    m = Q.QuantizedBertEmbeddings(_bert_org(16, 20, 12), **_qp(Et=True))
    assert m.word_embeddings.weight_quantizer.init is Q.MSE_Estimator
    assert m.word_embeddings.weight_quantizer.range_estimator.opt_method == Q.OptMethod.golden_section
    assert m.token_type_embeddings.weight_quantizer.init is not Q.MSE_Estimator and m.position_embeddings.weight_quantizer.init is not Q.MSE_Estimator


def test_int8_table_cache_follows_the_weight_and_the_range():
    from outeffhop_amd import quantization as Q

    torch.manual_seed(5)
    q = Q.quantize_model(nn.Embedding(50, 16), **_qp()).eval()
    t0 = q.kernel_table()
    assert t0[0].data_ptr() == q.weight.data_ptr() and t0[1] is None  # full precision: the table as it is
    q.quantized_weights()
    t1 = q.kernel_table()  # the range is still being estimated: the fake-quantised table of get_params, no grid to apply
    assert t1[1] is None and torch.equal(t1[0], q.weight_quantizer.quantizer(q.weight.detach()))
    q.fix_ranges()
    tab, scale, lo, hi = q.kernel_table()
    qz = q.weight_quantizer.quantizer
    assert tab.dtype == torch.int8 and tab.shape == (50, 16) and (lo, hi) == (-128.0, 127.0) and scale == float(np.float32(float(qz.scale)))
    assert torch.equal(tab.float() * qz.scale, qz(q.weight.detach()))  # scale * idx IS the fake-quantised table
    assert q.kernel_table()[0] is tab and q.kernel_table()[0] is tab  # not rebuilt otherwise
    with torch.no_grad():
        q.weight[3, 3] += 1.0  # an in-place change of the table
    tab2 = q.kernel_table()[0]
    assert tab2 is not tab and tab2[3, 3] != tab[3, 3] and q.kernel_table()[0] is tab2
    q.weight_quantizer.set_quant_range(torch.tensor(-0.5), torch.tensor(0.5))  # a range change
    tab3, scale3, _, _ = q.kernel_table()
    assert tab3 is not tab2 and scale3 != scale and q.kernel_table()[0] is tab3
    # an unsigned grid (a table without a negative entry) has integers up to 255: no int8 form, the grid is applied on the fly
    u = Q.quantize_model(nn.Embedding(20, 8), **_qp()).eval()
    with torch.no_grad():
        u.weight.abs_()
    u.quantized_weights()
    u(torch.tensor([[1]]))
    u.fix_ranges()
    tab, scale, lo, hi = u.kernel_table()
    assert tab.data_ptr() == u.weight.data_ptr() and scale is not None and (lo, hi) == (0.0, 255.0)


def test_header_binding_and_struct_layout_agree(tmp_path):
    from outeffhop_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(oeh_[a-z0-9_]+)\s*\(", txt))
    assert {"oeh_embed_sum_quant", "oeh_embed_sum_variant"} <= declared and declared == set(_lib.EXPORTS)
    assert _lib.EXPORTS[-2:] == ("oeh_embed_sum_quant", "oeh_embed_sum_variant")  # appended
    lib = _lib.load()
    assert hasattr(lib, "oeh_embed_sum_quant") and hasattr(lib, "oeh_embed_sum_variant") and lib.oeh_abi_version() == 6
    for name, val in (("OEH_TAB_PLAIN", 0), ("OEH_TAB_GRID", 1), ("OEH_TAB_I8", 2), ("OEH_ID_I32", 0), ("OEH_ID_I64", 1)):
        assert re.search(rf"#define {name} {val}\b", txt) and getattr(_lib, name) == val
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HDR}"', "int main(void) {"]
    structs = (("oeh_embed_desc", _lib.oeh_embed_desc), ("oeh_embed_lookup", _lib.oeh_embed_lookup))
    for cname, st in structs:
        lines.append(f'  printf("{cname}.size %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], check=True, capture_output=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, st in structs:
        assert int(out[f"{cname}.size"]) == C.sizeof(st)
        for f, _ in st._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(st, f).offset, (cname, f)


def _desc(B=2, S=3, cols=72, dtype=2, n_tab=2, form=0, ids=4096, table=4096):
    from outeffhop_amd import _lib

    d = _lib.oeh_embed_desc()
    d.B, d.S, d.cols, d.dtype, d.n_tab, d.eps = B, S, cols, dtype, n_tab, 1e-5
    d.sum_stride = d.y_stride = cols
    for t in range(3):
        l = d.tab[t]
        l.table, l.ids, l.n_rows, l.row_stride, l.id_stride_b, l.id_stride_s = table, ids, 7, cols, S, 1
        l.form, l.scale, l.int_min, l.int_max = form, 0.01, -128.0, 127.0
    return d


def test_argument_validation_without_gpu():
    """Every refusal with fake pointers: none of these reaches a launch (B * S == 0 returns before it)."""
    from outeffhop_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(4096)

    def call(d, gamma=one, beta=one, sum_out=one, y=one, sum_idx=None, y_idx=None, bad=None):
        return lib.oeh_embed_sum_quant(None if d is None else C.byref(d), gamma, beta, sum_out, y, sum_idx, y_idx, bad, None)

    def edit(**kw):  # a descriptor with B * S == 0 (so that an accepted one does not launch) and the named edits
        d = _desc(B=0)
        for k, v in kw.items():
            obj, names = d, k.split("__")
            for n in names[:-1]:
                obj = getattr(obj, n) if not n.isdigit() else obj[int(n)]
            setattr(obj, names[-1], v)
        return d

    assert call(edit()) == 0 and call(edit(cols=8192, n_tab=3)) == 0 and call(edit(n_tab=1)) == 0 and call(_desc(S=0)) == 0
    assert call(edit(), gamma=None, beta=None) == 0  # no LayerNorm: y is the sum
    # OEH_EINVAL
    assert call(None) == EINVAL and call(edit(), y=None) == EINVAL and call(edit(tab__1__table=None)) == EINVAL
    assert call(edit(n_tab=0)) == EINVAL and call(edit(n_tab=4)) == EINVAL
    assert call(edit(tab__1__ids=None)) == EINVAL and call(edit(tab__0__ids=None)) == 0  # dense rows: lookup 0 only
    assert call(edit(cols=0)) == EINVAL and call(edit(B=-1)) == EINVAL and call(_desc(S=-1)) == EINVAL
    assert call(edit(tab__0__n_rows=-1)) == EINVAL and call(edit(tab__1__row_stride=-72)) == EINVAL and call(edit(tab__1__id_stride_s=-1)) == EINVAL
    assert call(edit(y_stride=-72)) == EINVAL and call(edit(sum_stride=-1)) == EINVAL
    assert call(edit(dtype=3)) == EINVAL and call(edit(dtype=7)) == EINVAL and call(edit(tab__0__id_dtype=2)) == EINVAL and call(edit(tab__1__form=3)) == EINVAL
    assert call(edit(tab__1__form=1, tab__1__scale=0.0)) == EINVAL and call(edit(tab__1__form=2, tab__1__scale=-1.0)) == EINVAL
    assert call(edit(tab__1__form=1, tab__1__scale=float("inf"))) == EINVAL and call(edit(tab__1__form=0, tab__1__scale=0.0)) == 0
    assert call(edit(tab__0__form=1, tab__0__int_min=127.0)) == EINVAL
    assert call(edit(fq_sum__1__enable=1, fq_sum__1__scale=0.0, fq_sum__1__qmax=255.0)) == EINVAL  # no grid
    assert call(edit(fq_sum__1__enable=1, fq_sum__1__scale=0.1, fq_sum__1__qmax=255.0, fq_sum__1__zero_point=300.0)) == EINVAL
    assert call(edit(fq_sum__1__enable=1, fq_sum__1__scale=0.1, fq_sum__1__qmax=255.0)) == 0
    assert call(edit(fq_sum__0__enable=1, fq_sum__0__scale=0.1, fq_sum__0__qmax=255.0)) == EINVAL  # no sum in front of lookup 0
    assert call(edit(fq_sum__2__enable=1, fq_sum__2__scale=0.1, fq_sum__2__qmax=255.0)) == EINVAL  # n_tab == 2
    assert call(edit(fq_out__enable=1, fq_out__scale=0.0, fq_out__qmax=255.0)) == EINVAL
    assert call(edit(), sum_idx=one) == EINVAL and call(edit(), y_idx=one) == EINVAL  # an index dump of a quantiser that is off
    assert call(edit(reserved=1)) == EINVAL and call(edit(reserved2=1)) == EINVAL and call(edit(tab__1__reserved=1)) == EINVAL
    assert call(edit(eps=-1e-5)) == EINVAL and call(edit(eps=float("nan"))) == EINVAL
    assert call(edit(eps=-1e-5), gamma=None, beta=None) == 0  # eps belongs to the LayerNorm
    assert call(edit(), gamma=None) == EINVAL  # beta without gamma
    assert call(edit(fq_out__enable=1, fq_out__scale=0.1, fq_out__qmax=255.0), gamma=None, beta=None) == EINVAL
    d = _desc()
    d.y_stride = 8
    assert call(d) == EINVAL  # rows of the output would overlap
    d = _desc()
    d.tab[0].ids, d.tab[0].n_rows = None, 5
    assert call(d) == EINVAL  # dense rows: fewer than B * S
    # OEH_ENOTSUP, behind every OEH_EINVAL
    assert call(edit(cols=8200)) == ENOTSUP and call(edit(cols=8193, dtype=0)) == ENOTSUP
    assert call(_desc(B=1 << 16, S=1 << 15)) == ENOTSUP
    assert call(edit(tab__1__form=2, tab__1__int_max=255.0, tab__1__int_min=0.0)) == ENOTSUP and call(edit(tab__1__form=2, tab__1__int_min=-32768.0)) == ENOTSUP
    assert call(edit(tab__1__form=1, tab__1__int_max=255.0, tab__1__int_min=0.0)) == 0  # a float table takes any grid
    big = dict(fq_out__enable=1, fq_out__scale=1e-3, fq_out__qmax=65535.0, fq_out__zero_point=30000.0)
    assert call(edit(**big)) == 0 and call(edit(**big), y_idx=one) == ENOTSUP  # a 16-bit grid: values yes, a uint8 dump no
    big = dict(fq_sum__1__enable=1, fq_sum__1__scale=1e-3, fq_sum__1__qmax=65535.0)
    assert call(edit(**big)) == 0 and call(edit(**big), sum_idx=one) == ENOTSUP
    assert call(edit(cols=8200, eps=-1.0)) == EINVAL and call(edit(cols=8200, tab__0__ids=4097)) == ENOTSUP  # the order
    # OEH_EALIGN, last
    assert call(edit(tab__1__ids=4098)) == EALIGN and call(edit(tab__1__ids=4100)) == 0 and call(edit(tab__1__ids=4100, tab__1__id_dtype=1)) == EALIGN
    assert call(edit(tab__0__form=2, tab__0__table=4098)) == EALIGN and call(edit(tab__0__form=2, tab__0__table=4100)) == 0
    assert call(edit(tab__0__table=4098)) == EALIGN and call(edit(tab__0__table=4098, dtype=0)) == 0
    assert call(edit(), y=C.c_void_p(4097)) == EALIGN and call(edit(), bad=C.c_void_p(4098)) == EALIGN


def test_launch_form_names_host_only():
    from outeffhop_amd import ops

    v = ops.embed_sum_variant
    assert v(32, 128, 768) == "embed/wave/CH4/T3/f32"
    assert v(32, 128, 768, torch.float16, n_tab=2) == "embed/wave/CH2/T2/f16"
    assert v(1, 1, 8, n_tab=1) == "embed/wave/CH1/T1/f32"
    assert v(4, 16, 1024) == "embed/wave/CH4/T3/f32" and v(4, 16, 1032) == "embed/block/CH2/T3/f32"
    assert v(4, 16, 8192) == "embed/block/CH8/T3/f32" and v(4, 16, 8192, torch.bfloat16) == "embed/block/CH4/T3/bf16"
    assert v(4, 16, 8200) is None and v(4, 16, 768, n_tab=4) is None and v(4, 16, 768, n_tab=0) is None
    assert v(4, 16, 770) == "embed/scalar/CH4/T3/f32" and v(4, 16, 772, torch.float16) == "embed/scalar/CH4/T3/f16"
    assert v(4, 16, 1) == "embed/scalar/CH1/T3/f32" and v(1, 1, 8191, n_tab=1) == "embed/scalar/CH32/T1/f32"
    assert v(4, 16, 768, row_stride=770) == "embed/scalar/CH4/T3/f32" and v(4, 16, 768, row_stride=776) == "embed/wave/CH4/T3/f32"
    assert v(4, 16, 768, table_offset=4) == "embed/scalar/CH4/T3/f32"  # a float table off the 16-byte vector
    # int8 tables: a row is read 4 (fp32) / 8 (16-bit) bytes at a time
    assert v(4, 16, 768, int8=True) == "embed/wave/CH4/T3/f32" and v(4, 16, 768, int8=True, table_offset=4) == "embed/wave/CH4/T3/f32"
    assert v(4, 16, 768, torch.float16, int8=True, table_offset=4) == "embed/scalar/CH4/T3/f16"
    assert v(4, 16, 768, torch.float16, int8=True, table_offset=8) == "embed/wave/CH2/T3/f16"
    assert v(4, 16, 768, int8=True, table_offset=2) is None  # refused: OEH_EALIGN
    assert v(4, 16, 768, int8=True, row_stride=770) == "embed/scalar/CH4/T3/f32"
    # the same form as the block tail's kernel for the same row, which is what makes the two bit-identical
    for cols, dt in ((8, torch.float32), (768, torch.float16), (1032, torch.float32), (8192, torch.bfloat16), (770, torch.float32)):
        assert v(4, 16, cols, dt).split("/")[1:3] == ops.resid_ln_variant(64, cols, dt).split("/")[1:3]


def test_no_cpu_fallback():
    from outeffhop_amd import _lib, ops

    with pytest.raises(_lib.OehError):
        ops.embed_sum_quant([ops.EmbedLookup(torch.zeros(4, 72), torch.zeros(2, 3, dtype=torch.int64))])
    with pytest.raises(ValueError):
        ops.embed_sum_quant([])


def test_opt_front_position_ids_left_padded_with_past():
    """quantized_opt.py:39-51: positions count the kept tokens along the WHOLE mask (past included) and are then cut to the new tokens; a
    padded position reads row offset - 1."""
    from outeffhop_amd import quantization as Q

    g = load_golden("embed_front.npz")
    meta = json.loads(str(g["meta_json"]))["opt"]
    pe = Q.QuantizedOPTLearnedPositionalEmbedding(_OPTPositions(meta["positions"], 8), **_qp())
    mask = torch.from_numpy(g["opt.mask"])
    assert mask[1, 0] == 0 and mask[1, -1] == 1 and mask[0].all()  # left-padded
    got = pe.position_ids(mask, 5)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), g["opt.positions_past5"]) and np.array_equal(got.numpy(), ER.opt_positions(g["opt.mask"], 5))
    assert got[1, 0] == 1 and got[1, -1] == meta["lengths"][1] - 1 + 2 and got[0, 0] == 5 + 2
    assert np.array_equal(pe.position_ids(mask.bool()).numpy(), ER.opt_positions(g["opt.mask"]))
    # through the front: the new tokens of a cached step read those rows
    et = Q.quantize_model(nn.Embedding(50, 8), **_qp()).eval()
    qa = Q.QuantizedActivation(**_qp())
    ids = torch.randint(0, 50, (2, mask.shape[1] - 5))
    h = Q.opt_embed_front(et, pe.eval(), qa, ids, mask, past_key_values_length=5)
    assert torch.equal(h, et.weight[ids] + pe.quant_embedding.weight[got])
