"""The host modules of the quantised model fronts - QuantEmbedding, QuantizedBertEmbeddings, QuantizedOPTLearnedPositionalEmbedding,
opt_embed_front - on the GPU against the reference's recorded run (tests/golden/embed_front.npz, written by
tests/golden/make_embed_golden.py; weights and ids regenerated from the seeds in it by tests/_embed_ref.py).  `-m gpu`.

Calibrate -> fix -> eval through OUR classes: every range buffer within the bound tests/test_ln_modules_gpu.py applies to the same quantity
(1e-6 relative), the indices of every quantised sum EQUAL to the reference's, the LayerNorm's output indices by tests/_ln_ref.py's tie-band
rule around the float64 evaluation of the stored sum with the reference's own recorded distance from float64 as the unit (the fixture's seed
keeps the reference itself inside that rule: make_embed_golden.py checks it).  The fused launch is counted, and every condition that rules
it out takes the torch ops and gives the same bits."""
import json
import types

import numpy as np
import pytest

from tests import _embed_ref as ER
from tests import _ln_ref as R
from tests.conftest import load_golden

torch = pytest.importorskip("torch")
nn = torch.nn
pytestmark = pytest.mark.gpu
RANGE_TOL = 1e-6  # tests/test_ln_modules_gpu.py: test_bert_self_output_estimates_the_reference_ranges


@pytest.fixture(scope="module")
def Q():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import quantization

    return quantization


@pytest.fixture(scope="module")
def fx():
    g = load_golden("embed_front.npz")
    return g, json.loads(str(g["meta_json"]))


def _qp(Q):
    cfg = Q.get_quant_config()
    cfg.act_quant.options = dict(percentile=99.999)  # validate_clm.py:444-454, as the fixture's run
    qp = Q.val_qparams(cfg)
    qp["quant_dict"] = {}
    return qp


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _load_weights(holder, seed):
    shapes = {k: tuple(v.shape) for k, v in holder.state_dict().items()}
    holder.load_state_dict({k: torch.from_numpy(v) for k, v in ER.front_state_dict(shapes, seed).items()}, strict=True)


def _managers(Q, mod):
    return {n: m for n, m in mod.named_modules() if isinstance(m, Q.QuantizationManager)}


def _check_ranges(Q, mod, g, stage):
    worst, seen = 0.0, 0
    for n, mg in _managers(Q, mod).items():
        for buf, key in (("_delta", "delta"), ("_zero_float", "zero_float")):
            k = f"{stage}.q.{n}.{key}"
            if k in g.files:
                want, got = float(g[k]), float(getattr(mg.quantizer, buf))
                worst, seen = max(worst, abs(got - want) / abs(want)), seen + 1
                assert abs(got - want) <= RANGE_TOL * abs(want), (stage, n, key, got, want)
    assert seen == sum(1 for k in g.files if k.startswith(stage + ".q.") and (k.endswith(".delta") or k.endswith(".zero_float")))
    return worst


def _spec(g, prefix, n):
    from outeffhop_amd.ops import FakeQuantSpec

    return FakeQuantSpec.from_delta(float(g[f"{prefix}.final.q.{n}.delta"]), float(g[f"{prefix}.final.q.{n}.zero_float"]))


def _deq(idx, sp):
    return (np.float32(sp.scale) * (np.asarray(idx, dtype=np.float32) - np.float32(sp.zero_point))).astype(np.float32)


def _idx_of(y, sp):
    """The indices of an fp32 tensor that sits on the grid (checked: every value is scale * (idx - zp))."""
    v = y.detach().float().cpu().numpy()
    idx = np.rint(v.astype(np.float64) / sp.scale) + sp.zero_point
    R.check_on_grid(v, idx, sp.scale, sp.zero_point)
    return idx


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


# ---- BERT -----------------------------------------------------------------------------------------------------------------------------
def _bert(Q, meta):
    m = meta["bert"]
    E = m["E"]
    org = types.SimpleNamespace(word_embeddings=nn.Embedding(m["vocab"], E, padding_idx=0), position_embeddings=nn.Embedding(m["positions"], E),
                                token_type_embeddings=nn.Embedding(m["types"], E), LayerNorm=nn.LayerNorm(E, eps=m["eps"]), dropout=nn.Dropout(0.0),
                                position_ids=torch.arange(m["positions"]).expand((1, -1)), position_embedding_type="absolute")
    _load_weights(nn.ModuleDict({k: v for k, v in vars(org).items() if isinstance(v, nn.Module) and k != "dropout"}), m["weight_seed"])
    batch = lambda seeds: (_cuda(ER.token_ids(seeds[0], (m["B"], m["S"]), m["vocab"])), _cuda(ER.token_ids(seeds[1], (m["B"], m["S"]), m["types"])))  # noqa: E731
    return Q.QuantizedBertEmbeddings(org, **_qp(Q)).cuda().eval(), batch, m


@pytest.fixture(scope="module")
def bert_run(Q, fx):
    """Our class calibrated on the fixture's two batches and frozen; the worst range distance per stage; the launches counted on the way."""
    g, meta = fx
    mod, batch, m = _bert(Q, meta)
    mod.set_quant_state(True, True)
    worst = []
    with torch.no_grad():
        for i, seeds in enumerate(m["calib_seeds"]):
            mod(*batch(seeds))
            worst.append(_check_ranges(Q, mod, g, f"bert.after{i + 1}"))
        calls_estimating = mod._fused_embed_calls
        mod.fix_ranges()
        worst.append(_check_ranges(Q, mod, g, "bert.final"))
    return mod, batch, m, worst, calls_estimating


def test_bert_embeddings_estimate_the_reference_ranges(Q, fx, bert_run):
    mod, batch, m, worst, calls_estimating = bert_run
    assert calls_estimating == 0  # ranges still moving: the torch ops with the estimators
    print(f"\nQuantizedBertEmbeddings calibration: worst relative distance of a range buffer from the reference's per stage {worst} (limit {RANGE_TOL})")
    # the frozen word table is held as int8 indices: a quarter of the fp32 copy
    tab, scale, lo, hi = mod.word_embeddings.kernel_table()
    assert tab.dtype == torch.int8 and tab.shape == (m["vocab"], m["E"]) and (lo, hi) == (-128.0, 127.0)


def _torch_path_sums(Q, mod, ids, tt):
    """The module's torch path with a hook on each sum quantiser (a hook rules the fused launch out): their inputs' indices, and y."""
    from outeffhop_amd import ops

    rec, hs = {}, []
    for name in ("sum_input_token_type_embd_act_quantizer", "sum_pos_embd_act_quantizer"):
        q = getattr(mod, name)
        hs.append(q.register_forward_hook(lambda md, inp, out, name=name: rec.__setitem__(name, (inp[0].detach().clone(), out.detach().clone()))))
    before = mod._fused_embed_calls
    try:
        with torch.no_grad():
            y = mod(ids, tt)
    finally:
        for h in hs:
            h.remove()
    assert mod._fused_embed_calls == before
    idx = {n: ops.fake_quant(rec[n][0], getattr(mod, n).fixed_spec(), want_idx=True)[1].cpu().numpy() for n in rec}
    return idx, rec, y


def test_bert_embeddings_fixed_ranges_against_the_reference(Q, fx, bert_run):
    from outeffhop_amd import ops

    g, meta = fx
    mod, batch, m, _, _ = bert_run
    ids, tt = batch(m["eval_seeds"])
    assert np.array_equal(ids.cpu().numpy(), g["bert.input_ids"]) and np.array_equal(tt.cpu().numpy(), g["bert.token_type_ids"])
    names = ("sum_input_token_type_embd_act_quantizer", "sum_pos_embd_act_quantizer")
    s1, s2, so = (_spec(g, "bert", n + ".activation_quantizer") for n in (*names, "LayerNorm"))
    before = mod._fused_embed_calls
    with torch.no_grad():
        y = mod(ids, tt)
    assert mod._fused_embed_calls == before + 1 and mod.LayerNorm._fused_ln_calls == 0 and y.shape == (m["B"], m["S"], m["E"])
    # the sums: the torch path's, through hooks, and the kernel's own dump - both EQUAL to the reference's
    idx, rec, y_torch = _torch_path_sums(Q, mod, ids, tt)
    assert np.array_equal(idx[names[0]], g["bert.sum1_idx"]), "word + token type: indices differ from the reference's"
    assert np.array_equal(idx[names[1]], g["bert.sum2_idx"]), "+ position: indices differ from the reference's"
    pos = mod.position_ids[:, :m["S"]]
    lk = [ops.EmbedLookup(*((e.kernel_table()[0], i) + e.kernel_table()[1:])) for e, i in
          ((mod.word_embeddings, ids), (mod.token_type_embeddings, tt), (mod.position_embeddings, pos))]
    w, b = mod.LayerNorm.get_params()
    s, y_k, sidx, yidx = ops.embed_sum_quant(lk, w, b, mod.LayerNorm.eps, fq_sums=[getattr(mod, n).fixed_spec() for n in names], fq_out=mod.LayerNorm.out_spec(),
                                             dtype=torch.float32, want_idx=True)
    assert np.array_equal(sidx.cpu().numpy(), g["bert.sum2_idx"]) and np.array_equal(_bits(s), _deq(g["bert.sum2_idx"], s2).view(np.int32))
    assert np.array_equal(_bits(y_k), _bits(y)) and np.array_equal(_bits(y_torch), _bits(y))  # one launch form: the fused and the separate ops agree bit for bit
    # the LayerNorm's output: the tie-band rule around float64 on the stored sum, and against the reference's indices
    y64 = R.layer_norm64(_deq(g["bert.sum2_idx"], s2), w.detach().float().cpu().numpy(), b.detach().float().cpu().numpy(), mod.LayerNorm.eps)
    oidx = _idx_of(y, so)
    assert np.array_equal(oidx, yidx.cpu().numpy().astype(np.float64))
    share, off = R.check_indices(oidx, y64, so.scale, so.zero_point, so.qmax, float(g["bert.err_ref"]), ref_idx=g["bert.out_idx"])
    assert float(g["bert.band_ref"]) <= 1e-3  # the reference alone stays inside the cap (the fixture's seed)
    print(f"\nQuantizedBertEmbeddings fixed: tie band {share:.1e} of the elements, LayerNorm indices that differ from the reference's {off:.1e}")


def test_bert_embeddings_fusing_conditions(Q, fx, bert_run):
    """_fused_embed_calls rises only under the fusing conditions; each condition that rules the launch out gives the same bits by torch ops."""
    g, meta = fx
    mod, batch, m, _, _ = bert_run
    ids, tt = batch(m["eval_seeds"])
    with torch.no_grad():
        n0 = mod._fused_embed_calls
        want = mod(ids, tt)
        assert mod._fused_embed_calls == n0 + 1
        Q.FUSED_EMBED = False
        try:
            got = mod(ids, tt)
        finally:
            Q.FUSED_EMBED = True
        assert mod._fused_embed_calls == n0 + 1 and np.array_equal(_bits(got), _bits(want)), "FUSED_EMBED = False"
        mod.train()  # (the fixture's dropout has p = 0: training changes the path, not the values)
        try:
            got = mod(ids, tt)
        finally:
            mod.eval()
        assert mod._fused_embed_calls == n0 + 1 and np.array_equal(_bits(got), _bits(want)), "training mode"
        for member in (mod.word_embeddings, mod.sum_pos_embd_act_quantizer, mod.LayerNorm):
            h = member.register_forward_hook(lambda *a: None)
            try:
                got = mod(ids, tt)
            finally:
                h.remove()
            assert mod._fused_embed_calls == n0 + 1 and np.array_equal(_bits(got), _bits(want)), "a forward hook"
        # dense rows in the place of the word lookup: fused, the same bits
        dense = nn.functional.embedding(ids, mod.word_embeddings.get_params()[0])
        got = mod(None, tt, None, dense)
        assert mod._fused_embed_calls == n0 + 2 and np.array_equal(_bits(got), _bits(want)), "inputs_embeds"
        # explicit position ids and the default token types (zeros)
        got = mod(ids, tt, mod.position_ids[:, :m["S"]].expand(m["B"], -1).contiguous())
        assert mod._fused_embed_calls == n0 + 3 and np.array_equal(_bits(got), _bits(want))
        # a quantiser that is still estimating: the torch ops, range estimation included - the module's output is the composed ops' on the
        # range the estimator moved to
        from outeffhop_amd import ops

        idx, rec, _ = _torch_path_sums(Q, mod, ids, tt)
        q2 = mod.sum_pos_embd_act_quantizer
        qz = q2.activation_quantizer.quantizer
        kept = (qz._delta, qz._zero_float)
        q2.estimate_ranges()
        try:
            got = mod(ids, tt)
            assert mod._fused_embed_calls == n0 + 3 and qz._delta is not kept[0]
            s2 = ops.fake_quant(rec["sum_pos_embd_act_quantizer"][0], qz.spec())
            assert np.array_equal(_bits(got), _bits(mod.LayerNorm(s2))), "a still-estimating quantiser"
        finally:
            qz._delta, qz._zero_float = kept
            q2.fix_ranges()
        assert np.array_equal(_bits(mod(ids, tt)), _bits(want)) and mod._fused_embed_calls == n0 + 4
    # autograd on the tables: the torch ops (the kernel is forward-only)
    mod.full_precision()  # (a quantised module's eval-mode table is a detached cached copy: no gradient to show)
    try:
        mod.word_embeddings.weight.requires_grad_(True)
        out = mod(ids, tt)
        assert mod._fused_embed_calls == n0 + 4 and out.requires_grad
    finally:
        mod.word_embeddings.weight.requires_grad_(False)
        mod.quantized()


# ---- OPT ------------------------------------------------------------------------------------------------------------------------------
class _OPTPositions(nn.Embedding):
    """transformers' OPTLearnedPositionalEmbedding as far as the constructor of the quantised class reads it."""

    def __init__(self, num_embeddings, embedding_dim):
        self.offset = 2
        super().__init__(num_embeddings + self.offset, embedding_dim)


@pytest.fixture(scope="module")
def opt_run(Q, fx):
    g, meta = fx
    m = meta["opt"]
    org = nn.ModuleDict(dict(embed_tokens=nn.Embedding(m["vocab"], m["E"], padding_idx=1), embed_positions=_OPTPositions(m["positions"], m["E"])))
    _load_weights(org, m["weight_seed"])
    qp = _qp(Q)
    front = nn.ModuleDict(dict(embed_tokens=Q.quantize_model(org["embed_tokens"], **qp), embed_positions=Q.QuantizedOPTLearnedPositionalEmbedding(org["embed_positions"], **qp),
                               embed_sum_act_quantizer=Q.QuantizedActivation(**qp))).cuda().eval()
    mask = _cuda(g["opt.mask"])
    run = lambda ids: Q.opt_embed_front(front["embed_tokens"], front["embed_positions"], front["embed_sum_act_quantizer"], ids, mask)  # noqa: E731
    for md in front.values():
        md.quantized()
    worst = []
    with torch.no_grad():
        for i, seed in enumerate(m["calib_seeds"]):
            run(_cuda(ER.token_ids(seed, (m["B"], m["S"]), m["vocab"])))
            worst.append(_check_ranges(Q, front, g, f"opt.after{i + 1}"))
        calls_estimating = front["embed_positions"]._fused_embed_calls
        for md in front.values():
            md.fix_ranges()
        worst.append(_check_ranges(Q, front, g, "opt.final"))
    return front, run, mask, m, worst, calls_estimating


def test_opt_front_against_the_reference(Q, fx, opt_run):
    g, meta = fx
    front, run, mask, m, worst, calls_estimating = opt_run
    assert calls_estimating == 0
    print(f"\nOPT front calibration: worst relative distance of a range buffer from the reference's per stage {worst} (limit {RANGE_TOL})")
    ids = _cuda(ER.token_ids(m["eval_seed"], (m["B"], m["S"]), m["vocab"]))
    assert np.array_equal(ids.cpu().numpy(), g["opt.input_ids"])
    pe = front["embed_positions"]
    sp = _spec(g, "opt", "embed_sum_act_quantizer.activation_quantizer")
    with torch.no_grad():
        n0 = pe._fused_embed_calls
        h = run(ids)
        assert pe._fused_embed_calls == n0 + 1 and h.shape == (m["B"], m["S"], m["E"])
        assert np.array_equal(_idx_of(h, sp), g["opt.sum_idx"].astype(np.float64)), "the embedding sum's indices differ from the reference's"
        assert np.array_equal(_bits(h), _deq(g["opt.sum_idx"], sp).view(np.int32))
        # every condition that rules the launch out: the torch ops, the same bits
        Q.FUSED_EMBED = False
        try:
            got = run(ids)
        finally:
            Q.FUSED_EMBED = True
        assert pe._fused_embed_calls == n0 + 1 and np.array_equal(_bits(got), _bits(h)), "FUSED_EMBED = False"
        for member in (front["embed_tokens"], pe, front["embed_sum_act_quantizer"], pe.quant_embedding):
            hk = member.register_forward_hook(lambda *a: None)
            try:
                got = run(ids)
            finally:
                hk.remove()
            assert pe._fused_embed_calls == n0 + 1 and np.array_equal(_bits(got), _bits(h)), "a forward hook"
        pe.train()
        try:
            got = run(ids)
        finally:
            pe.eval()
        assert pe._fused_embed_calls == n0 + 1 and np.array_equal(_bits(got), _bits(h)), "training mode"
        # inputs_embeds, and a cached step (the last 4 tokens behind 28 past ones): fused, the rows of the full call
        dense = nn.functional.embedding(ids, front["embed_tokens"].get_params()[0])
        got = Q.opt_embed_front(front["embed_tokens"], pe, front["embed_sum_act_quantizer"], None, mask, inputs_embeds=dense)
        assert pe._fused_embed_calls == n0 + 2 and np.array_equal(_bits(got), _bits(h))
        got = Q.opt_embed_front(front["embed_tokens"], pe, front["embed_sum_act_quantizer"], ids[:, -4:], mask, past_key_values_length=m["S"] - 4)
        assert pe._fused_embed_calls == n0 + 3 and np.array_equal(_bits(got), _bits(h[:, -4:]))
        # project_in sits between the lookup and the sum: the torch ops
        proj = nn.Linear(m["E"], m["E"], bias=False).cuda()
        got = Q.opt_embed_front(front["embed_tokens"], pe, front["embed_sum_act_quantizer"], ids, mask, project_in=proj)
        assert pe._fused_embed_calls == n0 + 3 and got.shape == h.shape
