"""Every compiled instance of the LayerNorm-row family - oeh_resid_ln_kernel, oeh_embed_kernel, oeh_ln_train_fwd_kernel and
oeh_ln_train_bwd_kernel, 224 kernels - at the first and at the last width of its (form, CH) range, by the registry of tests/_ln_inst.py
(which tests/test_ln_instances_cpu.py holds against the built library).  `-m gpu`.

Yardsticks and limits are the existing ones, unchanged: `_check_call` of tests/test_ln_gpu.py, `_case` / `_check_y` of
tests/test_embed_gpu.py and `_check_case` of tests/test_ln_train_gpu.py - the sum and its indices bit for bit the torch expression; y, dx,
dr, mean, rstd, dgamma, dbeta within 4 err64 of float64 (+ half a storage ulp where stored in 16 bits); indices by the tie-band rule; values
on the grid.  Before a case runs, the library's variant name for the strides of the tensors actually passed must be the case's.  The
training cases take their inputs from `train_draw`, which asks of the yardstick what `_case` asks for the embedding front: a unit of at
least half an fp32 ulp of the largest output.

Exact, per instance:
  forward, p = 0    sum and y are ops.resid_ln_quant's without quantisers, bit for bit - in every form, element accesses at CH 16 and 32 too
  backward, p = 0   dx is dr, bit for bit (nothing scales it); and the float64 comparison of `_check_case(p=0.0)`
  embedding         one lookup: resid_ln_quant(row0, None); two: resid_ln_quant(row0, row1) on the gathered rows; three: two chained
                    resid_ln_quant calls through the first call's quantised sum output - sum, y and both index dumps bit for bit (the
                    kernels share one program text behind the last add: csrc/oeh_ln_row.h)
  element accesses at a width that is a vector multiple (rows cols + 1 elements apart): the columns behind a row's end keep their
  sentinels in every output, and the outputs' bits do not depend on where they are written.
The worst ratio per group is printed (-s)."""
import numpy as np
import pytest

from tests import _ln_inst as I

torch = pytest.importorskip("torch")
F = torch.nn.functional
pytestmark = pytest.mark.gpu

from tests import test_embed_gpu as E  # noqa: E402
from tests import test_ln_gpu as LN  # noqa: E402
from tests import test_ln_train_gpu as TR  # noqa: E402

DT = (torch.float16, torch.bfloat16, torch.float32)  # IN -> the storage dtype
EPS = LN.EPS
_bits = LN._bits


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _wide(t, stride, fill):
    """(allocation, view): t's values as rows `stride` elements apart, `fill` behind each row's end; (None, t) where stride is the row length."""
    cols = t.shape[-1]
    if stride == cols:
        return None, t
    big = torch.full((*t.shape[:-1], stride), fill, dtype=t.dtype, device=t.device)
    big[..., :cols] = t
    return big, big[..., :cols]


def _blank(shape, stride, dtype, fill):
    """(allocation, view) of an output with rows `stride` elements apart, all `fill`; (None, None) where stride is the row length."""
    if stride == shape[-1]:
        return None, None
    big = torch.full((*shape[:-1], stride), fill, dtype=dtype, device="cuda")
    return big, big[..., :shape[-1]]


def _untouched(big, cols, fill):
    return big is None or bool((big[..., cols:] == fill).all())


def _strip(name):
    return name.split("/G")[0]


def _eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy()) if a.dtype == torch.uint8 else np.array_equal(_bits(a), _bits(b))


# ---- the block tail ---------------------------------------------------------------------------------------------------------------------
def _run_ln(ops, c):
    dtype, cols, st = DT[c["IN"]], c["cols"], c["stride"]
    x, r, gamma, beta = LN._inputs(I.ROWS, cols, dtype, c["seed"])
    (bx, x), (br, r) = _wide(x, st, 7.0), _wide(r, st, 7.0)
    assert ops.resid_ln_variant(I.ROWS, cols, dtype, row_stride=x.stride(0)) == I.variant_name(c), c["name"]
    (big_y, out), (big_s, sum_out) = _blank(x.shape, st, dtype, -3.0), _blank(x.shape, st, dtype, -5.0)
    ratio, share, _ = LN._check_call(ops, x, r if c["r"] else None, gamma, beta if c["beta"] else None, c["sq"], c["oq"], c["name"],
                                     want_sum=c["sum"], out=out, sum_out=sum_out)
    assert _untouched(big_y, cols, -3.0) and _untouched(big_s, cols, -5.0) and _untouched(bx, cols, 7.0) and _untouched(br, cols, 7.0), f"{c['name']}: a store beyond a row's end"
    return {"y": ratio}, share


# ---- the embedding front ----------------------------------------------------------------------------------------------------------------
def _run_embed(ops, c):
    dtype, cols, st, nt, B, S = DT[c["IN"]], c["cols"], c["stride"], c["nt"], c["B"], c["S"]
    quantise = [[], [c["last"]], [c["mid"], c["last"]]][nt - 1]
    k = E._case(ops, c["seed"], cols, dtype, B, S, (512, 2, 7)[:nt], [(B, S), (B, 1), (1, S)][:nt], torch.int64 if c["id64"] else torch.int32,
                quantise, with_beta=c["beta"], out_bits=8 if c["oq"] else None)
    gathered = [F.embedding(i.long().expand(B, S), tb.wq).reshape(B * S, cols) for tb, i in zip(k.tabs, k.ids)]
    for tb in k.tabs:  # the three forms of a table as rows `st` elements apart
        tb.w, tb.wq = _wide(tb.w, st, 9.0)[1], _wide(tb.wq, st, 9.0)[1]
        tb.i8 = None if tb.i8 is None else _wide(tb.i8, st, 9)[1]  # (no int8 form of a table whose grid is not int8's: `lookup` takes the grid form)
    form = c["tab"]
    assert ops.embed_sum_variant(B, S, cols, dtype, n_tab=nt, int8=form == "int8", row_stride=k.tabs[0].w.stride(0)) == I.variant_name(c), c["name"]
    lk = [tb.lookup(ops, form, i) for tb, i in zip(k.tabs, k.ids)]
    g, b, fq_out = (k.gamma, k.b, k.fq_out) if c["ln"] else (None, None, None)
    (big_y, out), (big_s, sum_out) = _blank((B, S, cols), st, dtype, -3.0), _blank((B, S, cols), st, dtype, -5.0)
    s, y, sidx, yidx = E._esq(ops, dtype, lk, g, b, EPS, fq_sums=k.specs, fq_out=fq_out, want_idx=True, out=out, sum_out=sum_out)
    assert _untouched(big_y, cols, -3.0) and _untouched(big_s, cols, -5.0), f"{c['name']}: a store beyond a row's end"
    assert np.array_equal(_bits(s), _bits(k.s_want)), f"{c['name']}: the sum differs from F.embedding + add + ops.fake_quant"
    assert _eq(sidx, k.sidx_want if nt > 1 and c["last"] else None), f"{c['name']}: sum indices differ from ops.fake_quant"
    assert _eq(E._esq(ops, dtype, lk, g, b, EPS, fq_sums=k.specs, fq_out=fq_out), y), f"{c['name']}: y differs without the sum output"
    ratio, share = 0.0, 0.0
    if c["ln"]:
        ratio, share = E._check_y(ops, y, yidx, k.s_want, k.gamma, k.b, fq_out, dtype, False, c["name"])
    else:
        assert _eq(y, k.s_want) and yidx is None, f"{c['name']}: without a LayerNorm y is the final sum"
    # the block tail's kernel on the gathered rows, in the same launch form
    assert I.ln_name(c["IN"], B * S, cols, st).split("/")[1:3] == I.variant_name(c).split("/")[1:3]
    rows = [_wide(t, st, 7.0)[1] for t in gathered]
    if nt == 3:
        rows = [ops.resid_ln_quant(rows[0], rows[1], k.gamma, None, EPS, fq_sum=k.specs[0], want_sum=True)[0], rows[2]]
    ref = ops.resid_ln_quant(rows[0], rows[1] if nt > 1 else None, k.gamma, b, EPS, fq_sum=k.specs[-1] if nt > 1 else None, fq_out=fq_out, want_idx=True)
    assert _eq(s.view(B * S, cols), ref[0]) and _eq(None if sidx is None else sidx.view(B * S, cols), ref[2]), f"{c['name']}: the sum differs from the block tail's"
    if c["ln"]:
        assert _eq(y.view(B * S, cols), ref[1]) and _eq(None if yidx is None else yidx.view(B * S, cols), ref[3]), f"{c['name']}: y differs from the block tail's"
    return {"y": ratio}, share


# ---- the training tail ------------------------------------------------------------------------------------------------------------------
def train_draw(c):
    """(seed, (x, r, gamma, beta, dy, dsum) on the CPU, absent parts None) of a training case: the first of the seeds c["seed"] + 0, 7919, ...
    whose draw is usable.  The condition is the one `_case` of tests/test_embed_gpu.py asks, of the yardstick alone and without the GPU: err64
    of y - the unit of its float64 comparison - is at least half an fp32 ulp of the largest output.  Five rows have ten outlier elements,
    which carry the largest errors; where CPU fp32 happens to land within a fraction of an ulp of float64 on all of them, four times THAT is
    nothing a second fp32 evaluation can be held to: numpy's fp32 evaluation of the same formula is 4.2 to 5.0 err64 away on three of the
    draws this leaves out.  (cols == 1: y is beta exactly in every evaluation, the unit is 0 and the comparison exact.)"""
    dtype, cols, p = DT[c["IN"]], c["cols"], c["p"]
    for attempt in range(32):
        seed = c["seed"] + 7919 * attempt
        x, r, gamma, beta, dy, dsum = TR._inputs(I.ROWS, cols, dtype, seed, device="cpu")
        if c["kernel"] == "ln_train_bwd":
            dsum = dsum if c["dsum"] else None
        else:
            r, beta, dsum = (r if c["r"] else None), (beta if c["beta"] else None), (dsum if c["index"] % 4 < 2 else None)
        keep = TR.T.keep_mask(I.ROWS, cols, p, seed)
        d = torch.where(torch.from_numpy(keep), x.float() * torch.tensor(TR.T.inv_keep(p)), torch.zeros(()))
        s = (d if r is None else d + r.float()).to(dtype)  # (the torch expression `_check_case` holds the kernel's sum to, bit for bit)
        y64, err64 = TR._reference(s, gamma, beta, dy, None, keep, TR.T.inv_keep(p))["y"]
        if cols == 1 or err64 >= 0.5 * float(np.spacing(np.float32(np.abs(y64).max()))):
            return seed, (x, r, gamma, beta, dy, dsum)
    pytest.fail(f"no usable draw for {c['name']}")


def _run_train(ops, c):
    dtype, cols, st, p = DT[c["IN"]], c["cols"], c["stride"], c["p"]
    bwd = c["kernel"] == "ln_train_bwd"
    seed, draw = train_draw(c)
    x, r, gamma, beta, dy, dsum = (None if t is None else t.cuda() for t in draw)
    x, r, dy, dsum = (None if t is None else _wide(t, st, 7.0)[1] for t in (x, r, dy, dsum))
    assert _strip(ops.drop_resid_ln_variant(I.ROWS, cols, dtype, backward=bwd, p=p, row_stride=x.stride(0))) == _strip(I.variant_name(c)), c["name"]
    want_dr, want_dbeta = (c["dr"], c["dbeta"]) if bwd else (True, True)
    ratios = TR._check_case(ops, x, r, gamma, beta, dy, dsum, p, seed, c["name"], want_dr=want_dr, want_dbeta=want_dbeta)
    kw = dict(p=p, seed=seed) if p > 0 else {}
    fwd = ops.drop_resid_ln_fwd(x, r, gamma, beta, EPS, **kw)
    back = ops.drop_resid_ln_bwd(dy, fwd[0], gamma, fwd[2], fwd[3], dsum=dsum, **kw)
    if p == 0.0:
        s0, y0 = ops.resid_ln_quant(x, r, gamma, beta, EPS, want_sum=True)
        assert _eq(fwd[0], s0) and _eq(fwd[1], y0), f"{c['name']}: without dropout the forward is not the inference kernel"
        assert _eq(back[0], back[1]), f"{c['name']}: without dropout dx is not dr"
    if st != cols:  # the outputs as rows of wider allocations: the same bits, and nothing behind a row's end
        (big_y, out), (big_s, sum_out) = _blank(x.shape, st, dtype, -3.0), _blank(x.shape, st, dtype, -5.0)
        (big_dx, dx), (big_dr, dr) = _blank(x.shape, st, dtype, -3.0), _blank(x.shape, st, dtype, -5.0)
        fwd2 = ops.drop_resid_ln_fwd(x, r, gamma, beta, EPS, out=out, sum_out=sum_out, **kw)
        back2 = ops.drop_resid_ln_bwd(dy, fwd[0], gamma, fwd[2], fwd[3], dsum=dsum, dx=dx, dr=dr, **kw)
        assert all(_eq(a, b_) for a, b_ in zip(fwd + back, fwd2 + back2)), f"{c['name']}: the bits depend on where the outputs are written"
        assert all(_untouched(big, cols, fill) for big, fill in ((big_y, -3.0), (big_s, -5.0), (big_dx, -3.0), (big_dr, -5.0))), f"{c['name']}: a store beyond a row's end"
    return ratios, 0.0


_RUN = {"ln": _run_ln, "embed": _run_embed, "ln_train_fwd": _run_train, "ln_train_bwd": _run_train}


@pytest.mark.parametrize("group", I.GROUPS, ids=I.GROUP_IDS)
def test_every_instance_and_width(ops, group):
    cases = I.cases_of(group)
    assert cases, group
    worst, band = {}, 0.0
    for c in cases:
        assert I.instance_of(c) == c["inst"], c["name"]
        ratios, share = _RUN[c["kernel"]](ops, c)
        band = max(band, share)
        for key, v in ratios.items():
            worst[key] = max(worst.get(key, 0.0), v)
    print(f"\n{'-'.join(str(g) for g in group)}: {len(cases)} cases at cols {sorted({c['cols'] for c in cases})}; max |value - f64| / err64 (limit 4): "
          + ", ".join(f"{key} {v:.2f}" for key, v in worst.items()) + (f"; tie band <= {band:.1e} of the elements" if band else ""))
