"""Every launch branch of the embedding-front kernel (csrc/oeh_embed.hip; include/oeh.h: oeh_embed_sum_quant) at the smallest shape that
reaches it.  `-m gpu`.

Yardsticks.  The final sum and the indices of its quantiser are compared BIT FOR BIT with F.embedding on the fake-quantised tables, torch's
add in the storage type and the existing `ops.fake_quant`, on the GPU.  The fake-quantised table is `SymmetricUniformQuantizer(W) + 0.0`:
the quantiser's scale * round(-0.3) is -0, which no int8 index can say, so the kernel's grid and int8 forms define a zero entry as +0
(include/oeh.h) and `+ 0.0` states that and nothing else.  The three table forms - the fake-quantised table as it is, the raw table with the
grid, the int8 indices with the scale - must give the same bits.  Where oeh_embed_sum_variant and oeh_resid_ln_variant name the same launch
form, y and its indices equal `ops.resid_ln_quant` on the stored sum bit for bit; everywhere y obeys tests/_ln_ref.py's check_values /
check_indices against a float64 evaluation of the stored sum, with the helpers' factor and band cap and the unit of tests/test_ln_gpu.py
(the distance of CPU fp32 F.layer_norm from float64 on the same case).

Launch forms (oeh_ln_row.h: ln_plan; VEC = 4 fp32 / 8 16-bit elements):
  cols 8, 72, 768, 1024   one wave per row, four rows per workgroup: B * S = 1, 6, 15 leave waves of the last workgroup without a row
  cols 1032, 8192         one workgroup per row
  cols 1, 4 (16-bit)      element accesses; also: table row strides, output strides and bases off the 16-byte vector
Of oeh_embed_kernel's 84 instances (IN x CH x FORM x 1, 2, 3 lookups) this list reaches the first and the last CH of the two 16-byte forms
and, with elements, CH = 1 and - through the stride tests - part of CH = 4 and, with three lookups, CH = 16: not fp32 wave CH = 2, not the
workgroup form's middle CH, not CH = 32 with elements (52 of the 84 in a kernel trace).  tests/test_ln_instances_gpu.py runs every compiled instance at both ends of its range, from the
registry of tests/_ln_inst.py; this file keeps the (B, S) grids, the table forms, the optional parts, ids outside a table and refusals."""
import itertools
import types

import numpy as np
import pytest

from tests import _ln_ref as R

torch = pytest.importorskip("torch")
F = torch.nn.functional
pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
COLS = (1, 4, 8, 72, 768, 1024, 1032, 8192)
GRIDS = ((1, 1), (2, 3), (3, 5), (4, 16))
TABLE_ROWS = (1, 2, 7, 512)
EPS = 1e-5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from outeffhop_amd import ops as _ops

    return _ops


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _f64(t):
    return t.detach().cpu().float().numpy().astype(np.float64)


def _name(dtype):
    return str(dtype).split(".")[-1]


def _round_storage(dtype):
    return None if dtype == torch.float32 else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy())


def _spec_of(ops, t, n_bits=8):
    return ops.FakeQuantSpec(*R.grid_from_minmax(float(t.min()), float(t.max()), n_bits))


def _cpu_case(s, gamma, beta):
    """(float64 result, err64 = max distance of CPU fp32 F.layer_norm from it, that fp32 result) on the stored sum `s`."""
    s32 = s.detach().cpu().float()
    g32, b32 = gamma.detach().cpu().float(), None if beta is None else beta.detach().cpu().float()
    y64 = R.layer_norm64(s32.numpy(), g32.numpy(), None if b32 is None else b32.numpy(), EPS)
    y32 = F.layer_norm(s32, (s32.shape[-1],), g32, b32, EPS).numpy().astype(np.float64)
    return y64, float(np.abs(y32 - y64).max()), y32


class Table:
    """One embedding table in its three forms, and the ids of one lookup into it."""

    def __init__(self, n_rows, cols, dtype, gen, outliers=False):
        from outeffhop_amd import quantization as Q

        w = 0.05 * torch.randn(n_rows, cols, generator=gen)
        if outliers and cols >= 8:
            w[:, 3] *= 40.0
            w[:, cols - 2] *= -25.0
        self.w = w.to(dtype).cuda()
        qz = Q.SymmetricUniformQuantizer(n_bits=8)
        qz.set_quant_range(self.w.min(), self.w.max())
        self.wq = qz(self.w) + 0.0  # (see the module docstring)
        self.scale, self.lo, self.hi = float(qz.scale), float(qz.int_min), float(qz.int_max)
        self.i8 = qz.to_integer_forward(self.w).to(torch.int8) if self.lo >= -128 and self.hi <= 127 else None
        self.n_rows = n_rows

    def lookup(self, ops, form, ids):
        if form == "plain":
            return ops.EmbedLookup(self.wq, ids)
        if form == "grid" or self.i8 is None:
            return ops.EmbedLookup(self.w, ids, self.scale, self.lo, self.hi)
        return ops.EmbedLookup(self.i8, ids, self.scale, self.lo, self.hi)


def _ids(n_rows, B, S, id_dtype, gen, shape=None):
    """Random ids with repeats, the first and the last row among them; shape (B, S) or a broadcastable one."""
    shape = shape or (B, S)
    ids = torch.randint(0, n_rows, shape, generator=gen)
    flat = ids.view(-1)
    flat[0] = n_rows - 1
    flat[-1] = 0
    if flat.numel() > 2:
        flat[1] = flat[2]
    return ids.to(id_dtype).cuda()


def _yardstick(ops, tables, ids, quantise, n_bits=8):
    """(final sum, indices of its quantiser or None, the FakeQuantSpec per sum) by separate ops on the GPU."""
    s = F.embedding(ids[0].long().expand(*torch.broadcast_shapes(*[i.shape for i in ids])), tables[0].wq)
    specs, sidx = [], None
    for t in range(1, len(tables)):
        shape = torch.broadcast_shapes(*[i.shape for i in ids])
        s = torch.add(s, F.embedding(ids[t].long().expand(*shape), tables[t].wq))
        sidx = None
        if quantise[t - 1]:
            spec = _spec_of(ops, s, n_bits)
            if n_bits <= 8:
                s, sidx = ops.fake_quant(s, spec, want_idx=True)
            else:
                s = ops.fake_quant(s, spec)
            specs.append(spec)
        else:
            specs.append(None)
    return s, sidx, specs


def _check_y(ops, y, yidx, s_want, gamma, beta, fq_out, dtype, same_form, label):
    """y of a call with a LayerNorm against the block tail's kernel (same launch form) and against float64 (always)."""
    y64, err64, _ = _cpu_case(s_want, gamma, beta)
    if same_form:
        ref = ops.resid_ln_quant(s_want, None, gamma, beta, EPS, fq_out=fq_out, want_idx=fq_out is not None and fq_out.qmax <= 255)
        y_ref = ref[1] if isinstance(ref, tuple) else ref
        assert np.array_equal(_bits(y), _bits(y_ref)), f"{label}: y differs from ops.resid_ln_quant on the stored sum"
        if isinstance(ref, tuple) and yidx is not None:
            assert np.array_equal(yidx.cpu().numpy(), ref[3].cpu().numpy()), f"{label}: y indices differ from ops.resid_ln_quant"
    if fq_out is None:
        return R.check_values(_f64(y), y64, err64, _name(dtype)), 0.0
    if yidx is not None:
        idx = yidx.cpu().numpy().astype(np.float64)
    else:  # no dump (a 16-bit grid has none): the index is read back from the value, which sits on the grid - exactly in fp32, and in fp16
        # within 2^-11 |y| of its grid point, far below half a step of an 8-bit grid (check_on_grid below confirms the reading)
        assert dtype != torch.bfloat16
        idx = np.rint(_f64(y) / fq_out.scale) + fq_out.zero_point
    # (the band cap is stated for 8-bit grids; a 16-bit grid's step is 257 times finer: tests/test_ln_gpu.py)
    share, _ = R.check_indices(idx, y64, fq_out.scale, fq_out.zero_point, fq_out.qmax, err64, max_band=1e-3 * fq_out.qmax / 255.0)
    R.check_on_grid(y.detach().cpu().float().numpy(), idx, fq_out.scale, fq_out.zero_point, _round_storage(dtype))
    return 0.0, share


def _usable(y64, err64, fq_out):
    """The helpers' condition on the INPUTS, asked of the yardstick alone, before the kernel under test runs: the tie band of the output
    grid holds at most the cap of the elements (check_indices on float64's own indices passes exactly then).  With fewer than a thousand
    elements a single one in the band is over the cap, and tables of one or two rows repeat it: such a draw is no case."""
    t = y64 / fq_out.scale + fq_out.zero_point
    try:
        R.check_indices(np.clip(np.rint(t), 0.0, fq_out.qmax), y64, fq_out.scale, fq_out.zero_point, fq_out.qmax, err64, max_band=1e-3 * fq_out.qmax / 255.0)
    except AssertionError:
        return False
    return True


def _case(ops, seed, cols, dtype, B, S, rows, shapes=None, id_dtype=torch.int64, quantise=None, with_beta=True, n_bits=8, out_bits=8):
    """Tables of `rows` rows each, ids, LayerNorm parameters and every yardstick of one call, from the first of the seeds 100 * seed + 0, 1,
    ... whose draw is usable: err64, the unit of every float64 comparison, is at least half an fp32 ulp of the largest output, and the output
    grid's tie band is within the cap (`_usable`; out_bits None: no output grid).  Both are asked of the yardsticks alone."""
    n_tab = len(rows)
    quantise = [True] * (n_tab - 1) if quantise is None else quantise
    for attempt in range(32):
        gen = torch.Generator().manual_seed(100 * seed + attempt)
        c = types.SimpleNamespace(B=B, S=S, cols=cols, dtype=dtype)
        c.gamma, c.beta = _ln_params(cols, gen)
        c.tabs = [Table(n, cols, dtype, gen, outliers=(n == 512)) for n in rows]
        c.ids = [_ids(tb.n_rows, B, S, id_dtype, gen, sh) for tb, sh in zip(c.tabs, shapes or [(B, S)] * n_tab)]
        c.s_want, c.sidx_want, c.specs = _yardstick(ops, c.tabs, c.ids, quantise, n_bits)
        c.b = c.beta if with_beta else None
        c.y64, c.err64, y32 = _cpu_case(c.s_want, c.gamma, c.b)
        c.fq_out = ops.FakeQuantSpec(*R.grid_from_minmax(float(y32.min()), float(y32.max()), out_bits)) if out_bits else None
        # the unit has to be one: on a row of a few elements CPU fp32 can happen to land within a fraction of an fp32 ulp of float64
        # everywhere, and four times THAT is nothing a second fp32 evaluation can be held to (asked of the yardstick, as the band is)
        # (cols == 1: y is beta, exactly, in every evaluation - the unit is 0 and the comparison exact)
        if cols > 1 and c.err64 < 0.5 * float(np.spacing(np.float32(np.abs(c.y64).max()))):
            continue
        if c.fq_out is None or _usable(c.y64, c.err64, c.fq_out):
            return c
    pytest.fail(f"no usable draw for seed {seed}")


def _esq(ops, dtype, lookups, *args, **kw):
    """ops.embed_sum_quant with the storage dtype named (int8 tables alone do not say it)."""
    return ops.embed_sum_quant(lookups, *args, dtype=dtype, **kw)


def _ln_params(cols, gen):
    return (1.0 + 0.25 * torch.randn(cols, generator=gen)).cuda(), (0.1 * torch.randn(cols, generator=gen)).cuda()


def _same_form(ops, B, S, cols, dtype, n_tab, int8=False):
    return ops.embed_sum_variant(B, S, cols, dtype, n_tab=n_tab, int8=int8).split("/")[1:3] == ops.resid_ln_variant(B * S, cols, dtype).split("/")[1:3]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cols", COLS)
def test_every_form_grid_and_lookup_count(ops, cols, dt):
    dtype = DTYPES[dt]
    worst, band = 0.0, 0.0
    for k, ((B, S), n_tab) in enumerate(itertools.product(GRIDS, (1, 2, 3))):
        id_dtype = torch.int32 if k % 2 else torch.int64
        rows = [TABLE_ROWS[(k + 3 * t + 3) % 4] for t in range(n_tab)]  # (lookup 0 starts at the 512-row table)
        # lookup 1 as a (B, 1) column and lookup 2 as BERT's (1, S) position row: strides of 0 in the kernel
        c = _case(ops, 70000 + 16 * cols + k, cols, dtype, B, S, rows, [(B, S), (B, 1), (1, S)][:n_tab], id_dtype)
        tabs, ids, gamma, beta, s_want, sidx_want, specs, fq_out = c.tabs, c.ids, c.gamma, c.beta, c.s_want, c.sidx_want, c.specs, c.fq_out
        label = f"{B}x{S}x{cols} {dt} T{n_tab}"
        first = None
        for form in ("plain", "grid", "int8"):
            lk = [tb.lookup(ops, form, i) for tb, i in zip(tabs, ids)]
            s, y, sidx, yidx = _esq(ops, dtype, lk, gamma, beta, EPS, fq_sums=specs, fq_out=fq_out, want_idx=True)
            assert s.shape == (B, S, cols) and y.shape == (B, S, cols) and s.dtype == dtype and y.dtype == dtype
            assert np.array_equal(_bits(s), _bits(s_want)), f"{label} {form}: the sum differs from F.embedding + add + ops.fake_quant"
            if n_tab > 1:
                assert np.array_equal(sidx.cpu().numpy(), sidx_want.cpu().numpy()), f"{label} {form}: sum indices differ from ops.fake_quant"
            else:
                assert sidx is None
            if first is None:
                first = (y, yidx)
                int8 = all(tb.i8 is not None for tb in tabs)
                same = _same_form(ops, B, S, cols, dtype, n_tab) and _same_form(ops, B, S, cols, dtype, n_tab, int8)
                assert same  # dense, aligned tensors take the block tail's plan
                _, share = _check_y(ops, y, yidx, s_want, gamma, beta, fq_out, dtype, same, f"{label} {form}")
                band = max(band, share)
                # without the output quantiser: values against float64
                y_plain = _esq(ops, dtype, lk, gamma, beta, EPS, fq_sums=specs)
                ratio, _ = _check_y(ops, y_plain, None, s_want, gamma, beta, None, dtype, same, f"{label} {form} unquantised")
                worst = max(worst, ratio)
            else:  # the three table forms: the same bits
                assert np.array_equal(_bits(y), _bits(first[0])) and np.array_equal(yidx.cpu().numpy(), first[1].cpu().numpy()), f"{label}: {form} differs from plain"
    print(f"\nembed_sum_quant {ops.embed_sum_variant(4, 16, cols, dtype)} cols {cols} {dt}: max |y - f64| / err64 = {worst:.2f} (limit 4), "
          f"tie band <= {band:.1e} of the elements")


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("cols", (72, 770, 1032))
def test_every_subset_of_the_optional_parts(ops, cols, dt):
    dtype = DTYPES[dt]
    B, S = 3, 5
    same = ops.embed_sum_variant(B, S, cols, dtype).split("/")[1:3] == ops.resid_ln_variant(B * S, cols, dtype).split("/")[1:3]
    assert same
    for mask in range(64):
        q1, q2, with_ln, with_beta, with_oq, with_sum = (bool(mask & (1 << i)) for i in range(6))
        if not with_ln and (with_beta or with_oq):
            continue  # beta and the output quantiser are the LayerNorm's
        label = f"{cols} {dt} parts {mask:06b}"
        c = _case(ops, 71000 + cols, cols, dtype, B, S, (512, 2, 7), [(B, S), (B, S), (1, S)], quantise=[q1, q2], with_beta=with_beta, out_bits=8 if with_oq else None)
        tabs, ids, gamma, s_want, sidx_want, specs, fq_out = c.tabs, c.ids, c.gamma, c.s_want, c.sidx_want, c.specs, c.fq_out
        g, b = (gamma if with_ln else None), c.b
        lk = [tb.lookup(ops, ("grid", "int8", "plain")[mask % 3], i) for tb, i in zip(tabs, ids)]
        res = _esq(ops, dtype, lk, g, b, EPS, fq_sums=specs, fq_out=fq_out, want_sum=with_sum, want_idx=with_sum and (q2 or with_oq))
        if not with_sum:
            assert torch.is_tensor(res)
            s, y, sidx, yidx = None, res, None, None
        elif q2 or with_oq:
            s, y, sidx, yidx = res
        else:
            (s, y), sidx, yidx = res, None, None
        if s is not None:
            assert np.array_equal(_bits(s), _bits(s_want)), label
        if sidx is not None:
            assert q2 and np.array_equal(sidx.cpu().numpy(), sidx_want.cpu().numpy()), label
        if not with_ln:
            assert np.array_equal(_bits(y), _bits(s_want)), f"{label}: without a LayerNorm y is the final sum"
        else:
            _check_y(ops, y, yidx, s_want, gamma, b, fq_out, dtype, True, label)


def test_sixteen_bit_grids(ops):
    """qmax 65535 on the sum and on the output (the OPT final LayerNorm's width): values only - a uint8 dump of such a grid is refused."""
    from outeffhop_amd import _lib

    B, S, dtype = 3, 5, torch.float32
    for cols in (768, 1032, 770):
        c = _case(ops, 72000 + cols, cols, dtype, B, S, (512, 7), id_dtype=torch.int32, n_bits=16, out_bits=16)
        tabs, ids, gamma, beta, s_want, specs, fq_out = c.tabs, c.ids, c.gamma, c.beta, c.s_want, c.specs, c.fq_out
        assert specs[0].qmax == 65535.0 and fq_out.qmax == 65535.0
        lk = [tb.lookup(ops, "int8", i) for tb, i in zip(tabs, ids)]
        s, y = _esq(ops, dtype, lk, gamma, beta, EPS, fq_sums=specs, fq_out=fq_out, want_sum=True)
        assert np.array_equal(_bits(s), _bits(s_want))
        _check_y(ops, y, None, s_want, gamma, beta, fq_out, torch.float32, True, f"{cols} 16-bit grids")
    for kw in (dict(fq_sums=specs), dict(fq_sums=[None], fq_out=fq_out)):
        with pytest.raises(_lib.OehError) as e:
            _esq(ops, dtype, lk, gamma, beta, EPS, want_idx=True, **kw)
        assert e.value.code == -95


@pytest.mark.parametrize("dt", list(DTYPES))
def test_dense_rows_strides_and_offset_bases(ops, dt):
    """inputs_embeds as lookup 0; tables, outputs and ids that are views into larger allocations.  A pad of one 16-byte vector keeps the
    16-byte forms (the same bits as the dense call), a pad of 3 elements or a base one element off forces the element form (another
    summation order: the sum still bit for bit, y by the float64 rule and, against the block tail's kernel in ITS element form, bit for bit)."""
    dtype = DTYPES[dt]
    B, S = 3, 5
    for cols in (72, 1032):
        c = _case(ops, 73000 + cols, cols, dtype, B, S, (512, 2, 7))
        tabs, ids, gamma, beta, s_want, sidx_want, specs, fq_out = c.tabs, c.ids, c.gamma, c.beta, c.s_want, c.sidx_want, c.specs, c.fq_out
        dense = F.embedding(ids[0], tabs[0].wq)  # what the word lookup gives, handed over as inputs_embeds
        kw = dict(fq_sums=specs, fq_out=fq_out, want_idx=True)
        want = _esq(ops, dtype, [tb.lookup(ops, "plain", i) for tb, i in zip(tabs, ids)], gamma, beta, EPS, **kw)
        rest = [tb.lookup(ops, "int8", i) for tb, i in zip(tabs[1:], ids[1:])]
        got = _esq(ops, dtype, [ops.EmbedLookup(dense)] + rest, gamma, beta, EPS, **kw)
        for a, b in zip(got, want):
            assert np.array_equal(_bits(a) if a.dtype != torch.uint8 else a.cpu().numpy(), _bits(b) if b.dtype != torch.uint8 else b.cpu().numpy()), (cols, "dense")

        def padded(t, pad, fill):  # the same values as rows of a wider allocation
            big = torch.full((*t.shape[:-1], t.shape[-1] + pad), fill, dtype=t.dtype, device="cuda")
            big[..., :t.shape[-1]] = t
            return big, big[..., :t.shape[-1]]

        for pad in (16, 3):
            views = [padded(tb.w, pad, 9.0)[1] for tb in tabs]
            views8 = [padded(tb.i8, pad, 9)[1] for tb in tabs]
            big_d, dense_v = padded(dense, pad, 9.0)
            big_out = torch.full((B, S, cols + pad), -3.0, dtype=dtype, device="cuda")
            big_sum = torch.full((B, S, cols + pad), -5.0, dtype=dtype, device="cuda")
            ids_v = [padded(i, 3, 10 ** 6)[1] for i in ids]  # id rows 3 elements apart from dense
            for which, lk in (("grid", [ops.EmbedLookup(v, i, tb.scale, tb.lo, tb.hi) for v, i, tb in zip(views, ids_v, tabs)]),
                              ("int8", [ops.EmbedLookup(v, i, tb.scale, tb.lo, tb.hi) for v, i, tb in zip(views8, ids_v, tabs)]),
                              ("dense", [ops.EmbedLookup(dense_v)] + rest)):
                if which == "dense" and pad == 3:
                    continue  # (a (B, S, cols) view with a padded last dimension does collapse to rows: covered by pad 16 and the offset case)
                got = _esq(ops, dtype, lk, gamma, beta, EPS, out=big_out[..., :cols], sum_out=big_sum[..., :cols], **kw)
                assert got[1].data_ptr() == big_out.data_ptr() and got[0].data_ptr() == big_sum.data_ptr()
                assert np.array_equal(_bits(got[0]), _bits(s_want)) and np.array_equal(got[2].cpu().numpy(), sidx_want.cpu().numpy()), (cols, pad, which)
                assert (big_out[..., cols:] == -3.0).all() and (big_sum[..., cols:] == -5.0).all()  # nothing beyond a row's end
                if pad == 16:  # the same launch form on the same values: the same bits throughout
                    assert np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(got[3].cpu().numpy(), want[3].cpu().numpy()), (cols, pad, which)
                else:
                    assert ops.embed_sum_variant(B, S, cols, dtype, row_stride=cols + pad).split("/")[1:3] == ops.resid_ln_variant(B * S, cols, dtype, row_stride=cols + pad).split("/")[1:3]
                    ref = ops.resid_ln_quant(got[0], None, gamma, beta, EPS, fq_out=fq_out, want_idx=True)  # (the strided sum: the element form there too)
                    assert np.array_equal(_bits(got[1]), _bits(ref[1])) and np.array_equal(got[3].cpu().numpy(), ref[3].cpu().numpy()), (cols, pad, which)
                    _check_y(ops, got[1], got[3], s_want, gamma, beta, fq_out, dtype, False, f"{cols} {dt} pad {pad} {which}")

        def offset(t):  # the same values one element off a 16-byte boundary
            buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
            v = buf[1:1 + t.numel()].view(t.shape)
            v.copy_(t)
            assert v.data_ptr() % 16 != 0
            return v
        for which in range(4):
            lk = [tb.lookup(ops, "grid", i) for tb, i in zip(tabs, ids)]
            g, b = gamma, beta
            if which < 3:
                lk[which] = ops.EmbedLookup(offset(tabs[which].w), ids[which], tabs[which].scale, tabs[which].lo, tabs[which].hi)
            else:
                lk[0] = ops.EmbedLookup(offset(dense))
                g = offset(gamma)
            got = _esq(ops, dtype, lk, g, b, EPS, **kw)
            assert np.array_equal(_bits(got[0]), _bits(s_want)) and np.array_equal(got[2].cpu().numpy(), sidx_want.cpu().numpy()), (cols, "offset", which)
            _check_y(ops, got[1], got[3], s_want, gamma, beta, fq_out, dtype, False, f"{cols} {dt} offset {which}")
            assert np.abs(got[3].cpu().numpy().astype(np.int32) - want[3].cpu().numpy().astype(np.int32)).max() <= 1


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
@pytest.mark.parametrize("cols", (72, 770, 1032))
def test_ids_outside_the_table_never_become_addresses(ops, cols, dt):
    """Ids -1 and n_rows (and the extremes of their types) in tables that are slices of larger allocations with sentinel rows on both sides -
    even a missing guard would read allocated memory.  Those rows are NaN, bad_rows counts them once each, every other row is the row of
    the call without them, and no sentinel shows."""
    dtype = DTYPES[dt]
    B, S = 4, 16
    gen = torch.Generator().manual_seed(7400 + cols)
    gamma, beta = _ln_params(cols, gen)
    tabs = [Table(n, cols, dtype, gen) for n in (7, 2, 512)]
    for id_dtype in (torch.int32, torch.int64):
        ids = [_ids(tb.n_rows, B, S, id_dtype, gen) for tb in tabs]
        s_want, _, specs = _yardstick(ops, tabs, ids, [True, True])
        fq_out = ops.FakeQuantSpec(0.04, 128.0)
        bad_ids = [i.clone() for i in ids]
        info = torch.iinfo(id_dtype)
        bad_ids[0][0, 1], bad_ids[0][1, 2] = -1, tabs[0].n_rows
        bad_ids[1][1, 2], bad_ids[1][2, 3] = tabs[1].n_rows, -1  # (1, 2): two bad ids in one row count once
        bad_ids[2][3, 15], bad_ids[2][3, 0] = info.min, info.max
        bad = torch.zeros(B, S, dtype=torch.bool)
        for b, s in ((0, 1), (1, 2), (2, 3), (3, 15), (3, 0)):
            bad[b, s] = True
        for form in ("grid", "int8"):
            def guarded(tb):  # the table between sentinel rows of one allocation (four a side: an int8 table has to start on 4 bytes)
                src = tb.w if form == "grid" else tb.i8
                big = torch.full((tb.n_rows + 8, cols), 3.0e4 if form == "grid" else 100, dtype=src.dtype, device="cuda")
                big[4:-4] = src
                return big[4:-4]
            mk = lambda idl: [ops.EmbedLookup(guarded(tb), i, tb.scale, tb.lo, tb.hi) for tb, i in zip(tabs, idl)]  # noqa: E731
            s0, y0, n0 = _esq(ops, dtype, mk(ids), gamma, beta, EPS, fq_sums=specs, fq_out=fq_out, want_sum=True, check_ids=True)
            assert n0 == 0 and np.array_equal(_bits(s0), _bits(s_want)) and not torch.isnan(y0).any()
            s1, y1, n1 = _esq(ops, dtype, mk(bad_ids), gamma, beta, EPS, fq_sums=specs, fq_out=fq_out, want_sum=True, check_ids=True)
            assert n1 == int(bad.sum()) == 5
            bc = bad.cuda()
            assert torch.isnan(s1[bc]).all() and torch.isnan(y1[bc]).all(), "a row with a bad id must be NaN throughout"
            assert np.array_equal(_bits(s1[~bc]), _bits(s0[~bc])) and np.array_equal(_bits(y1[~bc]), _bits(y0[~bc])), "the other rows are untouched"
            # without the counter and without the sum: the same y
            y2 = _esq(ops, dtype, mk(bad_ids), gamma, beta, EPS, fq_sums=specs, fq_out=fq_out)
            assert torch.isnan(y2[bc]).all() and np.array_equal(_bits(y2[~bc]), _bits(y0[~bc]))
    # no LayerNorm (the OPT front): y is the sum, NaN in the same rows
    y3, n3 = _esq(ops, dtype, mk(bad_ids)[:2], fq_sums=specs[:1], check_ids=True)
    assert n3 == 3 and torch.isnan(y3[0, 1]).all() and torch.isnan(y3[1, 2]).all() and torch.isnan(y3[2, 3]).all() and not torch.isnan(y3[3]).any()


def test_two_calls_are_bitwise_equal(ops):
    for cols, dtype in ((768, torch.float32), (8192, torch.float32), (770, torch.float16), (1032, torch.bfloat16)):
        gen = torch.Generator().manual_seed(7600 + cols)
        gamma, beta = _ln_params(cols, gen)
        tabs = [Table(n, cols, dtype, gen) for n in (512, 2, 7)]
        ids = [_ids(tb.n_rows, 4, 16, torch.int64, gen) for tb in tabs]
        lk = [tb.lookup(ops, "int8", i) for tb, i in zip(tabs, ids)]
        kw = dict(fq_sums=[ops.FakeQuantSpec(0.01, 120.0), ops.FakeQuantSpec(0.012, 131.0)], fq_out=ops.FakeQuantSpec(0.04, 128.0), want_sum=True)
        a = _esq(ops, dtype, lk, gamma, beta, EPS, **kw)
        b = _esq(ops, dtype, lk, gamma, beta, EPS, **kw)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_refusals_on_the_device(ops):
    from outeffhop_amd import _lib

    gen = torch.Generator().manual_seed(7700)
    tb = Table(7, 72, torch.float32, gen)
    ids = _ids(7, 2, 3, torch.int64, gen)
    gamma, beta = _ln_params(72, gen)
    with pytest.raises(_lib.OehError):
        ops.embed_sum_quant([ops.EmbedLookup(tb.w, ids.cpu())])
    with pytest.raises(_lib.OehError):
        ops.embed_sum_quant([ops.EmbedLookup(tb.w, ids)], gamma.cpu())
    wide = torch.zeros(2, 8200, device="cuda")
    with pytest.raises(_lib.OehError) as e:
        ops.embed_sum_quant([ops.EmbedLookup(wide, ids % 2)])
    assert e.value.code == -95
    with pytest.raises(_lib.OehError) as e:
        ops.embed_sum_quant([ops.EmbedLookup(tb.w, ids)], gamma, beta, -1.0)
    assert e.value.code == -22
    with pytest.raises(ValueError):
        ops.embed_sum_quant([ops.EmbedLookup(tb.w, ids), ops.EmbedLookup(tb.w[:, :8], ids)])  # rows of another length
    with pytest.raises(ValueError):
        ops.embed_sum_quant([ops.EmbedLookup(tb.i8, ids)])  # an int8 table without its scale
    with pytest.raises(ValueError):
        ops.embed_sum_quant([ops.EmbedLookup(tb.i8, ids, tb.scale)])  # int8 tables alone do not say the storage dtype
    with pytest.raises(ValueError):
        ops.embed_sum_quant([ops.EmbedLookup(tb.w, ids)], None, beta)  # beta without the LayerNorm's weight
    y = ops.embed_sum_quant([ops.EmbedLookup(tb.i8, ids, tb.scale)], dtype=torch.float16)
    sc16 = torch.tensor(tb.scale).half().float().item()  # e = RN(RN(scale) * idx) in the storage type named by dtype=
    assert y.dtype == torch.float16 and np.array_equal(_bits(y), _bits(F.embedding(ids, (tb.i8.float() * sc16).half())))
    assert ops.embed_sum_quant([ops.EmbedLookup(tb.w, ids[:0])]).shape == (0, 3, 72)
