"""Host side of the training block tail (include/oeh.h: oeh_drop_resid_ln_fwd / oeh_drop_resid_ln_bwd, outeffhop_amd/layers.py) without a
GPU: the ABI, every refusal, the launch-form names, the backward's scratch size, which calls go to the torch chain, and the module swap."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import _ln_train_ref as T

torch = pytest.importorskip("torch")
nn = torch.nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "oeh.h")
NEW = ("oeh_drop_resid_ln_fwd", "oeh_drop_resid_ln_bwd_work_bytes", "oeh_drop_resid_ln_bwd", "oeh_drop_resid_ln_mask", "oeh_drop_resid_ln_variant")
EINVAL, ENOTSUP = -22, -95


def test_header_binding_and_struct_layout_agree(tmp_path):
    from outeffhop_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(oeh_[a-z0-9_]+)\s*\(", txt))
    assert set(NEW) <= declared and declared == set(_lib.EXPORTS)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW) and lib.oeh_abi_version() == 6
    assert int(re.search(r"#define OEH_LN_TRAIN_MAX_GROUPS (\d+)", txt).group(1)) == _lib.LN_TRAIN_MAX_GROUPS
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    st = _lib.oeh_ln_train_desc
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HDR}"', "int main(void) {", '  printf("size %zu\\n", sizeof(oeh_ln_train_desc));']
    lines += [f'  printf("{f} %zu\\n", offsetof(oeh_ln_train_desc, {f}));' for f, _ in st._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], check=True, capture_output=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(out[f]) == getattr(st, f).offset, f


def _desc(rows=4, cols=72, dtype=2, eps=1e-5, stride=None, p=0.0):
    from outeffhop_amd import _lib

    d = _lib.oeh_ln_train_desc()
    d.rows, d.cols, d.dtype, d.eps = rows, cols, dtype, eps
    d.x_stride = d.r_stride = d.sum_stride = d.y_stride = d.dsum_stride = cols if stride is None else stride
    d.drop.p = p
    return d


def _calls():
    from outeffhop_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(4096)
    ref = lambda d: None if d is None else C.byref(d)  # noqa: E731

    def fwd(d, x=one, gamma=one, s=one, y=one, mean=one, rstd=one):
        return lib.oeh_drop_resid_ln_fwd(ref(d), x, one, gamma, one, s, y, mean, rstd, None)

    def bwd(d, dy=one, s=one, gamma=one, mean=one, rstd=one, dx=one, dr=one, dgamma=one, work=one):
        return lib.oeh_drop_resid_ln_bwd(ref(d), dy, one, s, gamma, mean, rstd, dx, dr, dgamma, one, work, None)

    def mask(d, keep=one):
        return lib.oeh_drop_resid_ln_mask(ref(d), keep, None)

    return lib, fwd, bwd, mask


def test_every_refusal_without_gpu():
    lib, fwd, bwd, mask = _calls()
    for call in (fwd, bwd, mask):
        assert call(None) == EINVAL
        assert call(_desc(cols=0)) == EINVAL and call(_desc(rows=-1)) == EINVAL
        assert call(_desc(cols=8200)) == ENOTSUP and call(_desc(rows=2 ** 31)) == ENOTSUP
        for p in (-0.1, 1.0, 1.5, float("nan")):
            assert call(_desc(p=p)) == EINVAL
            assert call(_desc(cols=8200, p=p)) == EINVAL  # p is looked at first
        d = _desc()
        d.drop.reserved = 1
        assert call(d) == EINVAL
        d = _desc()
        d.reserved = 1
        assert call(d) == EINVAL
    for call in (fwd, bwd):
        assert call(_desc(dtype=3)) == EINVAL and call(_desc(dtype=7)) == EINVAL
        assert call(_desc(eps=-1e-5)) == EINVAL and call(_desc(eps=float("nan"))) == EINVAL
        assert call(_desc(stride=-72)) == EINVAL and call(_desc(stride=8)) == EINVAL  # rows of the outputs would overlap
        assert call(_desc(cols=8193, dtype=0)) == ENOTSUP
    for name in ("x", "gamma", "s", "y", "mean", "rstd"):
        assert fwd(_desc(), **{name: None}) == EINVAL, name
    for name in ("dy", "s", "gamma", "mean", "rstd", "dx", "dgamma", "work"):
        assert bwd(_desc(), **{name: None}) == EINVAL, name
    assert mask(_desc(), keep=None) == EINVAL
    # each output's own stride: forward sum_out and y, backward dx and (when given) dr
    # (an input's stride below cols is no refusal - rows may repeat or overlap - but such a call goes on to launch: not made here)
    for field, call in (("sum_stride", fwd), ("y_stride", fwd), ("x_stride", bwd), ("r_stride", bwd)):
        d = _desc()
        setattr(d, field, 8)
        assert call(d) == EINVAL, field
    d = _desc()
    d.dsum_stride = -1
    assert fwd(d) == EINVAL and bwd(d) == EINVAL
    # nothing to do: no launch, no device needed
    assert fwd(_desc(rows=0)) == 0 and fwd(_desc(rows=0, cols=8192, p=0.5)) == 0 and mask(_desc(rows=0, p=0.25)) == 0


def _variant(rows, cols, dtype=None, **kw):
    from outeffhop_amd import ops

    return ops.drop_resid_ln_variant(rows, cols, dtype or torch.float32, **kw)


def test_launch_form_names_host_only():
    f16, bf16 = torch.float16, torch.bfloat16
    assert _variant(4096, 8) == "ln_train/fwd/wave/CH1/f32"
    assert _variant(4096, 768) == "ln_train/fwd/wave/CH4/f32"
    assert _variant(4096, 768, f16, p=0.1) == "ln_train/fwd/wave/CH2/f16/drop"
    assert _variant(4096, 1024) == "ln_train/fwd/wave/CH4/f32"
    assert _variant(4096, 1032) == "ln_train/fwd/block/CH2/f32"
    assert _variant(4096, 8192) == "ln_train/fwd/block/CH8/f32"
    assert _variant(4096, 8192, bf16) == "ln_train/fwd/block/CH4/bf16"
    assert _variant(4096, 8200) is None and _variant(4096, 8200, backward=True) is None
    assert _variant(4096, 770) == "ln_train/fwd/scalar/CH4/f32"            # cols % 4 != 0: element accesses
    assert _variant(4096, 772, f16) == "ln_train/fwd/scalar/CH4/f16"       # a multiple of 4 is not one of the 16-bit vector (8)
    assert _variant(4096, 768, row_stride=770) == "ln_train/fwd/scalar/CH4/f32"
    assert _variant(4096, 768, row_stride=776) == "ln_train/fwd/wave/CH4/f32"
    assert _variant(4096, 1) == "ln_train/fwd/scalar/CH1/f32" and _variant(1, 8191) == "ln_train/fwd/scalar/CH32/f32"
    # the backward: the same form and CH, then workgroups x rows of a slab (a workgroup's; in the wave form each of its four waves')
    assert _variant(4096, 768, f16, backward=True, p=0.1) == "ln_train/bwd/wave/CH2/f16/drop/G512x2"
    assert _variant(8192, 768, backward=True) == "ln_train/bwd/wave/CH4/f32/G512x4"
    assert _variant(1, 8, backward=True) == "ln_train/bwd/wave/CH1/f32/G1x1"
    assert _variant(12, 8, backward=True) == "ln_train/bwd/wave/CH1/f32/G3x1"
    assert _variant(4101, 8, backward=True) == "ln_train/bwd/wave/CH1/f32/G342x3"     # ceil(4101 / 2048) = 3 rows per wave, 1367 waves
    assert _variant(3, 1032, backward=True) == "ln_train/bwd/block/CH2/f32/G3x1"
    assert _variant(1027, 1032, backward=True) == "ln_train/bwd/block/CH2/f32/G343x3"  # ceil(1027 / 512) = 3 rows per workgroup, the last has 1
    assert _variant(5, 770, backward=True) == "ln_train/bwd/scalar/CH4/f32/G5x1"
    assert _variant(64, 8192, bf16, backward=True) == "ln_train/bwd/block/CH4/bf16/G64x1"


def test_work_bytes_monotone_and_aligned():
    from outeffhop_amd import _lib

    lib = _lib.load()
    wb = lambda **kw: int(lib.oeh_drop_resid_ln_bwd_work_bytes(C.byref(_desc(**kw))))  # noqa: E731
    for rows in (1, 3, 512, 513, 100000):
        prev = 0
        for cols in (1, 2, 7, 8, 72, 770, 1024, 1032, 8192):
            n = wb(rows=rows, cols=cols)
            assert n % 8 == 0 and n >= prev and n >= min(rows, _lib.LN_TRAIN_MAX_GROUPS) * 2 * cols * 8
            prev = n
    assert wb(rows=100000, cols=768) == wb(rows=512, cols=768) == 512 * 2 * 768 * 8  # float64 partials; bounded by the grid, not by the rows
    assert wb(rows=4, cols=8200) == 0 and wb(rows=4, cols=72, p=1.0) == 0  # a refused descriptor
    assert lib.oeh_drop_resid_ln_bwd_work_bytes(None) == 0


PHILOX_H = os.path.join(ROOT, "outeffhop_amd", "csrc", "oeh_philox.h")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_keep_mask_restatement_is_the_headers_row_stream(tmp_path):
    """csrc/oeh_philox.h: row_dropout_words compiled for the host (the device uses the same definition) gives the words of the numpy
    restatement the GPU tests compare the device's masks with - counter (c, row lo, row hi, 1); and the restatement's own layout: the
    fourth counter word sets the stream apart from the attention dropout's, a wider row only appends, the row's high word counts."""
    seed = 0x0123456789ABCDEF
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cases = [(0, 0), (5, 3), (257, 4100), (2047, 2 ** 32 + 3), (1, 2 ** 40 + 7)]
    lines = [f'  {{ auto r = oeh::row_dropout_words({c}u, {i}ull, {hex(seed & 0xFFFFFFFF)}u, {hex(seed >> 32)}u); '
             f'printf("%08x %08x %08x %08x\\n", r.x[0], r.x[1], r.x[2], r.x[3]); }}' for c, i in cases]
    src, exe = tmp_path / "rows.cpp", tmp_path / "rows"
    src.write_text(f'#include "{PHILOX_H}"\n#include <cstdio>\nint main() {{\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", str(src), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    thr = T.dropout_threshold(0.25)
    for line, (c, i) in zip(out, cases):
        w = T.philox4x32_10(c, i & 0xFFFFFFFF, i >> 32, 1, seed & 0xFFFFFFFF, seed >> 32)
        assert line == " ".join(f"{int(x):08x}" for x in w), (c, i)
        assert [int(x, 16) >= thr for x in line.split()] == list(T.keep_mask(1, 4 * c + 4, 0.25, seed, row0=i)[0, 4 * c:])
    a = T.keep_mask(5, 256, 0.25, seed)
    assert np.array_equal(a[:, :203], T.keep_mask(5, 203, 0.25, seed))
    assert np.array_equal(a[2:4], T.keep_mask(2, 256, 0.25, seed, row0=2))
    w = T.philox4x32_10(5, 3, 0, 1, 0x89ABCDEF, 0x01234567)  # element (i = 3, j = 20..23)
    assert [bool(x >= T.dropout_threshold(0.25)) for x in w] == list(a[3, 20:24])
    w0 = T.philox4x32_10(5, 3, 0, 0, 0x89ABCDEF, 0x01234567)  # the attention stream's counter of (b * H + h = 0, i = 3, j = 20..23)
    assert [int(x) for x in w0] != [int(x) for x in w]
    hi = T.keep_mask(1, 8, 0.5, seed, row0=2 ** 32 + 3)
    assert not np.array_equal(hi, T.keep_mask(1, 8, 0.5, seed, row0=3))  # the row's high word counts
    assert abs(float(T.keep_mask(64, 256, 0.25, seed).mean()) - 0.75) < 5 * np.sqrt(0.25 * 0.75 / (64 * 256))
    assert T.keep_mask(3, 9, 0.0, 1).all()
    assert tuple(int(x) for x in T.philox4x32_10(0, 0, 0, 0, 0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)  # Random123's known answer
    assert T.inv_keep(0.0) == 1.0 and T.inv_keep(0.5) == 2.0


def test_float64_helper_is_the_gradient_of_its_forward():
    """A self-check of the GPU tests' yardstick (tests/_ln_train_ref.py), not of the feature - it holds with or without the library:
    backward64 against torch's float64 autograd of dropout-mask -> add -> layer_norm with both outputs in the loss."""
    rs = np.random.RandomState(5)
    rows, cols, eps = 6, 24, 1e-5
    x, r, dy, dsum = (rs.standard_normal((rows, cols)) for _ in range(4))
    gamma, beta = 1.0 + 0.2 * rs.standard_normal(cols), 0.1 * rs.standard_normal(cols)
    keep, inv = T.keep_mask(rows, cols, 0.3, 77), float(T.inv_keep(0.3))
    tx, tr, tg, tb = (torch.tensor(a, requires_grad=True) for a in (x, r, gamma, beta))
    s = torch.where(torch.from_numpy(keep), tx * inv, torch.zeros((), dtype=torch.float64)) + tr
    y = torch.nn.functional.layer_norm(s, (cols,), tg, tb, eps)
    assert np.allclose(y.detach().numpy(), T.forward64(s.detach().numpy(), gamma, beta, eps), rtol=1e-12, atol=1e-12)
    ((y * torch.tensor(dy)).sum() + (s * torch.tensor(dsum)).sum()).backward()
    dx, dr, dg, db = T.backward64(dy, s.detach().numpy(), gamma, eps, keep, inv, dsum)
    for got, want in ((dx, tx.grad), (dr, tr.grad), (dg, tg.grad), (db, tb.grad)):
        assert np.allclose(got, want.numpy(), rtol=1e-11, atol=1e-12)


def test_kernel_covers_sends_the_rest_to_the_torch_chain(monkeypatch):
    from outeffhop_amd import layers as L

    class _Gpu(torch.Tensor):  # a CPU tensor that says it is on the GPU: _kernel_covers looks at metadata only
        is_cuda = True

    mk = lambda *shape, dtype=torch.float16: torch.zeros(*shape, dtype=dtype).as_subclass(_Gpu)  # noqa: E731
    x, w = mk(4, 6, 72), mk(72, dtype=torch.float32)
    assert L._kernel_covers(x, mk(4, 6, 72), w, 0.1, capturing=False)
    assert L._kernel_covers(x, None, w, 0.0, capturing=True)                        # no dropout: nothing a replay could repeat
    assert not L._kernel_covers(x, mk(4, 6, 72), w, 0.1, capturing=True)            # a replayed graph would repeat the mask
    assert not L._kernel_covers(x, mk(4, 6, 72, dtype=torch.float32), w, 0.0, capturing=False)   # dtypes differ
    assert not L._kernel_covers(mk(4, 72, dtype=torch.float64), None, w, 0.0, capturing=False)   # float64
    assert not L._kernel_covers(mk(2, 8200), None, mk(8200, dtype=torch.float32), 0.0, capturing=False)  # cols > 8192
    assert L._kernel_covers(mk(2, 8192), None, mk(8192, dtype=torch.float32), 0.0, capturing=False)
    assert not L._kernel_covers(mk(4, 72, 6).transpose(1, 2), None, w, 0.0, capturing=False)     # last dimension not contiguous
    assert not L._kernel_covers(x, mk(4, 72, 6).transpose(1, 2), w, 0.0, capturing=False)
    assert not L._kernel_covers(x, None, None, 0.0, capturing=False)                # no weight
    assert not L._kernel_covers(torch.zeros(4, 72), None, torch.ones(72), 0.0, capturing=False)  # CPU tensors
    # an uncovered call runs the torch chain and gives its result: CPU tensors here, in every flavour
    xc, rc = torch.randn(3, 5, 24), torch.randn(3, 5, 24)
    wc, bc = torch.randn(24).requires_grad_(), torch.randn(24).requires_grad_()
    before = dict(L.CALLS)
    s, y = L.dropout_add_layer_norm(xc, rc, wc, bc, p=0.0, eps=1e-6, want_sum=True)
    assert torch.equal(s, xc + rc) and torch.equal(y, torch.nn.functional.layer_norm(xc + rc, (24,), wc, bc, 1e-6)) and y.requires_grad
    y2 = L.dropout_add_layer_norm(xc, None, None, None, p=0.9, training=False)
    assert torch.equal(y2, torch.nn.functional.layer_norm(xc, (24,)))
    torch.manual_seed(3)
    y3 = L.dropout_add_layer_norm(xc, rc, wc, bc, p=0.5)
    torch.manual_seed(3)
    assert torch.equal(y3, torch.nn.functional.layer_norm(torch.nn.functional.dropout(xc, 0.5, True) + rc, (24,), wc, bc, 1e-5))
    assert L.CALLS["torch"] == before["torch"] + 3 and L.CALLS["forward"] == before["forward"]
    # the switch
    prev = L.set_fused_ln_train(False)
    assert L.FUSED_LN_TRAIN is False and L.set_fused_ln_train(prev) is False and L.FUSED_LN_TRAIN is prev


class BertSelfOutput(nn.Module):  # the Hugging Face module, by name and by submodules
    def __init__(self, inp, hidden, eps=1e-12, p=0.1):
        super().__init__()
        self.dense = nn.Linear(inp, hidden)
        self.LayerNorm = nn.LayerNorm(hidden, eps=eps)
        self.dropout = nn.Dropout(p)

    def forward(self, hidden_states, input_tensor):
        return self.LayerNorm(self.dropout(self.dense(hidden_states)) + input_tensor)


class BertOutput(BertSelfOutput):
    pass


class BertIntermediate(nn.Module):
    def __init__(self, hidden, inter):
        super().__init__()
        self.dense = nn.Linear(hidden, inter)

    def forward(self, x):
        return torch.nn.functional.gelu(self.dense(x))


class _Layer(nn.Module):
    def __init__(self, hidden=24, inter=48):
        super().__init__()
        self.attention = nn.Module()
        self.attention.output = BertSelfOutput(hidden, hidden)
        self.intermediate = BertIntermediate(hidden, inter)
        self.output = BertOutput(inter, hidden)

    def forward(self, x):
        a = self.attention.output(x, x)
        return self.output(self.intermediate(a), a)


def test_fuse_block_tails_swaps_by_name_and_keeps_the_state_dict():
    import types

    from outeffhop_amd import layers as L

    torch.manual_seed(0)
    model = nn.Sequential(_Layer(), _Layer())
    plain_sd = {k: v.clone() for k, v in model.state_dict().items()}
    params = {n: p for n, p in model.named_parameters()}
    x = torch.randn(2, 5, 24)
    model.eval()
    want = model(x)
    assert L.fuse_block_tails(model) == 4
    assert type(model[0].attention.output) is L.FusedBertSelfOutput and type(model[1].output) is L.FusedBertOutput
    assert type(model[0].intermediate) is BertIntermediate and not model[0].output.training
    assert L.fuse_block_tails(model) == 0  # nothing left to swap
    for n, p in model.named_parameters():
        assert p is params[n], n  # shared, not copied
    assert sorted(model.state_dict()) == sorted(plain_sd)
    res = model.load_state_dict(plain_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(model(x), want)  # (CPU: the torch chain behind the same interface)
    # built from a config: Hugging Face's names, sizes and signature
    cfg = types.SimpleNamespace(hidden_size=24, intermediate_size=48, layer_norm_eps=1e-12, hidden_dropout_prob=0.1)
    so, out = L.FusedBertSelfOutput(cfg), L.FusedBertOutput(cfg)
    assert sorted(so.state_dict()) == ["LayerNorm.bias", "LayerNorm.weight", "dense.bias", "dense.weight"]
    so.load_state_dict(BertSelfOutput(24, 24).state_dict(), strict=True)
    out.load_state_dict(BertOutput(48, 24).state_dict(), strict=True)
    assert out.dense.in_features == 48 and so.LayerNorm.eps == 1e-12 and so.dropout.p == 0.1
    assert out.eval()(torch.randn(2, 5, 48), x).shape == (2, 5, 24)
    m = L.FusedDropoutAddLayerNorm(24, eps=1e-6, p=0.2)
    assert sorted(n for n, _ in m.named_parameters()) == ["bias", "weight"] and m.eval()(x, x).shape == x.shape


def test_ops_raise_on_cpu_tensors():
    from outeffhop_amd import _lib, ops

    x, w = torch.zeros(4, 72), torch.ones(72)
    st = torch.zeros(4)
    with pytest.raises(_lib.OehError):
        ops.drop_resid_ln_fwd(x, None, w, w)
    with pytest.raises(_lib.OehError):
        ops.drop_resid_ln_bwd(x, x, w, st, st)
    with pytest.raises(_lib.OehError):
        ops.drop_resid_ln_mask(4, 72, 0.1, 1, "cpu")
