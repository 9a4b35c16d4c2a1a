"""Host side of the quantised block tail (QuantLayerNorm, QuantizedBertSelfOutput / QuantizedBertOutput, QuantizedOPTDecoderLayer and the
C entry point oeh_resid_ln_quant) without a GPU: class and key names against the reference's recorded ones, the ABI, the refusals, the
launch-form names, and the float64 helper of the GPU tests against the fixture."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import _ln_ref as R
from tests.conftest import load_golden

torch = pytest.importorskip("torch")
nn = torch.nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "oeh.h")


def _qp(**quant_dict):
    from outeffhop_amd import quantization as Q

    qp = Q.val_qparams(Q.get_quant_config())
    qp["quant_dict"] = dict(quant_dict)
    return qp


def _bert_org(E=768):
    return types.SimpleNamespace(dense=nn.Linear(E, E), LayerNorm=nn.LayerNorm(E, eps=1e-12), dropout=nn.Dropout(0.1))


def _opt_org(pre_ln, E=256, H=4, F=512):
    from outeffhop_amd.opt_attention import OPTAttentionWithExtras

    return types.SimpleNamespace(embed_dim=E, do_layer_norm_before=pre_ln, dropout=0.1, activation_fn=nn.ReLU(),
                                 self_attn=OPTAttentionWithExtras(E, H, is_decoder=True), self_attn_layer_norm=nn.LayerNorm(E),
                                 fc1=nn.Linear(E, F), fc2=nn.Linear(F, E), final_layer_norm=nn.LayerNorm(E))


def test_quantize_model_rewrites_layer_norm_and_linear_relu():
    from outeffhop_amd import quantization as Q

    ln = nn.LayerNorm(768, eps=1e-12)
    with torch.no_grad():
        ln.weight.normal_()
        ln.bias.normal_()
    q = Q.quantize_model(ln, **_qp())
    assert type(q) is Q.QuantLayerNorm and isinstance(q, nn.LayerNorm) and isinstance(q, Q.QuantizedModule)
    assert q.eps == 1e-12 and tuple(q.normalized_shape) == (768,) and torch.equal(q.weight, ln.weight) and torch.equal(q.bias, ln.bias)
    assert isinstance(q.weight_quantizer, Q.QuantizationManager) and isinstance(q.activation_quantizer, Q.QuantizationManager)
    assert type(q.weight_quantizer.quantizer) is Q.SymmetricUniformQuantizer and type(q.activation_quantizer.quantizer) is Q.AsymmetricUniformQuantizer
    seq = Q.quantize_model(nn.Sequential(nn.Linear(16, 32), nn.ReLU()), **_qp())
    assert type(seq) is nn.Sequential and len(seq) == 1 and type(seq[0]) is Q.QuantLinear and isinstance(seq[0].activation_function, nn.ReLU)
    with pytest.raises(NotImplementedError):
        Q.quantize_model(nn.GELU(), **_qp())
    # the torch path (CPU, full precision and quantised weights): F.layer_norm with the fake-quantised gamma
    x = torch.randn(3, 768)
    q.eval()
    assert torch.equal(q(x), nn.functional.layer_norm(x, (768,), ln.weight, ln.bias, 1e-12))
    q.quantized_weights()
    wq = q.weight_quantizer(ln.weight.detach())
    assert torch.equal(q(x), nn.functional.layer_norm(x, (768,), wq, ln.bias, 1e-12)) and not torch.equal(wq, ln.weight)
    assert q._fused_ln_calls == 0 and Q.FUSED_LN is True  # (the default follows tools/ln_bench.py: DESIGN.md section 13)


def _strict_load(mod, keys):
    own = mod.state_dict()
    assert set(own) <= set(keys), sorted(set(own) - set(keys))
    res = mod.load_state_dict({k: own[k] if k in own else torch.tensor(0.5) for k in keys}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert sorted(mod.state_dict()) == sorted(k for k in keys if ".range_estimator.quantizer." not in k)


def test_recorded_reference_state_dict_keys_load_strictly():
    from outeffhop_amd import quantization as Q

    g = load_golden("ln_tail.npz")
    keys = lambda p: json.loads(str(g[f"{p}.keys"]))  # noqa: E731
    _strict_load(Q.quantize_model(nn.LayerNorm(768), **_qp()), keys("ln768"))
    _strict_load(Q.QuantizedBertSelfOutput(_bert_org(), **_qp()), keys("bso"))
    _strict_load(Q.QuantizedBertOutput(_bert_org(), **_qp()), keys("bso"))
    for pre_ln, p in ((True, "opt_pre"), (False, "opt_post")):
        layer = Q.QuantizedOPTDecoderLayer(_opt_org(pre_ln), **_qp())
        _strict_load(layer, keys(p))
        assert layer.do_layer_norm_before is pre_ln and type(layer.self_attn) is Q.QuantizedOPTAttentionWithExtras
        assert type(layer.fc1_act) is Q.QuantLinear and isinstance(layer.fc1_act.activation_function, nn.ReLU)
        for name in ("self_attn_layer_norm", "final_layer_norm"):
            assert type(getattr(layer, name)) is Q.QuantLayerNorm
    # a loaded range is a usable range
    q = Q.quantize_model(nn.LayerNorm(72), **_qp())
    sd = {k: torch.tensor(0.5) for k in keys("ln72")}
    sd.update(q.state_dict())
    sd["activation_quantizer.quantizer._delta"], sd["activation_quantizer.quantizer._zero_float"] = torch.tensor(0.25), torch.tensor(100.2)
    q.load_state_dict(sd, strict=True)
    q.fix_ranges()
    s = q.activation_quantizer.quantizer.spec()
    assert (s.scale, s.zero_point, s.qmax) == (0.25, 100.0, 255.0)


def test_decomposed_layer_norm_and_log_quantiser_are_refused():
    from outeffhop_amd import quantization as Q

    with pytest.raises(NotImplementedError, match="layer_norm_res_self_output"):
        Q.QuantizedBertSelfOutput(_bert_org(64), **_qp(layer_norm_res_self_output=True))
    with pytest.raises(NotImplementedError, match="layer_norm_res_output"):
        Q.QuantizedBertOutput(_bert_org(64), **_qp(layer_norm_res_output=True))
    with pytest.raises(NotImplementedError, match="log"):
        Q.QuantizedBertOutput(_bert_org(64), **_qp(y="log"))
    Q.QuantizedBertOutput(_bert_org(64), **_qp(layer_norm_res_self_output=True))  # the other class's key
    org = _opt_org(True, 64, 1, 128)
    org.activation_fn = nn.GELU()
    with pytest.raises(AssertionError):
        Q.QuantizedOPTDecoderLayer(org, **_qp())


def test_header_binding_and_struct_layout_agree(tmp_path):
    from outeffhop_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(oeh_[a-z0-9_]+)\s*\(", txt))
    assert {"oeh_resid_ln_quant", "oeh_resid_ln_variant"} <= declared and declared == set(_lib.EXPORTS)
    lib = _lib.load()
    assert hasattr(lib, "oeh_resid_ln_quant") and hasattr(lib, "oeh_resid_ln_variant") and lib.oeh_abi_version() == 6
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    st = _lib.oeh_ln_desc
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HDR}"', "int main(void) {", '  printf("size %zu\\n", sizeof(oeh_ln_desc));']
    lines += [f'  printf("{f} %zu\\n", offsetof(oeh_ln_desc, {f}));' for f, _ in st._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], check=True, capture_output=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(out[f]) == getattr(st, f).offset, f


def _desc(rows=4, cols=72, dtype=2, eps=1e-5, stride=None):
    from outeffhop_amd import _lib

    d = _lib.oeh_ln_desc()
    d.rows, d.cols, d.dtype, d.eps = rows, cols, dtype, eps
    d.x_stride = d.r_stride = d.sum_stride = d.y_stride = cols if stride is None else stride
    return d


def test_argument_validation_without_gpu():
    from outeffhop_amd import _lib

    lib = _lib.load()
    one = C.c_void_p(4096)
    call = lambda d, x=one, gamma=one, y=one, sum_idx=None, y_idx=None: lib.oeh_resid_ln_quant(  # noqa: E731
        None if d is None else C.byref(d), x, one, gamma, one, one, y, sum_idx, y_idx, None)
    EINVAL, ENOTSUP = -22, -95
    assert call(None) == EINVAL
    assert call(_desc(), x=None) == EINVAL and call(_desc(), gamma=None) == EINVAL and call(_desc(), y=None) == EINVAL
    assert call(_desc(cols=0)) == EINVAL and call(_desc(rows=-1)) == EINVAL and call(_desc(dtype=3)) == EINVAL and call(_desc(dtype=7)) == EINVAL
    assert call(_desc(eps=-1e-5)) == EINVAL and call(_desc(eps=float("nan"))) == EINVAL
    assert call(_desc(stride=-72)) == EINVAL and call(_desc(stride=8)) == EINVAL  # rows of the outputs would overlap
    assert call(_desc(cols=8200)) == ENOTSUP and call(_desc(cols=8193, dtype=0)) == ENOTSUP
    assert call(_desc(rows=0)) == 0 and call(_desc(rows=0, cols=8192)) == 0  # nothing to do: no launch, no device needed
    d = _desc()
    d.reserved = 1
    assert call(d) == EINVAL
    d = _desc()
    d.fq_sum.enable, d.fq_sum.scale, d.fq_sum.zero_point, d.fq_sum.qmax = 1, 0.0, 0.0, 255.0
    assert call(d) == EINVAL  # no grid
    d.fq_sum.scale, d.fq_sum.zero_point = 0.1, 300.0
    assert call(d) == EINVAL  # zero point beyond the grid
    d = _desc(rows=0)
    d.fq_out.enable, d.fq_out.scale, d.fq_out.zero_point, d.fq_out.qmax = 1, 1e-3, 30000.0, 65535.0
    assert call(d) == 0 and call(d, y_idx=one) == ENOTSUP  # a 16-bit grid works for the values; its indices do not fit the uint8 dump
    assert call(d, sum_idx=one) == EINVAL  # an index dump of a quantiser that is off


def test_launch_form_names_host_only():
    from outeffhop_amd import ops

    assert ops.resid_ln_variant(4096, 8) == "ln/wave/CH1/f32"
    assert ops.resid_ln_variant(4096, 768) == "ln/wave/CH4/f32"
    assert ops.resid_ln_variant(4096, 768, torch.float16) == "ln/wave/CH2/f16"
    assert ops.resid_ln_variant(4096, 1024) == "ln/wave/CH4/f32"
    assert ops.resid_ln_variant(4096, 1032) == "ln/block/CH2/f32"
    assert ops.resid_ln_variant(4096, 8192) == "ln/block/CH8/f32"
    assert ops.resid_ln_variant(4096, 8192, torch.bfloat16) == "ln/block/CH4/bf16"
    assert ops.resid_ln_variant(4096, 8200) is None
    assert ops.resid_ln_variant(4096, 770) == "ln/scalar/CH4/f32"          # cols % 4 != 0: element accesses
    assert ops.resid_ln_variant(4096, 772, torch.float16) == "ln/scalar/CH4/f16"  # a multiple of 4 is not one of the 16-bit vector (8)
    assert ops.resid_ln_variant(4096, 768, row_stride=770) == "ln/scalar/CH4/f32"
    assert ops.resid_ln_variant(4096, 768, row_stride=776) == "ln/wave/CH4/f32"
    assert ops.resid_ln_variant(4096, 1) == "ln/scalar/CH1/f32" and ops.resid_ln_variant(1, 8191) == "ln/scalar/CH32/f32"


def test_no_cpu_fallback():
    from outeffhop_amd import _lib, ops

    x = torch.zeros(4, 72)
    with pytest.raises(_lib.OehError):
        ops.resid_ln_quant(x, None, torch.ones(72), torch.zeros(72))


def test_float64_helper_reproduces_the_reference_outputs():
    """tests/_ln_ref.py against ln_tail.npz: the reference's QuantLayerNorm output indices are those of the float64 formula outside the tie
    band of its own error err_ref, and its values sit on the recorded grid."""
    from outeffhop_amd import quantization as Q
    from outeffhop_amd.ops import FakeQuantSpec

    g = load_golden("ln_tail.npz")
    meta = json.loads(str(g["meta_json"]))
    for p in ("ln768", "ln72"):
        m = meta[p]
        N = m["N"]
        sd = R.tail_state_dict({"weight": (N,), "bias": (N,)}, m["weight_seed"])
        x = R.with_outliers(R.normal(m["eval_seed"], (2, 16, N)))
        wq = Q.SymmetricUniformQuantizer(n_bits=8)
        w = torch.from_numpy(sd["weight"])
        wq.set_quant_range(w.min(), w.max())
        assert float(wq.delta) == pytest.approx(float(g[f"{p}.final.q.weight_quantizer.delta"]), rel=1e-6)
        y64 = R.layer_norm64(x, wq(w).numpy(), sd["bias"], m["eps"])
        sp = FakeQuantSpec.from_delta(float(g[f"{p}.final.q.activation_quantizer.delta"]), float(g[f"{p}.final.q.activation_quantizer.zero_float"]))
        err = float(g[f"{p}.err_ref"])
        share, flipped = R.check_indices(g[f"{p}.out_idx"], y64, sp.scale, sp.zero_point, sp.qmax, err, factor=1.0)
        R.check_on_grid(g[f"{p}.out"], g[f"{p}.out_idx"], sp.scale, sp.zero_point)
        print(f"\n{p}: err_ref {err:.3e} = {err / (2.0 ** -24 * np.abs(y64).max()):.2f} x 2^-24 |y|max, tie band {share:.1e}, reference indices off float64 {flipped:.1e}")
