#!/usr/bin/env python3
"""Generate tests/golden/ln_tail.npz by IMPORTING the reference (CPU, next to the reference checkout only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ln_golden.py

The block tails of the reference's quantised models - QuantLayerNorm alone (autoquant_utils.py:64-72), QuantizedBertSelfOutput
(quantized_bert.py:541-571) and QuantizedOPTDecoderLayer (quantized_opt.py:277-384, both LayerNorm orders) - in fp32, the reference's
validate dtype, with the shims tests/golden/make_golden.py documents (imported from there, not copied).  Data only: seeds of the inputs and
weights (tests/_ln_ref.py regenerates them), every quantiser's delta / zero_float after two calibration batches and fix_ranges (and after
each batch), the reference's state_dict key lists, outputs and intermediate INDICES (a fake-quantised tensor is scale * (idx - zp): the
tests rebuild the values), and per LayerNorm the reference's own distance from a float64 evaluation (err_ref)."""
import copy
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
MG = importlib.util.module_from_spec(spec)
spec.loader.exec_module(MG)
spec = importlib.util.spec_from_file_location("_ln_ref", os.path.join(os.path.dirname(HERE), "_ln_ref.py"))
R = importlib.util.module_from_spec(spec)
spec.loader.exec_module(R)

OPT = dict(B=2, S=32, E=256, H=4, F=512)
BERT = dict(B=2, S=16, E=768)
CAP = 1e-3  # whole layer: the share of outputs that may differ by one step


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def load_weights(mod, seed):
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    mod.load_state_dict({k: t(v) for k, v in R.tail_state_dict(shapes, seed).items()}, strict=True)
    return mod


def managers(qmod):
    from quantization.quantization_manager import QuantizationManager

    return {n: m for n, m in qmod.named_modules() if isinstance(m, QuantizationManager)}


def record(qmod, names):
    """Hooks on the named QuantizationManagers: pre-quantiser input (fp32) and indices of the last forward."""
    rec, hs = {}, []
    ms = managers(qmod)
    for n in names:
        def hook(mod, inp, out, n=n):
            rec[n] = (inp[0].detach().clone(), mod.quantizer.to_integer_forward(inp[0].detach()).clone())
        hs.append(ms[n].register_forward_hook(hook))
    return rec, hs


def ln_err_ref(ln_mod, stored_in, pre):
    """The reference's fp32 LayerNorm result `pre` against the float64 formula on the same stored input and the gamma / beta it used."""
    w, b = ln_mod.get_params()
    y64 = R.layer_norm64(stored_in.numpy(), w.detach().numpy(), b.detach().numpy(), ln_mod.eps)
    return float(np.abs(pre.numpy().astype(np.float64).reshape(y64.shape) - y64).max())


def calibrate(qmod, fwd, batches, arrays, prefix):
    qmod.set_quant_state(weight_quant=True, act_quant=True) if hasattr(qmod, "set_quant_state") else qmod.quantized()
    qmod.eval()
    with torch.no_grad():
        for i, b in enumerate(batches):
            fwd(qmod, b)
            MG._dump_quantizers(f"{prefix}.after{i + 1}", qmod, arrays)
        qmod.fix_ranges()
        MG._dump_quantizers(f"{prefix}.final", qmod, arrays)


def gen_ln_alone(arrays, meta):
    from quantization.autoquant_utils import quantize_model

    for N, seed in ((768, 4100), (72, 4200)):
        prefix = f"ln{N}"
        ln = load_weights(nn.LayerNorm(N), seed)
        q = quantize_model(ln, **MG._qparams())
        xs = [t(R.with_outliers(R.normal(seed + 1 + i, (2, 16, N)))) for i in range(3)]
        calibrate(q, lambda m, x: m(x), xs[:2], arrays, prefix)
        rec, hs = record(q, ["activation_quantizer"])
        with torch.no_grad():
            out = q(xs[2])
        pre, idx = rec["activation_quantizer"]
        arrays[f"{prefix}.out_idx"] = idx.numpy().astype(np.uint8)
        arrays[f"{prefix}.out"] = out.numpy()
        arrays[f"{prefix}.err_ref"] = np.float64(ln_err_ref(q, xs[2], pre))
        arrays[f"{prefix}.keys"] = np.array(json.dumps(sorted(q.state_dict().keys())))
        meta[prefix] = dict(N=N, weight_seed=seed, calib_seeds=[seed + 1, seed + 2], eval_seed=seed + 3, eps=q.eps)
        print(prefix, "err_ref", arrays[f"{prefix}.err_ref"])


def dense_margin(pre, idx_mgr, err):
    """How far (in units of `err`) the closest pre-quantiser value is from a rounding tie of its grid."""
    qz = idx_mgr.quantizer
    tt = pre.numpy().astype(np.float64) / float(qz.scale) + float(qz.zero_point)
    return float((np.abs((tt - np.floor(tt)) - 0.5) * float(qz.scale)).min() / err)


def gen_bert_self_output(arrays, meta):
    from transformers_language.models.quantized_bert import QuantizedBertSelfOutput

    B, S, E = BERT["B"], BERT["S"], BERT["E"]
    prefix = "bso"
    for seed in (4300,):
        org = types.SimpleNamespace(dense=nn.Linear(E, E), LayerNorm=nn.LayerNorm(E, eps=1e-12), dropout=nn.Dropout(0.1))
        holder = nn.ModuleDict(dict(dense=org.dense, LayerNorm=org.LayerNorm))
        load_weights(holder, seed)
        q = QuantizedBertSelfOutput(org, **MG._qparams())
        pairs = [(t(R.normal(seed + 1 + 2 * i, (B, S, E))), t(R.with_outliers(R.normal(seed + 2 + 2 * i, (B, S, E))))) for i in range(3)]
        q.eval()
        q.full_precision()
        with torch.no_grad():
            fp_out = q(*pairs[2])
        scratch = {}
        calibrate(q, lambda m, p: m(*p), pairs[:2], scratch, prefix)
        names = ["dense.activation_quantizer", "res_act_quantizer.activation_quantizer", "LayerNorm.activation_quantizer"]
        rec, hs = record(q, names)
        with torch.no_grad():
            out = q(*pairs[2])
            w, b = q.dense.get_params()
            d64 = pairs[2][0].double() @ w.double().t() + b.double()
        dpre, didx = rec[names[0]]
        derr = float((dpre.double() - d64).abs().max())
        margin = dense_margin(dpre, managers(q)[names[0]], derr)
        # (margin < 1: the closest dense value sits within the reference's own fp32 GEMM error of a rounding tie - another fp32-grade GEMM may
        # move that index by a step, and with it one row of the sum; recorded so that the tests can tell such a row from a wrong one)
        arrays.update(scratch)
        spre, sidx = rec[names[1]]
        lpre, lidx = rec[names[2]]
        stored = managers(q)[names[1]].quantizer(spre)
        arrays[f"{prefix}.fp_out"] = fp_out.numpy()
        arrays[f"{prefix}.dense_idx"] = didx.numpy().astype(np.uint8)
        arrays[f"{prefix}.sum_idx"] = sidx.numpy().astype(np.uint8)
        arrays[f"{prefix}.out_idx"] = lidx.numpy().astype(np.uint8)
        arrays[f"{prefix}.out"] = out.numpy()
        arrays[f"{prefix}.err_ref"] = np.float64(ln_err_ref(q.LayerNorm, stored, lpre))
        arrays[f"{prefix}.dense_margin"] = np.float64(margin)
        arrays[f"{prefix}.keys"] = np.array(json.dumps(sorted(q.state_dict().keys())))
        meta[prefix] = dict(B=B, S=S, E=E, weight_seed=seed, calib_seeds=[[seed + 1, seed + 2], [seed + 3, seed + 4]], eval_seeds=[seed + 5, seed + 6], eps=1e-12)
        print(prefix, "seed", seed, "dense margin", margin, "err_ref", arrays[f"{prefix}.err_ref"])


def build_opt_layer(pre_ln, seed):
    from transformers_language.models.opt_attention import OPTAttentionWithExtras
    from transformers_language.models.softmax import SOFTMAX_MAPPING

    E, H, F = OPT["E"], OPT["H"], OPT["F"]
    org = types.SimpleNamespace(embed_dim=E, do_layer_norm_before=pre_ln, dropout=0.1, activation_fn=nn.ReLU(),
                                self_attn=OPTAttentionWithExtras(E, H, is_decoder=True, softmax_fn=SOFTMAX_MAPPING["softmax1"]),
                                self_attn_layer_norm=nn.LayerNorm(E), fc1=nn.Linear(E, F), fc2=nn.Linear(F, E), final_layer_norm=nn.LayerNorm(E))
    holder = nn.ModuleDict({k: v for k, v in vars(org).items() if isinstance(v, nn.Module) and k != "activation_fn"})
    load_weights(holder, seed)
    return org


def gen_opt_layer(arrays, meta):
    from transformers_language.models.quantized_opt import QuantizedOPTDecoderLayer

    B, S, E = OPT["B"], OPT["S"], OPT["E"]
    mask = MG._opt_mask(B, S, [S, S - 9])
    arrays["opt.mask"] = mask.numpy()
    for pre_ln in (True, False):
        prefix = "opt_pre" if pre_ln else "opt_post"
        for seed in range(4400 if pre_ln else 4500, 9000, 10):
            q = QuantizedOPTDecoderLayer(build_opt_layer(pre_ln, seed), **MG._qparams())
            xs = [t(R.with_outliers(R.normal(seed + 1 + i, (B, S, E)))) for i in range(3)]
            scratch = {}
            calibrate(q, lambda m, x: m(x, attention_mask=mask), xs[:2], scratch, prefix)
            names = ["self_attn.out_proj.activation_quantizer", "self_attn_res_act_quantizer.activation_quantizer", "self_attn_layer_norm.activation_quantizer",
                     "final_layer_norm.activation_quantizer", "fc2.activation_quantizer", "ffn_res_act_quantizer.activation_quantizer"]
            rec, hs = record(q, names)
            with torch.no_grad():
                out = q(xs[2], attention_mask=mask)[0]
            last = names[3] if not pre_ln else names[5]
            # the same layer in float64 (the fp32 ranges, the weights re-quantised in float64): how many final indices the reference's own fp32 arithmetic moves
            q64 = copy.deepcopy(q)
            for m in q64.modules():
                m._forward_hooks.clear()
                if hasattr(m, "cached_params"):
                    m.cached_params = None
            q64 = q64.double()
            rec64, _ = record(q64, [last])
            with torch.no_grad():
                q64(xs[2].double(), attention_mask=mask.double())
            idx32, idx64 = rec[last][1].numpy(), rec64[last][1].numpy()
            diff = np.abs(idx32.astype(np.int64) - idx64.astype(np.int64))
            share = float((diff != 0).mean())
            print(prefix, "seed", seed, "share of final indices fp32 vs float64:", share, "max step", diff.max())
            if share > CAP or diff.max() > 1:
                continue
            arrays.update(scratch)
            for n in names:
                arrays[f"{prefix}.idx.{n}"] = rec[n][1].numpy().astype(np.uint8)
            mg = managers(q)
            sum1 = mg[names[1]].quantizer(rec[names[1]][0])
            if pre_ln:
                arrays[f"{prefix}.err_ref.self_attn_layer_norm"] = np.float64(ln_err_ref(q.self_attn_layer_norm, xs[2], rec[names[2]][0]))
                arrays[f"{prefix}.err_ref.final_layer_norm"] = np.float64(ln_err_ref(q.final_layer_norm, sum1.reshape(-1, E), rec[names[3]][0]))
            else:
                sum2 = mg[names[5]].quantizer(rec[names[5]][0])
                arrays[f"{prefix}.err_ref.self_attn_layer_norm"] = np.float64(ln_err_ref(q.self_attn_layer_norm, sum1, rec[names[2]][0]))
                arrays[f"{prefix}.err_ref.final_layer_norm"] = np.float64(ln_err_ref(q.final_layer_norm, sum2.reshape(-1, E), rec[names[3]][0]))
            arrays[f"{prefix}.out"] = out.numpy()
            arrays[f"{prefix}.share_ref"] = np.float64(share)
            arrays[f"{prefix}.keys"] = np.array(json.dumps(sorted(q.state_dict().keys())))
            meta[prefix] = dict(**OPT, pre_ln=pre_ln, weight_seed=seed, calib_seeds=[seed + 1, seed + 2], eval_seed=seed + 3, lengths=[S, S - 9], last=last)
            break
        else:
            raise SystemExit("no seed within the cap")


def main():
    MG._shim()
    sys.path.insert(0, os.path.join(MG.REF, "OutEffHop"))
    torch.manual_seed(0)
    arrays, meta = {}, {}
    gen_ln_alone(arrays, meta)
    gen_bert_self_output(arrays, meta)
    gen_opt_layer(arrays, meta)
    arrays["meta_json"] = np.array(json.dumps(meta))
    MG.save("ln_tail.npz", **arrays)


if __name__ == "__main__":
    main()
