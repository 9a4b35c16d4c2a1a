#!/usr/bin/env python3
"""Generate tests/golden/embed_front.npz by IMPORTING the reference (CPU, next to the reference checkout only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_embed_golden.py

The fronts of the reference's quantised models in fp32, the reference's validate dtype, with the shims tests/golden/make_golden.py documents
(imported from there, not copied):
  bert   QuantizedBertEmbeddings (quantized_bert.py:146-218) - B2 S16 E768, a 512-row word table with the residual stream's outlier channels
  opt    the OPT decoder front, quantized_opt.py:549-569 - B2 S32 E256, a left-padded mask.  The reference's QuantizedOPTDecoder does not
         construct here (its mask helpers are gone from the installed transformers, make_golden._shim stubs them), so the front is COMPOSED
         from the reference's own classes in the order of those lines: quantize_model(nn.Embedding) -> QuantEmbedding,
         QuantizedOPTLearnedPositionalEmbedding, `+`, QuantizedActivation.
Data only: seeds of the weights and ids (tests/_embed_ref.py regenerates them), every quantiser's delta / zero_float after each of two
calibration batches and after fix_ranges, the reference's state_dict key lists, the id tensors, the INDICES of every quantised sum and of
the LayerNorm output (a fake-quantised tensor is scale * (idx - zp): the tests rebuild the values), and the reference's LayerNorm distance
from a float64 evaluation (err_ref).  The seed is the first for which the reference's own LayerNorm indices obey tests/_ln_ref.check_indices
against float64 with the helper's factor and its 1e-3 band cap - checked here, on the CPU."""
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


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MG = _load("make_golden", os.path.join(HERE, "make_golden.py"))
LG = _load("make_ln_golden", os.path.join(HERE, "make_ln_golden.py"))
ER = _load("_embed_ref", os.path.join(os.path.dirname(HERE), "_embed_ref.py"))
R = ER.R


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def load_weights(mod, seed):
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    mod.load_state_dict({k: t(v) for k, v in ER.front_state_dict(shapes, seed).items()}, strict=True)
    return mod


def gen_quant_embedding(arrays, meta):
    from quantization.autoquant_utils import quantize_model

    q = quantize_model(nn.Embedding(7, 8, padding_idx=0), **MG._qparams())
    arrays["qemb.keys"] = np.array(json.dumps(sorted(q.state_dict().keys())))
    q.quantized()
    q.eval()
    with torch.no_grad():
        q(torch.tensor([[1, 2]]))  # the table's range is estimated by the first forward
    arrays["qemb.keys_calibrated"] = np.array(json.dumps(sorted(q.state_dict().keys())))


def gen_bert(arrays, meta):
    from transformers_language.models.quantized_bert import QuantizedBertEmbeddings

    d = ER.BERT
    B, S, E = d["B"], d["S"], d["E"]
    prefix = "bert"
    names = ["sum_input_token_type_embd_act_quantizer.activation_quantizer", "sum_pos_embd_act_quantizer.activation_quantizer",
             "LayerNorm.activation_quantizer"]
    for seed in range(5100, 9000, 10):
        org = types.SimpleNamespace(word_embeddings=nn.Embedding(d["vocab"], E, padding_idx=0), position_embeddings=nn.Embedding(d["positions"], E),
                                    token_type_embeddings=nn.Embedding(d["types"], E), LayerNorm=nn.LayerNorm(E, eps=d["eps"]), dropout=nn.Dropout(0.1),
                                    position_ids=torch.arange(d["positions"]).expand((1, -1)), position_embedding_type="absolute")
        load_weights(nn.ModuleDict({k: v for k, v in vars(org).items() if isinstance(v, nn.Module) and k != "dropout"}), seed)
        q = QuantizedBertEmbeddings(org, **MG._qparams())
        batches = [(t(ER.token_ids(seed + 1 + 2 * i, (B, S), d["vocab"])), t(ER.token_ids(seed + 2 + 2 * i, (B, S), d["types"]))) for i in range(3)]
        scratch = {}
        LG.calibrate(q, lambda m, b: m(input_ids=b[0], token_type_ids=b[1]), batches[:2], scratch, prefix)
        rec, hs = LG.record(q, names)
        with torch.no_grad():
            out = q(input_ids=batches[2][0], token_type_ids=batches[2][1])
        mg = LG.managers(q)
        stored = mg[names[1]].quantizer(rec[names[1]][0])
        lpre, lidx = rec[names[2]]
        err = LG.ln_err_ref(q.LayerNorm, stored, lpre)
        w, b = q.LayerNorm.get_params()
        y64 = R.layer_norm64(stored.numpy(), w.detach().numpy(), b.detach().numpy(), d["eps"])
        qz = mg[names[2]].quantizer
        try:
            share, off = R.check_indices(lidx.numpy(), y64, float(qz.scale), float(qz.zero_point), 255.0, err)
        except AssertionError as e:
            print(prefix, "seed", seed, "rejected:", e)
            continue
        print(prefix, "seed", seed, "err_ref", err, "tie band", share, "reference indices off float64", off)
        arrays.update(scratch)
        arrays[f"{prefix}.input_ids"] = batches[2][0].numpy()
        arrays[f"{prefix}.token_type_ids"] = batches[2][1].numpy()
        arrays[f"{prefix}.sum1_idx"] = rec[names[0]][1].numpy().astype(np.uint8)
        arrays[f"{prefix}.sum2_idx"] = rec[names[1]][1].numpy().astype(np.uint8)
        arrays[f"{prefix}.out_idx"] = lidx.numpy().astype(np.uint8)
        arrays[f"{prefix}.err_ref"] = np.float64(err)
        arrays[f"{prefix}.band_ref"] = np.float64(share)
        arrays[f"{prefix}.keys"] = np.array(json.dumps(sorted(q.state_dict().keys())))
        meta[prefix] = dict(**{k: v for k, v in d.items()}, weight_seed=seed, calib_seeds=[[seed + 1, seed + 2], [seed + 3, seed + 4]],
                            eval_seeds=[seed + 5, seed + 6])
        assert np.array_equal(out.numpy(), (np.float32(float(qz.scale)) * (lidx.numpy().astype(np.float32) - np.float32(float(qz.zero_point)))))
        return
    raise SystemExit("no seed within the cap")


def gen_opt(arrays, meta):
    from quantization.autoquant_utils import quantize_model
    from quantization.base_quantized_classes import QuantizedActivation
    from transformers.models.opt.modeling_opt import OPTLearnedPositionalEmbedding
    from transformers_language.models.quantized_opt import QuantizedOPTLearnedPositionalEmbedding

    d = ER.OPT
    B, S, E, seed, past = d["B"], d["S"], d["E"], 5300, 0
    prefix = "opt"
    org = nn.ModuleDict(dict(embed_tokens=nn.Embedding(d["vocab"], E, padding_idx=1), embed_positions=OPTLearnedPositionalEmbedding(d["positions"], E)))
    load_weights(org, seed)
    qp = MG._qparams()
    front = nn.ModuleDict(dict(embed_tokens=quantize_model(org["embed_tokens"], **qp),
                               embed_positions=QuantizedOPTLearnedPositionalEmbedding(org["embed_positions"], **qp),
                               embed_sum_act_quantizer=QuantizedActivation(**qp)))
    arrays["optpos.keys"] = np.array(json.dumps(sorted(front["embed_positions"].state_dict().keys())))
    mask = t(ER.opt_mask(B, S, d["lengths"]))

    def fwd(m, ids):  # quantized_opt.py:549-569 without project_in
        inputs_embeds = m["embed_tokens"](ids)
        pos_embeds = m["embed_positions"](mask, past)
        return m["embed_sum_act_quantizer"](inputs_embeds + pos_embeds)

    for m in front.values():
        m.quantized()
    front.eval()
    batches = [t(ER.token_ids(seed + 1 + i, (B, S), d["vocab"])) for i in range(3)]
    with torch.no_grad():
        for i, ids in enumerate(batches[:2]):
            fwd(front, ids)
            MG._dump_quantizers(f"{prefix}.after{i + 1}", front, arrays)
        for m in front.values():
            m.fix_ranges()
        MG._dump_quantizers(f"{prefix}.final", front, arrays)
        name = "embed_sum_act_quantizer.activation_quantizer"
        rec, hs = LG.record(front, [name])
        fwd(front, batches[2])
        # the positions of a cached step, for the id rule alone (quantized_opt.py:39-51)
        attention_mask = mask.long()
        positions = (torch.cumsum(attention_mask, dim=1).type_as(attention_mask) * attention_mask).long() - 1
        arrays[f"{prefix}.positions_past5"] = (positions[:, 5:] + front["embed_positions"].offset).numpy()
    arrays[f"{prefix}.input_ids"] = batches[2].numpy()
    arrays[f"{prefix}.mask"] = mask.numpy()
    arrays[f"{prefix}.sum_idx"] = rec[name][1].numpy().astype(np.uint8)
    arrays[f"{prefix}.optpos_keys_calibrated"] = np.array(json.dumps(sorted(front["embed_positions"].state_dict().keys())))
    meta[prefix] = dict(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in d.items()}, weight_seed=seed, calib_seeds=[seed + 1, seed + 2],
                        eval_seed=seed + 3, offset=int(front["embed_positions"].offset))
    print(prefix, "sum indices", arrays[f"{prefix}.sum_idx"].shape)


def main():
    MG._shim()
    sys.path.insert(0, os.path.join(MG.REF, "OutEffHop"))
    torch.manual_seed(0)
    arrays, meta = {}, {}
    gen_quant_embedding(arrays, meta)
    gen_bert(arrays, meta)
    gen_opt(arrays, meta)
    arrays["meta_json"] = np.array(json.dumps(meta))
    MG.save("embed_front.npz", **arrays)


if __name__ == "__main__":
    main()
