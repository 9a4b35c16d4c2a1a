"""Seeded inputs and weights of tests/golden/embed_front.npz: tests/golden/make_embed_golden.py (next to the reference) and the tests (GPU box)
regenerate the same bits from numpy's legacy RandomState streams; the fixture stores seeds, ranges, key lists, indices and error figures only.
numpy only; no GPU, no package import."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("_ln_ref_for_embed", os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ln_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

BERT = dict(B=2, S=16, E=768, vocab=512, types=2, positions=512, eps=1e-12)
OPT = dict(B=2, S=32, E=256, vocab=512, positions=64, lengths=(32, 23))


def front_state_dict(shapes: dict, seed: int):
    """`_ln_ref.tail_state_dict` (tables N(0, 0.05), LayerNorm weights 1 + N(0, 0.2), biases N(0, 0.1)) with the residual stream's outlier
    channels (`_ln_ref.OUTLIER_CHANNELS`) in the token table, which is where a model's stream gets them from."""
    out = R.tail_state_dict(shapes, seed)
    for name in out:
        if name.endswith("word_embeddings.weight") or name.endswith("embed_tokens.weight"):
            out[name] = R.with_outliers(out[name])
    return out


def token_ids(seed: int, shape, n_rows: int):
    """int64 ids in [0, n_rows) with repeats, the first and the last row among them."""
    ids = np.random.RandomState(seed).randint(0, n_rows, size=tuple(shape)).astype(np.int64)
    flat = ids.reshape(-1)
    flat[0], flat[-1] = 0, n_rows - 1
    if flat.size > 3:
        flat[2] = flat[1]
    return ids


def opt_mask(B: int, S: int, lengths):
    """(B, S) int64, left-padded: row b keeps its last lengths[b] positions."""
    m = np.zeros((B, S), dtype=np.int64)
    for b, n in enumerate(lengths):
        m[b, S - n:] = 1
    return m


def opt_positions(mask, past: int = 0, offset: int = 2):
    """quantized_opt.py:39-51 in numpy: cumsum(mask) * mask - 1, cut to the new tokens, + offset."""
    mask = np.asarray(mask, dtype=np.int64)
    return (np.cumsum(mask, axis=1) * mask - 1)[:, past:] + offset
