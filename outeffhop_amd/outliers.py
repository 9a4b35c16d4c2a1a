"""The reference's result metrics - maximum infinity norm and average kurtosis of layer outputs - measured on the device.

The reference hooks the layers of interest and, per batch and hooked tensor, runs x.norm(dim=1, p=inf) and `kurtosis(x)` and feeds every
sample's value to an AverageMeter through .item() (validate_clm.py:565-621, validate_mlm.py:497-533, validate_vit1.py:620-693,
run_clm_ddp.py:735-760).  `OutlierMeter` keeps the same running sums in device memory: each hooked tensor costs one
`ops.outlier_stats` call (one pass over the tensor, no host synchronisation), and `summary()` makes the one device-to-host copy.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Iterable, Optional, Sequence

import torch

from . import _lib, ops


class OutlierMeter:
    """Forward hooks on the sub-modules `names` of `model`.  The hooked tensor is the module's output (the first element of a tuple
    output) and, for the names in `inputs`, its first input as well, keyed name + ".input" with the infinity norm only
    (validate_mlm.py:524-533).  Each tensor is viewed as (B, -1).  kurtosis_batches: the kurtosis is accumulated during the first so
    many forward passes of a module only (the reference's `batch_idx <= 100` for OPT is kurtosis_batches=101, `<= 256` for BERT 257);
    None: always."""

    def __init__(self, model: torch.nn.Module, names: Sequence[str], *, inputs: Iterable[str] = (), kurtosis_batches: Optional[int] = None,
                 eps: float = 1e-6):
        self.names = list(names)
        self.inputs = set(inputs)
        unknown = self.inputs - set(self.names)
        if unknown:
            raise ValueError(f"inputs must be among names: {sorted(unknown)}")
        self.kurtosis_batches = kurtosis_batches
        self.eps = float(eps)
        self.keys = []  # every meter, in the order the reference's dict would get them
        for n in self.names:
            self.keys.append(n)
            if n in self.inputs:
                self.keys.append(n + ".input")
        self._row = {k: i for i, k in enumerate(self.keys)}
        if len(self._row) != len(self.keys):
            raise ValueError("duplicate names")
        self._meters = None  # (len(keys), 4) float64 on the model's GPU: {sum_inf, n_inf, sum_kurt, n_kurt} per key
        self._calls = {n: 0 for n in self.names}
        self._handles = []
        modules = dict(model.named_modules())
        for n in self.names:
            if n not in modules:
                raise KeyError(f"{n!r} is not a sub-module of the model")
            self._handles.append(modules[n].register_forward_hook(self._hook(n)))

    def _hook(self, name: str):
        def hook(module, args, output):
            out = output[0] if isinstance(output, (tuple, list)) else output
            want_kurt = self.kurtosis_batches is None or self._calls[name] < self.kurtosis_batches
            self._calls[name] += 1
            self._measure(name, out, 1 | (2 if want_kurt else 0))
            if name in self.inputs:
                self._measure(name + ".input", args[0], 1)

        return hook

    def _measure(self, key: str, x: torch.Tensor, accumulate: int) -> None:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.OehError("OutlierMeter needs GPU tensors: the HIP library is the only implementation")
        if self._meters is None:
            self._meters = torch.zeros((len(self.keys), 4), dtype=torch.float64, device=x.device)
        x = x.detach()
        if x.dim() < 2:
            x = x.reshape(x.shape[0] if x.dim() else 1, -1)
        ops.outlier_stats(x, self.eps, meter=self._meters[self._row[key]], accumulate=accumulate)

    @staticmethod
    def summarize(keys: Sequence[str], meters, layer_names: Optional[Sequence[str]] = None, ffn_substr: str = ".fc") -> "OrderedDict[str, float]":
        """The metrics dict of validate_clm.py:598-621 from host values: meters[i] = (sum_inf, n_inf, sum_kurt, n_kurt) of keys[i].
        Every key's average inf-norm under the key itself, then max_inf_norm, max_ffn_inf_norm (keys containing `ffn_substr`),
        max_layer_inf_norm (over `layer_names`; None: over all keys), avg_kurtosis, max_kurtosis, max_kurtosis_layers.  A maximum
        over an empty selection (no key with `ffn_substr`, no kurtosis recorded) is left out."""
        inf_avg, kurt_avg = OrderedDict(), OrderedDict()
        for k, m in zip(keys, meters):
            s_inf, n_inf, s_kurt, n_kurt = (float(v) for v in m)
            if n_inf > 0:
                inf_avg[k] = s_inf / n_inf
            if n_kurt > 0:
                kurt_avg[k] = s_kurt / n_kurt
        layers = list(inf_avg) if layer_names is None else list(layer_names)
        metrics = OrderedDict(inf_avg)

        def put(name, values):
            values = list(values)
            if values:
                metrics[name] = max(values)

        put("max_inf_norm", inf_avg.values())
        put("max_ffn_inf_norm", (v for k, v in inf_avg.items() if ffn_substr in k))
        put("max_layer_inf_norm", (inf_avg[k] for k in layers if k in inf_avg))
        if kurt_avg:
            metrics["avg_kurtosis"] = sum(kurt_avg.values()) / len(kurt_avg)
        put("max_kurtosis", kurt_avg.values())
        put("max_kurtosis_layers", (kurt_avg[k] for k in layers if k in kurt_avg))
        return metrics

    def summary(self, layer_names: Optional[Sequence[str]] = None, ffn_substr: str = ".fc") -> "OrderedDict[str, float]":
        """The one device-to-host copy: the reference's metrics dict (`summarize`)."""
        if self._meters is None:
            return OrderedDict()
        return self.summarize(self.keys, self._meters.cpu().tolist(), layer_names, ffn_substr)

    def reset(self) -> None:
        if self._meters is not None:
            self._meters.zero_()
        self._calls = {n: 0 for n in self.names}

    def remove(self) -> None:
        for h in self._handles:
            h.remove()
        self._handles = []
