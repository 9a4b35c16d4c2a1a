#!/usr/bin/env python3
"""Generate tests/golden/outlier_stats.npz by IMPORTING the reference's `kurtosis`.

Run ONLY in the build container (where /root/reference is mounted, CPU only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_outlier_golden.py

`kurtosis` is loaded from the reference's transformers_language/utils.py as a file.  That file imports two names from the
reference's `quantization` package which `kurtosis` does not use; stub modules of those names stand in (the kind of shim
make_golden.py applies).  Nothing of the reference's text is stored, only data.

The reference takes its AverageMeter from timm.utils.  timm is not installed here, so the five-line sum / count class below
stands in: update(val) adds val to a Python float sum and 1 to a count, avg = sum / count - what timm's class does for n = 1.

Contents (fp32 unless said otherwise), per input kind K in KINDS:
  short_K      (4, 777) input
  long_base    ONE (3, 40000) draw of N(0, 1).  The long input of every kind is long_input(long_base, K): the base itself, the base
               + 1000, x 1e-3, with its outlier columns or planted value, and for Student-t(3) z / sqrt(chi2 / 3) with z the base and
               chi2 the squares of three shifted copies of it - additions, products, quotients and square roots only, which IEEE
               arithmetic rounds identically everywhere.  Six independent (3, 40000) fp32 arrays do not compress and would be 2.9 MB.
               tests/test_outlier_stats_*.py restate `long_input`.
  kurt_short_K, kurt_long_K, inf_short_K, inf_long_K   the reference's kurtosis(x) and x.norm(dim=1, p=inf)
  kurt_err_short_K, kurt_err_long_K (float64)           |reference - float64 evaluation| / |float64 evaluation| per row
and one AverageMeter scenario (three batches, two names, kurtosis during the first two batches only, as validate_clm.py:565-621
runs it): scenario_keys, scenario_batches (which short inputs were fed), scenario_meters (2, 4) float64 = (sum_inf, n_inf,
sum_kurt, n_kurt) per name, scenario_metric_keys / scenario_metric_values (float64): the final metrics dict in order.
"""
import importlib.machinery
import importlib.util
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch

REF = "/root/reference/OutEffHop"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

KINDS = ("normal", "student_t3", "outlier_columns", "large_mean", "tiny", "planted")
SHORT, LONG = (4, 777), (3, 40000)


def load_reference_kurtosis():
    for name, attrs in (("quantization", ()), ("quantization.range_estimators", ("RangeEstimators",)), ("quantization.utils", ("StopForwardException",))):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, None)
            m.__path__ = []
            for a in attrs:
                setattr(m, a, type(a, (), {}))
            sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("_ref_tl_utils", os.path.join(REF, "transformers_language", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kurtosis


def structure(x: np.ndarray, kind: str) -> np.ndarray:
    x = x.copy()
    if kind == "outlier_columns":
        x[:, ::97] *= np.float32(60.0)
    if kind == "planted":
        x[-1, -1] = np.float32(-50.0)
    return x


def long_input(base: np.ndarray, kind: str) -> np.ndarray:
    z = base.astype(np.float64)
    if kind == "student_t3":
        a, b, c = np.roll(z, 1, axis=0), np.roll(z, 2, axis=0), np.roll(z, 1, axis=1)
        z = z / np.sqrt((a * a + b * b + c * c) / 3.0)
    if kind == "large_mean":
        z = z + 1000.0
    if kind == "tiny":
        z = z * 1e-3
    return structure(z.astype(np.float32), kind)


def draw(rng, kind: str, shape) -> np.ndarray:
    if kind == "student_t3":
        x = rng.standard_t(3, size=shape)
    else:
        x = rng.standard_normal(size=shape)
    if kind == "large_mean":
        x = x + 1000.0
    if kind == "tiny":
        x = x * 1e-3
    return x.astype(np.float32)


def f64_kurtosis(x: np.ndarray, eps: float = 1e-6) -> np.ndarray:
    x = x.astype(np.float64)
    mu = x.mean(axis=1, keepdims=True)
    return ((x - mu) ** 4).mean(axis=1) / (x.std(axis=1, ddof=1) ** 4 + eps)


class Meter:  # stands in for timm.utils.AverageMeter (not installed here): update(val) with n = 1
    def __init__(self):
        self.sum, self.count = 0.0, 0

    def update(self, val):
        self.sum += val
        self.count += 1

    @property
    def avg(self):
        return self.sum / self.count


def main():
    kurtosis = load_reference_kurtosis()
    rng = np.random.default_rng(20240611)
    base = np.random.default_rng(20240612).standard_normal(size=LONG).astype(np.float32)
    out = {"long_base": base}
    for kind in KINDS:
        short = structure(draw(rng, kind, SHORT), kind)
        draw(rng, kind, (4096,))  # (not stored: an earlier form of this fixture resampled its long inputs from these; drawing them keeps the short inputs)
        out[f"short_{kind}"] = short
        for tag, x in (("short", short), ("long", long_input(base, kind))):
            t = torch.from_numpy(x)
            k = kurtosis(t).numpy().astype(np.float32)
            out[f"kurt_{tag}_{kind}"] = k
            out[f"inf_{tag}_{kind}"] = t.norm(dim=1, p=np.inf).numpy().astype(np.float32)
            k64 = f64_kurtosis(x)
            out[f"kurt_err_{tag}_{kind}"] = np.abs(k.astype(np.float64) - k64) / np.abs(k64)
            print(f"{kind:16s} {tag:5s} reference vs float64: {out[f'kurt_err_{tag}_{kind}'].max():.2e}")

    # the evaluation loop of validate_clm.py:565-621 on two names, three batches, kurtosis while batch_idx <= 1
    keys = ("model.decoder.layers.0.fc2", "model.decoder.layers.0")
    batches = (("student_t3", "normal"), ("outlier_columns", "planted"), ("normal", "large_mean"))
    inf_m, kurt_m = OrderedDict(), OrderedDict()
    for batch_idx, fed in enumerate(batches):
        for name, kind in zip(keys, fed):
            x = torch.from_numpy(out[f"short_{kind}"])
            x = x.view(x.size(0), -1)
            for v in x.norm(dim=1, p=np.inf):
                inf_m.setdefault(name, Meter()).update(v.item())
            if batch_idx <= 1:
                for v in kurtosis(x):
                    kurt_m.setdefault(name, Meter()).update(v.item())
    metrics = OrderedDict((name, m.avg) for name, m in inf_m.items())
    metrics["max_inf_norm"] = max(m.avg for m in inf_m.values())
    metrics["max_ffn_inf_norm"] = max(m.avg for k, m in inf_m.items() if ".fc" in k)
    metrics["max_layer_inf_norm"] = max(inf_m[k].avg for k in keys[1:])
    metrics["avg_kurtosis"] = sum(m.avg for m in kurt_m.values()) / len(kurt_m)
    metrics["max_kurtosis"] = max(m.avg for m in kurt_m.values())
    metrics["max_kurtosis_layers"] = max(kurt_m[k].avg for k in keys[1:])
    out["scenario_keys"] = np.array(keys)
    out["scenario_batches"] = np.array(batches)
    out["scenario_meters"] = np.array([[inf_m[k].sum, inf_m[k].count, kurt_m[k].sum, kurt_m[k].count] for k in keys], dtype=np.float64)
    out["scenario_metric_keys"] = np.array(list(metrics))
    out["scenario_metric_values"] = np.array(list(metrics.values()), dtype=np.float64)
    path = os.path.join(OUT, "outlier_stats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
