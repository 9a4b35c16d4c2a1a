#!/usr/bin/env python3
"""Generate tests/golden/mse_ranges.npz by IMPORTING the reference's MSE range estimator.

Run ONLY in the build container (where /root/reference is mounted, CPU only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mse_golden.py

The reference's `quantization` package is imported from its own tree (it needs torch, numpy and scipy only).  Nothing of its text is
stored, only data: inputs, the estimator's loss arrays and ranges, and the description of its constructor.

Every case runs the reference's MSE_Estimator (quantization/range_estimators.py:114-382) on TWO successive batches of 4096 fp32
values and records its state after each.  Per case C in CASES:
  x_C           (2, 4096) fp32        the two batches
  loss_C        float64               the reference's loss_array after each batch: (2, N + 1) or (2, N + 1, max_int_skew, 2)  [grid cases]
  xmin_C, xmax_C (2,) fp32            current_xmin / current_xmax after each batch
  margin_C      (2,) float64          (second-smallest - smallest) / smallest accumulated loss after each batch  [grid cases]; the script
                                      asserts that every one is above MIN_MARGIN = 1e-5: the fp32 sums of the reference and the float64 sums
                                      of the package differ by at most (log2 n + 2) * 2^-24 ~ 8e-7 relative, so both choose the same candidate
  f64dist_C     (2, 2) float64        [golden-section cases] |range found with the reference's fp32-summed loss - range found by the
                                      reference's search with the SAME terms summed in float64| for (xmin, xmax) after each batch: what the
                                      reference's fp32 sums do to the search's result
and  cases (names), case_quantizer, case_opt_method, case_n_bits, case_num_candidates, case_kind;
     signature_names / signature_kinds / signature_defaults: inspect.signature(MSE_Estimator.__init__) (defaults as str(), enum members
     by name); opt_method_names: OptMethod.list_names().

Inputs (numpy legacy streams): N(0, 1); Student-t(3); N(0, 1) as a (64, 64) block with every 16th column x 60; softmax rows of
2 * N(0, 1) over 64 columns (one-sided).
"""
import inspect
import os
import sys

import numpy as np
import torch

REF = "/root/reference/OutEffHop"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
N = 4096
MIN_MARGIN = 1e-5

# name: (quantiser, input kind, opt_method, n_bits, num_candidates)
CASES = {
    "sym_two_sided_8": ("symmetric", "normal", "grid", 8, 100),
    "sym_two_sided_4": ("symmetric", "student_t3", "grid", 4, 100),
    "sym_one_sided_8": ("symmetric", "softmax", "grid", 8, 100),
    "asym_one_sided_8": ("asymmetric", "softmax", "grid", 8, 100),
    "asym_two_sided_2d": ("asymmetric", "outlier_columns", "grid", 8, 10),
    "golden_sym": ("symmetric", "normal", "golden_section", 8, 100),
    "golden_asym": ("asymmetric", "student_t3", "golden_section", 8, 100),
}


def draw(kind: str, seed: int) -> np.ndarray:
    rs = np.random.RandomState(seed)
    if kind == "normal":
        x = rs.standard_normal(size=N)
    elif kind == "student_t3":
        x = rs.standard_t(3, size=N)
    elif kind == "outlier_columns":
        x = rs.standard_normal(size=(64, 64))
        x[:, 3::16] *= 60.0
    else:  # softmax rows
        z = 2.0 * rs.standard_normal(size=(64, 64))
        e = np.exp(z - z.max(axis=1, keepdims=True))
        x = e / e.sum(axis=1, keepdims=True)
    return x.reshape(-1).astype(np.float32)


def main():
    sys.path.insert(0, REF)
    from quantization.quantizers.uniform_quantizers import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    from quantization.range_estimators import MSE_Estimator, OptMethod
    from quantization.utils import to_numpy

    class F64Sum(MSE_Estimator):  # the reference's search on the same fp32 terms, summed in float64
        def loss_fx(self, data, neg_thr, pos_thr, per_channel_loss=False):
            y = self.quantize(data, x_min=neg_thr, x_max=pos_thr)
            return to_numpy(torch.sum(((data - y) ** 2).double()))

    out = {"cases": np.array(list(CASES))}
    for i, (name, (qname, kind, method, n_bits, num_cand)) in enumerate(CASES.items()):
        x = np.stack([draw(kind, 7000 + 10 * i), draw(kind, 7001 + 10 * i)])
        out[f"x_{name}"] = x
        qcls = SymmetricUniformQuantizer if qname == "symmetric" else AsymmetricUniformQuantizer
        ests = [cls(num_candidates=num_cand, opt_method=OptMethod[method], quantizer=qcls(n_bits=n_bits)) for cls in (MSE_Estimator, F64Sum)]
        losses, mins, maxs, margins, dists = [], [], [], [], []
        for b in range(2):
            data = torch.from_numpy(x[b])
            xmin, xmax = ests[0](data)
            mins.append(np.float32(xmin.reshape(-1)[0].item()))
            maxs.append(np.float32(xmax.reshape(-1)[0].item()))
            if method == "grid":
                la = ests[0].loss_array[0].copy()
                losses.append(la)
                srt = np.sort(la.reshape(-1))
                margins.append((srt[1] - srt[0]) / srt[0])
                assert margins[-1] > MIN_MARGIN, (name, b, margins[-1])
            else:
                lo64, hi64 = ests[1](data)
                dists.append([abs(float(xmin.reshape(-1)[0]) - float(lo64.reshape(-1)[0])), abs(float(xmax.reshape(-1)[0]) - float(hi64.reshape(-1)[0]))])
        out[f"xmin_{name}"], out[f"xmax_{name}"] = np.array(mins, np.float32), np.array(maxs, np.float32)
        if method == "grid":
            out[f"loss_{name}"] = np.stack(losses)
            out[f"margin_{name}"] = np.array(margins, np.float64)
            assert ests[0].one_sided_dist == (kind == "softmax")
            print(f"{name:18s} loss {out[f'loss_{name}'].shape} range ({mins[-1]:.6g}, {maxs[-1]:.6g}) margins {margins[0]:.2e} {margins[1]:.2e}")
        else:
            out[f"f64dist_{name}"] = np.array(dists, np.float64)
            print(f"{name:18s} range ({mins[-1]:.6g}, {maxs[-1]:.6g}) fp32-sum effect {np.max(dists):.2e}")
    vals = list(CASES.values())
    for j, key in enumerate(("case_quantizer", "case_kind", "case_opt_method")):
        out[key] = np.array([v[j] for v in vals])
    out["case_n_bits"] = np.array([v[3] for v in vals])
    out["case_num_candidates"] = np.array([v[4] for v in vals])
    params = [p for p in inspect.signature(MSE_Estimator.__init__).parameters.values()]
    out["signature_names"] = np.array([p.name for p in params])
    out["signature_kinds"] = np.array([p.kind.name for p in params])
    out["signature_defaults"] = np.array(["<empty>" if p.default is inspect.Parameter.empty else (p.default.name if isinstance(p.default, OptMethod) else str(p.default))
                                          for p in params])
    out["opt_method_names"] = np.array(OptMethod.list_names())
    path = os.path.join(OUT, "mse_ranges.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
