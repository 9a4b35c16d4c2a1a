#!/usr/bin/env python3
"""Which instances of the LayerNorm-row kernels a traced run launched, held against the built library:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 -m pytest tests/test_ln_instances_gpu.py -m gpu -q
    python tools/ln_trace_names.py <dir> [out.txt]
Reads every *kernel_stats.csv / *kernel_trace.csv under <dir>; writes one line per launched instance (tests/_ln_inst.py's key, the kernel's
name as the profiler gives it, calls where the stats table has them) and the instances the library has that the run did not launch."""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _ln_inst as I  # noqa: E402

KERNELS = {"oeh_resid_ln_kernel": ("ln", 3), "oeh_embed_kernel": ("embed", 4), "oeh_ln_train_fwd_kernel": ("ln_train_fwd", 4),
           "oeh_ln_train_bwd_kernel": ("ln_train_bwd", 4)}


def key_of(name: str):
    """The instance key of a kernel name, mangled or demangled; None for any other kernel."""
    m = re.search(r"(oeh_resid_ln_kernel|oeh_embed_kernel|oeh_ln_train_fwd_kernel|oeh_ln_train_bwd_kernel)(<([^>]*)>|I)", name)
    if not m:
        return None
    kernel, width = KERNELS[m.group(1)]
    if m.group(3) is not None:
        args = [int({"true": "1", "false": "0"}.get(a.strip(), re.sub(r"^\(\w+\)", "", a.strip()))) for a in m.group(3).split(",")]
    else:
        args = I.targs(name[m.start():])
    return (kernel,) + tuple(args[:width])


def main():
    d = sys.argv[1]
    seen = {}
    # the stats table (one row per kernel, with its calls) where there is one, else the trace (one row per launch)
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)) or sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("Kernel_Name") or ""
                k = key_of(name)
                if k is None:
                    continue
                first, calls = seen.get(k, (name, 0))
                seen[k] = (first, calls + int(row.get("Calls") or 1))
    built = I.built_instances()
    missing = sorted(built - set(seen))
    lines = [f"# {len(seen)} instances of the LayerNorm-row kernels launched; the library has {len(built)}; not launched: {len(missing)}"]
    lines += [f"{k!s:40s} calls {seen[k][1]:5d}  {seen[k][0]}" for k in sorted(seen)]
    lines += [f"NOT LAUNCHED {k}" for k in missing]
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            fh.write(text)
    print(lines[0])
    for k in missing[:40]:
        print("NOT LAUNCHED", k)
    return 0


if __name__ == "__main__":
    sys.exit(main())
