#!/usr/bin/env python3
"""Device assembly of two source trees, kernel by kernel: the proof that a refactor under outeffhop_amd/csrc changed nothing the GPU executes.

  device_asm_diff.py <other-tree>/outeffhop_amd/csrc [unit ...] [--jobs N] [--keep DIR]

Every named unit (default: all of the Makefile's SRCS) is compiled to device assembly in this tree and in the other one - the compile command
is the Makefile's own for that unit's object (`make -n`, so the per-unit FULLROW_FLAGS / PRELOAD_FLAGS are in it) with `-c` replaced by
`--cuda-device-only -S` - and the two texts are compared function by function after dropping comment lines, assembler directives, labels and
the numbering of local labels (the per-build __hip_cuid_ symbol is data and never part of a function).  One line per kernel:

  <unit> <symbol> identical
  <unit> <symbol> differs (n → m instructions)

The comparison is textual: it does not look for particular instructions.  Exit status 1 if a kernel differs, 2 if a kernel exists in only
one of the trees, 0 otherwise.  Host only: no GPU is needed.
"""
from __future__ import annotations

import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "outeffhop_amd", "csrc")
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+_(\d+)")


def units_of(csrc: str) -> list[str]:
    for line in open(os.path.join(csrc, "Makefile")):
        if line.startswith("SRCS :="):
            return line.split(":=", 1)[1].split()
    raise SystemExit(f"{csrc}/Makefile: no SRCS")


def compile_command(csrc: str, unit: str, out: str) -> list[str]:
    """The Makefile's command for the unit's object, turned into a device-only assembly run."""
    obj = "/nonexistent-objdir"
    dry = subprocess.run(["make", "-C", csrc, "-n", "-B", f"OBJDIR={obj}", f"{obj}/{unit[:-4]}.o"], capture_output=True, text=True, check=True).stdout
    for line in dry.splitlines():
        words = shlex.split(line)
        if "-c" in words and unit in words:
            i = words.index("-o")
            del words[i:i + 2]
            words[words.index("-c")] = "-S"
            return words + ["--cuda-device-only", "-o", out]
    raise SystemExit(f"{csrc}: make -n shows no compile command for {unit}")


def functions(path: str) -> dict[str, list[str]]:
    """symbol -> its instruction lines."""
    funcs: dict[str, list[str]] = {}
    wanted: set[str] = set()
    cur = None
    for raw in open(path):
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if line.startswith(".type") and "@function" in line:
            wanted.add(line.split()[1].split(",")[0])
            continue
        if line.endswith(":") and " " not in line:
            name = line[:-1]
            if name in wanted:
                cur = funcs.setdefault(name, [])
            elif name.startswith(".Lfunc_end"):
                cur = None
            continue  # (labels themselves are dropped; branches keep their renumbered targets)
        if line.startswith("."):
            continue
        if cur is not None:
            cur.append(LOCAL_LABEL.sub(r".L\1_\2", " ".join(line.split())))
    return funcs


def assemble(csrc: str, unit: str, out: str) -> dict[str, list[str]]:
    r = subprocess.run(compile_command(csrc, unit, out), cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{csrc}/{unit}: compile failed\n{r.stderr}")
    return functions(out)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("other", help="<other-tree>/outeffhop_amd/csrc")
    ap.add_argument("units", nargs="*")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--keep", help="write the assembly files here instead of a temporary directory")
    a = ap.parse_args()
    a.other = os.path.abspath(a.other)
    units = a.units or units_of(HERE)
    with tempfile.TemporaryDirectory(prefix="oeh_asm_") as scratch, ThreadPoolExecutor(a.jobs) as pool:
        tmp = a.keep or scratch
        for side in ("this", "other"):
            os.makedirs(os.path.join(tmp, side), exist_ok=True)
        jobs = {(u, side): pool.submit(assemble, csrc, u, os.path.join(tmp, side, u[:-4] + ".s"))
                for u in units for side, csrc in (("other", a.other), ("this", HERE))}
        status = 0
        for u in units:
            old, new = jobs[(u, "other")].result(), jobs[(u, "this")].result()
            for name in sorted(set(old) | set(new)):
                if name not in old or name not in new:
                    print(f"{u} {name} only in {'this tree' if name in new else 'the other tree'}")
                    status = 2
                elif old[name] == new[name]:
                    print(f"{u} {name} identical")
                else:
                    print(f"{u} {name} differs ({len(old[name])} → {len(new[name])} instructions)")
                    status = max(status, 1)
    return status


if __name__ == "__main__":
    sys.exit(main())
