"""The hot argument prefix of the one-pass kernel reaches the waves in SGPRs only if the built code object says so: the kernel descriptor's
kernarg preload length.  It comes from a per-unit compiler option (csrc/Makefile: PRELOAD_FLAGS) and from the kernel's parameter list (leading
scalars; a by-value struct is never preloaded), so a toolchain or Makefile change can drop it without any test of the results noticing - the
compiled kernel keeps a prologue of scalar loads and computes the same.  Read it back from the built library (no GPU needed)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# oeh_attn_flash_hot_kernel<D = 64, IN, MQ>: fp16 / bf16, one and two query blocks per wave; <64, f16, 2> is the headline launch
HOT = [f"oeh_attn_flash_hot_kernelILi64ELi{i}ELi{mq}E" for i in (0, 1) for mq in (2, 1)]
STRUCT_ONLY = "oeh_attn_flash_kernelILi64ELi0ELi2ELb0ELb0ELb0ELi0ELb0ELb0E"


@pytest.fixture(scope="module")
def code_objects(tmp_path_factory):
    from outeffhop_amd import _lib

    if not (os.path.exists(f"{LLVM}/llvm-readelf") and os.path.exists(f"{LLVM}/llvm-objdump")):
        pytest.skip("no ROCm llvm tools")
    tmp = str(tmp_path_factory.mktemp("co"))
    lib = os.path.join(tmp, "lib.so")
    shutil.copy(_lib.LIB_PATH, lib)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", lib], check=True, capture_output=True, cwd=tmp)
    cos = sorted(glob.glob(lib + ".*gfx950"))
    assert cos, "no gfx950 code object in the built library"
    # kernel-descriptor symbol (.symbol of the code-object metadata) -> code object
    syms = {}
    for co in cos:
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        for m in re.finditer(r"\.symbol:\s+(\S+\.kd)", notes):
            syms[m.group(1)] = co
    return syms


def _descriptor(syms, fragment):
    """the one kernel whose name contains `fragment`: its descriptor's directives as {name: int}"""
    hits = [s for s in syms if fragment in s]
    assert len(hits) == 1, f"{fragment}: {len(hits)} kernels in the code-object metadata"
    txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "-j", ".rodata", f"--disassemble-symbols={hits[0]}", syms[hits[0]]],
                         check=True, capture_output=True, text=True).stdout
    d = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_(\w+)\s+(\d+)", txt)}
    assert "next_free_vgpr" in d, f"{hits[0]}: no kernel descriptor in the disassembly"
    return d


@pytest.mark.parametrize("kernel", HOT)
def test_hot_prefix_kernels_are_built_with_kernarg_preload(code_objects, kernel):
    d = _descriptor(code_objects, kernel)
    # 16 user SGPRs less the kernarg segment pointer: the 14 dwords of AttnHot, all of them
    assert d.get("user_sgpr_kernarg_preload_length", 0) == 14, d


def test_struct_only_kernel_has_no_preload(code_objects):
    """the AttnParams-only entry is compiled as before (a by-value struct is not preloaded): nothing to move, no compatibility prologue"""
    d = _descriptor(code_objects, STRUCT_ONLY)
    assert d.get("user_sgpr_kernarg_preload_length", 0) == 0, d
