"""The built library's code-object metadata for the headline list decoder (es_scl_wide_kernel<64, 8, false>, lists of 8 in one-wave
blocks): the register budget it was compiled for, and a ceiling on its VGPR spills.  The spills it has sit outside the f loops (frame
draw, the per-bit decision); a new one is a change to look at in the ISA, because a spill inside an f loop costs scratch traffic per
evaluation."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "echoseal_amd", "libechoseal_hip.so")
LLVM = "/opt/rocm/llvm/bin"
HEADLINE = "_ZN12_GLOBAL__N_118es_scl_wide_kernelILi64ELi8ELb0EEEvNS_8WideArgsE"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def _kernel_metadata(tmp_path):
    objcopy, bundler, readelf = _tool("llvm-objcopy") or shutil.which("objcopy"), _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not (objcopy and bundler and readelf) or not os.path.exists(LIB):
        pytest.skip("ROCm LLVM tools or the built library missing")
    fat = tmp_path / "fat.bin"
    subprocess.check_call([objcopy, "-O", "binary", "--only-section=.hip_fatbin", LIB, str(fat)])
    data = fat.read_bytes()
    offs = [m.start() for m in re.finditer(re.escape(MAGIC), data)] + [len(data)]
    for k in range(len(offs) - 1):                  # one offload bundle per translation unit
        b, co = tmp_path / f"b{k}.bin", tmp_path / f"co{k}.elf"
        b.write_bytes(data[offs[k]:offs[k + 1]])
        if subprocess.run([bundler, "--unbundle", "--type=o", "--input", str(b), "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--output", str(co)], capture_output=True).returncode:
            continue
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n  - \.agpr_count:", notes):
            if re.search(r"\.name:\s+" + re.escape(HEADLINE) + r"\s", block):
                return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}
    raise AssertionError(f"{HEADLINE} not found in {LIB}")


def test_headline_list_decoder_budget_and_spills(tmp_path):
    md = _kernel_metadata(tmp_path)
    assert md["vgpr_count"] <= 168, md              # __launch_bounds__(64, 3): three waves per SIMD
    assert md["vgpr_spill_count"] <= 16, md
