"""The built library's gfx950 code objects, read without a GPU: one per translation unit, unbundled from libechoseal_hip.so's
.hip_fatbin with the ROCm LLVM tools.  For tests of kernel metadata (register budgets, spills) and of the ISA itself.  A test that
uses them skips when the tools or the built library are missing."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "echoseal_amd", "libechoseal_hip.so")
LLVM = "/opt/rocm/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def code_objects(tmp_path, lib=LIB):
    """Paths of the gfx950 code objects in `lib`, one per translation unit with device code."""
    objcopy, bundler = _tool("llvm-objcopy") or shutil.which("objcopy"), _tool("clang-offload-bundler")
    if not (objcopy and bundler) or not os.path.exists(lib):
        pytest.skip("ROCm LLVM tools or the built library missing")
    fat = tmp_path / "fat.bin"
    subprocess.check_call([objcopy, "-O", "binary", "--only-section=.hip_fatbin", lib, str(fat)])
    data = fat.read_bytes()
    offs = [m.start() for m in re.finditer(re.escape(MAGIC), data)] + [len(data)]
    out = []
    for k in range(len(offs) - 1):                  # one offload bundle per translation unit
        b, co = tmp_path / f"b{k}.bin", tmp_path / f"co{k}.elf"
        b.write_bytes(data[offs[k]:offs[k + 1]])
        if subprocess.run([bundler, "--unbundle", "--type=o", "--input", str(b), f"--targets={TARGET}", "--output", str(co)],
                          capture_output=True).returncode:
            continue
        out.append(co)
    return out


def kernel_metadata(co):
    """{kernel symbol: {vgpr_count, vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size}} of one code object."""
    readelf = _tool("llvm-readelf")
    if not readelf:
        pytest.skip("llvm-readelf missing")
    notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    md = {}
    for block in re.split(r"\n  - \.agpr_count:", notes):
        name = re.search(r"\.name:\s+(\S+)\s", block)
        if name:
            md[name.group(1)] = {k: int(v) for k, v in re.findall(
                r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}
    return md


def disassembly(co):
    """{function symbol: [mnemonic, ...]} of one code object: every function, kernels and out-of-line callees alike."""
    objdump = _tool("llvm-objdump")
    if not objdump:
        pytest.skip("llvm-objdump missing")
    text = subprocess.run([objdump, "-d", "--mcpu=gfx950", str(co)], capture_output=True, text=True, check=True).stdout
    funcs, cur = {}, None
    for line in text.splitlines():
        head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if head:
            cur = funcs.setdefault(head.group(1), [])
        elif cur is not None:
            op = re.match(r"^\s+([a-z_][a-z0-9_]*)\b", line)
            if op:
                cur.append(op.group(1))
    return funcs
