"""The peak-addressed entry points (es_llr_at_batch, es_header_at_batch, es_front_peak_batch) at the boundary, without a GPU:
declared in the header under ABI version 2, exported by the built library, bound by _native with the header's argument counts.

Their kernels are new instantiations (a template flag) of the demodulator and the header decoder; the instantiations behind
es_llr_batch / es_header_batch keep the VGPRs, SGPRs, LDS and scratch they had before the flag existed (values read from that
build and written down here), and the new ones use no scratch."""
import ctypes
import os
import re
import subprocess

import pytest

from code_objects import LIB, ROOT, _tool, code_objects

HEADER = os.path.join(ROOT, "include", "echoseal_hip.h")
NEW = {"es_llr_at_batch": 15, "es_header_at_batch": 15, "es_front_peak_batch": 15}

# (kernel, taps, addressed) -> vgpr_count, sgpr_count, group_segment_fixed_size (LDS bytes), private_segment_fixed_size (scratch)
EXISTING = {
    ("es_llr_wave_kernel", 160): (150, 106, 17184, 0),
    ("es_llr_wave_kernel", 576): (159, 106, 41344, 0),
    ("es_header_kernel", 160): (57, 67, 4320, 0),
    ("es_header_kernel", 576): (62, 67, 9312, 0),
}
FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def test_header_declares_the_new_functions_under_abi_2():
    import echoseal_amd._native as nat
    assert os.path.samefile(nat.HEADER_PATH, HEADER) and nat.CONSTANTS["ES_ABI_VERSION"] == 2
    for name, n in NEW.items():
        assert len(nat.DECLARATIONS[name]) == n, name


def test_native_binds_the_new_functions():
    import echoseal_amd._native as nat
    for name, n in NEW.items():
        res, args = nat.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n == len(nat.DECLARATIONS[name]), name
    assert nat.ES_ABI_VERSION == 2


def test_library_exports_the_new_functions():
    if not os.path.exists(LIB):
        pytest.skip("library not built")
    nm = _tool("llvm-nm") or _tool("nm")
    if not nm:
        pytest.skip("nm missing")
    syms = set(subprocess.run([nm, "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split())
    for name in NEW:
        assert name in syms, name


def _resources(tmp_path):
    readelf = _tool("llvm-readelf")
    if not readelf:
        pytest.skip("llvm-readelf missing")
    out = {}
    for co in code_objects(tmp_path):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n  - \.agpr_count:", notes):
            name = re.search(r"\.name:\s+(\S+)\s", block)
            k = name and re.search(r"(es_llr_wave_kernel|es_header_kernel)ILi(\d+)ELb([01])E", name.group(1))
            if k:
                vals = dict(re.findall(r"\.(" + "|".join(FIELDS) + r"):\s+(\d+)", block))
                out[(k.group(1), int(k.group(2)), k.group(3) == "1")] = tuple(int(vals[f]) for f in FIELDS)
    return out


def test_existing_instantiations_keep_their_resources(tmp_path):
    res = _resources(tmp_path)
    for (kernel, taps), want in EXISTING.items():
        assert res.get((kernel, taps, False)) == want, (kernel, taps, res.get((kernel, taps, False)))


def test_addressed_instantiations_use_no_scratch(tmp_path):
    res = _resources(tmp_path)
    for kernel, taps in EXISTING:
        got = res.get((kernel, taps, True))
        assert got is not None, (kernel, taps)
        assert got[3] == 0, (kernel, taps, got)
