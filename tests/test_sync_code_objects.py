"""The ISA of the sync and demodulator code objects, read from the built library without a GPU.

No flat memory instructions: a flat access that resolves to LDS must not be merged wider than its alignment, and the compiler
only knows that when the pointer is typed.  Through a generic pointer it once merged two LDS doubles into an 8-byte-aligned
flat_load_dwordx4, a memory-aperture violation that aborted the queue.  So every function of these code
objects, out-of-line callees included, reaches LDS through address_space(3) and global memory through address_space(1) pointers.

Register budget of the fused sync kernel: three waves per SIMD (<= 168 VGPRs, the slot one list-decoder wave leaves behind), and
no more VGPR spills or scratch than when the picker was first typed."""
import pytest

from code_objects import LIB, code_objects, disassembly, kernel_metadata

FLAT_FREE = ("es_xcorr32_kernel", "es_xcorr_kernel", "es_llr_wave_kernel")

# es_xcorr32_kernel<R, TC, true>: (VGPR spills, private segment bytes) ceilings
FUSED = {
    "_ZN12_GLOBAL__N_117es_xcorr32_kernelILi17ELi2048ELb1EE": (0, 64),
    "_ZN12_GLOBAL__N_117es_xcorr32_kernelILi19ELi1215ELb1EE": (0, 64),
    "_ZN12_GLOBAL__N_117es_xcorr32_kernelILi19ELi0ELb1EE": (6, 96),
}


def _find(cos, kernel):
    for co in cos:
        funcs = disassembly(co)
        if any(kernel in f for f in funcs):
            return co, funcs
    raise AssertionError(f"no code object of {LIB} defines {kernel}")


@pytest.mark.parametrize("kernel", FLAT_FREE)
def test_no_flat_memory_instructions(tmp_path, kernel):
    _, funcs = _find(code_objects(tmp_path), kernel)
    flat = {f: n for f, ops in funcs.items() if (n := sum(op.startswith("flat_") for op in ops))}
    assert not flat, flat


def test_fused_sync_register_budget(tmp_path):
    co, _ = _find(code_objects(tmp_path), "es_xcorr32_kernel")
    md = kernel_metadata(co)
    for prefix, (spills, private) in FUSED.items():
        (name,) = [k for k in md if k.startswith(prefix)]
        m = md[name]
        assert m["vgpr_count"] <= 168, (name, m)
        assert m["vgpr_spill_count"] <= spills, (name, m)
        assert m["private_segment_fixed_size"] <= private, (name, m)
