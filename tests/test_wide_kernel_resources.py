"""The built library's code-object metadata for the headline list decoder (es_scl_wide_kernel<64, 8, false>, lists of 8 in one-wave
blocks): the register budget it was compiled for, and a ceiling on its VGPR spills.  The spills it has sit outside the f loops (frame
draw, the per-bit decision); a new one is a change to look at in the ISA, because a spill inside an f loop costs scratch traffic per
evaluation."""
from code_objects import LIB, code_objects, kernel_metadata

HEADLINE = "_ZN12_GLOBAL__N_118es_scl_wide_kernelILi64ELi8ELb0EEEvNS_8WideArgsE"


def _kernel_metadata(tmp_path):
    for co in code_objects(tmp_path):
        md = kernel_metadata(co)
        if HEADLINE in md:
            return md[HEADLINE]
    raise AssertionError(f"{HEADLINE} not found in {LIB}")


def test_headline_list_decoder_budget_and_spills(tmp_path):
    md = _kernel_metadata(tmp_path)
    assert md["vgpr_count"] <= 168, md              # __launch_bounds__(64, 3): three waves per SIMD
    assert md["vgpr_spill_count"] <= 16, md
