"""The built library's code objects for lists of 257..1024 paths (es_scl_wide_large.hip): the four instantiations of the lane-per-path
list decoder at 512 and 1024 lanes per block (the reference's code and run-time K) exist, and their register counts fit the
residency their launch bounds promise -- two waves per SIMD at 512 lanes (one block per CU: its LDS), four at 1024 (a block of 16
waves is four per SIMD, so at most 128 VGPRs: the 1024-lane kernel spills to scratch, which this size accepts)."""
import pytest

from code_objects import LIB, code_objects, kernel_metadata

KERNELS = {
    "_ZN12_GLOBAL__N_118es_scl_wide_kernelILi512ELi512ELb0EEEvNS_8WideArgsE": 256,
    "_ZN12_GLOBAL__N_118es_scl_wide_kernelILi512ELi512ELb1EEEvNS_8WideArgsE": 256,
    "_ZN12_GLOBAL__N_118es_scl_wide_kernelILi1024ELi1024ELb0EEEvNS_8WideArgsE": 128,
    "_ZN12_GLOBAL__N_118es_scl_wide_kernelILi1024ELi1024ELb1EEEvNS_8WideArgsE": 128,
}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    md = {}
    for co in code_objects(tmp_path_factory.mktemp("co")):
        md.update(kernel_metadata(co))
    return md


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_large_list_instantiation_fits_its_residency(metadata, name):
    assert name in metadata, f"{name} not found in {LIB}"
    assert metadata[name]["vgpr_count"] <= KERNELS[name], metadata[name]
