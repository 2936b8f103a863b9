"""Register / scratch budget of k3p_yz_chunked from the built gfx950 code object (no GPU): 128 VGPRs, two workgroups per CU at 64 KB of LDS."""
import pytest

from test_kernel_resources import LIB, kr
from test_kernel_resources_tilex import pytestmark  # noqa: F401  (skipped without the built library and ROCm's llvm tools)


@pytest.mark.parametrize("kernel", ["rbc3::k3p_yz_chunked<4>", "rbc3f::k3p_yz_chunked<8>"])
def test_chunked_register_and_scratch_budget(kernel):
    r = kr.kernel_resources(LIB)[kernel]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["agpr_count"] == 0, (kernel, r)
    assert r["vgpr_count"] <= 128, (kernel, r)
