"""Register / scratch budget of k3_tilex_all, read from the gfx950 code object inside the built library (no GPU), as
tests/test_kernel_resources.py does for the other hot kernels."""
import os
import shutil

import pytest

from test_kernel_resources import LIB, kr

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")) and shutil.which("c++filt")),
                                reason="needs the built library and ROCm's llvm tools")

# every shipped instantiation -> VGPR cap of the waves per SIMD it is built for (last template argument; two: 256, three: 168)
CAPS = {
    "rbc3::k3_tilex_all<32, 16, 16, 2>": 256,
    "rbc3::k3_tilex_all<32, 8, 16, 2>": 256,
    "rbc3f::k3_tilex_all<32, 16, 16, 2>": 256,
    "rbc3f::k3_tilex_all<32, 8, 16, 3>": 168,
}


@pytest.mark.parametrize("kernel", sorted(CAPS))
def test_tilex_register_and_scratch_budget(kernel):
    table = kr.kernel_resources(LIB)
    assert kernel in table, sorted(k for k in table if "tilex" in k)
    r = table[kernel]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["agpr_count"] == 0, (kernel, r)
    assert r["vgpr_count"] <= CAPS[kernel], (kernel, r)
