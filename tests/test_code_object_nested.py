"""Register budget of the camera rays' nested list-mode closest hit, read from the shipped
library's gfx950 code object (the AMDHSA metadata note: yocto_raytracing_amd/codeid.py
kernel_resources, as tests/test_code_object.py reads it).

k_primary_persist<unsigned, 0, true> calls packet_first_list (packet_trace.h) by default. It has
to stay within 64 VGPRs (8 waves per SIMD), spill no VGPR and use no private memory, and its
SGPR spills must not exceed those of the flat walk it replaces: 24, the count in the parent
commit's code object (4deb0dd, the same compile flags) and tests/test_code_object.py's ceiling
for this kernel. The nested walk as first written spilled 28 and one VGPR; keeping one mask of
the lanes still walking instead of `live` and `done`, and no wave index across the walk, brought
it back to 24.
"""
import re

import pytest

from helpers import ROOT

LIB = ROOT / "yocto_raytracing_amd" / "libyrt.so"
KERNEL = r"k_primary_persistIjLi0ELb1EE"
PARENT_SGPR_SPILLS = 24


@pytest.fixture(scope="module")
def resources():
    if not LIB.exists():
        from yocto_raytracing_amd import build

        build.build_library()
    from yocto_raytracing_amd.codeid import kernel_resources

    return kernel_resources(LIB)


def test_nested_primary_register_budget(resources):
    hits = {k: v for k, v in resources.items() if re.search(KERNEL, k)}
    assert len(hits) == 1, sorted(hits)
    (name, r), = hits.items()
    print(name, r)
    assert r["vgpr"] <= 64, r
    assert r["vgpr_spill"] == 0 and r["private"] == 0, r
    assert r["sgpr_spill"] <= PARENT_SGPR_SPILLS, r
