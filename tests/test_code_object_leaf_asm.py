"""Register figures of the three kernels whose triangle leaves are leaf_asm.h's scans, read from
the shipped library's gfx950 code object (yocto_raytracing_amd/codeid.py kernel_resources, as
tests/test_code_object.py reads it), pinned as ceilings at the shipped values.

The scans name s16-s29 and take their operands outside that range, so what lives only inside a
leaf can no longer sit there; as first written they cost k_primary_persist's list mode three SGPR
spills and the fused any-hit kernel one (DESIGN.md section 5 says what brought them back). None of
the figures may exceed the ceilings the kernels had before (tests/test_code_object_nested.py,
tests/test_code_object_any_nested.py, tests/test_code_object_fused.py).
"""
import re

import pytest

from helpers import ROOT

LIB = ROOT / "yocto_raytracing_amd" / "libyrt.so"
# kernel -> the shipped figures (ceilings); LDS in bytes
SHIPPED = {
    r"k_primary_persistIjLi0ELb1EE": {"vgpr": 64, "sgpr": 78, "sgpr_spill": 24, "lds": 13304},
    r"k_shadow_shade_persist": {"vgpr": 64, "sgpr": 78, "sgpr_spill": 40, "lds": 67288},
    r"k_shadow_persistILi0EE": {"vgpr": 61, "sgpr": 78, "sgpr_spill": 29, "lds": 312},
}
# the ceilings from before the scans
BEFORE = {
    r"k_primary_persistIjLi0ELb1EE": {"vgpr": 64, "sgpr_spill": 24},
    r"k_shadow_shade_persist": {"vgpr": 64, "sgpr": 80, "sgpr_spill": 40, "lds": 80 * 1024},
    r"k_shadow_persistILi0EE": {"sgpr_spill": 29},
}


@pytest.fixture(scope="module")
def resources():
    if not LIB.exists():
        from yocto_raytracing_amd import build

        build.build_library()
    from yocto_raytracing_amd.codeid import kernel_resources

    return kernel_resources(LIB)


def test_pinned_figures_are_within_the_earlier_ceilings():
    assert set(SHIPPED) == set(BEFORE)
    for k, before in BEFORE.items():
        for field, v in before.items():
            assert SHIPPED[k][field] <= v, (k, field)


@pytest.mark.parametrize("kernel", list(SHIPPED))
def test_leaf_scan_kernel_register_figures(resources, kernel):
    hits = {k: v for k, v in resources.items() if re.search(kernel, k)}
    assert len(hits) == 1, sorted(hits)
    (name, r), = hits.items()
    print(name, r)
    assert r["vgpr_spill"] == 0 and r["private"] == 0, r
    assert r["block"] == 1024, r
    for field, v in SHIPPED[kernel].items():
        assert r[field] <= v, (field, r)
