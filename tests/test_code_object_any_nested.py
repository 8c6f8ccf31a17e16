"""Register budgets of the persistent any-hit grids with the nested walk, read from the shipped
library's gfx950 code object (the AMDHSA metadata note: yocto_raytracing_amd/codeid.py
kernel_resources, as tests/test_code_object.py reads it).

k_shadow_shade_persist and k_shadow_persist<0> call packet_occluded_nested (packet_trace.h) by
default. The fused kernel ships at 8 waves per SIMD with blocks of 1024: at most 64 VGPRs and 80
SGPRs, no VGPR spilled, no private memory, at most 80 KiB of LDS, and no more SGPR spills than
with the flat walk it replaces -- 40, the count in the parent commit's code object (88b99d5, the
same compile flags) and tests/test_code_object_fused.py's ceiling. k_shadow_persist<0> spills no
VGPR, uses no private memory, and its SGPR spills are ratcheted from the flat walk's 32
(tests/test_code_object.py's ceiling) down to the nested walk's 29. The walk as first written
had 52 and 35 and a spilled VGPR in the fused kernel's shading; DESIGN.md section 5 lists what
brought it back.
"""
import re

import pytest

from helpers import ROOT

LIB = ROOT / "yocto_raytracing_amd" / "libyrt.so"
FUSED = r"k_shadow_shade_persist"
PERSIST = r"k_shadow_persistILi0EE"
FUSED_SGPR_SPILLS = 40    # the parent's count, and the shipped build's
PERSIST_SGPR_SPILLS = 29  # the shipped build's (the parent: 32)


@pytest.fixture(scope="module")
def resources():
    if not LIB.exists():
        from yocto_raytracing_amd import build

        build.build_library()
    from yocto_raytracing_amd.codeid import kernel_resources

    return kernel_resources(LIB)


def _one(resources, pattern):
    hits = {k: v for k, v in resources.items() if re.search(pattern, k)}
    assert len(hits) == 1, sorted(hits)
    (name, r), = hits.items()
    print(name, r)
    return r


def test_fused_any_hit_register_budget(resources):
    r = _one(resources, FUSED)
    assert r["vgpr"] <= 64 and r["sgpr"] <= 80, r
    assert r["vgpr_spill"] == 0 and r["private"] == 0, r
    assert r["lds"] <= 80 * 1024, r
    assert r["block"] == 1024, r
    assert r["sgpr_spill"] <= FUSED_SGPR_SPILLS, r


def test_persistent_any_hit_register_budget(resources):
    r = _one(resources, PERSIST)
    assert r["vgpr_spill"] == 0 and r["private"] == 0, r
    assert r["sgpr_spill"] <= PERSIST_SGPR_SPILLS, r
