"""The register budget of k_shadow_shade_persist (level 0's shadow rays and shading in one
persistent grid), read from the shipped library's gfx950 code object like
tests/test_code_object.py reads the other timed kernels'.

It ships at the any-hit grid's 8 waves per SIMD: at most 64 VGPRs, none spilled, no scratch.
Its epilogue is k_shade's body, which alone needs 65: a spill there is a scratch round trip per
item on every wave of the frame.

The view point reaches the kernel as three scalars of their own: as part of the four-dword
kernel-argument load that brings it in, live across the whole kernel, it left an unused
16-byte spill slot behind, and with it 32 private bytes per lane.
"""
import re

import pytest

from helpers import ROOT

LIB = ROOT / "yocto_raytracing_amd" / "libyrt.so"
FUSED = r"k_shadow_shade_persist"
# the shipped build's SGPR spills (to VGPR lanes), ratcheted like the ceilings of
# tests/test_code_object.py (k_shadow_persist<0> has 32), DESIGN.md section 5
SGPR_SPILLS = 40


@pytest.fixture(scope="module")
def resources():
    if not LIB.exists():
        from yocto_raytracing_amd import build

        build.build_library()
    from yocto_raytracing_amd.codeid import kernel_resources

    return kernel_resources(LIB)


def test_fused_kernel_register_budget(resources):
    hits = {k: v for k, v in resources.items() if re.search(FUSED, k)}
    assert len(hits) == 1, sorted(hits)
    (name, r), = hits.items()
    print(name, r)
    assert r["vgpr_spill"] == 0 and r["private"] == 0, r
    assert r["vgpr"] <= 64 and r["sgpr"] <= 80, r  # 8 waves per SIMD
    assert r["block"] == 1024, r                   # two blocks per CU
    assert r["lds"] <= 80 * 1024, r                # ... which share its 160 KiB of LDS
    assert r["sgpr_spill"] <= SGPR_SPILLS, r


def test_two_kernel_path_is_still_there(resources):
    """every case the fused kernel does not take runs these"""
    for pat in (r"k_shadow_persistILi0EE", r"k_shadeILb0ELb1ELi256ELb1EE", r"k_shadeILb0ELb1ELi256ELb0EE"):
        assert len([k for k in resources if re.search(pat, k)]) == 1, pat
