"""Build-only checks of the compile-time knobs that survive in the device code.

The product is built with every knob at its default (yocto_raytracing_amd/build.py).
The knobs that remain are tunables with a measured default (register budgets,
block sizes, XCD run lengths, the persistent-grid threshold), the kept variants
that the suite runs as libraries of their own (tools/build_variants.py) or that
the ledger refers to (LDS staging of the top 4-wide records, the north star's
"hot node tiles in LDS"; the fused bundle lists, whose kernel the default build
still instantiates), and the four diagnostic builds. No non-default setting is
compiled by the normal build, so each is compiled here for gfx950 (device code
only) to keep it from rotting. A knob added to the sources without an entry
below fails test_every_knob_is_listed. The switches whose A/B was settled in
rounds 4-6 and whose losing side nothing ran were removed with that side
(DESIGN.md §5); it is last present at commit f416f4b.
"""
import concurrent.futures as cf
import os
import re
import subprocess

import pytest

from helpers import ROOT

CSRC = ROOT / "yocto_raytracing_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# knob -> the non-default defines compiled here
VARIANTS = {
    "YRT_SHADOW_LDS_RECORDS": ["-DYRT_SHADOW_LDS_RECORDS=341"],
    "YRT_DEBUG_BOUNDS": ["-DYRT_DEBUG_BOUNDS"],
    "YRT_WIDE_STATS": ["-DYRT_WIDE_STATS"],
    "YRT_LIST_TIMING": ["-DYRT_LIST_TIMING"],
    "YRT_TAIL_STATS": ["-DYRT_TAIL_STATS"],
    "YRT_SHARED_TAIL": ["-DYRT_SHARED_TAIL=0"],
    "YRT_TRACE_WAVES": ["-DYRT_TRACE_WAVES=7"],
    "YRT_SHADOW_WAVES": ["-DYRT_SHADOW_WAVES=6"],
    "YRT_SHADE_WAVES": ["-DYRT_SHADE_WAVES=5"],
    "YRT_CAMERA_LIST_MAX": ["-DYRT_CAMERA_LIST_MAX=12", "-DYRT_CAMERA_CUT_DEPTH=3"],
    "YRT_BUNDLE_ITEMS": ["-DYRT_BUNDLE_ITEMS=16", "-DYRT_BUNDLE_MIN_TOP=0"],
    "YRT_SHADE_LEVEL_WAVES": ["-DYRT_SHADE_LEVEL_WAVES=7"],
    "YRT_PRIMARY_LDS_RECORDS": ["-DYRT_PRIMARY_LDS_RECORDS=1023"],
    "YRT_PRIMARY_WAVES": ["-DYRT_PRIMARY_WAVES=6", "-DYRT_PRIMARY_SP_BLOCK=768"],
    "YRT_LISTS_MIN_SPP": ["-DYRT_LISTS_MIN_SPP=1"],
    # round 6: the camera lists' top cut and the fused bundle lists
    "YRT_CAMERA_CUT_DEPTH": ["-DYRT_CAMERA_CUT_DEPTH=0"],
    "YRT_BUNDLE_FUSED": ["-DYRT_BUNDLE_FUSED=1"],
    # the closest hit's stack with lane masks (the round-5 form; off: inner_pop_avail)
    "YRT_STACK_MASKS": ["-DYRT_STACK_MASKS=1"],
    # the compiled descent loop instead of descent_asm.h's
    "YRT_DESCENT_ASM": ["-DYRT_DESCENT_ASM=0"],
    "YRT_WIDE_ASM": ["-DYRT_WIDE_ASM=0"],
    # the any-hit grid's items as (block, light) pairs (the round-5 form; on: every light per item)
    "YRT_SHADOW_ITEM_LIGHTS": ["-DYRT_SHADOW_ITEM_LIGHTS=0", "-DYRT_SHADOW_ITEM_RUN=8"],
    "YRT_LEVEL_SEGMENTS": ["-DYRT_LEVEL_SEGMENTS=32"],
    # run()'s samples per chunk (host constants; tests/test_gpu_variants.py runs small frames as
    # several chunks with them)
    "YRT_CHUNK_LOG2": ["-DYRT_CHUNK_LOG2=11", "-DYRT_MIRROR_CHUNK_LOG2=11"],
    "YRT_PRIMARY_BLOCK": ["-DYRT_PRIMARY_BLOCK=256", "-DYRT_SHADOW_BLOCK=256", "-DYRT_SHADOW_BLOCK_CHUNK=64",
                          "-DYRT_SHADOW_LIGHT_MINOR=16", "-DYRT_XCD_CHUNK_PRIMARY=64",
                          "-DYRT_SHADOW_PERSIST_MIN_ITEMS=0", "-DYRT_PRIMARY_PERSIST_MIN_ITEMS=1000000",
                          "-DYRT_PRIMARY_BLOCK_CHUNK=64"],
}
# knobs covered by another entry's defines
COVERED = {"YRT_SHADOW_ITEM_RUN", "YRT_BUNDLE_MIN_TOP", "YRT_PRIMARY_SP_BLOCK", "YRT_SHADOW_BLOCK", "YRT_SHADOW_BLOCK_CHUNK", "YRT_SHADOW_LIGHT_MINOR", "YRT_XCD_CHUNK_PRIMARY",
           "YRT_SHADOW_PERSIST_MIN_ITEMS", "YRT_PRIMARY_PERSIST_MIN_ITEMS", "YRT_PRIMARY_BLOCK_CHUNK",
           "YRT_MIRROR_CHUNK_LOG2"}


def _knobs_in_sources():
    found = set()
    for p in list(CSRC.glob("*.h")) + list(CSRC.glob("*.hip")) + list(CSRC.glob("*.cpp")):
        found |= set(re.findall(r"#\s*if(?:n?def)?\s+(YRT_[A-Z0-9_]+)", p.read_text()))
    return found


def test_every_knob_is_listed():
    knobs = _knobs_in_sources()
    assert knobs, "no knobs found"
    missing = knobs - set(VARIANTS) - COVERED
    assert not missing, f"knobs without a build-only variant: {sorted(missing)}"
    stale = (set(VARIANTS) | COVERED) - knobs
    assert not stale, f"listed knobs no longer in the sources: {sorted(stale)}"


def _compile(defs):
    cmd = [HIPCC, "-O3", "-std=c++17", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-mllvm",
           "-structurizecfg-skip-uniform-regions=true", "-fno-slp-vectorize", "--offload-arch=gfx950",
           "--offload-device-only", "-c", str(CSRC / "wavefront.hip"), "-o", os.devnull, *defs]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return defs, r.returncode, r.stderr[-3000:]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_non_default_knobs_compile():
    with cf.ThreadPoolExecutor(max_workers=min(len(VARIANTS), max(1, (os.cpu_count() or 2) - 1))) as ex:
        results = list(ex.map(_compile, VARIANTS.values()))
    failed = [(d, err) for d, rc, err in results if rc != 0]
    assert not failed, "\n".join(f"{d}:\n{err}" for d, err in failed)
