"""Build variants of libyrt.so that differ only in compile-time defines, for in-process A/B
timing (tools/ab_variants.py) and for the tests that run the kept variants
(tests/test_gpu_variants.py, through tests/variant_worker.py with YRT_LIB set).

    python tools/build_variants.py w7:-DYRT_TRACE_WAVES=7 lds85:-DYRT_SHADOW_LDS_RECORDS=85
    python tools/build_variants.py --tests          # the suite's variants (TEST_VARIANTS)

writes yocto_raytracing_amd/variants/libyrt_<name>.so (git-ignored, travels to the GPU box).
A library whose commands (defines included), sources and headers are the ones it was built
from is left alone, and so is every such object of a library that is rebuilt.
"""
from __future__ import annotations

import concurrent.futures as cf
import hashlib
import importlib.util
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "yocto_raytracing_amd"


def _build_module():
    # build.py by path: no import of the package (which binds a library) and no sys.path entry,
    # so the tests can load this tool into their own process
    spec = importlib.util.spec_from_file_location("yrt_build", PKG / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


b = _build_module()

OUT_DIR = PKG / "variants"
MAX_WORKERS = 16

# the variants the suite runs (name -> defines): the compiled descent loops instead of the
# generated assembly, the closest hit's stack with lane masks, the any-hit grid's items as
# (block, light) pairs, frames of a few tiles split into several chunks, and level 0's shadow
# rays and shading as two kernels where the default build fuses them, the nested walks'
# triangle leaves as compiled loops instead of the generated leaf scans (leaf_asm.h), the
# persistent any-hit grids' walk as the flat loop (packet_occluded_wide2) instead of the nested
# one, and the camera rays' list-mode closest hit as the flat loop (packet_first) instead of the
# nested one
TEST_VARIANTS = {
    "compiled": ["-DYRT_DESCENT_ASM=0", "-DYRT_WIDE_ASM=0"],
    "masks": ["-DYRT_STACK_MASKS=1"],
    "itemlights": ["-DYRT_SHADOW_ITEM_LIGHTS=0", "-DYRT_SHADOW_ITEM_RUN=8"],
    "chunks": ["-DYRT_CHUNK_LOG2=11", "-DYRT_MIRROR_CHUNK_LOG2=11"],
    "unfused": ["-DYRT_SHADOW_SHADE_FUSE=0"],
    "cleaf": ["-DYRT_LEAF_ASM=0"],
    "flatany":["-DYRT_ANY_NESTED=0"],
    "flatwalk": ["-DYRT_FIRST_NESTED=0"],
}


# knobs kept for A/B against the default (tools/ab_variants.py) that the suite compares with it
# on a few frames of their own instead of running all of tests/test_gpu_variants.py's cases:
# the item paths' emulated divisions and per-item range checks, and the fused grid's shading
# computing each light's direction and distance again (tests/test_gpu_item_geometry_variants.py)
KNOB_VARIANTS = {
    "itemdiv": ["-DYRT_ITEM_MAGIC=0"],
    "nocarry": ["-DYRT_LIGHT_CARRY=0"],
}


def library_path(name: str) -> Path:
    return OUT_DIR / f"libyrt_{name}.so"


def test_specs() -> list:
    """every library the suite loads: TEST_VARIANTS first, in their order, then KNOB_VARIANTS"""
    return [f"{name}:{','.join(defs)}" for name, defs in (*TEST_VARIANTS.items(), *KNOB_VARIANTS.items())]


def _sources_digest() -> str:
    """sha256 over every source and header a variant is compiled from. The library's stamp
    keeps it, so a library that travelled without its objects (or lost its timestamps on the
    way) is still recognised as built from this tree"""
    h = hashlib.sha256()
    deps = [b.CSRC / s for s in b.SOURCES] + [b.CSRC / i for inc in b.INCLUDED.values() for i in inc] + b._headers()
    for p in sorted(set(deps)):
        h.update(p.name.encode() + b"\0" + hashlib.sha256(p.read_bytes()).digest())
    return h.hexdigest()


def _plan(spec: str):
    name, _, defs = spec.partition(":")
    if not name or "/" in name:
        raise ValueError(f"bad variant spec {spec!r}: NAME:-Dflag,...")
    defines = [d for d in defs.split(",") if d]
    vdir = OUT_DIR / name
    objs = []
    for src in b.SOURCES:  # host and device code both see the defines
        o = vdir / (Path(src).stem + ".o")
        if src.endswith(".hip"):
            cmd = [b.HIPCC, *b.COMMON, *b.DEVICE_FLAGS, *defines, f"--offload-arch={b.ARCH}", "-c", str(b.CSRC / src), "-o", str(o)]
        else:
            cmd = [b.CLANGXX, *b.COMMON, *b.HOST_DEFS, *defines, "-c", str(b.CSRC / src), "-o", str(o)]
        objs.append((src, o, cmd))
    lib = library_path(name)
    link = [b.HIPCC, "-shared", "-fPIC", f"--offload-arch={b.ARCH}", "-o", str(lib), *(str(o) for _, o, _ in objs), *b.LINK_LIBS]
    return lib, vdir, objs, link


def main(argv, default_library: bool = True, verbose: bool = True) -> list:
    """build the variants named by `argv` (NAME:-Dflag,... specs; --tests: TEST_VARIANTS) and
    return their paths; default_library: build libyrt.so itself first, as the A/B tools expect"""
    specs = []
    for a in argv:
        specs += test_specs() if a == "--tests" else [a]
    if default_library:
        b.build_library()
    OUT_DIR.mkdir(exist_ok=True)
    digest = _sources_digest()
    hdrs = b._headers()
    jobs, links, libs = [], [], []
    for spec in specs:
        lib, vdir, objs, link = _plan(spec)
        libs.append(lib)
        # the library's stamp: every command that made it (paths relative to the tree, which
        # may have moved since) and the digest of what they read
        stamp = [*(" ".join(map(str, cmd)) for _, _, cmd in objs), " ".join(map(str, link)), digest]
        stamp = [s.replace(str(ROOT), ".") for s in stamp]
        if not b._stale(lib, [], stamp):
            continue
        vdir.mkdir(exist_ok=True)
        for src, o, cmd in objs:
            if b._stale(o, [b.CSRC / src, *hdrs, *(b.CSRC / i for i in b.INCLUDED.get(src, []))], cmd):
                jobs.append((o, cmd))
        links.append((lib, link, stamp))

    def run(job):
        o, cmd = job
        b._run(cmd)
        b._stamp(o, cmd)

    # the longest compiles first (wavefront.hip, then the other device sources)
    jobs.sort(key=lambda j: (not j[1][-3].endswith("wavefront.hip"), not j[1][-3].endswith(".hip")))
    workers = max(1, min(MAX_WORKERS, os.cpu_count() or 1, len(jobs) or 1))
    with cf.ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(run, jobs))
    for lib, link, stamp in links:
        b._run(link)
        b._stamp(lib, stamp)
    if verbose:
        for lib in libs:
            print(lib)
    return libs


if __name__ == "__main__":
    main(sys.argv[1:])
