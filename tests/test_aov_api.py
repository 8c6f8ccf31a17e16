"""The AOV pass's interface without a GPU (yrt_render_aovs, include/yrt.h): argument checks
that return before any device call, the Python names, the CLI's --aov usage errors and the
k_aov kernel's register budget from the shipped library's gfx950 code object."""
import ctypes as C
import re
import subprocess

import pytest

from helpers import ROOT, scene_path

LIB = ROOT / "yocto_raytracing_amd" / "libyrt.so"
CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    return y


def test_null_arguments_are_status_codes(yrt):
    from yocto_raytracing_amd import _native as N

    p = yrt.render_params(resolution=8)
    planes = N.AovPlanes()
    assert N.lib.yrt_render_aovs(None, C.byref(p), 1, C.byref(planes), N.YRT_MEM_HOST, None) == 1
    # a null planes pointer is refused before the handle is looked at: any non-null one does
    handle = C.create_string_buffer(256)
    assert N.lib.yrt_render_aovs(C.cast(handle, C.c_void_p), C.byref(p), 1, None, N.YRT_MEM_HOST, None) == 1
    assert N.lib.yrt_render_aovs(C.cast(handle, C.c_void_p), None, 1, C.byref(planes), N.YRT_MEM_HOST, None) == 1


def test_unknown_aov_name_raises_before_any_native_call(yrt):
    scn = yrt.load_scene(str(scene_path("simple")))  # no BVH, no upload: neither is reached
    with pytest.raises(ValueError, match="nope"):
        yrt.render_aovs(scn, 8, 1, aovs=("nope",))
    with pytest.raises(ValueError):
        yrt.render_aovs(scn, 8, 1, aovs=())


def test_header_constants_equal_the_python_names():
    from yocto_raytracing_amd import _native as N

    header = (ROOT / "include" / "yrt.h").read_text()
    consts = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bYRT_AOV_([A-Z]+) = (\d+)", header)}
    assert consts.pop("count") == N.YRT_AOV_COUNT == len(N.AOVS)
    assert consts == N.AOVS
    assert sorted(N.AOVS.values()) == list(range(N.YRT_AOV_COUNT))
    assert C.sizeof(N.AovPlanes) == N.YRT_AOV_COUNT * C.sizeof(C.c_void_p)


def test_cli_aov_usage_errors():
    def run(*args):
        return subprocess.run([str(CLI), *args], capture_output=True, text=True, timeout=60)

    r = run("--aov", "nope", str(scene_path("simple")))
    assert r.returncode == 1 and "unknown --aov nope" in r.stderr and "loading scene" not in r.stdout
    r = run("--aov", "depth,", str(scene_path("simple")))
    assert r.returncode == 1 and "unknown --aov" in r.stderr
    r = run("--aov", "depth", "--gpus", "2", str(scene_path("simple")))
    assert r.returncode == 1 and "--aov" in r.stderr and "loading scene" not in r.stdout
    r = run("--aov")
    assert r.returncode == 1 and "missing value" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "--aov" in r.stderr


def test_k_aov_code_object_budget():
    """one k_aov in the library, and no scratch: its per-pixel sums and the walk fit the
    registers (a spill would put vector-memory round trips into the sample loop)"""
    from yocto_raytracing_amd.codeid import kernel_resources

    hits = {k: v for k, v in kernel_resources(LIB).items() if re.search(r"k_aov", k)}
    assert len(hits) == 1, sorted(hits)
    (name, r), = hits.items()
    print(f"k_aov: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs ({r['sgpr_spill']} spilled to VGPR lanes), "
          f"{r['lds']} B LDS, block {r['block']}")
    assert r["vgpr_spill"] == 0, r
    assert r["private"] == 0, r
