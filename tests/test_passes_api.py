"""The shading passes' interface without a GPU (yrt_render_passes, include/yrt.h): the enum, the
struct and the name table, argument checks that return before anything touches a device, the
Python wrapper's name check, the CLI's --passes usage errors and the new kernels' register
budgets from the shipped library's gfx950 code object."""
import ctypes as C
import re
import subprocess

import pytest

from helpers import ROOT, scene_path

LIB = ROOT / "yocto_raytracing_amd" / "libyrt.so"
CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
YRT_ERR_INVALID_ARG = 1


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    return y


def test_header_constants_equal_the_python_names():
    from yocto_raytracing_amd import _native as N

    header = (ROOT / "include" / "yrt.h").read_text()
    assert int(re.search(r"\bYRT_ERR_INVALID_ARG = (\d+)", header).group(1)) == YRT_ERR_INVALID_ARG
    consts = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bYRT_PASS_([A-Z]+) = (\d+)", header)}
    assert consts.pop("count") == N.YRT_PASS_COUNT == len(N.PASSES) == 5
    assert consts == N.PASSES == {"direct": 0, "diffuse": 1, "specular": 2, "reflection": 3, "ambient": 4}
    assert C.sizeof(N.PassPlanes) == N.YRT_PASS_COUNT * C.sizeof(C.c_void_p)
    assert N.PassPlanes.plane.offset == 0
    assert "yrt_render_passes" in N.EXPORTS
    # the AOV interface beside it is what it was
    assert N.YRT_AOV_COUNT == 6 and C.sizeof(N.AovPlanes) == 6 * C.sizeof(C.c_void_p)


def test_bad_masks_and_null_planes_are_refused_before_any_device_call(yrt):
    from yocto_raytracing_amd import _native as N

    p = yrt.render_params(resolution=8)
    handle = C.cast(C.create_string_buffer(256), C.c_void_p)  # never looked at: the checks come first
    pixels = (C.c_float * (4 * 64))()
    full = N.PassPlanes()
    for k in range(N.YRT_PASS_COUNT):
        full.plane[k] = C.addressof(pixels)

    def call(h, params, mask, planes):
        return N.lib.yrt_render_passes(h, params, mask, planes, None, N.YRT_MEM_HOST, None)

    assert call(None, C.byref(p), 1, C.byref(full)) == YRT_ERR_INVALID_ARG
    assert call(handle, None, 1, C.byref(full)) == YRT_ERR_INVALID_ARG
    assert call(handle, C.byref(p), 1, None) == YRT_ERR_INVALID_ARG
    assert call(handle, C.byref(p), 0, C.byref(full)) == YRT_ERR_INVALID_ARG
    for mask in (1 << 5, 1 << 5 | 1, 1 << 31, 0xFFFFFFFF):
        assert call(handle, C.byref(p), mask, C.byref(full)) == YRT_ERR_INVALID_ARG, hex(mask)
    for k in range(N.YRT_PASS_COUNT):  # pass k requested, its plane null
        planes = N.PassPlanes()
        for q in range(N.YRT_PASS_COUNT):
            planes.plane[q] = C.addressof(pixels) if q != k else None
        assert call(handle, C.byref(p), 0x1F, C.byref(planes)) == YRT_ERR_INVALID_ARG, k
        assert call(handle, C.byref(p), 1 << k, C.byref(planes)) == YRT_ERR_INVALID_ARG, k
    assert b"pass" in N.lib.yrt_last_error()


def test_unknown_pass_name_raises_before_any_native_call(yrt):
    scn = yrt.load_scene(str(scene_path("simple")))  # no BVH, no upload: neither is reached
    with pytest.raises(ValueError, match="nope"):
        yrt.render_passes(scn, 0.1, 8, 1, passes=("diffuse", "nope"))
    with pytest.raises(ValueError):
        yrt.render_passes(scn, 0.1, 8, 1, passes=())
    with pytest.raises(ValueError, match="beauty"):  # the beauty is the `beauty` flag, not a pass
        yrt.render_passes(scn, 0.1, 8, 1, passes=("beauty",))
    with pytest.raises(ValueError, match="devices"):
        yrt.render_passes(scn, 0.1, 8, 1, devices=(0, 0))


def test_cli_passes_usage_errors():
    def run(*args):
        return subprocess.run([str(CLI), *args], capture_output=True, text=True, timeout=60)

    r = run("--passes", "nope", str(scene_path("simple")))
    assert r.returncode == 1 and "unknown --passes nope" in r.stderr and "loading scene" not in r.stdout
    r = run("--passes", "diffuse,", str(scene_path("simple")))
    assert r.returncode == 1 and "unknown --passes" in r.stderr
    r = run("--passes", "diffuse", "--gpus", "2", str(scene_path("simple")))
    assert r.returncode == 1 and "--passes" in r.stderr and "loading scene" not in r.stdout
    r = run("--passes", "diffuse", "--algorithm", "megakernel", str(scene_path("simple")))
    assert r.returncode == 1 and "--passes" in r.stderr and "loading scene" not in r.stdout
    r = run("--passes")
    assert r.returncode == 1 and "missing value" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "--passes" in r.stderr


def test_pass_kernels_code_object_budget():
    """the four k_shade_passes (fused or not, at most four lights or more) and the one
    k_accumulate_passes keep everything in registers; the fused ones' LDS lets eight blocks
    share a CU's 160 KiB, more than their six waves per SIMD ask for"""
    from yocto_raytracing_amd.codeid import kernel_resources

    res = kernel_resources(LIB)
    shade = {k: v for k, v in res.items() if "k_shade_passes" in k}
    acc = {k: v for k, v in res.items() if "k_accumulate_passes" in k}
    assert len(shade) == 4 and len(acc) == 1, sorted(shade) + sorted(acc)
    for name, r in {**shade, **acc}.items():
        print(f"{name[:64]}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs ({r['sgpr_spill']} spilled to VGPR lanes), "
              f"{r['lds']} B LDS, block {r['block']}")
        assert r["vgpr_spill"] == 0 and r["private"] == 0, (name, r)
    fused = [r for k, r in shade.items() if "k_shade_passesILb1E" in k]
    assert len(fused) == 2
    for r in fused:
        assert 8 * r["lds"] <= 160 * 1024, r
        assert r["vgpr"] <= 80, r  # six waves of 256 threads per SIMD: 512 / 6 rounded down to 8
