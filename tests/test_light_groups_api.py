"""The light groups' interface without a GPU (yrt_render_light_groups, include/yrt.h): the
constant, the struct and the exports, Scene.lights(), argument checks that return before anything
touches a device, the Python wrapper's checks, the CLI's --light-groups usage errors and the new
kernels' register budgets from the shipped library's gfx950 code object."""
import ctypes as C
import re
import subprocess

import pytest

import light_groups_scene as LS
import passes_scene as PS
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
    assert int(re.search(r"#define YRT_LIGHT_GROUPS_MAX (\d+)", header).group(1)) == N.YRT_LIGHT_GROUPS_MAX == 8
    assert int(re.search(r"#define YRT_ABI_VERSION (\d+)", header).group(1)) == N.lib.yrt_abi_version() == 1
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(N.LightGroupPlanes) == (N.YRT_LIGHT_GROUPS_MAX + 2) * vp
    assert N.LightGroupPlanes.group.offset == 0
    assert N.LightGroupPlanes.ambient.offset == N.YRT_LIGHT_GROUPS_MAX * vp
    assert N.LightGroupPlanes.beauty.offset == (N.YRT_LIGHT_GROUPS_MAX + 1) * vp
    assert "yrt_render_light_groups" in N.EXPORTS and "yrt_host_scene_lights" in N.EXPORTS
    # the passes' interface beside it is what it was
    assert N.YRT_PASS_COUNT == 5 and C.sizeof(N.PassPlanes) == 5 * vp


def test_scene_lights_are_the_emitters_in_instance_order(yrt):
    from yocto_raytracing_amd import _native as N

    five = LS.build(yrt)
    assert five.lights() == LS.LIGHTS == [7, 8, 10, 11, 12]
    assert five.info()["lights"] == 5
    assert PS.build(yrt).lights() == [7, 8]
    assert LS.build(yrt, more_lights=False).lights() == [7, 8]
    assert LS.build(yrt, lit=(0, 2)).lights() == [7, 10]  # a variant: the others are no lights
    assert LS.build(yrt, lit=()).lights() == []
    # the C call: a count alone, and a buffer shorter than the count
    n, two = C.c_int(), (C.c_int * 2)(-5, -5)
    assert N.lib.yrt_host_scene_lights(five.handle, None, 0, C.byref(n)) == 0 and n.value == 5
    assert N.lib.yrt_host_scene_lights(five.handle, two, 2, C.byref(n)) == 0 and n.value == 5 and list(two) == [7, 8]
    assert N.lib.yrt_host_scene_lights(None, None, 0, C.byref(n)) == YRT_ERR_INVALID_ARG
    assert N.lib.yrt_host_scene_lights(five.handle, None, 0, None) == YRT_ERR_INVALID_ARG


def test_bad_arguments_are_refused_before_any_device_call(yrt):
    from yocto_raytracing_amd import _native as N

    p = yrt.render_params(resolution=8)
    handle = C.cast(C.create_string_buffer(256), C.c_void_p)  # never looked at: the checks come first
    pixels = (C.c_float * (4 * 64))()
    full = N.LightGroupPlanes()
    for g in range(N.YRT_LIGHT_GROUPS_MAX):
        full.group[g] = C.addressof(pixels)
    full.ambient = full.beauty = C.addressof(pixels)

    def call(h, params, group_of, ngroups, planes, mem=N.YRT_MEM_HOST, nlights=None):
        arr = None if group_of is None else (C.c_int * max(len(group_of), 1))(*group_of)
        n = (0 if group_of is None else len(group_of)) if nlights is None else nlights
        return N.lib.yrt_render_light_groups(h, params, arr, n, ngroups, planes, mem, None)

    ok = LS.GROUP_OF
    assert call(None, C.byref(p), ok, 3, C.byref(full)) == YRT_ERR_INVALID_ARG
    assert call(handle, None, ok, 3, C.byref(full)) == YRT_ERR_INVALID_ARG
    assert call(handle, C.byref(p), None, 3, C.byref(full)) == YRT_ERR_INVALID_ARG
    assert call(handle, C.byref(p), ok, 3, None) == YRT_ERR_INVALID_ARG
    for ngroups in (0, -1, 9, 1 << 30):
        assert call(handle, C.byref(p), [0], ngroups, C.byref(full)) == YRT_ERR_INVALID_ARG, ngroups
    assert b"ngroups" in N.lib.yrt_last_error()
    for bad in ([0, 1, 3], [0, -2, 1], [3], [1 << 30]):  # an entry outside [-1, 3)
        assert call(handle, C.byref(p), bad, 3, C.byref(full)) == YRT_ERR_INVALID_ARG, bad
    assert b"group_of" in N.lib.yrt_last_error()
    assert call(handle, C.byref(p), ok, 3, C.byref(full), nlights=-1) == YRT_ERR_INVALID_ARG
    for k in range(3):  # group k's plane null; ambient and beauty may be null
        planes = N.LightGroupPlanes()
        for g in range(3):
            planes.group[g] = C.addressof(pixels) if g != k else None
        assert call(handle, C.byref(p), ok, 3, C.byref(planes)) == YRT_ERR_INVALID_ARG, k
    assert b"plane" in N.lib.yrt_last_error()
    for mem in (-1, 2, 77):
        assert call(handle, C.byref(p), ok, 3, C.byref(full), mem=mem) == YRT_ERR_INVALID_ARG, mem
    assert b"mem" in N.lib.yrt_last_error()
    # everything else in order: the count is compared with the scene's, which this handle has not
    assert call(handle, C.byref(p), ok, 3, C.byref(full)) == YRT_ERR_INVALID_ARG
    assert b"light count" in N.lib.yrt_last_error()


def test_bad_groups_raise_before_any_native_call(yrt):
    scn = yrt.load_scene(str(scene_path("simple")))  # no BVH, no upload: neither is reached
    n = len(scn.lights())
    assert n >= 1
    for bad in ([-2] * n, [8] * n, [0.5] * n, ["0"] * n, [True] * n):
        with pytest.raises(ValueError, match="light group"):
            yrt.render_light_groups(scn, 0.1, 8, 1, groups=bad)
    with pytest.raises(ValueError, match="lights"):
        yrt.render_light_groups(scn, 0.1, 8, 1, groups=[0] * (n + 1))
    with pytest.raises(ValueError, match="lights"):
        yrt.render_light_groups(scn, 0.1, 8, 1, groups=[])
    with pytest.raises(ValueError, match="devices"):
        yrt.render_light_groups(scn, 0.1, 8, 1, groups=[0] * n, devices=(0, 0))
    with pytest.raises(TypeError):
        yrt.render_light_groups(scn, 0.1, 8, 1)  # groups is required


def test_cli_light_groups_usage_errors(tmp_path):
    def run(*args):
        return subprocess.run([str(CLI), *args], capture_output=True, text=True, timeout=60)

    simple = str(scene_path("simple"))
    for bad in ("0,x", "0,", "", "0,8", "-2", "1.5"):
        r = run("--light-groups", bad, simple)
        assert r.returncode == 1 and "--light-groups" in r.stderr and "loading scene" not in r.stdout, bad
    r = run("--light-groups", "0,8", simple)
    assert "out of range" in r.stderr
    r = run("--light-groups", "0", "--gpus", "2", simple)
    assert r.returncode == 1 and "--light-groups" in r.stderr and "loading scene" not in r.stdout
    r = run("--light-groups", "0", "--algorithm", "megakernel", simple)
    assert r.returncode == 1 and "--light-groups" in r.stderr and "loading scene" not in r.stdout
    r = run("--light-groups")
    assert r.returncode == 1 and "missing value" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and "--light-groups" in r.stderr
    # a wrong count: known once the scene is loaded, before anything is built or uploaded
    import yocto_raytracing_amd as yrt

    five = tmp_path / "five.yrtscene"
    LS.build(yrt).save(str(five))
    for wrong in ("0,1,0,-1", "0,1,0,-1,2,2"):
        r = run("--light-groups", wrong, "-o", str(tmp_path / "out.hdr"), str(five))
        assert r.returncode == 1 and "the scene has 5" in r.stderr and "creating bvh" not in r.stdout, wrong
    assert not list(tmp_path.glob("out*"))


def test_group_kernels_code_object_budget():
    """the four k_shade_groups (fused or not, at most four lights or more) and the one
    k_accumulate_groups keep every vector register in registers and have no private segment:
    one accumulator, group-major. The fused ones' LDS (ten planes of 3 x 257 floats and the sRGB
    table) lets five blocks share a CU's 160 KiB, the five waves per SIMD of their launch bound,
    whose 512 / 5 registers, rounded down to 8, are the ceiling of all four."""
    from yocto_raytracing_amd.codeid import kernel_resources

    res = kernel_resources(LIB)
    shade = {k: v for k, v in res.items() if "k_shade_groups" in k}
    acc = {k: v for k, v in res.items() if "k_accumulate_groups" in k}
    assert len(shade) == 4 and len(acc) == 1, sorted(shade) + sorted(acc)
    for name, r in {**shade, **acc}.items():
        print(f"{name[:64]}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs ({r['sgpr_spill']} spilled to VGPR lanes), "
              f"{r['lds']} B LDS, block {r['block']}")
        assert r["vgpr_spill"] == 0 and r["private"] == 0, (name, r)
        assert r["block"] == 256, (name, r)
    fused = [r for k, r in shade.items() if "k_shade_groupsILb1E" in k]
    assert len(fused) == 2
    for r in fused:
        assert r["lds"] >= 4 * (10 * 3 * 257 + 256), r
        assert 5 * r["lds"] <= 160 * 1024, r
    for r in shade.values():
        assert r["vgpr"] <= 96, r
