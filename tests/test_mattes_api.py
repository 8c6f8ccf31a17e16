"""The ID-matte pass's interface without a GPU (yrt_render_mattes, yrt_host_scene_instances,
include/yrt.h): Scene.instances(), argument checks that return before any device call, the
Python names against the header, render_mattes' ValueErrors, matte()'s arithmetic, the CLI's
--mattes usage errors and the k_matte kernels' code-object budget."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from helpers import ROOT, scene_path

LIB = ROOT / "yocto_raytracing_amd" / "libyrt.so"
CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    return y


def test_instances_of_a_created_scene_are_what_was_added(yrt):
    """five instances that share a shape and a material, as the built scene of test_gpu_aov.py"""
    s = yrt.Scene.create()
    assert s.instances() == []
    mats = [s.add_material(kd=(0.1 * k, 0.2, 0.3)) for k in range(1, 5)]
    tri = dict(pos=[[0, 0, 0], [1, 0, 0], [0, 1, 0]], triangles=[[0, 1, 2]])
    shapes = [s.add_shape(**tri) for _ in range(4)]
    eye = np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, np.float32)])
    added = [(shapes[0], mats[0]), (shapes[1], mats[1]), (shapes[2], mats[2]), (shapes[3], mats[3]),
             (shapes[1], mats[0])]
    for k, (shp, mat) in enumerate(added):
        assert s.add_instance(eye, shp, mat) == k
    assert s.instances() == added
    assert all(isinstance(v, int) for sm in s.instances() for v in sm)


def test_instances_of_instance1k_lie_within_the_scene_counts(yrt):
    from yocto_raytracing_amd import _native as N

    s = yrt.load_scene(str(scene_path("instance1k")))
    ins, info = s.instances(), s.info()
    assert info["instances"] == len(ins) >= 1000  # (the 1000 of its name and the room around them)
    assert all(0 <= shp < info["shapes"] and 0 <= mat < info["materials"] for shp, mat in ins)
    # the call shape of yrt_host_scene_lights: n is always set, the arrays may be NULL, cap bounds the writes
    n = C.c_int(-1)
    assert N.lib.yrt_host_scene_instances(s.handle, None, None, 0, C.byref(n)) == 0 and n.value == len(ins)
    shp = (C.c_int * 4)(*[-7] * 4)
    n = C.c_int(-1)
    assert N.lib.yrt_host_scene_instances(s.handle, shp, None, 3, C.byref(n)) == 0 and n.value == len(ins)
    assert list(shp) == [ins[0][0], ins[1][0], ins[2][0], -7]
    assert N.lib.yrt_host_scene_instances(None, None, None, 0, C.byref(n)) == 1
    assert N.lib.yrt_host_scene_instances(s.handle, None, None, 0, None) == 1
    assert N.lib.yrt_host_scene_instances(s.handle, shp, None, -1, C.byref(n)) == 1


def test_null_arguments_are_status_codes(yrt):
    from yocto_raytracing_amd import _native as N

    p = yrt.render_params(resolution=8)
    planes = N.MattePlanes()
    assert N.lib.yrt_render_mattes(None, C.byref(p), 1, 1, C.byref(planes), N.YRT_MEM_HOST, None) == 1
    # a null planes pointer is refused before the handle is looked at: any non-null one does
    handle = C.create_string_buffer(256)
    h = C.cast(handle, C.c_void_p)
    assert N.lib.yrt_render_mattes(h, C.byref(p), 1, 1, None, N.YRT_MEM_HOST, None) == 1
    assert N.lib.yrt_render_mattes(h, None, 1, 1, C.byref(planes), N.YRT_MEM_HOST, None) == 1
    assert N.lib.yrt_scene_matte_dropped(None, (C.c_ulonglong * 3)()) == 1
    assert N.lib.yrt_scene_matte_dropped(h, None) == 1


def test_header_constants_equal_the_python_names():
    from yocto_raytracing_amd import _native as N

    header = (ROOT / "include" / "yrt.h").read_text()
    consts = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\bYRT_MATTE_([A-Z_]+) = (\d+)", header)}
    assert consts.pop("key_count") == N.YRT_MATTE_KEY_COUNT == len(N.MATTE_KEYS) == 3
    assert consts == N.MATTE_KEYS == {"instance": 0, "material": 1, "shape": 2}
    assert int(re.search(r"#define YRT_MATTE_LAYERS_MAX (\d+)", header).group(1)) == N.YRT_MATTE_LAYERS_MAX == 2
    vp = C.sizeof(C.c_void_p)
    assert C.sizeof(N.MattePlanes) == 12 * vp
    assert N.MattePlanes.ids.offset == 0 and N.MattePlanes.coverage.offset == 6 * vp
    # ids[key][layer]: the layers of a key are neighbours
    mp = N.MattePlanes()
    mp.ids[2][1] = 0x1234
    assert C.cast(C.byref(mp), C.POINTER(C.c_void_p))[5] == 0x1234
    for name in ("yrt_render_mattes", "yrt_scene_matte_dropped", "yrt_host_scene_instances"):
        assert name in N.EXPORTS
    assert {"render_mattes", "matte"} <= set(yrt_all())


def yrt_all():
    import yocto_raytracing_amd as y

    return y.__all__


def test_render_mattes_value_errors_come_before_any_native_call(yrt):
    scn = yrt.load_scene(str(scene_path("simple")))  # no BVH, no upload: neither is reached
    with pytest.raises(ValueError, match="nope"):
        yrt.render_mattes(scn, 8, 1, keys=("instance", "nope"))
    with pytest.raises(ValueError):
        yrt.render_mattes(scn, 8, 1, keys=())
    for ranks in (0, 1, 5, 12, 16, True):
        with pytest.raises(ValueError, match="ranks"):
            yrt.render_mattes(scn, 8, 1, ranks=ranks)


def test_matte_adds_the_selected_coverages_in_rank_order(yrt):
    ids = np.array([[[3, 7, 3, -1], [5, -1, -1, -1]],
                    [[-1, -1, -1, -1], [7, 3, 9, 2]]], np.int32)
    third = np.float32(1) / np.float32(3)
    cov = np.array([[[0.5, 0.25, 0.125, 0.0], [1.0, 0.0, 0.0, 0.0]],
                    [[0.0, 0.0, 0.0, 0.0], [third, third, 0.1, 0.2]]], np.float32)
    m = {"ids": ids, "coverage": cov}
    got = yrt.matte(m, [3])
    assert got.dtype == np.float32 and got.shape == (2, 2)
    # an id present at two ranks (a hand-made table; the pass never gives one) counts at both
    np.testing.assert_array_equal(got, np.array([[0.625, 0.0], [0.0, third]], np.float32))
    np.testing.assert_array_equal(yrt.matte(m, {7, 5}), np.array([[0.25, 1.0], [0.0, third]], np.float32))
    # rank order, from +0: ((0 + 1/3) + 1/3) + 0.1, each sum rounded to float32
    want = np.float32(np.float32(np.float32(0) + third) + third)
    want = np.float32(np.float32(want + np.float32(0.1)) + np.float32(0.2))
    assert yrt.matte(m, [2, 9, 3, 7])[1, 1].view(np.uint32) == want.view(np.uint32)
    # -1, the unused ranks' id, is never selected unless asked for
    assert not yrt.matte(m, []).any() and not yrt.matte(m, [100]).any()
    cov2 = cov.copy()
    cov2[1, 0, 0] = 0.75  # (not a table of the pass: an unused rank has coverage 0)
    assert not yrt.matte({"ids": ids, "coverage": cov2}, [3, 7, 5, 9, 2]).item(2)
    assert yrt.matte({"ids": ids, "coverage": cov2}, [-1])[1, 0] == np.float32(0.75)
    # nothing selected is +0, not -0
    assert not np.signbit(yrt.matte(m, [100])).any()
    with pytest.raises(ValueError):
        yrt.matte({"ids": ids, "coverage": cov[..., :3]}, [3])


def test_cli_matte_usage_errors():
    def run(*args):
        return subprocess.run([str(CLI), *args], capture_output=True, text=True, timeout=60)

    r = run("--mattes", "nope", str(scene_path("simple")))
    assert r.returncode == 1 and "unknown --mattes nope" in r.stderr and "loading scene" not in r.stdout
    r = run("--mattes", "instance,", str(scene_path("simple")))
    assert r.returncode == 1 and "unknown --mattes" in r.stderr
    r = run("--mattes", "instance", "--gpus", "2", str(scene_path("simple")))
    assert r.returncode == 1 and "--mattes" in r.stderr and "loading scene" not in r.stdout
    r = run("--mattes")
    assert r.returncode == 1 and "missing value" in r.stderr
    r = run("--matte-ranks")
    assert r.returncode == 1 and "missing value" in r.stderr
    for bad in ("5", "0", "16", "x"):
        r = run("--mattes", "instance", "--matte-ranks", bad, str(scene_path("simple")))
        assert r.returncode == 1 and "--matte-ranks" in r.stderr and "loading scene" not in r.stdout, bad
    r = run("--help")
    assert r.returncode == 0 and "--mattes" in r.stderr and "--matte-ranks" in r.stderr


def test_k_matte_code_object_budget():
    """exactly the six k_matte<layers, keys> kernels, none with scratch: the tables and the walk
    fit the registers (a spill, or a table indexed at run time, would put vector-memory round
    trips into the sample loop). The VGPR counts are printed, not gated."""
    from yocto_raytracing_amd.codeid import kernel_resources

    hits = {k: v for k, v in kernel_resources(LIB).items() if re.search(r"k_matte", k)}
    got = {}
    for name, r in hits.items():
        m = re.search(r"7k_matteILi(\d)ELi(\d)EE", name)
        assert m, name
        got[(int(m.group(1)), int(m.group(2)))] = r
        print(f"k_matte<{m.group(1)}, {m.group(2)}>: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs ({r['sgpr_spill']} spilled "
              f"to VGPR lanes), {r['lds']} B LDS, block {r['block']}")
    assert len(hits) == 6 and sorted(got) == [(l, k) for l in (1, 2) for k in (1, 2, 3)], sorted(hits)
    for r in got.values():
        assert r["vgpr_spill"] == 0, r
        assert r["private"] == 0, r
