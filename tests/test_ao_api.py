"""The ambient occlusion pass's interface without a GPU (yrt_render_ao, yrt_ao_params_default,
yrt_ao_tables, yrt_host_scene_shape_kinds, include/yrt.h): argument checks that return before any
device call, the defaults, Scene.shape_kinds(), the Python names against the header, the CLI's
--ao usage errors and the k_ao kernel's code-object budget."""
import ctypes as C
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import ROOT, scene_path

LIB = ROOT / "yocto_raytracing_amd" / "libyrt.so"
CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
FLT_MAX = float(np.finfo(np.float32).max)
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    return y


def test_defaults_are_as_documented(yrt):
    from yocto_raytracing_amd import _native as N

    a = N.AoParams(-1, -1.0, -1.0)
    N.lib.yrt_ao_params_default(C.byref(a))
    assert a.rays == 16 and a.distance == FLT_MAX and a.bias == float(np.float32(0.01))
    N.lib.yrt_ao_params_default(None)  # a null pointer is ignored
    header = (ROOT / "include" / "yrt.h").read_text()
    assert int(re.search(r"#define YRT_AO_RAYS_MAX (\d+)", header).group(1)) == N.YRT_AO_RAYS_MAX == 64
    assert C.sizeof(N.AoParams) == 12 and (N.AoParams.rays.offset, N.AoParams.distance.offset, N.AoParams.bias.offset) == (0, 4, 8)
    for name in ("yrt_render_ao", "yrt_ao_params_default", "yrt_ao_tables", "yrt_host_scene_shape_kinds"):
        assert name in N.EXPORTS
    assert {"render_ao", "ao_tables"} <= set(yrt.__all__)


# (rays, distance, bias) that yrt_render_ao refuses, after defaulting
BAD_PARAMS = [(-1, 1.0, 0.0), (65, 1.0, 0.0), (1 << 20, 1.0, 0.0),
              (16, NAN, 0.0), (16, 0.0, 0.0), (16, -0.0, 0.0), (16, -2.0, 0.0), (16, -INF, 0.0),
              (16, 1.0, NAN), (16, 1.0, -0.25), (16, INF, INF), (16, 1.0, -INF), (16, 1.0, 1.0), (16, 1.0, 3.0),
              (16, INF, FLT_MAX)]


def test_invalid_arguments_return_before_any_device_call(yrt):
    """no GPU, and a handle that is no scene: every refusal comes before the handle is looked at"""
    from yocto_raytracing_amd import _native as N

    p = yrt.render_params(resolution=8)
    out = np.full((8, 16, 4), 77, np.float32)
    handle = C.create_string_buffer(256)
    h = C.cast(handle, C.c_void_p)
    good = N.AoParams(0, INF, 0.01)
    call = lambda hh, pp, aa, oo, mem=N.YRT_MEM_HOST: N.lib.yrt_render_ao(hh, pp, aa, oo, mem, None)  # noqa: E731
    assert call(None, C.byref(p), C.byref(good), out.ctypes.data) == 1 and b"handle" in N.lib.yrt_last_error()
    assert call(h, None, C.byref(good), out.ctypes.data) == 1
    assert call(h, C.byref(p), None, out.ctypes.data) == 1
    assert call(h, C.byref(p), C.byref(good), None) == 1
    for rays, distance, bias in BAD_PARAMS:
        bad = N.AoParams(rays, distance, bias)
        assert call(h, C.byref(p), C.byref(bad), out.ctypes.data) == 1, (rays, distance, bias)
        assert N.lib.yrt_last_error().startswith(b"ao:"), (rays, distance, bias)
    for mem in (-1, 2):
        assert call(h, C.byref(p), C.byref(good), out.ctypes.data, mem) == 1 and b"mem" in N.lib.yrt_last_error()
    p.camera = -1
    assert call(h, C.byref(p), C.byref(good), out.ctypes.data) == 1 and b"camera" in N.lib.yrt_last_error()
    assert (out == 77).all()
    assert N.lib.yrt_ao_tables(None, None) == 1


def test_shape_kinds(yrt):
    from yocto_raytracing_amd import _native as N

    s = yrt.Scene.create()
    assert s.shape_kinds() == []
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    added = [s.add_shape(pos=pos, triangles=[[0, 1, 2]]), s.add_shape(pos=pos, radius=[.1, .1, .1], lines=[[0, 1], [1, 2]]),
             s.add_shape(pos=pos, radius=[.1, .1, .1], points=[0, 2]), s.add_shape(pos=pos, triangles=[[0, 2, 1]])]
    assert added == [0, 1, 2, 3] and s.shape_kinds() == [0, 1, 2, 0]
    # the golden scene with every primitive kind: kinds agree with the primitive totals
    lines = yrt.load_scene(str(scene_path("lines")))
    kinds, info = lines.shape_kinds(), lines.info()
    assert len(kinds) == info["shapes"] and set(kinds) == {0, 1, 2}
    assert info["triangles"] and info["lines"] and info["points"]
    # the call shape of yrt_host_scene_instances: n is always set, kind may be NULL, cap bounds the writes
    n = C.c_int(-1)
    assert N.lib.yrt_host_scene_shape_kinds(lines.handle, None, 0, C.byref(n)) == 0 and n.value == len(kinds)
    buf = (C.c_int * 4)(*[-7] * 4)
    assert N.lib.yrt_host_scene_shape_kinds(lines.handle, buf, 3, C.byref(n)) == 0 and n.value == len(kinds)
    assert list(buf) == kinds[:3] + [-7]
    assert N.lib.yrt_host_scene_shape_kinds(None, None, 0, C.byref(n)) == 1
    assert N.lib.yrt_host_scene_shape_kinds(lines.handle, None, 0, None) == 1
    assert N.lib.yrt_host_scene_shape_kinds(lines.handle, buf, -1, C.byref(n)) == 1


@pytest.mark.parametrize("args,message", [
    (["--ao", "0"], "K must be from 1 to 64"), (["--ao", "65"], "K must be from 1 to 64"),
    (["--ao", "8,"], "--ao takes"), (["--ao", "8,1,0.1,2"], "--ao takes"), (["--ao", "x"], "--ao takes"),
    (["--ao", "8", "--gpus", "2"], "one GPU")])
def test_cli_usage_errors(args, message):
    r = subprocess.run([str(CLI), *args, str(scene_path("simple"))], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and message in r.stderr, r.stderr[:300]


def test_check_ao_args_builds_and_passes(tmp_path):
    """tools/check_ao_args.cpp (ao_args.h, the one-plane list, the tables' header) as a stand-alone
    program of the host compiler: no GPU and no libyrt.so are involved"""
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "check_ao_args"
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", str(ROOT / "tools" / "check_ao_args.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ok"


def test_k_ao_register_budget():
    """k_ao in the shipped library's gfx950 code object (the AMDHSA metadata note, as
    tests/test_code_object_nested.py reads it): 79 VGPRs (6 waves per SIMD), 31 SGPR spills (to
    VGPR lanes), no VGPR spill and no private memory when the pass was written (DESIGN.md section
    5); pinned as ceilings. One kernel: K, bias and distance are arguments, not template values."""
    if not LIB.exists():
        from yocto_raytracing_amd import build

        build.build_library()
    from yocto_raytracing_amd.codeid import kernel_resources

    hits = {k: v for k, v in kernel_resources(LIB).items() if re.search(r"\d+k_aoE", k)}
    assert len(hits) == 1, sorted(hits)
    (name, r), = hits.items()
    print(name, r)
    assert r["vgpr"] <= 80, r
    assert r["vgpr_spill"] == 0 and r["private"] == 0, r
    assert r["sgpr_spill"] <= 31, r
