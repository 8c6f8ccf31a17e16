"""The camera models' interface without a GPU (yrt_render_camera, yrt_camera_rays,
yrt_camera_model_default, yrt_host_scene_camera, include/yrt.h): the symbols and defaults, argument
checks that return before any device call, the stand-alone host check (tools/
check_camera_models.cpp), the host's rays of csrc/camera_models.h against the numpy model
(tests/camera_model.py) and the oracle's eval_camera, Scene.camera(), the lens test's geometry
on the model alone, and the CLI's usage errors."""
import ctypes as C
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import camera_model as CM
import shade_rays_scene as SS
from helpers import ROOT, scene_path

LIB = ROOT / "yocto_raytracing_amd" / "libyrt.so"
CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
INF, NAN = float("inf"), float("nan")
# (resolution = rows, width, samples per axis): s = 9 gives q >= 64, the rotation changes within a pixel
FRAMES = ((7, 13, 3), (13, 7, 3), (5, 5, 9))
PANORAMA_BOUND = CM.PANORAMA_BOUND


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    return y


@pytest.fixture(scope="module")
def cameras(yrt, tmp_path_factory):
    """name -> (Scene.camera() dict, what Oracle() loads): the `basic` scene's camera and a
    hand-made one, saved as a scene of its own for the oracle"""
    s = yrt.Scene.create()
    s.add_camera(CM.hand_frame(), fovy=CM.HAND_FOVY, aspect=CM.HAND_ASPECT, focus=CM.HAND_FOCUS)
    path = tmp_path_factory.mktemp("camera") / "hand.yrtscene"
    s.save(str(path))
    return {"basic": (yrt.load_scene(str(scene_path("basic"))).camera(0), "basic"), "hand": (s.camera(0), str(path))}


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    """tools/check_camera_models.cpp built by the host compiler, warnings as errors, no contraction"""
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("check_camera") / "check_camera_models"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror",
                    str(ROOT / "tools" / "check_camera_models.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    return exe


def hexf(x) -> str:
    return struct.pack(">f", float(np.float32(x))).hex()


def host_rays(exe, tmp_path, cam, model, aperture, res, width, s):
    """(res, width, s * s, 8) float32: camera_model_eval on the host, through the check program"""
    out = tmp_path / "rays.bin"
    args = [str(exe), "rays", str(out), str(model), hexf(aperture), str(width), str(res), str(s)]
    args += [hexf(v) for v in cam["frame"]] + [hexf(cam["fovy"]), hexf(cam["aspect"]), hexf(cam["focus"])]
    subprocess.run(args, check=True, capture_output=True, text=True, timeout=60)
    return np.fromfile(out, np.float32).reshape(res, width, s * s, 8)


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 1. symbols, defaults, refusals ----
def test_symbols_and_defaults_are_as_documented(yrt):
    from yocto_raytracing_amd import _native as N

    m = N.CameraModel(7, 7.0, 7.0, 7)
    N.lib.yrt_camera_model_default(C.byref(m))
    assert (m.model, m.aperture, m.focus, m.chunk_pixels) == (0, -1.0, 0.0, 0)
    N.lib.yrt_camera_model_default(None)  # a null pointer is ignored
    header = (ROOT / "include" / "yrt.h").read_text()
    enum = re.search(r"YRT_CAMERA_PERSPECTIVE = (\d), YRT_CAMERA_ORTHOGRAPHIC = (\d), YRT_CAMERA_EQUIRECT = (\d)", header)
    assert [int(g) for g in enum.groups()] == [N.CAMERA_MODELS[k] for k in ("perspective", "orthographic", "equirect")] == [0, 1, 2]
    assert C.sizeof(N.CameraModel) == 16
    assert [getattr(N.CameraModel, f).offset for f in ("model", "aperture", "focus", "chunk_pixels")] == [0, 4, 8, 12]
    for name in ("yrt_render_camera", "yrt_camera_rays", "yrt_camera_model_default", "yrt_host_scene_camera"):
        assert name in N.EXPORTS and re.search(rf"\b{name}\(", header), name
    assert {"raytrace_camera", "camera_rays"} <= set(yrt.__all__)
    assert hasattr(yrt.DeviceScene, "render_camera_into") and hasattr(yrt.DeviceScene, "camera_rays_into")
    assert CM.MODELS == N.CAMERA_MODELS


# (model, aperture, focus, chunk_pixels) that both entry points refuse
BAD_MODELS = [(-1, 0.0, 0.0, 0), (3, 0.0, 0.0, 0), (1 << 20, 0.0, 0.0, 0),
              (0, NAN, 0.0, 0), (0, INF, 0.0, 0), (0, -INF, 0.0, 0),
              (0, 0.0, NAN, 0), (1, 0.0, INF, 0), (2, 0.0, -INF, 0),
              (0, 0.0, 0.0, -1), (1, 0.0, 0.0, -(1 << 31))]


@pytest.mark.parametrize("entry", ["yrt_render_camera", "yrt_camera_rays"])
def test_invalid_arguments_return_before_any_device_call(yrt, entry):
    """no GPU, and a handle that is no scene: every refusal comes before the handle is looked at"""
    from yocto_raytracing_amd import _native as N

    p = yrt.render_params(resolution=8)
    out = np.full((8, 16, 8), 77, np.float32)
    handle = C.create_string_buffer(256)
    h = C.cast(handle, C.c_void_p)
    good = N.CameraModel(0, -1.0, 0.0, 0)
    fn = getattr(N.lib, entry)
    call = lambda hh, pp, mm, oo, mem=N.YRT_MEM_HOST: fn(hh, pp, mm, oo, mem, None)  # noqa: E731
    assert call(None, C.byref(p), C.byref(good), out.ctypes.data) == 1 and b"handle" in N.lib.yrt_last_error()
    assert call(h, None, C.byref(good), out.ctypes.data) == 1 and b"params" in N.lib.yrt_last_error()
    assert call(h, C.byref(p), None, out.ctypes.data) == 1 and b"model" in N.lib.yrt_last_error()
    assert call(h, C.byref(p), C.byref(good), None) == 1 and b"out" in N.lib.yrt_last_error()
    for model, aperture, focus, chunk in BAD_MODELS:
        bad = N.CameraModel(model, aperture, focus, chunk)
        assert call(h, C.byref(p), C.byref(bad), out.ctypes.data) == 1, (model, aperture, focus, chunk)
        assert N.lib.yrt_last_error().startswith(b"camera:"), (model, aperture, focus, chunk)
    for mem in (-1, 2):
        assert call(h, C.byref(p), C.byref(good), out.ctypes.data, mem) == 1 and b"mem" in N.lib.yrt_last_error()
    p.camera = -1
    assert call(h, C.byref(p), C.byref(good), out.ctypes.data) == 1 and b"camera index" in N.lib.yrt_last_error()
    assert (out == 77).all()


def test_unknown_model_names_raise_before_any_native_call(yrt):
    with pytest.raises(ValueError, match="unknown camera model"):
        yrt.DeviceScene.render_camera_into(None, None, 0, model="fisheye")
    with pytest.raises(ValueError, match="unknown camera model"):
        yrt.DeviceScene.camera_rays_into(None, None, 0, model="pinhole")


# ---- 2. the stand-alone host check ----
def test_check_camera_models_builds_and_passes(check_exe):
    """camera_models.h, camera_args.h and the tables' header as a stand-alone program of the host
    compiler (-Wall -Werror -ffp-contract=off): no GPU and no libyrt.so are involved"""
    r = subprocess.run([str(check_exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ok"
    assert subprocess.run([str(check_exe), "rays"], capture_output=True, timeout=60).returncode == 2  # a usage error


# ---- 3. the host's formulas against the numpy model and the oracle ----
@pytest.mark.parametrize("res,width,s", FRAMES)
@pytest.mark.parametrize("name", ["basic", "hand"])
def test_host_rays_equal_the_model(yrt, cameras, check_exe, tmp_path, name, res, width, s):
    cam, oracle_scene = cameras[name]
    dc = CM.scene_camera(cam)
    tabs = yrt.ao_tables()
    # the thin lens and the orthographic film: the numpy model, bit for bit
    lens = host_rays(check_exe, tmp_path, cam, CM.PERSPECTIVE, 0.3, res, width, s)
    same_bits(lens, CM.rays(dc, CM.PERSPECTIVE, width, res, s, aperture=0.3, tabs=tabs))
    orth = host_rays(check_exe, tmp_path, cam, CM.ORTHOGRAPHIC, 0.3, res, width, s)
    same_bits(orth, CM.rays(dc, CM.ORTHOGRAPHIC, width, res, s))
    # the pinhole: the oracle's eval_camera, bit for bit (and the model's)
    pin = host_rays(check_exe, tmp_path, cam, CM.PERSPECTIVE, 0.0, res, width, s)
    same_bits(pin.reshape(-1, 8), SS.camera_rays(oracle_scene, s, 0, res, width))
    same_bits(pin, CM.rays(dc, CM.PERSPECTIVE, width, res, s))
    assert (lens[..., 0:3] != pin[..., 0:3]).any(axis=-1).mean() > 0.9  # the lens moves the origins
    # the panorama: origins exact, directions within 2^-18 of the float64 model
    pano = host_rays(check_exe, tmp_path, cam, CM.EQUIRECT, 0.3, res, width, s)
    same_bits(pano[..., 0:3], np.broadcast_to(dc["o"], pano[..., 0:3].shape).copy())
    same_bits(pano[..., 6:8], pin[..., 6:8])
    err = float(np.abs(pano[..., 3:6].astype(np.float64) - CM.rays64(dc, width, res, s)).max())
    print(f"panorama, host, {name} {width}x{res} s={s}: max |d - d64| = {err:.3e} (bound {PANORAMA_BOUND:.3e})")
    assert err <= PANORAMA_BOUND


# ---- 4. Scene.camera() ----
def test_scene_camera_returns_what_add_camera_was_given(yrt, tmp_path):
    from yocto_raytracing_amd import _native as N

    s = yrt.Scene.create()
    f = CM.hand_frame()
    assert s.add_camera(f, fovy=0.9, aspect=1.25, focus=3.5, aperture=0.125) == 0
    assert s.add_camera(np.r_[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 2, 6], fovy=0.6, aspect=2.0, focus=6.0) == 1
    c = s.camera(0)
    same_bits(c["frame"], f)
    assert (c["fovy"], c["aspect"], c["aperture"], c["focus"]) == (float(np.float32(0.9)), 1.25, 0.125, 3.5)
    c = s.camera(1)
    assert (c["aperture"], c["focus"], c["aspect"]) == (0.0, 6.0, 2.0) and c["frame"][9:].tolist() == [0, 2, 6]
    # every output may be NULL; a bad index or a null scene is refused
    foc = C.c_float()
    assert N.lib.yrt_host_scene_camera(s.handle, 1, None, None, None, None, C.byref(foc)) == 0 and foc.value == 6.0
    assert N.lib.yrt_host_scene_camera(s.handle, 0, None, None, None, None, None) == 0
    for index in (-1, 2):
        assert N.lib.yrt_host_scene_camera(s.handle, index, None, None, None, None, None) == 1
        with pytest.raises(yrt.YrtError):
            s.camera(index)
    assert N.lib.yrt_host_scene_camera(None, 0, None, None, None, None, None) == 1
    # a loaded .obj's aperture and focus (its `c` line: name, ortho, yfov, aspect, aperture, focus, frame)
    obj = tmp_path / "lens.obj"
    obj.write_text("c cam 0 0.8 1.5 0.25 4.5 1 0 0 0 1 0 0 0 1 1 2 3\nv 0 0 0\nv 1 0 0\nv 0 1 0\no tri\nf 1 2 3\n")
    c = yrt.load_scene(str(obj)).camera(0)
    assert (c["aperture"], c["focus"], c["aspect"], c["fovy"]) == (0.25, 4.5, 1.5, float(np.float32(0.8)))
    assert c["frame"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 2, 3]
    # and a saved scene keeps them
    s.save(str(tmp_path / "two.yrtscene"))
    c = yrt.load_scene(str(tmp_path / "two.yrtscene")).camera(0)
    assert (c["aperture"], c["focus"]) == (0.125, 3.5)


# ---- the lens test's geometry, on the model alone (tests/test_gpu_camera.py renders it) ----
def test_the_lens_tests_geometry_meets_its_conditions_on_the_model(yrt):
    """48 x 48, s = 4, aperture 0.5: the middle row's pixels strictly between the plateaus, left
    and right of the black gap's middle (column 30). In focus an edge has <= 1, out of focus >= 5
    (its blur is A |d - f| / d at the focal plane over a pixel of f / 48: 8 pixels), and the two
    swap with the focus. The issue's far quad (x > 0.5) projects to column 28 and its 8-pixel blur
    reaches the near edge's columns 24 and 25, which no count per edge can tell from the near
    edge's own blur (this test shows it: 2 > 1 on the near side); the far quad was moved to
    x > 1.5 (column 36), where 4 black columns separate the two blurs."""
    tabs, cam = yrt.ao_tables(), CM.lens_test_camera()
    row, split, edges = 24, 30, {}
    for focus in (2.0, 6.0):
        img = CM.quad_image(CM.rays(CM.scene_camera(cam, focus), CM.PERSPECTIVE, 48, 48, 4, aperture=0.5, tabs=tabs))
        edges[focus] = (CM.transitional(img[row], 0, split), CM.transitional(img[row], split, 48))
        assert img[row, :16].min() == 1 and img[row, 44:].min() == 1 and img[row, 29:31].max() == 0, focus
    print("transitional pixels (near edge, far edge) by focus:", edges)
    assert edges[2.0][0] <= 1 and edges[2.0][1] >= 5
    assert edges[6.0][0] >= 5 and edges[6.0][1] <= 1
    # the pinhole: both edges sharp; the issue's own geometry: the near side is polluted at focus 2
    pin = CM.quad_image(CM.rays(CM.scene_camera(cam, 2.0), CM.PERSPECTIVE, 48, 48, 4))
    assert CM.transitional(pin[row], 0, 48) <= 2
    asked = ((-2.0, -10.0, 0.0, 10.0, 1.0), (-6.0, 0.5, 30.0, 30.0, 1.0), CM.LENS_QUADS[2])
    img = CM.quad_image(CM.rays(CM.scene_camera(cam, 2.0), CM.PERSPECTIVE, 48, 48, 4, aperture=0.5, tabs=tabs), asked)
    assert CM.transitional(img[row], 0, 26) > 1
    # the orthographic film at focus 6 is 6 wide: x = 0 at column 24, x = 1.5 at column 36, whatever the depth
    orth = CM.quad_image(CM.rays(CM.scene_camera(cam, 6.0), CM.ORTHOGRAPHIC, 48, 48, 4))
    assert (orth[row, :24] == 1).all() and (orth[row, 24:36] == 0).all() and (orth[row, 36:] == 1).all()


# ---- 5. the CLI's usage errors ----
@pytest.mark.parametrize("args,message", [
    (["--camera-model", "fisheye"], "unknown --camera-model fisheye"),
    (["--aperture", "x"], "--aperture takes a finite number >= 0"), (["--aperture", "-0.5"], "--aperture takes"),
    (["--aperture", "nan"], "--aperture takes"), (["--aperture", "inf"], "--aperture takes"),
    (["--focus", "0"], "--focus takes a finite number > 0"), (["--focus", "2x"], "--focus takes"), (["--focus", "-1"], "--focus takes"),
    (["--camera-model", "equirect", "--aperture", "0.3"], "--aperture is the perspective model's lens"),
    (["--camera-model", "orthographic", "--gpus", "2"], "one GPU"),
    (["--aperture", "0.3", "--algorithm", "megakernel"], "wavefront algorithm"),
    (["--focus", "2", "--adaptive", "0.25"], "render the image alone"),
    (["--camera-model", "perspective", "--passes", "direct"], "render the image alone")])
def test_cli_usage_errors(args, message):
    r = subprocess.run([str(CLI), *args, str(scene_path("simple"))], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and message in r.stderr, r.stderr[:300]
