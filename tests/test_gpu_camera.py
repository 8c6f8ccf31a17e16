"""yrt_render_camera and yrt_camera_rays on the GPU (camera.hip: k_camera_rays, the ray-batch
pipeline, k_camera_resolve): the thin-lens perspective camera, the orthographic camera and the
equirectangular panorama of include/yrt.h.

The rays are pinned to the numpy model (tests/camera_model.py) bit for bit, the panorama's to
its float64 model within 2^-18; the image is pinned to the merged entry points by composition:
with aperture 0 it is yrt.raytrace's, and under every model it is the box filter of
yrt.shade_rays over yrt.camera_rays, all bit for bit. Frames of 37 x 24 and 24 x 37 pixels
(partial waves), s = 3 unless stated.

An empty window cannot be asked for: without a band interleave, which the call refuses,
yrt_render_params always resolves to at least one row and one column.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import camera_model as CM
import passes_scene as PS
import shade_rays_scene as SS
from helpers import MIRROR_DEPTH, ROOT, read_png_rgba8, scene_path
from camera_model import HAND_ASPECT, HAND_FOCUS, HAND_FOVY, PANORAMA_BOUND, hand_frame, lens_test_camera

pytestmark = pytest.mark.gpu

CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
FRAMES = ((24, 37), (37, 24))  # (resolution = rows, width)
S = 3
AMB = PS.AMB
DEPTH = {"basic": 16, "simple": 16, "refl": 16, "lines": 16, "mirrors": MIRROR_DEPTH}
STAT_KEYS = ("rays", "shadow_rays", "shadow_rays_culled", "depth_truncated", "camera_samples")
# the three models as keyword arguments of raytrace_camera / camera_rays
MODELS = {"perspective": dict(model="perspective", aperture=0.3), "orthographic": dict(model="orthographic"),
          "equirect": dict(model="equirect")}
YRT_OK, YRT_ERR_INVALID_ARG, YRT_ERR_UNSUPPORTED = 0, 1, 3


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on the MI355X box")
    return y


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


_scenes, _renders, _cameras = {}, {}, {}
IDENTITY = np.r_[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0].astype(np.float32)


def add_quad(s, corners, mat):
    sh = s.add_shape(corners, norm=[[0, 0, 1]] * 4, texcoord=[[0, 0], [1, 0], [1, 1], [0, 1]], triangles=[[0, 1, 2], [0, 2, 3]])
    s.add_instance(IDENTITY, sh, mat)


def build_lens_scene(yrt, panorama):
    """the lens test's scene (camera_model.LENS_QUADS: no lights, so under ambient 1 a pixel is
    the mean of kd over its samples); with `panorama` also a white quad behind the camera and
    a grey one above it, both outside the perspective view"""
    s = yrt.Scene.create()
    c = lens_test_camera()
    s.add_camera(c["frame"], fovy=c["fovy"], aspect=c["aspect"], focus=c["focus"])
    mats = {kd: s.add_material(kd=(kd, kd, kd)) for kd in (0.0, 0.5, 1.0)}
    for z, x0, x1, hy, kd in CM.LENS_QUADS + ((CM.LENS_BEHIND,) if panorama else ()):
        add_quad(s, [[x0, -hy, z], [x1, -hy, z], [x1, hy, z], [x0, hy, z]], mats[kd])
    if panorama:
        add_quad(s, [[-2, 5, -2], [2, 5, -2], [2, 5, 2], [-2, 5, 2]], mats[0.5])
    return s


def dev_scene(yrt, name):
    if name not in _scenes:
        if name == "hand":  # the hand-made camera of tests/test_camera_api.py and nothing else
            s = yrt.Scene.create()
            s.add_camera(hand_frame(), fovy=HAND_FOVY, aspect=HAND_ASPECT, focus=HAND_FOCUS)
        elif name in ("lens", "pano"):
            s = build_lens_scene(yrt, name == "pano")
        else:
            s = yrt.load_scene(str(scene_path(name)))
        yrt.build_bvh(s)
        _scenes[name] = (s, s.upload(0))
    return _scenes[name][1]


def model_camera(yrt, name, focus=None):
    """camera_model.dev_camera of the scene's camera 0"""
    ds = dev_scene(yrt, name)
    return CM.scene_camera(ds.host.camera(0), focus)


def raytrace(yrt, name, res, width):
    """(image, stats) of yrt.raytrace at S samples per axis (shared, not to be written to)"""
    key = (name, res, width)
    if key not in _renders:
        _renders[key] = yrt.raytrace(dev_scene(yrt, name), AMB, res, S, width=width, max_depth=DEPTH[name], return_stats=True)
    return _renders[key]


def camera(yrt, name, res, width, model, **kw):
    """(image, stats) of yrt.raytrace_camera under MODELS[model] (shared unless kw is given)"""
    def run():
        return yrt.raytrace_camera(dev_scene(yrt, name), AMB, res, S, width=width, max_depth=DEPTH[name], return_stats=True,
                                   **{**MODELS[model], **kw})
    if kw:
        return run()
    key = (name, res, width, model)
    if key not in _cameras:
        _cameras[key] = run()
    return _cameras[key]


# ---- 1. the rays ----
@pytest.mark.parametrize("res,width,s", [(*FRAMES[0], S), (*FRAMES[1], S), (5, 5, 9)])  # s = 9: q >= 64
@pytest.mark.parametrize("name", ["basic", "hand"])
def test_rays_equal_the_model(yrt, name, res, width, s):
    ds, tabs = dev_scene(yrt, name), yrt.ao_tables()
    shape = (res, width, s * s, 8)
    lens = yrt.camera_rays(ds, res, s, model="perspective", aperture=0.3, focus=2.5, width=width).reshape(shape)
    same_bits(lens, CM.rays(model_camera(yrt, name, 2.5), CM.PERSPECTIVE, width, res, s, aperture=0.3, tabs=tabs))
    orth = yrt.camera_rays(ds, res, s, model="orthographic", aperture=0.3, width=width).reshape(shape)
    same_bits(orth, CM.rays(model_camera(yrt, name), CM.ORTHOGRAPHIC, width, res, s))
    pin = yrt.camera_rays(ds, res, s, aperture=0.0, width=width).reshape(shape)
    same_bits(pin, CM.rays(model_camera(yrt, name), CM.PERSPECTIVE, width, res, s))
    assert (lens[..., 0:3] != pin[..., 0:3]).any(axis=-1).mean() > 0.9
    dc = model_camera(yrt, name)
    pano = yrt.camera_rays(ds, res, s, model="equirect", aperture=0.3, focus=2.5, width=width).reshape(shape)
    same_bits(pano[..., 0:3], np.broadcast_to(dc["o"], pano[..., 0:3].shape).copy())
    same_bits(pano[..., 6:8], pin[..., 6:8])
    err = float(np.abs(pano[..., 3:6].astype(np.float64) - CM.rays64(dc, width, res, s)).max())
    print(f"panorama, GPU, {name} {width}x{res} s={s}: max |d - d64| = {err:.3e} (bound {PANORAMA_BOUND:.3e})")
    assert err <= PANORAMA_BOUND


@pytest.mark.parametrize("model", list(MODELS))
def test_a_windows_rays_are_the_crop_of_the_frames(yrt, model):
    res, width = FRAMES[0]
    ds = dev_scene(yrt, "hand")
    full = yrt.camera_rays(ds, res, S, width=width, **MODELS[model]).reshape(res, width, S * S, 8)
    for x0, y0, tw, th in ((5, 3, 17, 11), (width - 10, res - 6, 10, 6)):
        got = yrt.camera_rays(ds, res, S, width=width, window=(x0, y0, tw, th), **MODELS[model]).reshape(th, tw, S * S, 8)
        same_bits(got, np.ascontiguousarray(full[y0:y0 + th, x0:x0 + tw]))


def test_the_scene_cameras_own_aperture_is_the_default(yrt):
    """aperture None (< 0 in the C-ABI) takes the camera's: a scene that asks for depth of field gets it"""
    s = yrt.Scene.create()
    s.add_camera(hand_frame(), fovy=HAND_FOVY, aspect=HAND_ASPECT, focus=HAND_FOCUS, aperture=0.3)
    yrt.build_bvh(s)
    own = yrt.camera_rays(s, 24, S, width=37)
    same_bits(own, yrt.camera_rays(dev_scene(yrt, "hand"), 24, S, width=37, aperture=0.3))
    assert (own != yrt.camera_rays(s, 24, S, width=37, aperture=0.0)).any()


# ---- 2. aperture 0 is yrt_render ----
@pytest.mark.parametrize("res,width", FRAMES)
@pytest.mark.parametrize("name", list(DEPTH))
def test_the_pinhole_is_raytrace(yrt, name, res, width):
    want, wstats = raytrace(yrt, name, res, width)
    got, stats = camera(yrt, name, res, width, "perspective", aperture=0.0)
    same_bits(got, want)
    assert {k: stats[k] for k in STAT_KEYS} == {k: wstats[k] for k in STAT_KEYS}
    assert stats["camera_samples"] == res * width * S * S
    if name == "mirrors":
        assert stats["rays"] > 2 * stats["camera_samples"]  # the mirror levels ran in the batch


# ---- 3. composition: the box filter of shade_rays over camera_rays ----
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("name", ["basic", "refl", "lines", "mirrors"])
def test_the_image_is_the_box_filter_of_the_shaded_rays(yrt, name, model):
    res, width = FRAMES[0] if model != "orthographic" else FRAMES[1]
    ds = dev_scene(yrt, name)
    got, stats = camera(yrt, name, res, width, model)
    rays = yrt.camera_rays(ds, res, S, width=width, **MODELS[model])
    colours, batch = yrt.shade_rays(ds, rays, AMB, max_depth=DEPTH[name], return_stats=True)
    same_bits(got, SS.box_filter(colours, S, res, width))
    assert {k: stats[k] for k in STAT_KEYS} == {k: batch[k] for k in STAT_KEYS}
    assert stats["camera_samples"] == res * width * S * S
    # the model matters: the image is not the pinhole's, and something is hit
    assert (got != raytrace(yrt, name, res, width)[0]).any() and got[..., :3].any()


# ---- 4. what changes no bit ----
@pytest.mark.parametrize("name,model", [("refl", "perspective"), ("simple", "equirect"), ("mirrors", "orthographic")])
def test_chunk_sizes_give_identical_bits(yrt, name, model):
    res, width = FRAMES[1]
    img, stats = camera(yrt, name, res, width, model)
    for chunk in ((7, 0) if name == "mirrors" else (1, 7, 0)):  # (one pixel a batch of the deep corridor: thousands of level waits)
        got, gstats = camera(yrt, name, res, width, model, chunk_pixels=chunk)
        same_bits(got, img)
        assert gstats == stats, chunk


@pytest.mark.parametrize("device_memory", [False, True])
@pytest.mark.parametrize("name,model", [("simple", "perspective"), ("mirrors", "equirect")])
def test_windows_equal_the_crop_and_keep_their_padding(yrt, name, model, device_memory):
    import torch

    res, width = FRAMES[0]
    full = camera(yrt, name, res, width, model)[0]
    ds = dev_scene(yrt, name)
    # inside with an odd origin and padded rows; the corner; touching the right and bottom edges
    for x0, y0, tw, th, stride in ((5, 3, 17, 11, 19), (0, 0, 9, 7, 12), (width - 10, res - 6, 10, 6, 13)):
        p = yrt.render_params(AMB, res, S, width=width, max_depth=DEPTH[name], window=(x0, y0, tw, th))
        p.out_stride = stride
        out = np.empty((th, stride, 4), np.float32)
        out.view(np.uint32)[...] = 0x7fc01234
        if device_memory:
            d_out = torch.from_numpy(out).to("cuda:0")
            torch.cuda.synchronize()
            ds.render_camera_into(p, d_out.data_ptr(), **MODELS[model])
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
        else:
            ds.render_camera_into(p, out.ctypes.data, device_memory=False, **MODELS[model])
        same_bits(out[:, :tw], np.ascontiguousarray(full[y0:y0 + th, x0:x0 + tw]))
        assert (out[:, tw:].view(np.uint32) == 0x7fc01234).all(), (x0, y0)
        assert ds.last_stats()["camera_samples"] == tw * th * S * S


@pytest.mark.parametrize("model", list(MODELS))
def test_rows_past_the_image_edge_are_zeros(yrt, model):
    res, width = FRAMES[0]
    full = camera(yrt, "simple", res, width, model)[0]
    p = yrt.render_params(AMB, res, S, width=width, window=(4, res - 3, 20, 5))  # two local rows past the edge
    out = np.full((5, 20, 4), 7, np.float32)
    ds = dev_scene(yrt, "simple")
    ds.render_camera_into(p, out.ctypes.data, device_memory=False, **MODELS[model])
    same_bits(out[:3], np.ascontiguousarray(full[res - 3:, 4:24]))
    assert not out[3:].any()
    assert ds.last_stats()["camera_samples"] == 3 * 20 * S * S


@pytest.mark.parametrize("name,model", [("refl", "perspective"), ("lines", "orthographic"), ("mirrors", "equirect")])
def test_runs_algorithms_lists_and_staging_give_identical_bits(yrt, name, model):
    res, width = FRAMES[0]
    img, stats = camera(yrt, name, res, width, model)
    again, astats = camera(yrt, name, res, width, model, chunk_pixels=0)
    same_bits(again, img)
    assert astats == stats
    got, gstats = camera(yrt, name, res, width, model, algorithm="wavefront_lane")
    same_bits(got, img)
    assert {k: gstats[k] for k in STAT_KEYS} == {k: stats[k] for k in STAT_KEYS}
    ds = dev_scene(yrt, name)
    try:
        ds.set_tile_lists("on")
        got, gstats = camera(yrt, name, res, width, model, chunk_pixels=0)
        same_bits(got, img)
        lists = ds.tile_lists()
        assert not lists["camera"] and not lists["bundles"] and gstats == stats
        ds.set_tile_lists("auto")
        ds.set_lds_staging(True)
        got, gstats = camera(yrt, name, res, width, model, chunk_pixels=0)
        same_bits(got, img)
        assert ds.lds_staging() == {"closest_hit": False, "any_hit": False} and gstats == stats
    finally:
        ds.set_tile_lists("auto")
        ds.set_lds_staging(False)


@pytest.mark.parametrize("model", list(MODELS))
def test_host_and_device_outputs_agree(yrt, model):
    import torch

    res, width = FRAMES[1]
    img = camera(yrt, "refl", res, width, model)[0]
    p = yrt.render_params(AMB, res, S, width=width)
    d_out = torch.full((res, width, 4), 7.0, dtype=torch.float32, device="cuda:0")
    d_rays = torch.zeros((res * width * S * S, 8), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    ds = dev_scene(yrt, "refl")
    ds.render_camera_into(p, d_out.data_ptr(), **MODELS[model])
    ds.camera_rays_into(p, d_rays.data_ptr(), **MODELS[model])
    torch.cuda.synchronize()
    same_bits(d_out.cpu().numpy(), img)
    same_bits(d_rays.cpu().numpy(), yrt.camera_rays(ds, res, S, width=width, **MODELS[model]))


# ---- 5. refusals with a real handle ----
def test_unsupported_and_invalid_calls_are_refused(yrt):
    from yocto_raytracing_amd import _native as N

    ds = dev_scene(yrt, "simple")
    out = np.full((24, 37, 4), 77, np.float32)
    rays = np.full((24 * 37 * S * S, 8), 77, np.float32)

    def call(m=(0, -1.0, 0.0, 0), mem=N.YRT_MEM_HOST, dst=out, entry="yrt_render_camera", **kw):
        p = yrt.render_params(AMB, 24, S, width=37, **kw)
        cm = N.CameraModel(*m)
        return getattr(N.lib, entry)(ds.handle, C.byref(p), C.byref(cm), dst.ctypes.data if dst is not None else None, mem, None)

    assert call(algorithm="megakernel") == YRT_ERR_UNSUPPORTED
    assert call(count_work=True) == YRT_ERR_UNSUPPORTED
    for band in ((8, 3, 1), (2, 1, 0), (1, 2, 0)):
        assert call(band=band) == YRT_ERR_UNSUPPORTED, band
        assert call(band=band, dst=rays, entry="yrt_camera_rays") == YRT_ERR_UNSUPPORTED, band
    for entry, dst in (("yrt_render_camera", out), ("yrt_camera_rays", rays)):
        for m in ((3, -1.0, 0.0, 0), (0, float("nan"), 0.0, 0), (1, 0.0, float("inf"), 0), (0, 0.0, 0.0, -1)):
            assert call(m, dst=dst, entry=entry) == YRT_ERR_INVALID_ARG and N.lib.yrt_last_error().startswith(b"camera:"), m
        assert call(mem=2, dst=dst, entry=entry) == YRT_ERR_INVALID_ARG
        assert call(dst=None, entry=entry) == YRT_ERR_INVALID_ARG
        assert call(camera=5, dst=dst, entry=entry) == YRT_ERR_INVALID_ARG and b"camera index out of range" in N.lib.yrt_last_error()
    # yrt_camera_rays: the window lies inside the image; it ignores the algorithm and count_work
    assert call(window=(4, 21, 20, 5), dst=rays, entry="yrt_camera_rays") == YRT_ERR_INVALID_ARG
    assert call(window=(30, 0, 20, 5), dst=rays, entry="yrt_camera_rays") == YRT_ERR_INVALID_ARG
    assert (out == 77).all() and (rays == 77).all()
    before = ds.last_stats()
    assert call(algorithm="megakernel", count_work=True, dst=rays, entry="yrt_camera_rays") == YRT_OK and (rays != 77).any()
    assert ds.last_stats() == before  # it touches no counter
    assert call() == YRT_OK and (out != 77).all()


# ---- 6. the lens does what a lens does ----
def test_depth_of_field_blurs_what_is_out_of_focus(yrt):
    """48 x 48, s = 4, aperture 0.5, the scene of camera_model.LENS_QUADS: a white quad at z = -2
    left of x = 0 (column 24), a white quad at z = -6 right of x = 1.5 (column 36), a black
    backdrop. In the middle row the pixels strictly between the plateaus are counted left and
    right of column 30: an edge in focus has <= 1, out of focus >= 5 (8 pixels of blur), and the two
    swap with the focus. tests/test_camera_api.py holds the same conditions on the model alone,
    and says why the far quad stands at x > 1.5 and not at the issue's x > 0.5."""
    ds = dev_scene(yrt, "lens")
    row, split, imgs = 24, 30, {}
    for focus in (2.0, 6.0):
        img = yrt.raytrace_camera(ds, 1.0, 48, 4, aperture=0.5, focus=focus)
        assert (img[..., 3] == 1).all() and (img[..., 0] == img[..., 1]).all() and (img[..., 0] == img[..., 2]).all()
        imgs[focus] = img[..., 0]
        print(f"focus {focus}: middle row", np.round(img[row, 12:, 0], 2).tolist())
        assert (img[row, :16, 0] == 1).all() and (img[row, 44:, 0] == 1).all() and (img[row, 29:31, 0] == 0).all()
    near2, far2 = CM.transitional(imgs[2.0][row], 0, split), CM.transitional(imgs[2.0][row], split, 48)
    near6, far6 = CM.transitional(imgs[6.0][row], 0, split), CM.transitional(imgs[6.0][row], split, 48)
    print("transitional pixels (near edge, far edge): focus 2", (near2, far2), "focus 6", (near6, far6))
    assert near2 <= 1 and far2 >= 5
    assert near6 >= 5 and far6 <= 1
    # the lens changes the image; aperture 0 is raytrace's
    pin = yrt.raytrace_camera(ds, 1.0, 48, 4, aperture=0.0, focus=2.0)
    same_bits(pin, yrt.raytrace(ds, 1.0, 48, 4))
    assert (imgs[2.0] != pin[..., 0]).any() and CM.transitional(pin[row, :, 0], 0, 48) <= 2
    # the orthographic film at focus 6 is 2 * 6 * 0.5 = 6 wide: x = 0 is column 24, x = 1.5 column 36,
    # whatever the quads' depths
    orth = yrt.raytrace_camera(ds, 1.0, 48, 4, model="orthographic", focus=6.0)[..., 0]
    assert (orth[row, :24] == 1).all() and (orth[row, 24:36] == 0).all() and (orth[row, 36:] == 1).all()


# ---- 7. the panorama ----
def test_the_panorama_sees_all_around(yrt):
    """the lens scene plus a white quad behind the camera (z = +6) and a grey one above it
    (y = +5): the panorama shows the first at its left and right edges and the second in its top
    rows, the perspective view neither"""
    lens, pano = dev_scene(yrt, "lens"), dev_scene(yrt, "pano")
    same_bits(yrt.raytrace_camera(pano, 1.0, 24, 2, aperture=0.0, width=48), yrt.raytrace(lens, 1.0, 24, 2, width=48))
    img = yrt.raytrace_camera(pano, 1.0, 24, 2, model="equirect", width=48)[..., 0]
    without = yrt.raytrace_camera(lens, 1.0, 24, 2, model="equirect", width=48)[..., 0]
    assert (img[10:14, :3] == 1).all() and (img[10:14, -3:] == 1).all()  # behind: +z at both edges
    assert (without[10:14, :3] == 0).all() and (without[10:14, -3:] == 0).all()
    assert (img[:2] == 0.5).all() and (without[0] == 0).all()  # above: the top rows look up
    assert (img[-1] == 0).all()  # nothing below
    assert (img[12, 20:24] == 1).all() and (img[12, 24:26] == 0).all()  # ahead: the near quad left of the centre


def test_the_panoramas_top_rows_look_up_into_the_sky(yrt):
    """edge_sky: the camera looks up (along its -z) at nothing; its frame's +y is horizontal, so
    the panorama's top rows graze over the floor, which lies 2 below and reaches 5 out: within
    atan(2 / 5) = 21.8 degrees of +y, rows 0 and 1 of 24, every sample is a miss. The floor shows
    where the panorama looks back and down (the image's left and right edges)."""
    ds = dev_scene(yrt, "edge_sky")
    img, stats = yrt.raytrace_camera(ds, AMB, 24, S, model="equirect", width=48, return_stats=True)
    assert not img[:2, :, :3].any() and (img[..., 3] == 1).all()
    assert img[12, 0, :3].any() and img[12, -1, :3].any()
    assert not img[12, 20:28, :3].any()  # straight up
    assert stats["camera_samples"] == 24 * 48 * S * S


# ---- 8. the CLI ----
@pytest.mark.parametrize("flags,kw", [(["--camera-model", "orthographic"], dict(model="orthographic")),
                                      (["--aperture", "0.3", "--focus", "2"], dict(aperture=0.3, focus=2.0)),
                                      (["--camera-model", "equirect", "--width", "48"], dict(model="equirect", width=48))])
def test_cli_writes_the_models_image(yrt, tmp_path, flags, kw):
    out = tmp_path / "o.png"
    r = subprocess.run([str(CLI), *flags, "-r", "24", "-s", "3", "-o", str(out), str(scene_path("refl"))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img = yrt.raytrace_camera(dev_scene(yrt, "refl"), 0.1, 24, 3, **kw)
    np.testing.assert_array_equal(read_png_rgba8(out)[..., :3], yrt.tonemap(img)[..., :3])
    assert (yrt.tonemap(img) != yrt.tonemap(yrt.raytrace(dev_scene(yrt, "refl"), 0.1, 24, 3, width=kw.get("width", 0)))).any()


def test_cli_without_the_flags_is_unchanged(yrt, tmp_path):
    out = tmp_path / "o.png"
    r = subprocess.run([str(CLI), "-r", "24", "-s", "3", "-o", str(out), str(scene_path("refl"))], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    np.testing.assert_array_equal(read_png_rgba8(out)[..., :3], yrt.tonemap(yrt.raytrace(dev_scene(yrt, "refl"), 0.1, 24, 3))[..., :3])
