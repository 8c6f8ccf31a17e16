"""Soft shadows on the GPU (yrt_render_soft_shadows, yrt_shade_rays_soft; wavefront.hip
k_soft_shadow and k_soft_shade) against tests/soft_shadow_model.py, bit for bit on every floor
pixel of a built scene: the contract at one sample per pixel for several K, radii and light
counts, radius 0 against yrt.raytrace on the golden scenes (every level of the new kernels
against shipped results), the mirror levels grounded in level 0, batch shapes, chunks, windows
and padding, the sample sums through the model at twice the frame, a rotated blocker, a deep
instance tree (instance1k, from its five cameras, the terms from the scene's own light groups),
edge scenes, handle state, statistics, a thin lens, and the CLI.

The band interleave is yrt_render_camera's: refused (YRT_ERR_UNSUPPORTED), so no band shard and
no empty band offset can be asked for; the refusal is what is tested."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import soft_shadow_model as SM
from helpers import MIRROR_DEPTH, ROOT, read_png_rgba8, scene_path

pytestmark = pytest.mark.gpu

CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
AMB = (0.1, 0.1, 0.1)
RES, WIDTH = 32, 48
LIGHTS = ((0, 5, 0), (2, 4, -1), (-2.5, 4.5, 1), (1, 6, 2), (-1, 3.5, -2))
EYE = (0.0, 7.0, 9.0)
YRT_ERR_INVALID_ARG, YRT_ERR_UNSUPPORTED = 1, 3


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on the MI355X box")
    return y


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def ident(o=(0, 0, 0), rot=None):
    r = np.eye(3, dtype=np.float32) if rot is None else np.asarray(rot, np.float32)
    return np.concatenate([r.reshape(-1), np.asarray(o, np.float32)]).astype(np.float32)


_scenes = {}


def built(yrt, tmp_path_factory, nlights=5, blocker=True, kr=0.0, rotated=False):
    """(Scene, DeviceScene, path, lights): the issue's scene, through Scene.create() / add_*, saved
    for the oracle. The floor is instance 0, the lights follow in order, the blocker comes last
    (so the twin without it has the same instance and light indices). lights: [(frame, lp0)]."""
    key = (nlights, blocker, kr, rotated)
    if key in _scenes:
        return _scenes[key]
    s = yrt.Scene.create()
    eye = np.asarray(EYE, np.float32)
    z = eye / np.linalg.norm(eye)
    x = np.cross([0, 1, 0], z).astype(np.float32)
    x /= np.linalg.norm(x)
    y = np.cross(z, x).astype(np.float32)
    s.add_camera(np.concatenate([x, y, z, eye]).astype(np.float32), fovy=0.6, aspect=1.5, focus=float(np.linalg.norm(eye)))
    m_floor = s.add_material(kd=(0.7, 0.7, 0.7), ks=(0.2, 0.2, 0.2), kr=(kr, kr, kr), rs=0.3)
    m_block = s.add_material(kd=(0.5, 0.4, 0.3), rs=0.4)
    up = np.tile(np.array([[0, 1, 0]], np.float32), (4, 1))
    tc = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    tris = np.array([[0, 2, 1], [0, 3, 2]], np.int32)

    def quad(h):
        return s.add_shape(np.array([[-h, 0, -h], [h, 0, -h], [h, 0, h], [-h, 0, h]], np.float32), norm=up, texcoord=tc,
                           triangles=tris)

    assert s.add_instance(ident(), quad(6.0), m_floor) == 0
    pt = s.add_shape(np.zeros((1, 3), np.float32), radius=np.array([0.001], np.float32), points=np.array([0], np.int32))
    lights = []
    for pos in LIGHTS[:nlights]:
        s.add_instance(ident(pos), pt, s.add_material(ke=(40.0, 40.0, 40.0)))
        lights.append((ident(pos), np.zeros(3, np.float32)))
    if blocker:
        rot = None
        if rotated:  # a turn about y, then a tilt about x: a frame that is not the identity
            a, b = 0.6, 0.3
            ry = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])
            rx = np.array([[1, 0, 0], [0, np.cos(b), np.sin(b)], [0, -np.sin(b), np.cos(b)]])
            rot = (ry @ rx).astype(np.float32)
        s.add_instance(ident((0.3, 1.5, -0.2), rot), quad(1.0), m_block)
    assert len(s.lights()) == nlights
    path = tmp_path_factory.mktemp("soft") / f"soft_{nlights}_{int(blocker)}_{kr}_{int(rotated)}.yrtscene"
    s.save(str(path))
    yrt.build_bvh(s)
    _scenes[key] = (s, s.upload(0), path, lights)
    return _scenes[key]


def model(yrt, tmp_path_factory, radii, K, nlights=5, rotated=False, res=RES, width=WIDTH, kr=0.0):
    """soft_model of the built scene against its twin without the blocker (and without kr)"""
    _, ds, path, lights = built(yrt, tmp_path_factory, nlights, True, kr, rotated)
    _, twin, _, _ = built(yrt, tmp_path_factory, nlights, False, 0.0, False)
    return SM.soft_model(yrt, ds, twin, path, lights, radii, K, AMB, res, width, key=(nlights, rotated, kr))


def guard(m, radii, K):
    """the vacuity guard: per light with a radius at least 20 floor pixels in each class"""
    for li, R in enumerate(radii):
        o = m["open"][li][m["floor"]]
        classes = (int((o == 0).sum()), int(((o > 0) & (o < K)).sum()), int((o == K).sum()))
        print(f"light {li} R={R} K={K}: open == 0 / partial / open == K: {classes} of {int(m['floor'].sum())} floor pixels")
        assert classes[0] >= 20 and classes[2] >= 20, (li, classes)
        if R > 0 and K > 1:
            assert classes[1] >= 20, (li, classes)


def compare(got, m):
    f = m["floor"]
    print(f"{int((got[f].view(np.uint32) != m['rgba'][f].view(np.uint32)).sum())} of {got[f].size} floor channels differ")
    same_bits(got[f], m["rgba"][f])


# ---- 1. the model, bit for bit, every floor pixel ----
@pytest.mark.parametrize("R", [0.5, 0.75])
@pytest.mark.parametrize("K", [1, 16, 64])
def test_one_sample_equals_the_model(yrt, tmp_path_factory, K, R):
    _, ds, _, _ = built(yrt, tmp_path_factory)
    radii = [R] * 5
    m = model(yrt, tmp_path_factory, radii, K)
    assert int(m["floor"].sum()) > 1000
    guard(m, radii, K)
    got = yrt.raytrace_soft(ds, AMB, RES, 1, radius=R, shadow_rays=K)
    compare(got, m)
    # the batch call over the same rays: the same bits everywhere
    rays = yrt.camera_rays(ds, RES, 1, aperture=0.0)
    same_bits(yrt.shade_rays_soft(ds, rays, AMB, radius=R, shadow_rays=K).reshape(RES, WIDTH, 4), got)


@pytest.mark.parametrize("nlights", [4, 1])
def test_four_lights_and_one_equal_the_model(yrt, tmp_path_factory, nlights):
    """at most four lights: the shading kernel reads the counts as one word"""
    _, ds, _, _ = built(yrt, tmp_path_factory, nlights)
    radii = [0.5] * nlights
    m = model(yrt, tmp_path_factory, radii, 16, nlights)
    guard(m, radii, 16)
    compare(yrt.raytrace_soft(ds, AMB, RES, 1, radius=0.5, shadow_rays=16), m)


@pytest.mark.parametrize("nlights", [5, 4])
def test_per_light_radii_with_a_point_light_among_them(yrt, tmp_path_factory, nlights):
    _, ds, _, _ = built(yrt, tmp_path_factory, nlights)
    radii = [0.5, 0.0, 0.75, 1.0, 1.0][:nlights]
    m = model(yrt, tmp_path_factory, radii, 16, nlights)
    guard(m, radii, 16)
    o = m["open"][1][m["floor"]]
    assert set(np.unique(o).tolist()) == {0, 16}, "a light of radius 0 is open or not"
    got, st = yrt.raytrace_soft(ds, AMB, RES, 1, light_radii=radii, shadow_rays=16, return_stats=True)
    compare(got, m)
    # statistics: K rays per (hit sample, light) with a radius, 1 without
    hits = int((yrt.render_aovs(ds, RES, 1, width=0, aovs=("position",))["position"][..., 3] == 1).sum())
    assert st["camera_samples"] == RES * WIDTH
    assert st["shadow_rays"] == hits * sum(16 if R > 0 else 1 for R in radii)
    assert st["rays"] == st["camera_samples"] + st["shadow_rays"] and st["shadow_rays_culled"] <= st["shadow_rays"]
    from yocto_raytracing_amd import _native as N

    # the radii's count is the scene's light count
    p = yrt.render_params(AMB, RES, 1)
    bad = np.asarray(radii + [0.5], np.float32)
    sp = N.SoftShadowParams(16, 0.0, bad.ctypes.data_as(C.POINTER(C.c_float)), len(bad))
    out = np.zeros((RES, WIDTH, 4), np.float32)
    assert N.lib.yrt_render_soft_shadows(ds.handle, C.byref(p), None, C.byref(sp), out.ctypes.data, 0, None) == YRT_ERR_INVALID_ARG
    assert b"light count" in N.lib.yrt_last_error() and not out.any()


# ---- 2. radius 0 is today's image ----
@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("name,res,depth", [("basic", 24, 16), ("refl", 24, 16), ("lines", 24, 16), ("mirrors", 24, MIRROR_DEPTH),
                                            ("instance1k", 16, 16)])
def test_radius_zero_is_raytrace(yrt, name, res, depth, K):
    s = yrt.load_scene(str(scene_path(name)))
    yrt.build_bvh(s)
    ds = s.upload(0)
    want, wst = yrt.raytrace(ds, AMB, res, 2, max_depth=depth, return_stats=True)
    got, st = yrt.raytrace_soft(ds, AMB, res, 2, radius=0.0, shadow_rays=K, max_depth=depth, return_stats=True)
    same_bits(got, want)
    assert (st["rays"], st["shadow_rays"], st["depth_truncated"]) == (wst["rays"], wst["shadow_rays"], wst["depth_truncated"])
    # and per-light zeros, through the array
    n = len(s.lights())
    same_bits(yrt.raytrace_soft(ds, AMB, res, 2, light_radii=[0.0] * n, shadow_rays=K, max_depth=depth), want)


# ---- 3. mirror levels, grounded in level 0 ----
def test_mirror_levels_equal_the_fold_over_level_zero(yrt, tmp_path_factory):
    K, R, kr = 16, 0.5, np.float32(0.4)
    _, ds, _, _ = built(yrt, tmp_path_factory, kr=0.4)
    m = model(yrt, tmp_path_factory, [R] * 5, K, kr=0.4)
    f = m["floor"]
    p, n = m["pos"][f], m["nrm"][f]
    v, _ = SM.normalize_len((np.asarray(EYE, np.float32) - p).astype(np.float32))
    dr = (((n * np.float32(2.0)).astype(np.float32) * SM.dot32(n, v)[:, None]).astype(np.float32) - v).astype(np.float32)
    rays = np.zeros((len(p), 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = p, dr, np.float32(1e-4), SM.FLT_MAX
    for depth in (4, 2):
        S = yrt.shade_rays_soft(ds, rays, AMB, radius=R, shadow_rays=K, max_depth=depth - 1)[:, :3]
        want = (((m["c"][f] + (S * kr).astype(np.float32)).astype(np.float32)) + m["la"][f]).astype(np.float32)
        got, st = yrt.raytrace_soft(ds, AMB, RES, 1, radius=R, shadow_rays=K, max_depth=depth, return_stats=True)
        assert (S != 0).any(), "no mirror ray sees anything"
        same_bits(got[f][:, :3], want)
        assert (got[f][:, 3] == 1).all()
    # max_depth = 1: the mirror ray is cut, 0 * kr is added, every mirror hit is counted
    want = ((m["c"][f] + (np.zeros_like(m["c"][f]) * kr).astype(np.float32)).astype(np.float32) + m["la"][f]).astype(np.float32)
    got, st = yrt.raytrace_soft(ds, AMB, RES, 1, radius=R, shadow_rays=K, max_depth=1, return_stats=True)
    same_bits(got[f][:, :3], want)
    ids = yrt.render_aovs(ds, RES, 1, aovs=("position", "ids"))
    assert st["depth_truncated"] == int(((ids["position"][..., 3] == 1) & (ids["ids"][..., 0] == 0)).sum())


# ---- 4. shapes ----
def test_batches_chunks_windows_and_memory(yrt, tmp_path_factory):
    from yocto_raytracing_amd import _native as N

    K, R = 16, 0.5
    _, ds, _, _ = built(yrt, tmp_path_factory)
    rays = yrt.camera_rays(ds, RES, 1, aperture=0.0)
    whole = yrt.shade_rays_soft(ds, rays, AMB, radius=R, shadow_rays=K)
    for n in (0, 1, 63, 64, 65, 257):
        at = 700  # (inside the frame: hits, partly shadowed)
        same_bits(yrt.shade_rays_soft(ds, rays[at:at + n], AMB, radius=R, shadow_rays=K), whole[at:at + n])
    img = whole.reshape(RES, WIDTH, 4)
    # several chunks change no bit; a device plane is the host plane
    same_bits(yrt.raytrace_soft(ds, AMB, RES, 1, radius=R, shadow_rays=K, chunk_pixels=100), img)
    same_bits(yrt.raytrace_soft(ds, AMB, RES, 1, radius=R, shadow_rays=K, device_memory=True), img)
    # windows with padded rows: the crop, the padding left untouched
    for x0, y0, tw, th, stride in ((5, 3, 17, 11, 19), (0, 0, 9, 7, 12), (WIDTH - 10, RES - 6, 10, 6, 13)):
        p = yrt.render_params(AMB, RES, 1, window=(x0, y0, tw, th))
        p.out_stride = stride
        out = np.full((th, stride, 4), 77, np.float32)
        ds.render_soft_shadows_into(p, out.ctypes.data, R, None, K, device_memory=False)
        same_bits(out[:, :tw], img[y0:y0 + th, x0:x0 + tw])
        assert (out[:, tw:] == 77).all()
    same_bits(yrt.raytrace_soft(ds, AMB, RES, 1, radius=R, shadow_rays=K, window=(3, 9, 20, 8)), img[9:17, 3:23])
    # the band interleave, the megakernel and counted work are refused, as by yrt_render_camera
    out = np.zeros((RES, WIDTH, 4), np.float32)
    sp = N.SoftShadowParams(K, R, None, 0)

    def call(**kw):
        p = yrt.render_params(AMB, RES, 1, **kw)
        return N.lib.yrt_render_soft_shadows(ds.handle, C.byref(p), None, C.byref(sp), out.ctypes.data, 0, None)

    for band in ((8, 3, 1), (2, 1, 0), (1, 2, 0)):
        assert call(band=band) == YRT_ERR_UNSUPPORTED, band
    assert call(algorithm="megakernel") == YRT_ERR_UNSUPPORTED and call(count_work=True) == YRT_ERR_UNSUPPORTED
    p = yrt.render_params(AMB, algorithm="megakernel")
    assert N.lib.yrt_shade_rays_soft(ds.handle, C.byref(p), C.byref(sp), rays.ctypes.data, 8, out.ctypes.data, 0, None) == YRT_ERR_UNSUPPORTED
    assert not out.any()
    # the per-lane walk gives the same bits
    same_bits(yrt.raytrace_soft(ds, AMB, RES, 1, radius=R, shadow_rays=K, algorithm="wavefront_lane"), img)


def test_two_samples_equal_the_box_filter_of_the_model_at_twice_the_frame(yrt, tmp_path_factory):
    """sample (ii, jj) of pixel (i, j) is pixel (2 i + ii, 2 j + jj) of the one-sample frame at
    twice the resolution and width, ray for ray (both operands of the divisions scale by two),
    and the rotation comes from the hit point: the model at the larger frame, box filtered"""
    K, R = 16, 0.5
    _, ds, _, _ = built(yrt, tmp_path_factory)
    m = model(yrt, tmp_path_factory, [R] * 5, K, res=2 * RES, width=2 * WIDTH)
    got = yrt.raytrace_soft(ds, AMB, RES, 2, radius=R, shadow_rays=K)
    big, fl = m["rgba"].reshape(RES, 2, WIDTH, 2, 4), m["floor"].reshape(RES, 2, WIDTH, 2)
    acc = np.zeros((RES, WIDTH, 3), np.float32)
    for jj in range(2):
        for ii in range(2):
            acc = (acc + big[:, jj, :, ii, :3]).astype(np.float32)
    want = (acc / np.float32(4)).astype(np.float32)
    whole = fl.all(axis=(1, 3))
    assert int(whole.sum()) > 1000
    same_bits(got[whole][:, :3], want[whole])
    # three samples per axis: the image is the box filter of the batch call over its camera rays
    for s in (2, 3):
        img = yrt.raytrace_soft(ds, AMB, RES, s, radius=R, shadow_rays=K)
        assert np.isfinite(img).all()
        cols = yrt.shade_rays_soft(ds, yrt.camera_rays(ds, RES, s, aperture=0.0), AMB, radius=R, shadow_rays=K)
        cols = cols.reshape(RES, WIDTH, s * s, 4)
        acc = np.zeros((RES, WIDTH, 3), np.float32)
        for q in range(s * s):
            acc = (acc + cols[:, :, q, :3]).astype(np.float32)
        same_bits(img[..., :3], (acc / np.float32(s * s)).astype(np.float32))
        # between the all-occluded image (the ambient term) and the unshadowed one: every
        # factor lies in [0, 1] and every term is >= 0, so a sum of rounded products of them is
        # monotone; 1e-5 covers the different order of the per-light roundings. On the pixels
        # whose 3 x 3 neighbourhood sees the floor alone, so that no sample meets the blocker.
        _, twin, _, _ = built(yrt, tmp_path_factory, 5, False)
        hi = yrt.raytrace(twin, AMB, RES, s)
        lo = yrt.render_light_groups(twin, AMB, RES, s, groups=[0] * 5, beauty=False)["ambient"]
        f = whole.copy()
        f[0, :] = f[-1, :] = f[:, 0] = f[:, -1] = False
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                f[1:-1, 1:-1] &= whole[1 + dj:RES - 1 + dj, 1 + di:WIDTH - 1 + di]
        assert int(f.sum()) > 500
        assert (img[f][:, :3] <= hi[f][:, :3] * np.float32(1 + 1e-5)).all() and (img[f][:, :3] >= lo[f][:, :3] * np.float32(1 - 1e-5)).all()
        assert (img[f][:, :3] < hi[f][:, :3]).any(), "no pixel is shadowed"


# ---- 5. transforms and a deep tree ----
def test_a_rotated_blocker_equals_the_model(yrt, tmp_path_factory):
    K, R = 16, 0.5
    _, ds, _, _ = built(yrt, tmp_path_factory, rotated=True)
    m = model(yrt, tmp_path_factory, [R] * 5, K, rotated=True)
    guard(m, [R] * 5, K)
    compare(yrt.raytrace_soft(ds, AMB, RES, 1, radius=R, shadow_rays=K), m)


@pytest.mark.parametrize("R", [2.0, 6.0])
def test_instance1k_equals_the_model(yrt, R):
    """a deep instance tree (the wide walk's instance entries, off-centre rays through them), at
    the colour level without a twin: open per (pixel, light) from the model and the oracle, the
    per-light term from render_light_groups on the scene itself (max_depth = 1), compared bit
    for bit on the hit pixels where every light with open > 0 also has its hard ray open --
    among them the pixels no ray of a light reaches and those every ray reaches (the hard
    image). Resolution 16, K = 16, R = 2 as the issue sets them, from each of the scene's five
    cameras: the lights stand 70 units away, so one view has about ten partly open (pixel,
    light) pairs at R = 2 and the guard counts them over the five views; R = 6 widens the
    penumbrae."""
    K, res = 16, 16
    s = yrt.load_scene(str(scene_path("instance1k")))
    yrt.build_bvh(s)
    ds = s.upload(0)
    lights = SM.scene_lights(scene_path("instance1k"), s.lights())
    ncam = s.info()["cameras"]
    assert len(lights) == 3 and ncam == 5
    classes = np.zeros(3, np.int64)  # (pixel, light) pairs closed, partly open; pixels every ray reaches
    for cam in range(ncam):
        m = SM.hard_shadowed_model(yrt, ds, scene_path("instance1k"), lights, [R] * 3, K, AMB, res, camera=cam)
        f = m["known"]
        partial = (m["open"] > 0) & (m["open"] < K)
        allopen = (m["open"] == K).all(axis=0) & f
        here = (int((m["open"] == 0)[:, f].sum()), int(partial[:, f].sum()), int(allopen.sum()))
        classes += here
        got, st = yrt.raytrace_soft(ds, AMB, res, 1, radius=R, shadow_rays=K, max_depth=1, camera=cam, return_stats=True)
        print(f"instance1k camera {cam} R={R}: closed pairs / partly open pairs / all-open pixels {here}, {int(f.sum())} known of "
              f"{int(m['hit'].sum())} hit pixels; {int((got[f].view(np.uint32) != m['rgba'][f].view(np.uint32)).sum())} channels differ")
        same_bits(got[f], m["rgba"][f])
        same_bits(got[allopen], yrt.raytrace(ds, AMB, res, 1, max_depth=1, camera=cam)[allopen])
        assert st["shadow_rays"] == K * int(m["hit"].sum()) * 3
        # chunks change no bit
        same_bits(yrt.raytrace_soft(ds, AMB, res, 1, radius=R, shadow_rays=K, max_depth=1, camera=cam, chunk_pixels=37), got)
    # the vacuity guard, over the five views
    print(f"instance1k R={R}: closed pairs / partly open pairs / all-open pixels over {ncam} cameras: {classes.tolist()}")
    assert (classes >= 20).all(), classes.tolist()


# ---- 6. edges and state ----
@pytest.mark.parametrize("name", ["sky", "empty", "unlit", "lightsonly"])
def test_edge_scenes_equal_raytrace(yrt, name):
    s = yrt.load_scene(str(scene_path(f"edge_{name}")))
    yrt.build_bvh(s)
    ds = s.upload(0)
    same_bits(yrt.raytrace_soft(ds, AMB, 24, 2, radius=0.5, shadow_rays=16), yrt.raytrace(ds, AMB, 24, 2))
    rays = yrt.camera_rays(ds, 24, 1, aperture=0.0)
    same_bits(yrt.shade_rays_soft(ds, rays, AMB, radius=0.5), yrt.shade_rays(ds, rays, AMB))


def test_state_repeatability_and_isolation(yrt, tmp_path_factory):
    K, R = 16, 0.5
    _, ds, _, _ = built(yrt, tmp_path_factory)
    before = yrt.raytrace(ds, AMB, RES, 2)
    img, stats = yrt.raytrace_soft(ds, AMB, RES, 2, radius=R, shadow_rays=K, return_stats=True)
    again, astats = yrt.raytrace_soft(ds, AMB, RES, 2, radius=R, shadow_rays=K, return_stats=True)
    same_bits(again, img)
    assert astats == stats
    same_bits(yrt.raytrace(ds, AMB, RES, 2), before)
    assert (img != before).any()
    try:
        ds.set_tile_lists("on")
        got, gstats = yrt.raytrace_soft(ds, AMB, RES, 2, radius=R, shadow_rays=K, return_stats=True)
        same_bits(got, img)
        lists = ds.tile_lists()
        assert not lists["camera"] and not lists["bundles"] and gstats == stats
        ds.set_tile_lists("auto")
        ds.set_lds_staging(True)
        got, gstats = yrt.raytrace_soft(ds, AMB, RES, 2, radius=R, shadow_rays=K, return_stats=True)
        same_bits(got, img)
        assert ds.lds_staging() == {"closest_hit": False, "any_hit": False} and gstats == stats
    finally:
        ds.set_tile_lists("auto")
        ds.set_lds_staging(False)
    # K = 0 is 16
    same_bits(yrt.raytrace_soft(ds, AMB, RES, 2, radius=R, shadow_rays=0), img)


# ---- 7. with a lens ----
def test_a_thin_lens_combines_with_soft_shadows(yrt, tmp_path_factory):
    K, R, s = 16, 0.5, 2
    _, ds, _, _ = built(yrt, tmp_path_factory)
    lens = dict(model="perspective", aperture=0.3, focus=9.0)
    img = yrt.raytrace_soft(ds, AMB, RES, s, radius=R, shadow_rays=K, **lens)
    cols = yrt.shade_rays_soft(ds, yrt.camera_rays(ds, RES, s, **lens), AMB, radius=R, shadow_rays=K).reshape(RES, WIDTH, s * s, 4)
    acc = np.zeros((RES, WIDTH, 3), np.float32)
    for q in range(s * s):
        acc = (acc + cols[:, :, q, :3]).astype(np.float32)
    same_bits(img[..., :3], (acc / np.float32(s * s)).astype(np.float32))
    assert (img != yrt.raytrace_soft(ds, AMB, RES, s, radius=R, shadow_rays=K)).any(), "the lens moves no pixel"


# ---- 8. the CLI ----
def test_cli_writes_the_image(yrt, tmp_path_factory):
    _, ds, path, _ = built(yrt, tmp_path_factory)
    out = tmp_path_factory.mktemp("soft_cli")
    run = lambda *a: subprocess.run([str(CLI), "-r", str(RES), "-s", "2", *a, str(path)], check=True, capture_output=True,  # noqa: E731
                                    text=True, timeout=120)
    run("-o", str(out / "hard.png"))
    run("-o", str(out / "zero.png"), "--soft-shadows", "0")
    run("-o", str(out / "soft.png"), "--soft-shadows", "0.5,16")
    assert (out / "zero.png").read_bytes() == (out / "hard.png").read_bytes()
    want = yrt.tonemap(yrt.raytrace_soft(ds, AMB, RES, 2, radius=0.5, shadow_rays=16))
    np.testing.assert_array_equal(read_png_rgba8(out / "soft.png"), want)
    assert (out / "soft.png").read_bytes() != (out / "hard.png").read_bytes()
