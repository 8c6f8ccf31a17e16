"""yrt_shade_rays on the GPU: shade() (raytrace.cpp:88-211) for caller rays, through the
wavefront pipeline's ray mode (wavefront.hip run_rays: k_rays_first, k_rays_shadow, k_rays_shade,
then the render's mirror levels) and the megakernel's one lane per ray.

The rays are the reference's own camera rays (oracle_camera_ray) of 37 x 24 frames -- 888 rays at
s = 1, 7 992 at s = 3 --, so every batch has a render to be compared with bit for bit: the batch
leaves the camera-relative records, the tile lists and the persistent grids, and must not leave
the reference's arithmetic. "built" is tests/passes_scene.py's scene with two more cameras
(tests/shade_rays_scene.py); the other scenes are golden fixtures.
"""
import numpy as np
import pytest

import passes_scene as PS
import shade_rays_scene as SS
from helpers import MIRROR_DEPTH, Oracle, assert_frame_parity, scene_path

pytestmark = pytest.mark.gpu

RES, WIDTH = SS.RES, SS.WIDTH
SCENES = ("built", "refl", "simple", "lines", "mirrors")
STAT_KEYS = ("rays", "shadow_rays", "shadow_rays_culled", "depth_truncated")
YRT_ERR_UNSUPPORTED = 3


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on the MI355X box")
    return y


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


_scenes, _rays, _shaded = {}, {}, {}


def scene(yrt, tmp_path_factory, name):
    """(the file the oracle reads, the device scene): one upload per scene"""
    if name not in _scenes:
        if name == "built":
            s = SS.build(yrt)
            path = tmp_path_factory.mktemp("shade_rays") / "built3.yrtscene"
            s.save(str(path))
        else:
            path = scene_path(name)
            s = yrt.load_scene(str(path))
        yrt.build_bvh(s)
        _scenes[name] = (s, path, s.upload(0))
    return _scenes[name][1:]


def rays_of(yrt, tmp_path_factory, name, s, camera=0):
    """shared, not to be written to"""
    key = (name, s, camera)
    if key not in _rays:
        _rays[key] = SS.camera_rays(scene(yrt, tmp_path_factory, name)[0], s, camera)
        assert _rays[key].shape == (RES * WIDTH * s * s, 8)
    return _rays[key]


def shaded(yrt, tmp_path_factory, name, s, max_depth=16):
    """(colours, stats) of the default algorithm on camera 0's rays (shared)"""
    key = (name, s, max_depth)
    if key not in _shaded:
        ds = scene(yrt, tmp_path_factory, name)[1]
        _shaded[key] = yrt.shade_rays(ds, rays_of(yrt, tmp_path_factory, name, s), PS.AMB, max_depth=max_depth,
                                      return_stats=True)
        assert _shaded[key][0].shape == (RES * WIDTH * s * s, 4) and _shaded[key][0].dtype == np.float32
    return _shaded[key]


# ---- 1. a camera's rays give that camera's render ----
@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("name", SCENES)
def test_camera_rays_equal_the_render(yrt, tmp_path_factory, name, s):
    """s = 1: the colours are the pixels. s = 3: the per-ray colours summed per pixel in float32,
    jj outer and ii inner from +0, over float32(9), are the pixels -- every sample's bits"""
    ds = scene(yrt, tmp_path_factory, name)[1]
    got, stats = shaded(yrt, tmp_path_factory, name, s)
    img, rstats = yrt.raytrace(ds, PS.AMB, RES, s, width=WIDTH, return_stats=True)
    assert (got[:, 3] == 1).all()
    assert (got[:, :3] > 0).any()
    if s == 1:
        same_bits(got.reshape(RES, WIDTH, 4), img)
    else:
        same_bits(SS.box_filter(got, s), img)
    assert {k: stats[k] for k in STAT_KEYS} == {k: rstats[k] for k in STAT_KEYS}
    assert stats["camera_samples"] == len(got) == rstats["camera_samples"]
    assert stats["rays"] > stats["camera_samples"]


# ---- 2. against the CPU restatement of the reference ----
@pytest.mark.parametrize("name", ["built", "refl"])
def test_camera_rays_equal_the_oracle(yrt, tmp_path_factory, name):
    """the bar of a frame against the oracle (helpers.assert_frame_parity): inside the oracle's
    pow envelope, the reference's bits where the envelope pins them, the count cap"""
    path = scene(yrt, tmp_path_factory, name)[0]
    want, lo, hi, nrays, _ = Oracle(path).envelope(RES, 1, amb=PS.AMB, width=WIDTH, max_depth=16)
    got, stats = shaded(yrt, tmp_path_factory, name, 1)
    got = got.reshape(RES, WIDTH, 4)
    assert_frame_parity(got, want, lo, hi, f"shaded camera rays {name}")
    assert stats["rays"] == nrays


# ---- 3. the view point is each ray's own origin ----
def test_mixed_origins_in_every_wave(yrt, tmp_path_factory):
    """three cameras' rays, shuffled so that every wave mixes the three origins: a level 0 that
    takes its view point from a camera, or one origin per wave, gets the speculars and the
    mirror directions of two cameras wrong"""
    ds = scene(yrt, tmp_path_factory, "built")[1]
    sets = [rays_of(yrt, tmp_path_factory, "built", 1, camera=k) for k in range(SS.NCAMERAS)]
    origins = {tuple(r[0, :3]) for r in sets}
    assert len(origins) == SS.NCAMERAS
    rays = np.concatenate(sets)
    n = RES * WIDTH
    assert len(rays) == 3 * n == 2664
    perm = np.random.default_rng(11).permutation(len(rays))
    for w in range(0, len(rays) - 63, 64):  # (the last, partial wave may hold fewer)
        assert len({tuple(o) for o in rays[perm[w:w + 64], :3]}) == SS.NCAMERAS, w
    got = np.empty((len(rays), 4), np.float32)
    got[perm] = yrt.shade_rays(ds, rays[perm], PS.AMB)
    frames = [yrt.raytrace(ds, PS.AMB, RES, 1, width=WIDTH, camera=k) for k in range(SS.NCAMERAS)]
    for k in range(SS.NCAMERAS):
        same_bits(got[k * n:(k + 1) * n].reshape(RES, WIDTH, 4), frames[k])
    # the three views differ, and the side view sees the mirrors' reflections
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[0], frames[2])
    refl = yrt.render_passes(ds, PS.AMB, RES, 1, width=WIDTH, camera=1, passes=("reflection",), beauty=False)
    assert (refl["reflection"][..., :3] > 0).any()


# ---- 4. batch sizes ----
def device_call(yrt, ds, rays, n, *, rows=None, stream=None, **params):
    """yrt_shade_rays on torch device tensors: the first n rays into a sentinel-filled buffer of
    n + 1 rows (or `rows`); returns the whole buffer"""
    import torch

    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).to("cuda:0")
    d_out = torch.full(((n + 1) if rows is None else rows, 4), -77.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    p = yrt.render_params(PS.AMB, **params)
    ds.shade_rays_into(p, d_rays.data_ptr(), n, d_out.data_ptr(), device_memory=True, stream=stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 888])
def test_a_prefix_of_the_batch_gives_a_prefix_of_the_colours(yrt, tmp_path_factory, n):
    """partial waves and blocks; the row after the last ray keeps its bytes"""
    ds = scene(yrt, tmp_path_factory, "built")[1]
    full, _ = shaded(yrt, tmp_path_factory, "built", 3)
    out = device_call(yrt, ds, rays_of(yrt, tmp_path_factory, "built", 3), n)
    same_bits(out[:n], full[:n])
    assert (out[n] == -77).all()
    assert ds.last_stats()["camera_samples"] == n


def test_an_empty_batch_writes_nothing_and_counts_nothing(yrt, tmp_path_factory):
    ds = scene(yrt, tmp_path_factory, "built")[1]
    rays = rays_of(yrt, tmp_path_factory, "built", 1)
    assert yrt.shade_rays(ds, rays[:5], PS.AMB, return_stats=True)[1]["rays"] > 0  # counters an empty call must not repeat
    out = device_call(yrt, ds, rays, 0, rows=3)
    assert (out == -77).all()
    assert not any(ds.last_stats().values())
    got = yrt.shade_rays(ds, np.zeros((0, 8), np.float32), PS.AMB)
    assert got.shape == (0, 4)
    assert not any(ds.last_stats().values())


# ---- 5. the ray's own tmin and tmax reach the closest-hit query ----
def test_tmin_and_tmax_clip_the_level_0_ray(yrt, tmp_path_factory):
    ds = scene(yrt, tmp_path_factory, "built")[1]
    rays = rays_of(yrt, tmp_path_factory, "built", 1)
    plain, _ = shaded(yrt, tmp_path_factory, "built", 1)
    first = yrt.intersect_first(ds, rays)
    hit, dist = first["hit"], first["dist"]
    assert 100 < hit.sum() < len(rays)
    black = np.array([0, 0, 0, 1], np.float32)

    short = rays.copy()
    short[hit, 7] = np.float32(0.5) * dist[hit]
    got = yrt.shade_rays(ds, short, PS.AMB)
    assert (got[hit] == black).all() and not got[hit][:, :3].view(np.uint32).any()
    same_bits(got[~hit], plain[~hit])

    far = rays.copy()
    far[hit, 7] = np.float32(2) * dist[hit]
    same_bits(yrt.shade_rays(ds, far, PS.AMB), plain)

    late = rays.copy()
    late[hit, 6] = np.float32(2) * dist[hit]
    gone = hit & ~yrt.intersect_first(ds, late)["hit"]
    assert gone.sum() > 50
    got = yrt.shade_rays(ds, late, PS.AMB)
    assert (got[gone] == black).all() and not got[gone][:, :3].view(np.uint32).any()
    assert (plain[gone][:, :3] > 0).any()  # (they were lit before)


# ---- 6. the algorithms ----
@pytest.mark.parametrize("algorithm", ["wavefront_lane", "megakernel"])
@pytest.mark.parametrize("name,s", [("built", 3), ("mirrors", 1)])
def test_the_other_algorithms_give_the_same_bits(yrt, tmp_path_factory, name, s, algorithm):
    ds = scene(yrt, tmp_path_factory, name)[1]
    want, wstats = shaded(yrt, tmp_path_factory, name, s)
    got, stats = yrt.shade_rays(ds, rays_of(yrt, tmp_path_factory, name, s), PS.AMB, algorithm=algorithm,
                                return_stats=True)
    same_bits(got, want)
    assert stats["rays"] == wstats["rays"] and stats["camera_samples"] == wstats["camera_samples"]
    assert stats["depth_truncated"] == wstats["depth_truncated"]


@pytest.mark.parametrize("algorithm", ["wavefront", "wavefront_lane"])
def test_the_mirror_corridor_at_its_full_depth(yrt, tmp_path_factory, algorithm):
    ds = scene(yrt, tmp_path_factory, "mirrors")[1]
    got, stats = yrt.shade_rays(ds, rays_of(yrt, tmp_path_factory, "mirrors", 1), PS.AMB, max_depth=MIRROR_DEPTH,
                                algorithm=algorithm, return_stats=True)
    img, rstats = yrt.raytrace(ds, PS.AMB, RES, 1, width=WIDTH, max_depth=MIRROR_DEPTH, return_stats=True)
    same_bits(got.reshape(RES, WIDTH, 4), img)
    assert {k: stats[k] for k in STAT_KEYS} == {k: rstats[k] for k in STAT_KEYS}
    assert stats["depth_truncated"] == 0


def test_unsupported_requests_leave_the_output_alone(yrt, tmp_path_factory):
    ds = scene(yrt, tmp_path_factory, "mirrors")[1]
    rays = rays_of(yrt, tmp_path_factory, "mirrors", 1)
    out = np.full((len(rays), 4), 33, np.float32)
    for kw in (dict(algorithm="megakernel", max_depth=17), dict(count_work=True),
               dict(count_work=True, algorithm="megakernel"), dict(count_work=True, algorithm="wavefront_lane")):
        p = yrt.render_params(PS.AMB, **kw)
        with pytest.raises(yrt.YrtError) as e:
            ds.shade_rays_into(p, rays.ctypes.data, len(rays), out.ctypes.data, device_memory=False)
        assert e.value.status == YRT_ERR_UNSUPPORTED, kw
    assert (out == 33).all()
    # the megakernel's own limit is 16 levels, which it takes
    p = yrt.render_params(PS.AMB, algorithm="megakernel", max_depth=16)
    ds.shade_rays_into(p, rays.ctypes.data, len(rays), out.ctypes.data, device_memory=False)
    same_bits(out, shaded(yrt, tmp_path_factory, "mirrors", 1)[0])


# ---- 7. max_depth cuts a path as in a render ----
def test_max_depth_truncation(yrt, tmp_path_factory):
    ds = scene(yrt, tmp_path_factory, "mirrors")[1]
    got, stats = shaded(yrt, tmp_path_factory, "mirrors", 1, max_depth=2)
    img, rstats = yrt.raytrace(ds, PS.AMB, RES, 1, width=WIDTH, max_depth=2, return_stats=True)
    same_bits(got.reshape(RES, WIDTH, 4), img)
    assert stats["depth_truncated"] == rstats["depth_truncated"] > 0
    assert {k: stats[k] for k in STAT_KEYS} == {k: rstats[k] for k in STAT_KEYS}
    deep, _ = shaded(yrt, tmp_path_factory, "mirrors", 1)
    assert not np.array_equal(deep, got)


# ---- 8. the handle's list and staging settings ----
def test_tile_lists_and_lds_staging_change_nothing(yrt, tmp_path_factory):
    path, ds = scene(yrt, tmp_path_factory, "instance1k")
    rays = rays_of(yrt, tmp_path_factory, "instance1k", 1)
    got = {}
    try:
        for mode in ("on", "off", "auto"):
            for staging in (True, False):
                ds.set_tile_lists(mode)
                ds.set_lds_staging(staging)
                got[(mode, staging)] = yrt.shade_rays(ds, rays, PS.AMB)
                tl = ds.tile_lists()
                assert (tl["camera"], tl["bundles"]) == (False, False), (mode, staging, tl)
                assert ds.lds_staging() == {"closest_hit": False, "any_hit": False}, (mode, staging)
    finally:
        ds.set_tile_lists("auto")
        ds.set_lds_staging(False)
    ref = got[("auto", False)]
    assert (ref[:, :3] > 0).any()
    for key, a in got.items():
        same_bits(a, ref)
    same_bits(ref.reshape(RES, WIDTH, 4), yrt.raytrace(ds, PS.AMB, RES, 1, width=WIDTH))


# ---- 9. renders and ray batches on one handle ----
@pytest.mark.parametrize("batch_s,frame_s", [(1, 3), (3, 1)])
def test_a_render_is_the_same_before_and_after_a_batch(yrt, tmp_path_factory, batch_s, frame_s):
    """the workspace is shared: a frame bigger than the batch, and one smaller than it"""
    ds = scene(yrt, tmp_path_factory, "built")[1]
    want, _ = shaded(yrt, tmp_path_factory, "built", batch_s)
    before, st0 = yrt.raytrace(ds, PS.AMB, RES, frame_s, width=WIDTH, return_stats=True)
    got = yrt.shade_rays(ds, rays_of(yrt, tmp_path_factory, "built", batch_s), PS.AMB)
    after, st1 = yrt.raytrace(ds, PS.AMB, RES, frame_s, width=WIDTH, return_stats=True)
    same_bits(got, want)
    same_bits(before, after)
    assert st0 == st1
    same_bits(yrt.shade_rays(ds, rays_of(yrt, tmp_path_factory, "built", batch_s), PS.AMB), want)


# ---- 10. device buffers on a caller's stream ----
def test_device_buffers_on_a_side_stream(yrt, tmp_path_factory):
    import torch

    ds = scene(yrt, tmp_path_factory, "built")[1]
    rays = rays_of(yrt, tmp_path_factory, "built", 3)
    want, _ = shaded(yrt, tmp_path_factory, "built", 3)
    st = torch.cuda.Stream(device="cuda:0")
    out = device_call(yrt, ds, rays, len(rays), stream=st.cuda_stream)
    same_bits(out[:len(rays)], want)
    assert (out[len(rays)] == -77).all()
