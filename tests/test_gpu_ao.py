"""The ambient occlusion pass on the GPU (yrt_render_ao, ao.hip k_ao) against tests/ao_model.py,
bit for bit in all four channels: the contract at one sample per pixel on a built scene with
every primitive kind and on a deep instance tree, the sample sums through the same model at
s times the frame, and windows, band shards, row stride, host planes, edge scenes, statistics,
isolation from yrt_render, repeatability and the CLI's .npy file."""
import subprocess

import numpy as np
import pytest

from ao_model import FLT_MAX, ao_model, camera_dirs
from helpers import ROOT, scene_path
from matte_model import built_scene, frame, rot_y

pytestmark = pytest.mark.gpu

CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
RES, WIDTH = 24, 37  # the AOV tests' frame: partial 8 x 8 tiles on both axes, three blocks across
ZERO_COUNTERS = ("depth_truncated", "stack_overflow", "box_tests", "instance_entries", "prim_tests", "shaded_hits",
                 "texture_lookups", "shadow_box_tests", "shadow_instance_entries", "shadow_prim_tests",
                 "wave_node_visits", "wave_prim_visits", "shadow_wave_node_visits", "shadow_rays_culled")


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on the MI355X box")
    return y


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def check_stats(st, pixels, s, K, triangle_samples):
    """the statistics identities of yrt_render_ao"""
    assert st["camera_samples"] == pixels * s * s
    assert st["shadow_rays"] == K * triangle_samples
    assert st["rays"] == st["camera_samples"] + st["shadow_rays"]
    for name in ZERO_COUNTERS:
        assert st[name] == 0, name


_scenes = {}


def golden(yrt, name):
    """(Scene, DeviceScene) of a golden scene"""
    if name not in _scenes:
        s = yrt.load_scene(str(scene_path(name)))
        yrt.build_bvh(s)
        _scenes[name] = (s, s.upload(0))
    return _scenes[name]


def built(yrt, tmp_path_factory):
    """a copy of the built scene of tests/matte_model.py (every primitive kind, rotated instances,
    perturbed normals) with two more instances: the quad again, standing on the floor and turned away
    from the camera, so that the camera sees the side its normals point away from; and a small
    plate in front of the floor's near edge, tilted 45 degrees towards the camera, whose hemisphere
    nothing reaches (on the bumpy floor a ray close to the horizon always finds the floor again)"""
    if "built" not in _scenes:
        b = built_scene(yrt, tmp_path_factory)
        s = yrt.load_scene(str(b.path))
        quad, m_floor = b.insts[4]
        assert s.add_instance(frame(rot_y(np.pi + 0.5), (2.4, 0.2, 1.0)), quad, m_floor) == len(b.insts)
        h = np.float32(np.sqrt(0.5))
        plate = s.add_shape(np.array([[-.3, 0, 0], [.3, 0, 0], [.3, .6, 0], [-.3, .6, 0]], np.float32),
                            norm=np.tile(np.array([[0, 0, 1]], np.float32), (4, 1)), texcoord=np.zeros((4, 2), np.float32),
                            triangles=np.array([[0, 1, 2], [0, 2, 3]], np.int32))
        tilt = np.array([[1, 0, 0], [0, h, -h], [0, h, h]], np.float32)
        assert s.add_instance(frame(tilt, (-1.0, 1.3, 4.6)), plate, m_floor) == len(b.insts) + 1
        path = tmp_path_factory.mktemp("ao") / "built_ao.yrtscene"
        s.save(str(path))
        yrt.build_bvh(s)
        _scenes["built"] = (s, s.upload(0), path)
    return _scenes["built"]


# ---- 1. the contract at one sample per pixel ----
@pytest.mark.parametrize("bias", [0.01, 0.25])
@pytest.mark.parametrize("distance", [float(FLT_MAX), 1.5])
@pytest.mark.parametrize("K", [1, 16, 64])
def test_one_sample_equals_the_model(yrt, tmp_path_factory, K, distance, bias):
    s, ds, path = built(yrt, tmp_path_factory)
    m = ao_model(yrt, ds, s, path, RES, WIDTH, K, distance, bias, key="built")
    a, w = m["plane"][..., 0], m["plane"][..., 3]
    # what the expected plane must contain for the comparison to mean something
    assert ((a == 1) & (w == 1) & m["tri"]).any(), "no open triangle pixel"
    if K > 1:  # (one ray per pixel is occluded or not)
        assert ((a > 0) & (a < w)).any(), "no partly occluded pixel"
    else:
        assert ((a == 0) & (w == 1)).any(), "no occluded pixel"
    assert ((m["kind"] == 1) & (a == w)).any() and ((m["kind"] == 2) & (a == w)).any(), "no line or point hit"
    assert m["flip"].any() and (m["tri"] & ~m["flip"]).any(), "the face-forward flip did not fire, or always did"
    assert (w == 0).any()
    got, st = yrt.render_ao(ds, RES, 1, rays=K, distance=distance, bias=bias, width=WIDTH, return_stats=True)
    print(f"K={K} distance={distance:g} bias={bias}: {np.sum(got.view(np.uint32) != m['plane'].view(np.uint32))} "
          f"channels differ; open share {m['count'][m['tri']].mean() / K:.3f}, flipped {m['flip'].sum()} pixels")
    same_bits(got, m["plane"])
    check_stats(st, RES * WIDTH, 1, K, int(m["tri"].sum()))


# ---- 2. a deep instance tree, identity frames, the wide walk's instance entries ----
def test_instance1k_equals_the_model(yrt):
    s, ds = golden(yrt, "instance1k")
    m = ao_model(yrt, ds, s, scene_path("instance1k"), RES, WIDTH, 16, float(FLT_MAX), 0.01)
    a, w = m["plane"][..., 0], m["plane"][..., 3]
    assert m["tri"].any() and ((a > 0) & (a < w)).any()
    got, st = yrt.render_ao(ds, RES, 1, rays=16, width=WIDTH, return_stats=True)
    same_bits(got, m["plane"])
    check_stats(st, RES * WIDTH, 1, 16, int(m["tri"].sum()))


# ---- 3. the sample sums, grounded through the model at s times the frame ----
@pytest.mark.parametrize("s", [2, 4])
def test_sample_sums_equal_the_model_at_the_larger_frame(yrt, tmp_path_factory, s):
    """sample (ii, jj) of pixel (i, j) is pixel (s i + ii, s j + jj) of the one-sample frame at
    resolution s and width s times as large, ray for ray (both operands of the divisions scale by
    a power of two); only the rotation index differs, so the model takes the small frame's"""
    K = 16
    hs, ds, path = built(yrt, tmp_path_factory)
    small, large = camera_dirs(path, RES, WIDTH, s), camera_dirs(path, RES * s, WIDTH * s)[0, 0]
    j, i = np.mgrid[0:RES, 0:WIDTH]
    r = np.zeros((RES * s, WIDTH * s), np.int64)
    for jj in range(s):
        for ii in range(s):
            np.testing.assert_array_equal(small[jj, ii].view(np.uint32), large[jj::s, ii::s].view(np.uint32))
            r[jj::s, ii::s] = ((i & 3) | (j & 3) << 2) ^ ((jj * s + ii) & 15)
    m = ao_model(yrt, ds, hs, path, RES * s, WIDTH * s, K, 1.5, 0.01, r=r, key="built")
    U = sum(m["count"][jj::s, ii::s] for jj in range(s) for ii in range(s))
    hits = sum(m["hit"][jj::s, ii::s].astype(np.int64) for jj in range(s) for ii in range(s))
    a = (U.astype(np.float32) / np.float32(K * s * s)).astype(np.float32)
    want = np.stack([a, a, a, (hits.astype(np.float32) / np.float32(s * s)).astype(np.float32)], -1)
    assert ((hits > 0) & (hits < s * s)).any() and ((U > 0) & (U < K * hits)).any()
    got, st = yrt.render_ao(ds, RES, s, rays=K, distance=1.5, bias=0.01, width=WIDTH, return_stats=True)
    np.testing.assert_array_equal(np.round(got[..., 0].astype(np.float64) * (K * s * s)).astype(np.int64), U)
    same_bits(got, want)
    check_stats(st, RES * WIDTH, s, K, int(m["tri"].sum()))


def test_three_samples_per_axis_keep_the_invariants(yrt, tmp_path_factory):
    s, K = 3, 16
    _, ds, _ = built(yrt, tmp_path_factory)
    got, st = yrt.render_ao(ds, RES, s, rays=K, distance=1.5, width=WIDTH, return_stats=True)
    depth = yrt.render_aovs(ds, RES, s, width=WIDTH, aovs=("depth",))["depth"]
    a, w = got[..., 0], got[..., 3]
    np.testing.assert_array_equal(w.view(np.uint32), depth[..., 3].view(np.uint32))
    same_bits(got[..., 1], a), same_bits(got[..., 2], a)
    assert (a >= 0).all() and (a <= w).all() and ((a > 0) & (a < w)).any()
    U = a.astype(np.float64) * (K * s * s)
    np.testing.assert_allclose(U, np.round(U), rtol=0, atol=1e-3)
    U = np.round(U).astype(np.int64)
    same_bits((U.astype(np.float32) / np.float32(K * s * s)).astype(np.float32), a)
    assert st["camera_samples"] == RES * WIDTH * s * s and st["rays"] == st["camera_samples"] + st["shadow_rays"]
    hits = int(np.round(w.astype(np.float64) * (s * s)).sum())
    assert st["shadow_rays"] % K == 0 and 0 < st["shadow_rays"] // K <= hits
    for name in ZERO_COUNTERS:
        assert st[name] == 0, name


# ---- 4. windows, bands, stride, host and device planes, edges, statistics ----
S4, K4, D4 = 2, 4, 1.5  # the frame of section 4, on `simple`


def triangle_samples(yrt, res, window=None):
    """the camera samples of section 4's frame that hit a triangle, from the shape matte's counts"""
    hs, ds = golden(yrt, "simple")
    m = yrt.render_mattes(ds, res, S4, keys=("shape",), ranks=8, width=WIDTH, window=window)
    assert m["dropped"]["shape"] == 0
    ids, counts = m["shape"]["ids"], np.round(m["shape"]["coverage"].astype(np.float64) * S4 * S4).astype(np.int64)
    kinds = np.asarray(hs.shape_kinds())
    return int(counts[(ids >= 0) & (kinds[np.maximum(ids, 0)] == 0)].sum())


def full_plane(yrt):
    if "full" not in _scenes:
        ds = golden(yrt, "simple")[1]
        img, st = yrt.render_ao(ds, RES, S4, rays=K4, distance=D4, width=WIDTH, return_stats=True)
        assert ((img[..., 0] > 0) & (img[..., 0] < img[..., 3])).any()
        check_stats(st, RES * WIDTH, S4, K4, triangle_samples(yrt, RES))
        img.setflags(write=False)
        _scenes["full"] = img
    return _scenes["full"]


def test_window_equals_the_crop(yrt):
    full = full_plane(yrt)
    ds = golden(yrt, "simple")[1]
    win, st = yrt.render_ao(ds, RES, S4, rays=K4, distance=D4, width=WIDTH, window=(5, 3, 19, 11), return_stats=True)
    same_bits(win, np.ascontiguousarray(full[3:14, 5:24]))
    check_stats(st, 19 * 11, S4, K4, triangle_samples(yrt, RES, window=(5, 3, 19, 11)))


@pytest.mark.parametrize("res,band", [(24, 8), (24, 3), (20, 8), (20, 3)])
def test_band_shards_reassemble(yrt, res, band):
    """shards of stride 3 at every offset; 20 rows end in a partial band of 4 (band 8) or 2 (band 3)"""
    ds = golden(yrt, "simple")[1]
    full = full_plane(yrt) if res == RES else yrt.render_ao(ds, res, S4, rays=K4, distance=D4, width=WIDTH)
    got = np.full_like(full, 77)
    seen = np.zeros(res, int)
    cast = 0
    for off in range(3):
        p = yrt.render_params(resolution=res, samples=S4, width=WIDTH, band=(band, 3, off))
        th = len(range(off, -(-res // band), 3)) * band
        plane = np.full((th, WIDTH, 4), 55, np.float32)
        ds.render_ao_into(p, plane.ctypes.data, K4, D4, device_memory=False)
        rows = 0
        for ly in range(th):
            j = ((ly // band) * 3 + off) * band + ly % band
            if j < res:
                seen[j] += 1
                rows += 1
                got[j] = plane[ly]
            else:  # local rows past the image edge (the partial last band) read as zeros
                assert not plane[ly].view(np.uint32).any()
        st = ds.last_stats()
        check_stats(st, rows * WIDTH, S4, K4, st["shadow_rays"] // K4)
        assert st["shadow_rays"] % K4 == 0
        cast += st["shadow_rays"]
    assert (seen == 1).all() and cast == K4 * triangle_samples(yrt, res)
    same_bits(got, np.asarray(full))


def test_row_padding_is_not_written_and_host_equals_device(yrt):
    import torch

    full = full_plane(yrt)
    ds = golden(yrt, "simple")[1]
    x0, y0, tw, th = 5, 3, 19, 11
    stride = tw + 5
    p = yrt.render_params(resolution=RES, samples=S4, width=WIDTH, window=(x0, y0, tw, th))
    p.out_stride = stride
    dev = torch.full((th, stride, 4), float("nan"), dtype=torch.float32, device="cuda:0")
    nan_bits = dev[0, 0, 0].cpu().numpy().view(np.uint32)
    torch.cuda.synchronize()
    ds.render_ao_into(p, dev.data_ptr(), K4, D4, device_memory=True)
    torch.cuda.synchronize()
    host = np.zeros((th, stride, 4), np.float32)
    host.view(np.uint32)[...] = 0x7fc01234  # the caller's bytes of a host plane's padding
    ds.render_ao_into(p, host.ctypes.data, K4, D4, device_memory=False)
    check_stats(ds.last_stats(), tw * th, S4, K4, triangle_samples(yrt, RES, window=(x0, y0, tw, th)))
    a = dev.cpu().numpy()
    want = np.ascontiguousarray(full[y0:y0 + th, x0:x0 + tw])
    assert (a[:, tw:].view(np.uint32) == nan_bits).all() and (host[:, tw:].view(np.uint32) == 0x7fc01234).all()
    same_bits(np.ascontiguousarray(a[:, :tw]), want)
    same_bits(np.ascontiguousarray(host[:, :tw]), want)


def test_device_plane_equals_host_plane(yrt):
    import torch

    dev = torch.zeros((RES, WIDTH, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    p = yrt.render_params(resolution=RES, samples=S4, width=WIDTH)
    ds = golden(yrt, "simple")[1]
    ds.render_ao_into(p, dev.data_ptr(), K4, D4, device_memory=True)
    torch.cuda.synchronize()
    check_stats(ds.last_stats(), RES * WIDTH, S4, K4, triangle_samples(yrt, RES))
    same_bits(dev.cpu().numpy(), np.asarray(full_plane(yrt)))


def test_empty_band_offset_writes_nothing_and_counts_nothing(yrt):
    ds = golden(yrt, "simple")[1]
    res = 12
    _, st = yrt.render_ao(ds, res, S4, rays=K4, width=WIDTH, return_stats=True)
    assert st["camera_samples"] == WIDTH * res * S4 * S4 and st["shadow_rays"] > 0
    # 12 rows are two bands of 8: offset 2 of 3 has none
    p = yrt.render_params(resolution=res, samples=S4, width=WIDTH, band=(8, 3, 2))
    plane = np.full((8, WIDTH, 4), 77, np.float32)
    ds.render_ao_into(p, plane.ctypes.data, K4, device_memory=False)
    st = ds.last_stats()
    assert st["rays"] == 0 and st["camera_samples"] == 0 and st["shadow_rays"] == 0
    assert (plane == 77).all()


@pytest.mark.parametrize("name", ["edge_sky", "edge_empty"])
def test_scenes_where_every_ray_misses(yrt, name):
    img, st = yrt.render_ao(golden(yrt, name)[1], 12, 2, width=19, return_stats=True)
    same_bits(img, np.zeros((12, 19, 4), np.float32))
    check_stats(st, 12 * 19, 2, 16, 0)


def test_the_pass_leaves_yrt_render_alone(yrt):
    ds = golden(yrt, "simple")[1]
    before = yrt.raytrace(ds, (0.1, 0.1, 0.1), RES, 3)
    lists = ds.tile_lists()
    yrt.render_ao(ds, RES, 3, rays=K4)
    assert ds.tile_lists() == lists
    after = yrt.raytrace(ds, (0.1, 0.1, 0.1), RES, 3)
    same_bits(after, before)


def test_two_runs_give_the_same_bits(yrt, tmp_path_factory):
    _, ds, _ = built(yrt, tmp_path_factory)
    one = yrt.render_ao(ds, RES, 3, rays=64, distance=2.0, width=WIDTH)
    two = yrt.render_ao(ds, RES, 3, rays=64, distance=2.0, width=WIDTH)
    assert ((one[..., 0] > 0) & (one[..., 0] < one[..., 3])).any()
    same_bits(one, two)


def test_cli_writes_the_npy_file(yrt, tmp_path):
    out = tmp_path / "o.png"
    r = subprocess.run([str(CLI), "--ao", "8,1.5,0.25", "-r", "36", "-s", "2", "-o", str(out), str(scene_path("simple"))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    a = np.load(tmp_path / "o.ao.npy")
    assert a.flags["C_CONTIGUOUS"] and a.dtype == np.dtype("<f4")
    same_bits(a, yrt.render_ao(golden(yrt, "simple")[1], 36, 2, rays=8, distance=1.5, bias=0.25))


# ---- 5. an unbounded distance ----
def test_infinite_distance_is_flt_max(yrt, tmp_path_factory):
    _, ds, _ = built(yrt, tmp_path_factory)
    inf = yrt.render_ao(ds, RES, 2, rays=16, distance=float("inf"), width=WIDTH)
    assert ((inf[..., 0] > 0) & (inf[..., 0] < inf[..., 3])).any()
    same_bits(inf, yrt.render_ao(ds, RES, 2, rays=16, distance=float(FLT_MAX), width=WIDTH))
