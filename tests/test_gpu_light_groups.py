"""Light groups on the GPU (yrt_render_light_groups; wavefront.hip k_shade_groups and
k_accumulate_groups) on 37 x 24 frames: partial 8 x 8 tiles on both axes. Without mirrors s = 1
and 2 take the fused shape and s = 3 the unfused one; with mirrors every s takes the mirror
levels. The five-light scene (light_groups_scene.py) takes the kernels that read occlusion
bytes per light, passes_scene's two lights the ones that load them with the surface.

A group's plane is the beauty of the scene variant that keeps the group's lights, rendered with
ambient 0: helpers.assert_frame_parity against the oracle's (the device pow) and bit-equal to the
GPU's own render of the uploaded variant. The ambient plane is the variant without lights,
rendered with the ambient: bit-equal to both (no pow). The beauty is yrt.raytrace's, with its
counters. Then the depth cut, the recomposition on the file fixtures, and the plumbing.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import light_groups_scene as LS
import passes_scene as PS
from helpers import MIRROR_DEPTH, ROOT, Oracle, assert_frame_parity, assert_same_floats, scene_path

pytestmark = pytest.mark.gpu

CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
RES, WIDTH = 24, 37
STAT_KEYS = ("rays", "camera_samples", "shadow_rays", "shadow_rays_culled", "depth_truncated")
YRT_ERR_INVALID_ARG, YRT_ERR_UNSUPPORTED = 1, 3
# name -> (more_lights, group_of)
SETUPS = {"five": (True, LS.GROUP_OF), "two-split": (False, [0, 1]), "two-merged": (False, [0, 0])}


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on the MI355X box")
    return y


def same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


_built, _files, _oracle, _groups = {}, {}, {}, {}


def built(yrt, tmp_path_factory, more, mirrors, lit=None):
    """(host scene, its .yrtscene file, device scene) of a variant of the built scene"""
    key = (more, mirrors, None if lit is None else tuple(lit))
    if key not in _built:
        s = LS.build(yrt, lit=lit, mirrors=mirrors, more_lights=more)
        path = tmp_path_factory.mktemp("light_groups") / "variant.yrtscene"
        s.save(str(path))
        yrt.build_bvh(s)
        _built[key] = (s, path, s.upload(0))
    return _built[key]


def file_scene(yrt, name):
    if name not in _files:
        s = yrt.load_scene(str(scene_path(name)))
        yrt.build_bvh(s)
        _files[name] = (s, s.upload(0))
    return _files[name]


def oracle_variant(yrt, tmp_path_factory, more, mirrors, lit, s, amb):
    """the oracle's beauty of a variant and its pow envelope (helpers.Oracle.envelope):
    (ref, lo, hi)"""
    key = (more, mirrors, tuple(lit), s, amb)
    if key not in _oracle:
        img, lo, hi, _, _ = Oracle(built(yrt, tmp_path_factory, more, mirrors, lit)[1]).envelope(
            RES, s, amb=amb, width=WIDTH, max_depth=16)
        assert img.shape == (RES, WIDTH, 4) and np.isfinite(img).all()
        _oracle[key] = (img, lo, hi)
    return _oracle[key]


def groups(yrt, tmp_path_factory, setup, mirrors, s, max_depth=16):
    """the planes of one render (shared: not to be written to) and the counters after it"""
    key = (setup, mirrors, s, max_depth)
    if key not in _groups:
        more, group_of = SETUPS[setup]
        ds = built(yrt, tmp_path_factory, more, mirrors)[2]
        out = yrt.render_light_groups(ds, PS.AMB, RES, s, groups=group_of, width=WIDTH, max_depth=max_depth)
        assert set(out) == {"groups", "ambient", "beauty"} and len(out["groups"]) == max(group_of) + 1
        for a in (*out["groups"], out["ambient"], out["beauty"]):
            assert a.shape == (RES, WIDTH, 4) and a.dtype == np.float32
        _groups[key] = (out, ds.last_stats())
    return _groups[key]


CASES = [(setup, mirrors, s) for setup in SETUPS for mirrors in (True, False) for s in (1, 2, 3)]


# ---- 1. each plane against the variant scene ----
@pytest.mark.parametrize("setup,mirrors,s", CASES)
def test_each_plane_is_the_beauty_of_its_variant(yrt, tmp_path_factory, setup, mirrors, s):
    more, group_of = SETUPS[setup]
    out, _ = groups(yrt, tmp_path_factory, setup, mirrors, s)
    lit_pixels = []
    for g, plane in enumerate(out["groups"]):
        lit = LS.lights_of(group_of, g)
        want, lo, hi = oracle_variant(yrt, tmp_path_factory, more, mirrors, lit, s, 0.0)
        assert_frame_parity(plane, want, lo, hi, f"light groups {setup} mirrors={mirrors} s={s} group {g}")
        gpu = yrt.raytrace(built(yrt, tmp_path_factory, more, mirrors, lit)[2], (0.0, 0.0, 0.0), RES, s, width=WIDTH)
        same_bits(plane, gpu)
        lit_pixels.append(int((plane[..., :3] > 0).any(axis=-1).sum()))
    assert min(lit_pixels) >= 100, lit_pixels  # every group lights a good part of the frame
    for a in range(len(out["groups"])):  # and no two planes are one image
        for b in range(a):
            assert (out["groups"][a] != out["groups"][b]).any(axis=-1).sum() >= 100, (a, b)
    want = oracle_variant(yrt, tmp_path_factory, more, mirrors, (), s, PS.AMB)[0]
    assert_same_floats(out["ambient"], want)
    same_bits(out["ambient"], yrt.raytrace(built(yrt, tmp_path_factory, more, mirrors, ())[2], PS.AMB, RES, s, width=WIDTH))
    assert (out["ambient"][..., :3] > 0).any()


# ---- 2. the beauty and the counters ----
@pytest.mark.parametrize("setup,mirrors,s", CASES)
def test_beauty_and_counters_are_raytraces(yrt, tmp_path_factory, setup, mirrors, s):
    out, stats = groups(yrt, tmp_path_factory, setup, mirrors, s)
    ds = built(yrt, tmp_path_factory, SETUPS[setup][0], mirrors)[2]
    img, rstats = yrt.raytrace(ds, PS.AMB, RES, s, width=WIDTH, return_stats=True)
    same_bits(out["beauty"], img)
    assert {k: stats[k] for k in STAT_KEYS} == {k: rstats[k] for k in STAT_KEYS}
    assert stats["shadow_rays"] > 0
    for a in (*out["groups"], out["ambient"]):
        same_bits(a[..., 3], img[..., 3])
    assert (img[..., 3] == 1).all()
    # and the image is what it was before the call
    same_bits(yrt.raytrace(ds, PS.AMB, RES, s, width=WIDTH), img)


# ---- 3. the depth cut ----
@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("max_depth", [1, 2])
def test_depth_cut_planes_are_the_variants_at_that_depth(yrt, tmp_path_factory, max_depth, s):
    """0 * kr where max_depth cuts the mirror ray, and depth_truncated counted once, not per plane"""
    out, stats = groups(yrt, tmp_path_factory, "five", True, s, max_depth)
    for g, plane in enumerate(out["groups"]):
        ds = built(yrt, tmp_path_factory, True, True, LS.lights_of(LS.GROUP_OF, g))[2]
        same_bits(plane, yrt.raytrace(ds, (0.0, 0.0, 0.0), RES, s, width=WIDTH, max_depth=max_depth))
    ds = built(yrt, tmp_path_factory, True, True, ())[2]
    same_bits(out["ambient"], yrt.raytrace(ds, PS.AMB, RES, s, width=WIDTH, max_depth=max_depth))
    img, rstats = yrt.raytrace(built(yrt, tmp_path_factory, True, True)[2], PS.AMB, RES, s, width=WIDTH,
                               max_depth=max_depth, return_stats=True)
    same_bits(out["beauty"], img)
    assert {k: stats[k] for k in STAT_KEYS} == {k: rstats[k] for k in STAT_KEYS}
    if max_depth == 1:  # every mirror the camera sees is cut (at depth 2 only a mirror seen in a mirror is)
        assert stats["depth_truncated"] > 0
        deep, _ = groups(yrt, tmp_path_factory, "five", True, s)
        assert any((a != b).any() for a, b in zip(out["groups"], deep["groups"]))


# ---- 4. the planes add up to the beauty (file fixtures: no variants) ----
@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name,depth", [("refl", 16), ("mirrors", MIRROR_DEPTH), ("instance1k", 16)])
def test_planes_add_up_to_the_beauty_within_the_rounding(yrt, name, depth, s):
    """The image is linear in each ke and in the ambient, so in exact arithmetic the planes add
    up to the beauty. In float32 every term of a plane or of the beauty is non-negative and
    reaches its pixel through at most N operations of relative error 2^-24 each: the nl
    additions of its level's light loop, three per mirror level at or above it (* kr, + c, + la),
    the s*s additions of the pixel and the division. (ld + ls itself is the same float in a plane
    and in the beauty.) With a factor 2 of slack, on the sum of both sides."""
    host, ds = file_scene(yrt, name)
    nl = len(host.lights())
    assert nl >= 1
    group_of = [k % 8 for k in range(nl)]
    out = yrt.render_light_groups(ds, PS.AMB, RES, s, groups=group_of, width=WIDTH, max_depth=depth)
    assert len(out["groups"]) == min(nl, 8)
    st = ds.last_stats()
    img, rstats = yrt.raytrace(ds, PS.AMB, RES, s, width=WIDTH, max_depth=depth, return_stats=True)
    same_bits(out["beauty"], img)
    planes = [a[..., :3].astype(np.float64) for a in (*out["groups"], out["ambient"])]
    beauty = img[..., :3].astype(np.float64)
    assert all(np.isfinite(a).all() and (a >= 0).all() for a in (*planes, beauty)), "the bound is for non-negative terms"
    total = sum(planes)
    n = nl + 3 * depth + s * s + 1
    err, bound = np.abs(beauty - total), 2 * n * 2.0 ** -24 * (beauty + total)
    print(f"{name} s={s}: {nl} lights, N = {n}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert (err <= bound).all()
    assert (total > 0).any()
    assert {k: st[k] for k in STAT_KEYS} == {k: rstats[k] for k in STAT_KEYS}


# ---- 5. plumbing ----
SHAPES = [(True, 2), (False, 2), (False, 3)]  # mirror levels, fused, unfused


def all_planes(out):
    return [*out["groups"], out["ambient"], out["beauty"]]


@pytest.mark.parametrize("mirrors,s", SHAPES)
def test_window_equals_the_crop(yrt, tmp_path_factory, mirrors, s):
    full, _ = groups(yrt, tmp_path_factory, "five", mirrors, s)
    x0, y0, tw, th = 3, 5, 21, 13  # not tile-aligned
    win = yrt.render_light_groups(built(yrt, tmp_path_factory, True, mirrors)[2], PS.AMB, RES, s, groups=LS.GROUP_OF,
                                  width=WIDTH, window=(x0, y0, tw, th))
    for a, b in zip(all_planes(win), all_planes(full)):
        same_bits(a, np.ascontiguousarray(b[y0:y0 + th, x0:x0 + tw]))


@pytest.mark.parametrize("mirrors,s", SHAPES)
def test_band_shards_reassemble_and_an_empty_shard_writes_nothing(yrt, tmp_path_factory, mirrors, s):
    full, _ = groups(yrt, tmp_path_factory, "five", mirrors, s)
    ds = built(yrt, tmp_path_factory, True, mirrors)[2]
    got = [np.full((RES, WIDTH, 4), np.nan, np.float32) for _ in range(LS.NGROUPS + 2)]
    band, stride = 8, 2
    for off in range(stride):
        p = yrt.render_params(PS.AMB, RES, s, width=WIDTH, band=(band, stride, off))
        th = len(range(off, -(-RES // band), stride)) * band
        planes = [np.full((th, WIDTH, 4), np.nan, np.float32) for _ in got]
        ds.render_light_groups_into(p, LS.GROUP_OF, [a.ctypes.data for a in planes[:LS.NGROUPS]],
                                    ambient_ptr=planes[-2].ctypes.data, beauty_ptr=planes[-1].ctypes.data,
                                    device_memory=False)
        for ly in range(th):
            j = ((ly // band) * stride + off) * band + ly % band
            assert j < RES
            for a, b in zip(got, planes):
                a[j] = b[ly]
    for a, b in zip(got, all_planes(full)):
        same_bits(a, b)
    assert ds.last_stats()["rays"] > 0  # the counters an empty call must not repeat
    p = yrt.render_params(PS.AMB, RES, s, width=WIDTH, band=(8, 4, 3))  # three bands of 8: offset 3 of 4 has none
    planes = [np.full((8, WIDTH, 4), 77, np.float32) for _ in got]
    ds.render_light_groups_into(p, LS.GROUP_OF, [a.ctypes.data for a in planes[:LS.NGROUPS]],
                                ambient_ptr=planes[-2].ctypes.data, beauty_ptr=planes[-1].ctypes.data, device_memory=False)
    assert all((a == 77).all() for a in planes)
    st = ds.last_stats()
    assert st["rays"] == 0 and st["camera_samples"] == 0


@pytest.mark.parametrize("mirrors,s", SHAPES)
@pytest.mark.parametrize("device_memory", [True, False])
def test_row_padding_is_not_written(yrt, tmp_path_factory, mirrors, s, device_memory):
    """out_stride, and with device planes a stream of the caller's"""
    import torch

    full, _ = groups(yrt, tmp_path_factory, "five", mirrors, s)
    x0, y0, tw, th = 3, 5, 21, 13
    stride = tw + 5
    p = yrt.render_params(PS.AMB, RES, s, width=WIDTH, window=(x0, y0, tw, th))
    p.out_stride = stride
    ds = built(yrt, tmp_path_factory, True, mirrors)[2]
    n = LS.NGROUPS + 2
    if device_memory:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            dev = [torch.full((th, stride, 4), -77.0, dtype=torch.float32, device="cuda:0") for _ in range(n)]
            ptr = [a.data_ptr() for a in dev]
            ds.render_light_groups_into(p, LS.GROUP_OF, ptr[:LS.NGROUPS], ambient_ptr=ptr[-2], beauty_ptr=ptr[-1],
                                        device_memory=True, stream=stream.cuda_stream)
            host = [a.cpu().numpy() for a in dev]  # (on the same stream: behind the render)
        stream.synchronize()
    else:
        host = [np.full((th, stride, 4), -77, np.float32) for _ in range(n)]
        ptr = [a.ctypes.data for a in host]
        ds.render_light_groups_into(p, LS.GROUP_OF, ptr[:LS.NGROUPS], ambient_ptr=ptr[-2], beauty_ptr=ptr[-1],
                                    device_memory=False)
    for a, b in zip(host, all_planes(full)):
        assert (a[:, tw:] == -77).all()
        same_bits(np.ascontiguousarray(a[:, :tw]), np.ascontiguousarray(b[y0:y0 + th, x0:x0 + tw]))


@pytest.mark.parametrize("mirrors,s", SHAPES)
def test_optional_planes_empty_groups_and_ungrouped_lights(yrt, tmp_path_factory, mirrors, s):
    full, stats = groups(yrt, tmp_path_factory, "five", mirrors, s)
    ds = built(yrt, tmp_path_factory, True, mirrors)[2]
    black = np.zeros((RES, WIDTH, 4), np.float32)
    black[..., 3] = 1
    out = yrt.render_light_groups(ds, PS.AMB, RES, s, groups=LS.GROUP_OF, width=WIDTH, ambient=False, beauty=False)
    assert list(out) == ["groups"]
    for a, b in zip(out["groups"], full["groups"]):
        same_bits(a, b)
    assert {k: ds.last_stats()[k] for k in STAT_KEYS} == {k: stats[k] for k in STAT_KEYS}
    out = yrt.render_light_groups(ds, PS.AMB, RES, s, groups=LS.GROUP_OF, width=WIDTH, beauty=False)
    assert list(out) == ["groups", "ambient"]
    same_bits(out["ambient"], full["ambient"])
    # group 1 empty; the others as before
    out = yrt.render_light_groups(ds, PS.AMB, RES, s, groups=[0, 2, 0, -1, 3], width=WIDTH)
    assert len(out["groups"]) == 4
    for g, base in ((0, 0), (2, 1), (3, 2)):
        same_bits(out["groups"][g], full["groups"][base])
    same_bits(out["groups"][1], black)
    same_bits(out["beauty"], full["beauty"])
    # no light in any plane: every shadow ray is still walked, the beauty still has every light
    out = yrt.render_light_groups(ds, PS.AMB, RES, s, groups=[-1] * 5, width=WIDTH)
    assert len(out["groups"]) == 1
    same_bits(out["groups"][0], black)
    same_bits(out["ambient"], full["ambient"])
    same_bits(out["beauty"], full["beauty"])
    assert {k: ds.last_stats()[k] for k in STAT_KEYS} == {k: stats[k] for k in STAT_KEYS}


@pytest.mark.parametrize("s", [2, 3])
def test_a_scene_without_lights(yrt, tmp_path_factory, s):
    ds = built(yrt, tmp_path_factory, True, True, ())[2]
    out = yrt.render_light_groups(ds, PS.AMB, RES, s, groups=[], width=WIDTH)
    black = np.zeros((RES, WIDTH, 4), np.float32)
    black[..., 3] = 1
    assert len(out["groups"]) == 1
    same_bits(out["groups"][0], black)
    img = yrt.raytrace(ds, PS.AMB, RES, s, width=WIDTH)
    same_bits(out["ambient"], img)
    same_bits(out["beauty"], img)


def test_tile_lists_on_and_off_give_the_same_planes(yrt):
    host, ds = file_scene(yrt, "instance1k")
    group_of = [k % 8 for k in range(len(host.lights()))]
    got = {}
    try:
        for mode in ("on", "off"):
            ds.set_tile_lists(mode)
            got[mode] = yrt.render_light_groups(ds, PS.AMB, RES, 3, groups=group_of, width=WIDTH)
            tl = ds.tile_lists()
            assert (tl["camera"], tl["bundles"]) == ((True, True) if mode == "on" else (False, False)), tl
    finally:
        ds.set_tile_lists("auto")
    for a, b in zip(all_planes(got["on"]), all_planes(got["off"])):
        same_bits(a, b)
    same_bits(got["on"]["beauty"], yrt.raytrace(ds, PS.AMB, RES, 3, width=WIDTH))


@pytest.mark.parametrize("mirrors,s", SHAPES)
def test_the_lane_algorithm_gives_the_same_planes(yrt, tmp_path_factory, mirrors, s):
    full, _ = groups(yrt, tmp_path_factory, "five", mirrors, s)
    lane = yrt.render_light_groups(built(yrt, tmp_path_factory, True, mirrors)[2], PS.AMB, RES, s, groups=LS.GROUP_OF,
                                   width=WIDTH, algorithm="wavefront_lane")
    for a, b in zip(all_planes(lane), all_planes(full)):
        same_bits(a, b)


def test_what_the_call_refuses_on_a_real_handle(yrt, tmp_path_factory):
    ds = built(yrt, tmp_path_factory, True, True)[2]
    planes = [np.full((RES, WIDTH, 4), 33, np.float32) for _ in range(LS.NGROUPS)]
    ptr = [a.ctypes.data for a in planes]
    for kw in (dict(algorithm="megakernel"), dict(count_work=True)):
        p = yrt.render_params(PS.AMB, RES, 1, width=WIDTH, **kw)
        with pytest.raises(yrt.YrtError) as e:
            ds.render_light_groups_into(p, LS.GROUP_OF, ptr, device_memory=False)
        assert e.value.status == YRT_ERR_UNSUPPORTED, kw
    p = yrt.render_params(PS.AMB, RES, 1, width=WIDTH)
    for wrong in ([0, 1, 0, -1], [0, 1, 0, -1, 2, 2]):  # not the scene's five lights
        with pytest.raises(yrt.YrtError) as e:
            ds.render_light_groups_into(p, wrong, ptr, device_memory=False)
        assert e.value.status == YRT_ERR_INVALID_ARG, wrong
    assert all((a == 33).all() for a in planes)


# ---- 6. the CLI ----
def test_cli_writes_the_planes_and_the_same_image(yrt, tmp_path_factory):
    d = tmp_path_factory.mktemp("light_groups_cli")
    _, path, _ = built(yrt, tmp_path_factory, True, True)
    common = ["-r", str(RES), "--width", str(WIDTH), "-s", "2", "-a", str(PS.AMB)]
    r = subprocess.run([str(CLI), *common, "-o", str(d / "plain.hdr"), str(path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(CLI), *common, "--light-groups", ",".join(map(str, LS.GROUP_OF)), "-o", str(d / "out.hdr"),
                        str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (d / "out.hdr").read_bytes() == (d / "plain.hdr").read_bytes()
    assert sorted(f.name for f in d.glob("out.*.npy")) == ["out.ambient.npy", "out.group0.npy", "out.group1.npy",
                                                           "out.group2.npy"]
    full, _ = groups(yrt, tmp_path_factory, "five", True, 2)
    for g in range(LS.NGROUPS):
        same_bits(np.load(d / f"out.group{g}.npy"), full["groups"][g])
    same_bits(np.load(d / "out.ambient.npy"), full["ambient"])
