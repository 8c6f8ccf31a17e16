"""The shading passes on the GPU (yrt_render_passes; wavefront.hip k_shade_passes and
k_accumulate_passes) on 37 x 24 frames: partial 8 x 8 tiles on both axes. s = 1 and 2 take the
fused shape, s = 3 the unfused one, a reflective scene the mirror levels.

AMBIENT and DIFFUSE equal, bit for bit, the oracle's beauty of the built scene (passes_scene.py)
with the other terms' material constants set to zero; SPECULAR and DIRECT pass
helpers.assert_frame_parity against theirs (the device pow) and equal the GPU's own beauty of that variant
bit for bit. With s = 1, beauty == (DIRECT + REFLECTION) + AMBIENT in float32 on every pixel,
which pins REFLECTION; with s = 2 and 3 the recompositions hold within the rounding of their
additions. Then the plumbing (window, bands, stride, masks, lists, algorithms), the counters
and the CLI.
"""
import subprocess

import numpy as np
import pytest

import passes_scene as PS
from helpers import (MIRROR_DEPTH, ROOT, Oracle, assert_frame_in_envelope, assert_frame_parity, assert_same_floats,
                     scene_path)

pytestmark = pytest.mark.gpu

CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
ALL = ("direct", "diffuse", "specular", "reflection", "ambient")
RES, WIDTH = 24, 37
STAT_KEYS = ("rays", "camera_samples", "shadow_rays", "shadow_rays_culled", "depth_truncated")
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


_scenes, _built, _oracle, _passes = {}, {}, {}, {}


def built(yrt, tmp_path_factory, variant=None):
    """(host scene, its .yrtscene file, device scene) of passes_scene.build(variant)"""
    if variant not in _built:
        s = PS.build(yrt, variant)
        path = tmp_path_factory.mktemp("passes") / f"built_{variant}.yrtscene"
        s.save(str(path))
        yrt.build_bvh(s)
        _built[variant] = (s, path, s.upload(0))
    return _built[variant]


def dev_scene(yrt, tmp_path_factory, name):
    if name == "built":
        return built(yrt, tmp_path_factory)[2]
    if name not in _scenes:
        s = yrt.load_scene(str(scene_path(name)))
        yrt.build_bvh(s)
        _scenes[name] = (s, s.upload(0))
    return _scenes[name][1]


def nlights(yrt, tmp_path_factory, name):
    dev_scene(yrt, tmp_path_factory, name)
    host = built(yrt, tmp_path_factory)[0] if name == "built" else _scenes[name][0]
    return host.info()["lights"]


def oracle_variant(yrt, tmp_path_factory, variant, s):
    """the oracle's beauty of a variant of the built scene, finite everywhere (a kd = 0 or
    ks = 0 variant would turn a NaN factor into a NaN the pass does not contain), and its
    pow envelope (helpers.Oracle.envelope): (ref, lo, hi)"""
    if (variant, s) not in _oracle:
        img, lo, hi, _, _ = Oracle(built(yrt, tmp_path_factory, variant)[1]).envelope(
            RES, s, amb=PS.VARIANT_AMB[variant], width=WIDTH, max_depth=16)
        assert img.shape == (RES, WIDTH, 4)
        assert np.isfinite(img).all(), f"the {variant} variant's oracle frame is not finite"
        assert (img[..., :3] > 0).any()
        _oracle[(variant, s)] = (img, lo, hi)
    return _oracle[(variant, s)]


def passes(yrt, tmp_path_factory, name, s, max_depth=16):
    """all five planes and the beauty of one render (shared: not to be written to), and the
    counters after it"""
    key = (name, s, max_depth)
    if key not in _passes:
        ds = dev_scene(yrt, tmp_path_factory, name)
        out = yrt.render_passes(ds, PS.AMB, RES, s, width=WIDTH, max_depth=max_depth)
        assert set(out) == set(ALL) | {"beauty"}
        for a in out.values():
            assert a.shape == (RES, WIDTH, 4) and a.dtype == np.float32
        _passes[key] = (out, ds.last_stats())
    return _passes[key]


# ---- 1. each pass against the oracle's beauty of a variant scene ----
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("name", ["ambient", "diffuse"])
def test_ambient_and_diffuse_equal_the_oracle(yrt, tmp_path_factory, name, s):
    """bit for bit, the sample order included: at s = 2 (fused) and s = 3 (k_accumulate_passes)
    only the jj/ii order of the sums gives these bits"""
    want = oracle_variant(yrt, tmp_path_factory, name, s)[0]
    got = passes(yrt, tmp_path_factory, "built", s)[0][name]
    assert_same_floats(got, want)  # (.w = 1 on both sides)


@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("name", ["specular", "direct"])
def test_specular_and_direct_equal_the_variants_beauty(yrt, tmp_path_factory, name, s):
    """DIRECT passes the whole bar of a frame. SPECULAR passes all of it but the count cap, whose
    premise -- that the reference alone stays inside it -- does not hold for this frame: 1484 of
    its 3552 channels are sums of specular terms alone, and glibc powf against the f64 pow
    rounded once (oracle mode 2, on the CPU) already differs in 0, 2 and 8 channels at s = 1, 2
    and 3, past the cap of 2. The GPU's planes differ from the oracle's in those same channels."""
    want, lo, hi = oracle_variant(yrt, tmp_path_factory, name, s)
    got = passes(yrt, tmp_path_factory, "built", s)[0][name]
    if name == "specular":
        assert_frame_in_envelope(got, want, lo, hi, f"pass {name} s={s}")
    else:
        assert_frame_parity(got, want, lo, hi, f"pass {name} s={s}")
    gpu = yrt.raytrace(built(yrt, tmp_path_factory, name)[2], (0.0, 0.0, 0.0), RES, s, width=WIDTH)
    same_bits(got, gpu)


def test_the_built_scene_has_partially_covered_pixels(yrt, tmp_path_factory):
    """a miss's +0 takes its place in the order of the sums: some pixels of the s = 3 frame are
    partly covered, in the built scene and in `lines`"""
    for name in ("built", "lines"):
        cov = yrt.render_aovs(dev_scene(yrt, tmp_path_factory, name), RES, 3, width=WIDTH, aovs=("depth",))["depth"][..., 3]
        assert ((cov > 0) & (cov < 1)).any(), name


# ---- 2. the exact recomposition at s = 1 ----
RECOMPOSE = [("built", 16), ("simple", 16), ("lines", 16), ("instance1k", 16), ("refl", 16),
             ("mirrors", MIRROR_DEPTH), ("mirrors", 30)]


@pytest.mark.parametrize("name,depth", RECOMPOSE)
def test_beauty_is_direct_plus_reflection_plus_ambient(yrt, tmp_path_factory, name, depth):
    """raytrace.cpp:182-206: c after the lights, + col * kr, + la, and c is never -0, so the
    float32 sum of the planes in that order is the beauty on every pixel, hit or miss"""
    out, stats = passes(yrt, tmp_path_factory, name, 1, depth)
    ds = dev_scene(yrt, tmp_path_factory, name)
    img, rstats = yrt.raytrace(ds, PS.AMB, RES, 1, width=WIDTH, max_depth=depth, return_stats=True)
    same_bits(out["beauty"], img)
    assert {k: stats[k] for k in STAT_KEYS} == {k: rstats[k] for k in STAT_KEYS}
    if (name, depth) == ("mirrors", 30):
        assert stats["depth_truncated"] > 0
    if (name, depth) == ("mirrors", MIRROR_DEPTH):
        assert stats["depth_truncated"] == 0
    with np.errstate(invalid="ignore", over="ignore"):
        total = ((out["direct"][..., :3] + out["reflection"][..., :3]).astype(np.float32)
                 + out["ambient"][..., :3]).astype(np.float32)
    assert_same_floats(total, out["beauty"][..., :3])
    for n in ALL:
        same_bits(out[n][..., 3], out["beauty"][..., 3])
    assert (out["beauty"][..., 3] == 1).all()


# ---- 3. REFLECTION ----
def test_reflection_is_the_beauty_on_the_pure_mirror(yrt, tmp_path_factory):
    out, _ = passes(yrt, tmp_path_factory, "built", 1)
    ids = yrt.render_aovs(dev_scene(yrt, tmp_path_factory, "built"), RES, 1, width=WIDTH, aovs=("ids",))["ids"]
    on_mirror = ids[..., 2] == PS.PURE_MIRROR
    assert on_mirror.sum() >= 8, int(on_mirror.sum())
    same_bits(out["reflection"][on_mirror], out["beauty"][on_mirror])
    assert (out["reflection"][on_mirror][:, :3] > 0).any()
    for n in ("direct", "diffuse", "specular", "ambient"):  # kd = ks = 0
        assert not out[n][on_mirror][:, :3].any(), n


@pytest.mark.parametrize("s", [1, 2, 3])
def test_reflection_of_a_scene_without_mirrors_is_plus_zero(yrt, tmp_path_factory, s):
    out, _ = passes(yrt, tmp_path_factory, "simple", s)
    assert not out["reflection"][..., :3].view(np.uint32).any()
    assert (out["direct"][..., :3] > 0).any()


@pytest.mark.parametrize("name", ["built", "refl"])
def test_reflective_scenes_have_a_reflection(yrt, tmp_path_factory, name):
    for s in (1, 3):
        out, _ = passes(yrt, tmp_path_factory, name, s)
        assert (out["reflection"][..., :3] > 0).any(), (name, s)


# ---- 4. the recompositions at s = 2 and s = 3 ----
@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", ["built", "refl", "simple", "instance1k"])
def test_recomposition_within_the_rounding_of_the_sums(yrt, tmp_path_factory, name, s):
    """one rounding of relative size at most 2^-24 per float32 addition or division on partial
    sums of non-negative terms, with a factor 2 of slack: N operations on the longer side"""
    out, stats = passes(yrt, tmp_path_factory, name, s)
    nl = nlights(yrt, tmp_path_factory, name)
    p = {n: out[n][..., :3].astype(np.float64) for n in (*ALL, "beauty")}
    assert all(np.isfinite(a).all() for a in p.values()), "the bound is stated for finite, non-negative terms"
    assert all((a >= 0).all() for a in p.values())
    n1 = s * s * (nl + 2) + 2
    err1 = np.abs(p["beauty"] - (p["direct"] + p["reflection"] + p["ambient"]))
    bound1 = 2 * n1 * 2.0 ** -24 * (np.abs(p["beauty"]) + p["direct"] + p["reflection"] + p["ambient"])
    n2 = 2 * s * s * nl + 2
    err2 = np.abs(p["direct"] - (p["diffuse"] + p["specular"]))
    bound2 = 2 * n2 * 2.0 ** -24 * (p["direct"] + p["diffuse"] + p["specular"])
    print(f"{name} s={s}: beauty max err/bound {np.max(err1 / np.maximum(bound1, 1e-300)):.3g}, "
          f"direct max err/bound {np.max(err2 / np.maximum(bound2, 1e-300)):.3g}")
    assert (err1 <= bound1).all()
    assert (err2 <= bound2).all()
    img, rstats = yrt.raytrace(dev_scene(yrt, tmp_path_factory, name), PS.AMB, RES, s, width=WIDTH, return_stats=True)
    same_bits(out["beauty"], img)
    assert {k: stats[k] for k in STAT_KEYS} == {k: rstats[k] for k in STAT_KEYS}


# ---- 5. plumbing ----
@pytest.mark.parametrize("name,s", [("built", 2), ("built", 3), ("simple", 2)])
def test_window_equals_the_crop(yrt, tmp_path_factory, name, s):
    full, _ = passes(yrt, tmp_path_factory, name, s)
    x0, y0, tw, th = 3, 5, 21, 13  # not tile-aligned
    win = yrt.render_passes(dev_scene(yrt, tmp_path_factory, name), PS.AMB, RES, s, width=WIDTH, window=(x0, y0, tw, th))
    for n in (*ALL, "beauty"):
        same_bits(win[n], np.ascontiguousarray(full[n][y0:y0 + th, x0:x0 + tw]))


@pytest.mark.parametrize("name,s", [("built", 2), ("built", 3), ("simple", 2)])
def test_band_shards_reassemble(yrt, tmp_path_factory, name, s):
    full, _ = passes(yrt, tmp_path_factory, name, s)
    ds = dev_scene(yrt, tmp_path_factory, name)
    got = {n: np.full((RES, WIDTH, 4), np.nan, np.float32) for n in (*ALL, "beauty")}
    band, stride = 8, 2
    for off in range(stride):
        p = yrt.render_params(PS.AMB, RES, s, width=WIDTH, band=(band, stride, off))
        th = len(range(off, -(-RES // band), stride)) * band
        planes = {n: np.full((th, WIDTH, 4), np.nan, np.float32) for n in (*ALL, "beauty")}
        ds.render_passes_into(p, {n: planes[n].ctypes.data for n in ALL}, beauty_ptr=planes["beauty"].ctypes.data,
                              device_memory=False)
        for ly in range(th):
            j = ((ly // band) * stride + off) * band + ly % band
            assert j < RES
            for n in got:
                got[n][j] = planes[n][ly]
    for n in got:
        same_bits(got[n], full[n])


def test_empty_band_offset_writes_nothing_and_counts_nothing(yrt, tmp_path_factory):
    ds = dev_scene(yrt, tmp_path_factory, "simple")
    res, s = 12, 2
    yrt.render_passes(ds, PS.AMB, res, s, width=WIDTH)
    assert ds.last_stats()["rays"] > 0  # the counters an empty call must not repeat
    p = yrt.render_params(PS.AMB, res, s, width=WIDTH, band=(8, 3, 2))  # two bands of 8: offset 2 of 3 has none
    planes = {n: np.full((8, WIDTH, 4), 77, np.float32) for n in (*ALL, "beauty")}
    ds.render_passes_into(p, {n: planes[n].ctypes.data for n in ALL}, beauty_ptr=planes["beauty"].ctypes.data,
                          device_memory=False)
    for a in planes.values():
        assert (a == 77).all()
    st = ds.last_stats()
    assert st["rays"] == 0 and st["camera_samples"] == 0


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("device_memory", [True, False])
def test_row_padding_is_not_written(yrt, tmp_path_factory, s, device_memory):
    import torch

    full, _ = passes(yrt, tmp_path_factory, "built", s)
    x0, y0, tw, th = 3, 5, 21, 13
    stride = tw + 5
    p = yrt.render_params(PS.AMB, RES, s, width=WIDTH, window=(x0, y0, tw, th))
    p.out_stride = stride
    names = (*ALL, "beauty")
    if device_memory:
        dev = {n: torch.full((th, stride, 4), -77.0, dtype=torch.float32, device="cuda:0") for n in names}
        torch.cuda.synchronize()
        ptr = {n: a.data_ptr() for n, a in dev.items()}
    else:
        host = {n: np.full((th, stride, 4), -77, np.float32) for n in names}
        ptr = {n: a.ctypes.data for n, a in host.items()}
    dev_scene(yrt, tmp_path_factory, "built").render_passes_into(p, {n: ptr[n] for n in ALL}, beauty_ptr=ptr["beauty"],
                                                                 device_memory=device_memory)
    if device_memory:
        torch.cuda.synchronize()
        host = {n: a.cpu().numpy() for n, a in dev.items()}
    for n in names:
        assert (host[n][:, tw:] == -77).all(), n
        same_bits(np.ascontiguousarray(host[n][:, :tw]), np.ascontiguousarray(full[n][y0:y0 + th, x0:x0 + tw]))


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", ALL)
def test_a_mask_of_one_pass_writes_only_that_plane(yrt, tmp_path_factory, name, s):
    """through the C-ABI with every plane pointer set: the planes the mask leaves out keep their
    bytes, and no beauty is asked for"""
    from yocto_raytracing_amd import _native as N
    import ctypes as C

    full, _ = passes(yrt, tmp_path_factory, "built", s)
    ds = dev_scene(yrt, tmp_path_factory, "built")
    planes = {n: np.full((RES, WIDTH, 4), 55, np.float32) for n in ALL}
    pp = N.PassPlanes()
    for n in ALL:
        pp.plane[N.PASSES[n]] = planes[n].ctypes.data
    p = yrt.render_params(PS.AMB, RES, s, width=WIDTH)
    N.check(N.lib.yrt_render_passes(ds.handle, C.byref(p), 1 << N.PASSES[name], C.byref(pp), None, N.YRT_MEM_HOST, None),
            "yrt_render_passes")
    for n in ALL:
        if n == name:
            same_bits(planes[n], full[n])
        else:
            assert (planes[n] == 55).all(), n
    # and the Python call without a beauty
    out = yrt.render_passes(ds, PS.AMB, RES, s, width=WIDTH, passes=(name,), beauty=False)
    assert list(out) == [name]
    same_bits(out[name], full[name])


def test_tile_lists_on_and_off_give_the_same_planes(yrt, tmp_path_factory):
    ds = dev_scene(yrt, tmp_path_factory, "instance1k")
    got = {}
    try:
        for mode in ("on", "off"):
            ds.set_tile_lists(mode)
            got[mode] = yrt.render_passes(ds, PS.AMB, RES, 3, width=WIDTH)
            tl = ds.tile_lists()
            assert (tl["camera"], tl["bundles"]) == ((True, True) if mode == "on" else (False, False)), tl
    finally:
        ds.set_tile_lists("auto")
    for n in (*ALL, "beauty"):
        same_bits(got["on"][n], got["off"][n])
    same_bits(got["on"]["beauty"], yrt.raytrace(ds, PS.AMB, RES, 3, width=WIDTH))


@pytest.mark.parametrize("name,s", [("built", 2), ("built", 3), ("simple", 2)])
def test_the_lane_algorithm_gives_the_same_planes(yrt, tmp_path_factory, name, s):
    full, _ = passes(yrt, tmp_path_factory, name, s)
    lane = yrt.render_passes(dev_scene(yrt, tmp_path_factory, name), PS.AMB, RES, s, width=WIDTH, algorithm="wavefront_lane")
    for n in (*ALL, "beauty"):
        same_bits(lane[n], full[n])


def test_megakernel_and_count_work_are_unsupported(yrt, tmp_path_factory):
    ds = dev_scene(yrt, tmp_path_factory, "simple")
    planes = {n: np.full((RES, WIDTH, 4), 33, np.float32) for n in ALL}
    for kw in (dict(algorithm="megakernel"), dict(count_work=True)):
        p = yrt.render_params(PS.AMB, RES, 1, width=WIDTH, **kw)
        with pytest.raises(yrt.YrtError) as e:
            ds.render_passes_into(p, {n: a.ctypes.data for n, a in planes.items()}, device_memory=False)
        assert e.value.status == YRT_ERR_UNSUPPORTED, kw
    assert all((a == 33).all() for a in planes.values())


# ---- 6. isolation ----
@pytest.mark.parametrize("name,s", [("built", 3), ("simple", 2), ("refl", 2)])
def test_raytrace_is_the_same_before_and_after(yrt, tmp_path_factory, name, s):
    ds = dev_scene(yrt, tmp_path_factory, name)
    before, st0 = yrt.raytrace(ds, PS.AMB, RES, s, width=WIDTH, return_stats=True)
    out = yrt.render_passes(ds, PS.AMB, RES, s, width=WIDTH)
    st1 = ds.last_stats()
    after, st2 = yrt.raytrace(ds, PS.AMB, RES, s, width=WIDTH, return_stats=True)
    same_bits(before, after)
    same_bits(out["beauty"], before)
    assert {k: st0[k] for k in STAT_KEYS} == {k: st1[k] for k in STAT_KEYS} == {k: st2[k] for k in STAT_KEYS}


# ---- 7. the CLI ----
def test_cli_writes_the_planes_and_the_same_image(yrt, tmp_path_factory):
    d = tmp_path_factory.mktemp("passes_cli")
    _, path, ds = built(yrt, tmp_path_factory)
    common = ["-r", str(RES), "--width", str(WIDTH), "-s", "2", "-a", str(PS.AMB)]
    r = subprocess.run([str(CLI), *common, "-o", str(d / "plain.hdr"), str(path)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(CLI), *common, "--passes", "diffuse,reflection", "-o", str(d / "out.hdr"), str(path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (d / "out.hdr").read_bytes() == (d / "plain.hdr").read_bytes()
    assert sorted(f.name for f in d.glob("out.*.npy")) == ["out.diffuse.npy", "out.reflection.npy"]
    full, _ = passes(yrt, tmp_path_factory, "built", 2)
    for n in ("diffuse", "reflection"):
        same_bits(np.load(d / f"out.{n}.npy"), full[n])
