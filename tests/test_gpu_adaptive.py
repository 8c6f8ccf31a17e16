"""yrt_render_adaptive on the GPU: a base frame at b*b samples per pixel, the contrast rule of
include/yrt.h between neighbouring pixels of it, and yrt_render's own s*s-sample value in the
pixels the rule flags (adaptive.hip: k_adaptive_flag; camera.hip: the pixel-batch pipeline over
the flagged list, k_camera_rays as the pinhole, the ray-batch driver, k_camera_resolve).

Frames of 37 x 24 and 24 x 37 pixels (partial waves, partial tiles), s = 3, b = 1. Every
expectation is bit for bit. The rule's numpy model (tests/adaptive_model.py) is applied to the
GPU's own raytrace(samples = b) frame, so the last ulp of the device pow cannot flip a flag
between the model and the kernel.
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import adaptive_model as AM
import passes_scene as PS
import shade_rays_scene as SS
from helpers import MIRROR_DEPTH, ROOT, SCENES, read_png_rgba8, scene_path

pytestmark = pytest.mark.gpu

CLI = ROOT / "yocto_raytracing_amd" / "yrt_raytrace"
FRAMES = ((24, 37), (37, 24))  # (resolution = rows, width)
S, B = 3, 1
AMB = PS.AMB
# scene -> (threshold, max_depth)
CASES = {"basic": (0.25, 16), "simple": (0.25, 16), "refl": (0.25, 16), "lines": (0.25, 16),
         "mirrors": (0.02, MIRROR_DEPTH)}
STAT_KEYS = ("rays", "shadow_rays", "shadow_rays_culled", "depth_truncated", "camera_samples")
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


_scenes, _renders, _adaptive = {}, {}, {}


def dev_scene(yrt, name):
    if name not in _scenes:
        path = scene_path(name) if name in CASES else SCENES / f"{name}.yrtscene"
        s = yrt.load_scene(str(path))
        yrt.build_bvh(s)
        _scenes[name] = (s, s.upload(0))
    return _scenes[name][1]


def render(yrt, name, res, width, s):
    """(image, stats) of yrt.raytrace at s samples per axis (shared, not to be written to)"""
    key = (name, res, width, s)
    if key not in _renders:
        _renders[key] = yrt.raytrace(dev_scene(yrt, name), AMB, res, s, width=width, max_depth=CASES[name][1],
                                     return_stats=True)
    return _renders[key]


def expected(yrt, name, res, width, threshold=None):
    """(flag, image) of the model on the GPU's own base and full renders"""
    base, full = render(yrt, name, res, width, B)[0], render(yrt, name, res, width, S)[0]
    flag = AM.flags(base, CASES[name][0] if threshold is None else threshold)
    return flag, AM.compose(flag, full, base)


def adaptive(yrt, name, res, width, **kw):
    """(image, mask, stats) of the whole frame at the scene's threshold (shared unless kw is given)"""
    def run():
        return yrt.raytrace_adaptive(dev_scene(yrt, name), AMB, res, S, width=width, max_depth=CASES[name][1],
                                     return_mask=True, return_stats=True,
                                     **{"threshold": CASES[name][0], "base_samples": B, **kw})
    if kw:
        return run()
    key = (name, res, width)
    if key not in _adaptive:
        _adaptive[key] = run()
    return _adaptive[key]


# ---- 1. the hot path: refined where flagged, the base frame elsewhere ----
@pytest.mark.parametrize("res,width", FRAMES)
@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_model_on_the_two_renders(yrt, name, res, width):
    flag, want = expected(yrt, name, res, width)
    share = flag.mean()
    print(f"{name} {width}x{res}: {int(flag.sum())} of {flag.size} pixels flagged ({share:.2f})")
    assert 0.1 <= share <= 0.9  # neither branch can hide
    img, mask, stats = adaptive(yrt, name, res, width)
    assert mask.dtype == np.uint8 and mask.shape == (res, width)
    np.testing.assert_array_equal(mask, flag.astype(np.uint8))
    same_bits(img, want)
    assert stats["refined_pixels"] == int(flag.sum())
    # the two renders differ in flagged pixels: the refinement is visible
    assert (render(yrt, name, res, width, S)[0][flag] != render(yrt, name, res, width, B)[0][flag]).any()


# ---- 2. the thresholds and base sizes that give a plain render ----
@pytest.mark.parametrize("name", list(CASES))
def test_thresholds_that_give_a_plain_render(yrt, name):
    res, width = FRAMES[0]
    base, full = render(yrt, name, res, width, B)[0], render(yrt, name, res, width, S)[0]
    img, mask, stats = adaptive(yrt, name, res, width, threshold=np.inf)
    same_bits(img, base)
    assert not mask.any() and stats["refined_pixels"] == 0
    assert {k: stats[k] for k in STAT_KEYS} == {k: render(yrt, name, res, width, B)[1][k] for k in STAT_KEYS}
    assert np.isfinite(base).all()
    img, mask, stats = adaptive(yrt, name, res, width, threshold=-1.0)
    same_bits(img, full)
    assert mask.all() and stats["refined_pixels"] == res * width
    img, mask, stats = adaptive(yrt, name, res, width, base_samples=S)
    same_bits(img, full)
    np.testing.assert_array_equal(mask, AM.flags(full, CASES[name][0]).astype(np.uint8))


# ---- 3. a window is the crop of the whole frame ----
@pytest.mark.parametrize("device_memory", [False, True])
@pytest.mark.parametrize("name", ["simple", "mirrors"])
def test_windows_equal_the_crop_and_keep_their_padding(yrt, name, device_memory):
    import torch

    res, width = FRAMES[0]
    full_img, full_mask, _ = adaptive(yrt, name, res, width)
    ds = dev_scene(yrt, name)
    # inside with padded rows; the corner; touching the right and bottom edges
    for x0, y0, tw, th, stride in ((5, 3, 17, 11, 19), (0, 0, 9, 7, 12), (width - 10, res - 6, 10, 6, 13)):
        p = yrt.render_params(AMB, res, S, width=width, max_depth=CASES[name][1], window=(x0, y0, tw, th))
        p.out_stride = stride
        out = np.empty((th, stride, 4), np.float32)
        out.view(np.uint32)[...] = 0x7fc01234
        mask = np.full((th, stride), 0xA5, np.uint8)
        if device_memory:
            d_out, d_mask = torch.from_numpy(out).to("cuda:0"), torch.from_numpy(mask).to("cuda:0")
            torch.cuda.synchronize()
            ds.render_adaptive_into(p, d_out.data_ptr(), CASES[name][0], B, refined_ptr=d_mask.data_ptr())
            torch.cuda.synchronize()
            out, mask = d_out.cpu().numpy(), d_mask.cpu().numpy()
        else:
            ds.render_adaptive_into(p, out.ctypes.data, CASES[name][0], B, refined_ptr=mask.ctypes.data,
                                    device_memory=False)
        what = (name, x0, y0, tw, th)
        crop = (slice(y0, y0 + th), slice(x0, x0 + tw))
        if (x0, y0) == (5, 3):  # both branches inside the window
            assert full_mask[crop].any() and not full_mask[crop].all(), what
        np.testing.assert_array_equal(mask[:, :tw], full_mask[crop], err_msg=str(what))
        same_bits(out[:, :tw], full_img[crop])
        assert (out[:, tw:].view(np.uint32) == 0x7fc01234).all(), what
        assert (mask[:, tw:] == 0xA5).all(), what
        assert ds.adaptive_refined() == int(full_mask[crop].sum()), what


def test_rows_past_the_image_edge_are_zeros(yrt):
    res, width = FRAMES[0]
    full_img, full_mask, _ = adaptive(yrt, "simple", res, width)
    p = yrt.render_params(AMB, res, S, width=width, window=(4, res - 3, 20, 5))  # two local rows past the edge
    out, mask = np.full((5, 20, 4), 7, np.float32), np.full((5, 20), 7, np.uint8)
    dev_scene(yrt, "simple").render_adaptive_into(p, out.ctypes.data, CASES["simple"][0], B,
                                                  refined_ptr=mask.ctypes.data, device_memory=False)
    same_bits(out[:3], full_img[res - 3:, 4:24])
    np.testing.assert_array_equal(mask[:3], full_mask[res - 3:, 4:24])
    assert not out[3:].any() and not mask[3:].any()


# ---- 4. chunk sizes, algorithms and tile lists change no bit ----
@pytest.mark.parametrize("name,chunks", [("simple", (7, 1, 10 ** 6)), ("refl", (7, 1, 10 ** 6)), ("mirrors", (7, 10 ** 6))])
def test_chunk_sizes_give_identical_bits(yrt, name, chunks):
    res, width = FRAMES[1]
    img, mask, stats = adaptive(yrt, name, res, width)
    assert 7 < stats["refined_pixels"] < 10 ** 6
    for chunk in chunks:
        got, gmask, gstats = adaptive(yrt, name, res, width, chunk_pixels=chunk)
        same_bits(got, img)
        np.testing.assert_array_equal(gmask, mask)
        assert gstats == stats, chunk


@pytest.mark.parametrize("name", ["refl", "lines", "mirrors"])
def test_algorithms_and_tile_lists_give_identical_bits(yrt, name):
    res, width = FRAMES[0]
    img, mask, stats = adaptive(yrt, name, res, width)
    got, gmask, gstats = adaptive(yrt, name, res, width, algorithm="wavefront_lane")
    same_bits(got, img)
    np.testing.assert_array_equal(gmask, mask)
    assert {k: gstats[k] for k in STAT_KEYS} == {k: stats[k] for k in STAT_KEYS}
    ds = dev_scene(yrt, name)
    try:
        for mode in ("on", "off"):
            ds.set_tile_lists(mode)
            got, gmask, gstats = adaptive(yrt, name, res, width, chunk_pixels=0)
            same_bits(got, img)
            np.testing.assert_array_equal(gmask, mask)
            assert {k: gstats[k] for k in STAT_KEYS} == {k: stats[k] for k in STAT_KEYS}, mode
    finally:
        ds.set_tile_lists("auto")


# ---- 5. the counters: the base render's plus the refined pixels' ray batch ----
@pytest.mark.parametrize("name", ["simple", "refl", "mirrors"])
def test_stats_are_the_base_renders_plus_the_batchs(yrt, name):
    res, width = FRAMES[0]
    img, mask, stats = adaptive(yrt, name, res, width)
    flag = mask.astype(bool)
    base_stats = render(yrt, name, res, width, B)[1]
    rays = SS.camera_rays(name, S, 0, res, width).reshape(res, width, S * S, 8)[flag].reshape(-1, 8)
    colours, batch = yrt.shade_rays(dev_scene(yrt, name), rays, AMB, max_depth=CASES[name][1], return_stats=True)
    for k in ("rays", "shadow_rays", "shadow_rays_culled", "depth_truncated"):
        assert stats[k] == base_stats[k] + batch[k], k
    assert stats["camera_samples"] == res * width * B * B + int(flag.sum()) * S * S
    assert stats["refined_pixels"] == int(flag.sum())
    # the batch's colours, box filtered, are the refined pixels
    c = colours.reshape(-1, S * S, 4)
    acc = np.zeros((len(c), 3), np.float32)
    for q in range(S * S):
        acc = (acc + c[:, q, :3]).astype(np.float32)
    same_bits(img[flag][:, :3], (acc / np.float32(S * S)).astype(np.float32))
    assert (img[flag][:, 3] == 1).all()
    if name == "mirrors":
        assert stats["rays"] > 2 * stats["camera_samples"]  # the mirror levels ran in the batches


def test_a_windows_base_render_covers_its_apron(yrt):
    """camera_samples counts the window grown by one pixel and clipped to the image"""
    res, width = FRAMES[0]
    ds = dev_scene(yrt, "simple")
    for (x0, y0, tw, th), grown in (((5, 3, 17, 11), 19 * 13), ((0, 0, 9, 7), 10 * 8),
                                     ((width - 10, res - 6, 10, 6), 11 * 7)):
        _, mask, stats = yrt.raytrace_adaptive(ds, AMB, res, S, threshold=0.25, width=width, window=(x0, y0, tw, th),
                                               return_mask=True, return_stats=True)
        assert stats["camera_samples"] == grown * B * B + int(mask.sum()) * S * S, (x0, y0)


# ---- 6. edge scenes ----
def test_a_sky_of_misses_flags_nothing(yrt):
    ds = dev_scene(yrt, "edge_sky")
    base = yrt.raytrace(ds, AMB, 24, B, width=37)
    img, mask, stats = yrt.raytrace_adaptive(ds, AMB, 24, S, threshold=0.0, width=37, return_mask=True,
                                             return_stats=True)
    same_bits(img, base)
    assert not mask.any() and stats["refined_pixels"] == 0 and ds.adaptive_refined() == 0
    assert stats["camera_samples"] == 24 * 37


@pytest.mark.parametrize("name", ["edge_empty", "edge_unlit"])
def test_edge_scenes_run_clean(yrt, name):
    ds = dev_scene(yrt, name)
    base, full = yrt.raytrace(ds, AMB, 24, B, width=37), yrt.raytrace(ds, AMB, 24, S, width=37)
    for threshold in (0.02, -1.0):
        img, mask = yrt.raytrace_adaptive(ds, AMB, 24, S, threshold=threshold, width=37, return_mask=True)
        flag = AM.flags(base, threshold)
        np.testing.assert_array_equal(mask, flag.astype(np.uint8))
        same_bits(img, AM.compose(flag, full, base))


# ---- 7. refusals with a real handle ----
def test_unsupported_and_invalid_calls_are_refused(yrt):
    from yocto_raytracing_amd import _native as N

    ds = dev_scene(yrt, "simple")
    out = np.full((24, 37, 4), 77, np.float32)
    a = N.AdaptiveParams(1, 0.25, 0)

    def call(**kw):
        p = yrt.render_params(AMB, 24, S, width=37, **kw)
        return N.lib.yrt_render_adaptive(ds.handle, C.byref(p), C.byref(a), out.ctypes.data, None, N.YRT_MEM_HOST, None)

    assert call(algorithm="megakernel") == YRT_ERR_UNSUPPORTED
    assert call(count_work=True) == YRT_ERR_UNSUPPORTED
    for band in ((8, 3, 1), (2, 1, 0), (1, 2, 0)):
        assert call(band=band) == YRT_ERR_UNSUPPORTED, band
    assert call(camera=5) == YRT_ERR_INVALID_ARG and b"camera index out of range" in N.lib.yrt_last_error()
    assert (out == 77).all()
    assert call() == YRT_OK and (out != 77).all()


# ---- 8. the CLI ----
def test_cli_writes_the_adaptive_image_and_the_mask(yrt, tmp_path):
    out = tmp_path / "o.png"
    r = subprocess.run([str(CLI), "--adaptive", "0.25", "-r", "24", "-s", "3", "-o", str(out), str(scene_path("refl"))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    img, mask = yrt.raytrace_adaptive(dev_scene(yrt, "refl"), 0.1, 24, 3, threshold=0.25, return_mask=True)
    np.testing.assert_array_equal(read_png_rgba8(out)[..., :3], yrt.tonemap(img)[..., :3])
    got = np.load(tmp_path / "o.refined.npy")
    assert got.dtype == np.uint8 and got.shape == mask.shape
    np.testing.assert_array_equal(got, mask)
    assert 0 < mask.sum() < mask.size
    assert f"refined {int(mask.sum())} of {mask.size} pixels" in r.stdout
    r = subprocess.run([str(CLI), "--adaptive", "0.25", "--gpus", "2", str(scene_path("refl"))], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "--adaptive renders on one GPU" in r.stderr
