"""Nothing carries from one call into the next on a handle: the pixel-batch renders
(yrt_render_adaptive, yrt_render_camera, yrt_render_soft_shadows) share one scratch buffer
(ds.batch_rays) and the batch driver's keep_counters flag (camera.hip render_pixel_batches), and
every other entry point runs between them on the same handle.

Frames of 37 x 24 and 24 x 37 pixels (partial waves), s = 3. Every call of a sequence on one
DeviceScene, run in one order and then in the reverse order, gives the bits and the
last_stats() of the same call on a freshly uploaded handle of the same scene. In particular the
first batch of a camera call after an adaptive call inherits no counts (it zeroes the counter
lines), and an adaptive call after a camera call keeps its base render's counts (its first
batch does not). The chunk sizes 7, 5 and 11 divide neither frame's pixel count nor each other, so
the scratch is regrown and every call ends on a partial chunk.
"""
import numpy as np
import pytest

from helpers import MIRROR_DEPTH, scene_path

pytestmark = pytest.mark.gpu

FRAMES = ((24, 37), (37, 24))  # (resolution = rows, width)
S = 3
AMB = 0.1
# scene -> (adaptive threshold that flags some but not all pixels, max_depth)
CASES = {"refl": (0.25, 16), "mirrors": (0.02, MIRROR_DEPTH)}
ORDER = ("adaptive", "camera", "soft", "shade_rays", "raytrace", "aovs", "ao")


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on the MI355X box")
    return y


_host, _fresh = {}, {}


def host_scene(yrt, name):
    if name not in _host:
        s = yrt.load_scene(str(scene_path(name)))
        yrt.build_bvh(s)
        _host[name] = s
    return _host[name]


def run(yrt, ds, call, name, res, width):
    """what `call` leaves behind on ds: ({label: array}, everything the handle reports of it)"""
    threshold, depth = CASES[name]
    kw = dict(width=width, max_depth=depth)
    if call == "adaptive":
        img, mask = yrt.raytrace_adaptive(ds, AMB, res, S, threshold=threshold, chunk_pixels=7, return_mask=True, **kw)
        out = {"image": img, "mask": mask}
    elif call == "camera":
        out = {"image": yrt.raytrace_camera(ds, AMB, res, S, model="perspective", aperture=0.3, chunk_pixels=5, **kw)}
    elif call == "soft":
        out = {"image": yrt.raytrace_soft(ds, AMB, res, S, radius=0.2, shadow_rays=4, chunk_pixels=11, **kw)}
    elif call == "shade_rays":
        rays = yrt.camera_rays(ds, res, S, width=width)
        out = {"rays": rays, "colours": yrt.shade_rays(ds, rays, AMB, max_depth=depth)}
    elif call == "raytrace":
        out = {"image": yrt.raytrace(ds, AMB, res, S, **kw)}
    elif call == "aovs":
        out = dict(yrt.render_aovs(ds, res, S, width=width))
    else:
        out = {"image": yrt.render_ao(ds, res, S, rays=4, width=width)}
    report = {"stats": ds.last_stats(), "refined": ds.adaptive_refined() if call == "adaptive" else None}
    if call not in ("aovs", "ao"):  # the tile passes build no lists and stage nothing: they leave the last report
        lists = ds.tile_lists()
        report.update(lists=(lists["camera"], lists["bundles"]), staging=ds.lds_staging())
    return out, report


def fresh(yrt, call, name, res, width):
    """`call` on a handle that has seen no other call (shared, not to be written to)"""
    key = (call, name, res, width)
    if key not in _fresh:
        ds = yrt.DeviceScene(host_scene(yrt, name), 0)
        try:
            _fresh[key] = run(yrt, ds, call, name, res, width)
        finally:
            ds.close()
    return _fresh[key]


def same(got, want, what):
    (gout, greport), (wout, wreport) = got, want
    assert greport == wreport, (what, greport, wreport)
    assert sorted(gout) == sorted(wout), what
    for k, w in wout.items():
        g = gout[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        np.testing.assert_array_equal(g.view(np.uint8), w.view(np.uint8), err_msg=str((what, k)))


@pytest.mark.parametrize("res,width", FRAMES)
@pytest.mark.parametrize("name", list(CASES))
def test_a_call_sequence_equals_fresh_handles_in_both_orders(yrt, name, res, width):
    ds = yrt.DeviceScene(host_scene(yrt, name), 0)
    try:
        for order in (ORDER, ORDER[::-1]):
            for call in order:
                same(run(yrt, ds, call, name, res, width), fresh(yrt, call, name, res, width),
                     (name, res, width, call, "forward" if order is ORDER else "reverse"))
    finally:
        ds.close()
    # the sequence exercised what it is about: some but not all pixels refined, in several
    # batches, and counts that a carried-over counter line would have changed
    adaptive, camera = fresh(yrt, "adaptive", name, res, width), fresh(yrt, "camera", name, res, width)
    refined = adaptive[1]["refined"]
    assert 7 < refined < res * width and refined == int(adaptive[0]["mask"].sum())
    assert adaptive[1]["stats"]["camera_samples"] == res * width + refined * S * S
    assert camera[1]["stats"]["camera_samples"] == res * width * S * S
    assert camera[1]["stats"]["rays"] > 0 and camera[1]["lists"] == (False, False)


@pytest.mark.parametrize("name", list(CASES))
def test_adaptive_over_a_list_in_a_padded_window(yrt, name):
    """the shared kernels with the flagged list, on a window with x0, y0 > 0 and out_stride >
    tile_w: a refined pixel is raytrace's at s samples bit for bit, the padding keeps its bytes"""
    res, width = FRAMES[0]
    threshold, depth = CASES[name]
    x0, y0, tw, th, stride = 5, 3, 17, 11, 19
    ds = host_scene(yrt, name).upload(0)
    full = yrt.raytrace(ds, AMB, res, S, width=width, max_depth=depth)
    p = yrt.render_params(AMB, res, S, width=width, max_depth=depth, window=(x0, y0, tw, th))
    p.out_stride = stride
    out = np.empty((th, stride, 4), np.float32)
    out.view(np.uint32)[...] = 0x7fc01234
    mask = np.full((th, stride), 0xA5, np.uint8)
    ds.render_adaptive_into(p, out.ctypes.data, threshold, 1, refined_ptr=mask.ctypes.data, chunk_pixels=7,
                            device_memory=False)
    flag = mask[:, :tw] == 1
    assert 0 < flag.sum() < flag.size and ds.adaptive_refined() == int(flag.sum())
    np.testing.assert_array_equal(out[:, :tw][flag].view(np.uint32), full[y0:y0 + th, x0:x0 + tw][flag].view(np.uint32))
    assert (out[:, tw:].view(np.uint32) == 0x7fc01234).all() and (mask[:, tw:] == 0xA5).all()
    assert np.isin(mask[:, :tw], (0, 1)).all()
