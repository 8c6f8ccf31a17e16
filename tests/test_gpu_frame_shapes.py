"""Frame geometry of yrt_render on the default library, against the oracle: a band offset
that has no bands, and frames on either side of the point where the persistent grids'
per-XCD head (head_items in wavefront.hip) becomes non-empty.

The grids deal their items as a head of whole super-runs, (n - n / T) / G * G items with
T = YRT_SHARED_TAIL and G = 8 * lcm(run, block chunk), and a shared tail of the rest. The
constants are read from the source, and the frames are asserted to straddle the boundary
they were chosen for, so a retune cannot move the test off it unnoticed. With today's
constants (T = 32; any hit: run 48, chunk 16, G = 384; closest hit: run 256, chunk 16,
G = 2048) the head of the any-hit grid is empty up to 395 items and 384 items from 396 on,
the primary grid's empty up to 2113 items and 2048 from 2114 on. Frames are 1 sample per
pixel, so an item is an 8 x 8 tile, and the lists are forced on, which puts the shadow rays
on the persistent any-hit grid at any size.
"""
from __future__ import annotations

import re
from functools import lru_cache
from math import gcd

import numpy as np
import pytest

from helpers import ROOT, Oracle, assert_frame_parity, scene_path

ALGOS = ("wavefront", "megakernel", "wavefront_lane")
WAVEFRONT_HIP = ROOT / "yocto_raytracing_amd" / "csrc" / "wavefront.hip"


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite needs one")
    return y


_scenes = {}


def dev_scene(yrt, name):
    if name not in _scenes:
        s = yrt.load_scene(str(scene_path(name)))
        yrt.build_bvh(s)
        _scenes[name] = (s, s.upload(0))
    return _scenes[name][1]


# ---- a band offset without bands ----

@pytest.mark.gpu
@pytest.mark.parametrize("algo", ALGOS)
def test_empty_band_offset_writes_nothing_and_counts_nothing(yrt, algo):
    """12 rows are two bands of 8: offset 2 of 3 has none. The call launches nothing, leaves the
    caller's buffer alone and reports no rays -- not the counts of the render before it (the
    wavefront algorithms zero their counters in the first chunk's setup kernel, which an empty
    window never launches)"""
    ds = dev_scene(yrt, "simple")
    res, s, width = 12, 2, 37
    ref, lo, hi, nrays, trunc = oracle_frame("simple", width, res, s)
    img, st = yrt.raytrace(ds, (0.1, 0.1, 0.1), res, s, width=width, return_stats=True, algorithm=algo)
    assert st["rays"] == nrays and st["camera_samples"] == width * res * s * s
    p = yrt.render_params(0.1, res, s, width=width, band=(8, 3, 2), algorithm=algo)
    out = np.full((8, width, 4), 77, np.float32)
    ds.render_into(p, out.ctypes.data, device_memory=False)
    st = ds.last_stats()
    assert st["rays"] == 0, st
    assert st["camera_samples"] == 0, st
    assert (out == 77).all()
    img, st = yrt.raytrace(ds, (0.1, 0.1, 0.1), res, s, width=width, return_stats=True, algorithm=algo)
    assert st["rays"] == nrays and st["camera_samples"] == width * res * s * s and st["depth_truncated"] == trunc
    assert_frame_parity(img, ref, lo, hi, f"simple {width}x{res} after an empty band, {algo}")


# ---- the head / tail boundary of the persistent grids ----

def _default(knob):
    m = re.search(rf"#define {knob} (\d+)", WAVEFRONT_HIP.read_text())
    assert m, f"{knob}: no default in wavefront.hip"
    return int(m.group(1))


def head_items(n, run, chunk):
    """head_items<RUN, CS>(n) of wavefront.hip"""
    T = _default("YRT_SHARED_TAIL")
    G = 8 * (run // gcd(run, chunk) * chunk)
    return (n - n // T) // G * G if T else 0


def any_hit_head(n):
    assert _default("YRT_SHADOW_ITEM_LIGHTS") == 1  # an item is a 64-sample block with all its lights
    return head_items(n, _default("YRT_SHADOW_ITEM_RUN"), _default("YRT_SHADOW_BLOCK_CHUNK"))


def primary_head(n):
    return head_items(n, _default("YRT_XCD_CHUNK_PRIMARY"), _default("YRT_PRIMARY_BLOCK_CHUNK"))


def tiles(w, h):
    return -(-w // 8) * -(-h // 8)


# (width, height): what the frame is for
FRAMES = {
    (96, 64): "96 tiles: both heads empty",
    (88, 72): "99 tiles: both heads empty",
    (80, 80): "100 tiles: both heads empty",
    (93, 70): "12 x 9 tiles, partial on both axes, both heads empty",
    (40, 632): "395 tiles: the last count with an empty any-hit head",
    (144, 176): "396 tiles: the first any-hit head, 384 items and a tail of 12",
    (152, 168): "399 tiles: any-hit head 384, tail 15",
    (160, 160): "400 tiles: any-hit head 384, tail 16",
    (157, 163): "20 x 21 tiles, partial on both axes, on an any-hit head of 384",
    (384, 352): "2112 tiles: the primary head still empty",
    (368, 368): "2116 tiles: primary head 2048, tail 68",
}


def test_frames_straddle_the_head_boundaries():
    """the frames sit where they were chosen to sit with the constants now in the source"""
    assert (any_hit_head(tiles(40, 632)), any_hit_head(tiles(144, 176))) == (0, 384)
    assert any_hit_head(395) == 0 and any_hit_head(396) > 0 and tiles(40, 632) == 395 and tiles(144, 176) == 396
    for wh, tail in (((152, 168), 15), ((160, 160), 16), ((157, 163), 36)):
        n = tiles(*wh)
        assert any_hit_head(n) > 0 and n - any_hit_head(n) == tail, (wh, n)
    for wh in ((96, 64), (88, 72), (80, 80), (93, 70)):
        assert any_hit_head(tiles(*wh)) == 0 and primary_head(tiles(*wh)) == 0
    lo, hi = tiles(384, 352), tiles(368, 368)
    assert (lo, hi) == (2112, 2116)
    assert primary_head(lo) == 0 and primary_head(hi) > 0 and hi - primary_head(hi) == 68
    # the primary grid is the persistent one at every size
    assert _default("YRT_PRIMARY_PERSIST_MIN_ITEMS") == 0


@lru_cache(maxsize=None)
def oracle_frame(name, width, height, samples=1):
    return Oracle(name).envelope(height, samples, width=width)


@pytest.mark.gpu
@pytest.mark.parametrize("width,height", list(FRAMES), ids=[f"{w}x{h}" for w, h in FRAMES])
def test_head_tail_boundary_frames(yrt, width, height):
    name = "instance1k"
    ds = dev_scene(yrt, name)
    nlights = ds.host.info()["lights"]
    assert nlights > 0
    ref, lo, hi, nrays, trunc = oracle_frame(name, width, height)
    assert trunc == 0
    hits, rem = divmod(nrays - width * height, nlights)  # the oracle's shadow rays: one per light and hit
    assert rem == 0 and 0 < hits <= width * height
    try:
        ds.set_tile_lists("on")
        on, st = yrt.raytrace(ds, (0.1, 0.1, 0.1), height, 1, width=width, return_stats=True)
        lists = ds.tile_lists()
        ds.set_tile_lists("off")
        off, st_off = yrt.raytrace(ds, (0.1, 0.1, 0.1), height, 1, width=width, return_stats=True)
    finally:
        ds.set_tile_lists("auto")
    assert lists["camera"] and lists["bundles"], lists
    assert on.shape == ref.shape == (height, width, 4)
    assert st["rays"] == nrays
    assert st["camera_samples"] == width * height
    assert st["shadow_rays"] == nlights * hits
    assert_frame_parity(on, ref, lo, hi, f"{name} {width}x{height} ({FRAMES[(width, height)]})")
    np.testing.assert_array_equal(on.view(np.uint32), off.view(np.uint32))
    assert st_off["rays"] == nrays and st_off["shadow_rays"] == nlights * hits
