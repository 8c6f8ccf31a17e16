"""The item geometry of the persistent grids (wavefront.hip, YRT_ITEM_MAGIC: the pixel
enumeration's divisions as multiply-high pairs, the item's tile on the scalar unit where an
item lies in one tile) on small frames of the default library, against the oracle.

Frames with partial tiles on both axes (45 x 27, 93 x 70), exactly one tile row (64 x 8) and
one tile column (8 x 200, tiles_x == 1); 1, 4, 16 and 64 samples per pixel, the shapes whose
items are whole pixels of one tile (the fused any-hit + shading grid; at 64 spp the pixel is
wave-uniform), and 9 spp, the per-lane form on the two-kernel path; interleaved bands whose
height is a multiple of the tile's (8, 16) and one that is not (5); a window with a nonzero
origin whose width cuts a tile. The tile lists are forced on, which puts the shadow rays on the
persistent any-hit grid at any size (tests/test_gpu_frame_shapes.py), and every frame is
rendered again with the lists off: the same bits.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

from helpers import Oracle, assert_frame_parity, scene_path

SCENES = ("instance1k", "simple")
FRAMES = ((45, 27), (93, 70), (64, 8), (8, 200))
SAMPLES = (1, 2, 4, 8, 3)
BANDS = ((8, 3, 1), (16, 2, 1), (5, 2, 1))
WINDOW = (5, 3, 43, 30)  # x0, y0, w, h in the 93 x 70 frame: columns 5 .. 47, rows 3 .. 32


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


@lru_cache(maxsize=None)
def oracle(name):
    return Oracle(name)


def render_both(yrt, ds, shape, **kw):
    """the frame with the lists forced on and off: (image, stats) of each"""
    out = []
    try:
        for mode in ("on", "off"):
            ds.set_tile_lists(mode)
            img = np.full(shape, 77, np.float32)
            ds.render_into(yrt.render_params(0.1, **kw), img.ctypes.data, device_memory=False)
            out.append((img, ds.last_stats()))
    finally:
        ds.set_tile_lists("auto")
    return out


def check(name, got, env, nsamples, rows=None):
    """both renders against the oracle's frame, pow envelope and counts (env: Oracle.envelope's
    result), and against each other bit for bit; rows: the buffer's rows the frame has (the others
    are written as zeros)"""
    (on, st), (off, st_off) = got
    ref, lo, hi, nrays, _ = env
    rows = np.arange(on.shape[0]) if rows is None else rows
    assert on[rows].shape == ref.shape
    print(f"{name}: rays {st['rays']}")
    for s in (st, st_off):
        assert s["rays"] == nrays
        assert s["camera_samples"] == nsamples
        assert s["shadow_rays"] == nrays - nsamples  # (no mirrors: one ray per sample, the rest shadow rays)
    assert_frame_parity(on[rows], ref, lo, hi, name)
    rest = np.setdiff1d(np.arange(on.shape[0]), rows)
    assert (on[rest] == 0).all()
    np.testing.assert_array_equal(on.view(np.uint32), off.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("samples", SAMPLES)
@pytest.mark.parametrize("width,height", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
@pytest.mark.parametrize("scene", SCENES)
def test_frames(yrt, scene, width, height, samples):
    ds = dev_scene(yrt, scene)
    env = oracle(scene).envelope(height, samples, width=width)
    assert env[4] == 0
    got = render_both(yrt, ds, (height, width, 4), resolution=height, samples=samples, width=width)
    check(f"{scene} {width}x{height} s{samples}", got, env, width * height * samples * samples)


@pytest.mark.gpu
@pytest.mark.parametrize("samples", (2, 8, 3))
@pytest.mark.parametrize("band", BANDS, ids=["x".join(map(str, b)) for b in BANDS])
def test_bands(yrt, band, samples):
    """93 x 70 in interleaved bands: local row ly is image row (ly // band * stride + offset) * band
    + ly % band; the window is whole bands, so the last band's rows past the image are zeros"""
    scene, (width, height) = "instance1k", (93, 70)
    ds = dev_scene(yrt, scene)
    size, stride, offset = band
    bands_total = -(-height // size)
    mine = len(range(offset, bands_total, stride))
    local = np.arange(mine * size)
    image_rows = (local // size * stride + offset) * size + local % size
    have = image_rows < height
    assert mine >= 2 and have.sum() >= 8
    env = oracle(scene).envelope(height, samples, width=width, rows=image_rows[have])
    got = render_both(yrt, ds, (len(local), width, 4), resolution=height, samples=samples, width=width, band=band)
    check(f"band {band} s{samples}", got, env, int(have.sum()) * width * samples * samples, rows=local[have])


@pytest.mark.gpu
@pytest.mark.parametrize("samples", (2, 8, 3))
@pytest.mark.parametrize("scene", SCENES)
def test_window(yrt, scene, samples):
    width, height = 93, 70
    x0, y0, w, h = WINDOW
    assert x0 % 8 and y0 % 8 and w % 8 and h % 8
    ds = dev_scene(yrt, scene)
    env = oracle(scene).envelope(height, samples, width=width, rows=np.arange(y0, y0 + h), x0=x0, ncols=w)
    got = render_both(yrt, ds, (h, w, 4), resolution=height, samples=samples, width=width, window=WINDOW)
    check(f"{scene} window s{samples}", got, env, w * h * samples * samples)
