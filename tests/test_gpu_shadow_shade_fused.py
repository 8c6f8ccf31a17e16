"""Level 0's shadow rays and shading in one persistent grid (k_shadow_shade_persist,
YRT_SHADOW_SHADE_FUSE in wavefront.hip) against the oracle and against the two kernels it
replaces.

The cases (tests/shadow_shade_cases.py) are frames of 37 x 24 pixels with the tile lists forced
on: 1, 4, 16 and 64 spp, which the fused kernel takes, and 9 spp, which it must not; scenes with
textures, instances, the lines' sine lighting, reflective materials cut at one level (the
truncated branch and its counter), no lights, lights only, only sky, nothing at all, 5 lights
(past the four of the occlusion-up-front shape) and 33 (past the 32 of a lane's mask); and one
band of a three-rank split whose window is padded past the frame.

Asserted per case: the frame equals the oracle's (helpers.assert_frame_parity; the differing and
sensitive channels are printed); rays, camera_samples and depth_truncated are the oracle's, shadow_rays what its ray
count leaves after the camera rays, shadow_rays_culled within them; the timed launches show a
shadow phase and no shade phase exactly where run() must fuse, and a shade phase everywhere
else. One child process renders every case with the `unfused` library (tools/build_variants.py):
frames, counts and the culled count must be equal bit for bit. A handle that renders a fused
frame, a 9-spp frame and the fused frame again gives the first frame's bits.
"""
from __future__ import annotations

import importlib.util
import json
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import shadow_shade_cases as SC
from helpers import ROOT, Oracle, assert_frame_parity, assert_same_floats

CHILD_TIMEOUT = 300  # seconds: the child loads torch, uploads ten scenes and renders 52 tiny frames
CASES = SC.cases()
STAT_KEYS = ("rays", "camera_samples", "shadow_rays", "shadow_rays_culled", "depth_truncated")


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite needs one")
    return y


@pytest.fixture(scope="module")
def scenes(yrt, tmp_path_factory):
    return SC.Scenes(yrt, tmp_path_factory.mktemp("shadow_shade"))


_rendered = {}


def rendered(yrt, scenes, cid):
    """the default library's render of a case, once (shared: not to be written to)"""
    if cid not in _rendered:
        _, scene, samples, band = next(c for c in CASES if c[0] == cid)
        _rendered[cid] = SC.render(yrt, scenes.get(scene)[2], scene, samples, band)
    return _rendered[cid]


@lru_cache(maxsize=None)
def oracle_frame(path, scene, samples, band):
    rows = None
    if band:
        b, stride, off = SC.BAND
        rows = np.array([j for j in range(SC.RES) if (j // b) % stride == off], np.int32)
    return Oracle(path).envelope(SC.RES, samples, amb=SC.AMB, rows=rows, width=SC.WIDTH,
                                 max_depth=SC.max_depth_of(scene))


def test_cases_cover_both_paths():
    """the case list holds what the kernel's conditions tell apart (no GPU needed)"""
    assert {s * s for s in SC.FUSED_SAMPLES} == {1, 4, 16, 64} and 64 % SC.CONTROL_SAMPLES ** 2
    assert min(SC.BUILT_LIGHTS) > 4 and min(SC.BUILT_LIGHTS) <= 32 < max(SC.BUILT_LIGHTS)
    assert SC.takes_fused(5, 8) and not SC.takes_fused(33, 8) and not SC.takes_fused(0, 2) and not SC.takes_fused(1, 3)
    assert SC.WIDTH % 8 and SC.RES % 8 == 0 and SC.BAND_TILE_H > SC.BAND[0]
    assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_case_matches_oracle_and_takes_its_path(yrt, scenes, cid):
    _, scene, samples, band = next(c for c in CASES if c[0] == cid)
    host, path, _ = scenes.get(scene)
    nlights = host.info()["lights"]
    img, st, launches = rendered(yrt, scenes, cid)
    ref, lo, hi, nrays, trunc = oracle_frame(str(path), scene, samples, band)
    rows = ref.shape[0]
    got = img[:rows]
    print(f"{cid}: {nlights} lights, launches {launches}, { {k: st[k] for k in STAT_KEYS} }")
    if band:  # the window's rows past the frame: written as nothing
        assert rows == SC.BAND[0] and img.shape[0] == SC.BAND_TILE_H
        assert (img[rows:] == 0).all()
    assert_frame_parity(got, ref, lo, hi, f"shadow+shade {cid}")
    # the counts
    assert st["rays"] == nrays
    assert st["camera_samples"] == rows * SC.WIDTH * samples * samples
    assert st["depth_truncated"] == trunc
    assert st["shadow_rays"] == nrays - st["camera_samples"]  # one level: camera rays and shadow rays
    assert st["shadow_rays_culled"] <= st["shadow_rays"]
    if scene == "refl":
        assert trunc > 0, "the reflective hits of a one-level render take the truncated branch"
    if nlights == 0:
        assert st["shadow_rays"] == 0 and "shadow" not in launches
    # the path
    assert launches.get("primary") == 1, launches
    if SC.takes_fused(nlights, samples):
        assert launches.get("shadow") == 1 and "shade" not in launches and "accumulate" not in launches, launches
    else:
        assert launches.get("shade") == 1, launches
        assert ("shadow" in launches) == (nlights > 0), launches


def _variant_tool():
    spec = importlib.util.spec_from_file_location("yrt_build_variants", ROOT / "tools" / "build_variants.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_fused_equals_unfused_bit_for_bit(yrt, scenes, tmp_path):
    """every case on the `unfused` library, in one fresh child: the same bits, the same counts,
    and a shade launch in every case. A child that dies fails the test and nothing more is
    started."""
    tool = _variant_tool()
    assert tool.TEST_VARIANTS["unfused"] == ["-DYRT_SHADOW_SHADE_FUSE=0"]
    (lib,) = tool.main(["unfused:" + ",".join(tool.TEST_VARIANTS["unfused"])], default_library=False, verbose=False)
    out = tmp_path / "unfused.npz"
    cmd = [sys.executable, str(ROOT / "tests" / "shadow_shade_worker.py"), str(out)]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, YRT_LIB=str(lib)), capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"the unfused child ran into its {CHILD_TIMEOUT} s limit\n{err[-4000:]}")
    assert r.returncode == 0, f"the unfused child ended with status {r.returncode}\n{r.stderr[-4000:]}"
    z = np.load(out)
    meta = json.loads(str(z["meta"]))
    assert meta["library"] == str(lib)
    nfused = 0
    for cid, _, _, _ in CASES:
        img, st, launches = rendered(yrt, scenes, cid)
        assert_same_floats(img, z[f"{cid}.img"])
        m = meta["cases"][cid]
        assert {k: st[k] for k in STAT_KEYS} == {k: m["stats"][k] for k in STAT_KEYS}, cid
        assert m["launches"].get("shade") == 1, (cid, m["launches"])
        nfused += "shade" not in launches
    assert nfused >= 4 * 6  # the default library did fuse: four sample counts of at least six lit scenes


@pytest.mark.gpu
def test_no_stale_occlusion_bytes(yrt, scenes):
    """a fused frame, a 9-spp frame (which writes the occlusion bytes the fused kernel leaves
    alone) and the fused frame again on one handle: the first frame's bits"""
    ds = scenes.get("simple")[2]
    a, st_a, la = SC.render(yrt, ds, "simple", 2, False)
    _, _, lb = SC.render(yrt, ds, "simple", SC.CONTROL_SAMPLES, False)
    c, st_c, lc = SC.render(yrt, ds, "simple", 2, False)
    assert "shade" not in la and "shade" in lb and "shade" not in lc, (la, lb, lc)
    assert_same_floats(c, a)
    assert {k: st_a[k] for k in STAT_KEYS} == {k: st_c[k] for k in STAT_KEYS}
