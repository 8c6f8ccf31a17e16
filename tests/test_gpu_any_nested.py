"""The persistent any-hit grids' walk as nested loops (packet_trace.h packet_occluded_nested, the
default) against the flat loop it replaces (`flatany`, tools/build_variants.py TEST_VARIANTS,
-DYRT_ANY_NESTED=0: shadow_item_light calls packet_occluded_wide2 as before). Both libraries
render the same frames, one fresh child per library and one child at a time
(tests/variant_worker.py and tests/any_nested_worker.py with YRT_LIB naming the library): the
images are equal as uint32 and the counts are equal.

Frames, a few thousand pixels each, tile lists forced on (level 0's shadow rays then run on the
persistent any-hit grid at any frame size):

  instance1k 45 x 27, 2 x 2 spp      the fused kernel; bundle lists; partial tiles on both axes
  instance1k 93 x 70, 8 x 8 spp      the fused kernel in the flagship's 64-spp form
  instance1k 64 x 8, 3 x 3 spp       9 spp does not fuse: k_shadow_persist<0> + k_shade
  instance100k 37 x 24, 2 x 2 spp    many instances per leaf, skip bits: the nested walk leaves a
                                     leaf whose lanes are all answered, the flat one enters the rest
  lines 37 x 24, 3 x 3 spp           seven instances, too few for bundles: the walk starts at the
                                     tree's root (tree mode); line leaves
  refl 37 x 24, 2 x 2 spp, depth 16  level 0 on k_shadow_persist<0>, the mirror levels on k_shadow
                                     (unchanged code)
  the frames scene 37 x 24, 2 x 2 and 8 x 8 spp (tests/any_nested_worker.py): rotated, identity and
                                     signed-zero-identity frames, a line shape and a point shape,
                                     and a light whose shadow rays cross them

Every frame has 0 < shadow_rays_culled < shadow_rays under either library, so waves start their
walk with some lanes answered (pre_done) and some walking. For the frames scene the test reads the
shadow rays on the CPU (helpers.Oracle on the scene the child saved): the camera samples' hit
points, and the closest hit of each one's ray towards the added light -- one occluder of the ray,
which intersect_any's walk has to meet unless it finds another first. Those occluders include
instances of each kind of frame and both the line and the point shape.

Two of the cases are also compared with the oracle's render (helpers.assert_frame_parity), under both
libraries.

A child that fails -- a signal, an abort, its time limit, an error -- fails its test, and no later
test starts another.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

from helpers import ROOT, Oracle, assert_frame_parity

CHILD_TIMEOUT = 300  # seconds: a child loads torch, uploads its scenes and renders tiny frames
STATS = ("rays", "camera_samples", "shadow_rays", "shadow_rays_culled", "depth_truncated")
LIBS = ("flatany", "default")
WIDTH, HEIGHT = 37, 24  # the frames scene's frame (tests/first_nested_worker.py)


def _tool():
    spec = importlib.util.spec_from_file_location("yrt_build_variants", ROOT / "tools" / "build_variants.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


def _case(scene, width, height, samples):
    return {"id": f"{scene}-{width}x{height}-s{samples}", "kind": "render", "scene": scene, "resolution": height,
            "width": width, "samples": samples, "max_depth": 16, "lists": "on", "algorithm": "wavefront",
            "count_work": False}


CASES = {c["id"]: c for c in (_case("instance1k", 45, 27, 2), _case("instance1k", 93, 70, 8),
                              _case("instance1k", 64, 8, 3), _case("instance100k", 37, 24, 2),
                              _case("lines", 37, 24, 3), _case("refl", 37, 24, 2))}
ORACLE_CASES = ("instance1k-45x27-s2", "lines-37x24-s3")


def lib_path(lib):
    if lib == "default":
        return ROOT / "yocto_raytracing_amd" / "libyrt.so"
    (path,) = TOOL.main([f"{lib}:{','.join(TOOL.TEST_VARIANTS[lib])}"], default_library=False, verbose=False)
    return path


_results = {}
_dead = None


def _child(kind, lib, tmp_path_factory):
    """the stored output of one worker on one library (kind: "cases" or "frames")"""
    global _dead
    if (kind, lib) in _results:
        return _results[kind, lib]
    if _dead:
        pytest.fail(f"no child is started after a failed one: {_dead}")
    path = lib_path(lib)
    assert path.exists(), f"{path}: build the library first"
    d = tmp_path_factory.mktemp(f"any_nested_{kind}_{lib}")
    out = d / "out.npz"
    if kind == "cases":
        cases = d / "cases.json"
        cases.write_text(json.dumps(list(CASES.values())))
        cmd = [sys.executable, str(ROOT / "tests" / "variant_worker.py"), str(cases), str(out)]
    else:
        cmd = [sys.executable, str(ROOT / "tests" / "any_nested_worker.py"), str(out), str(d / "frames.yrtscene")]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, YRT_LIB=str(path)), capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _dead = f"the {lib} {kind} child ran into its {CHILD_TIMEOUT} s limit"
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"{_dead}\n{err[-4000:]}")
    if r.returncode != 0:
        _dead = f"the {lib} {kind} child ended with status {r.returncode}"
        pytest.fail(f"{_dead}\n{r.stderr[-4000:]}")
    z = np.load(out)
    res = {"meta": json.loads(str(z["meta"])), "z": z, "dir": d}
    assert res["meta"]["library"] == str(path)
    _results[kind, lib] = res
    return res


def test_flatany_is_a_suite_variant_before_flatwalk():
    names = list(TOOL.TEST_VARIANTS)
    assert TOOL.TEST_VARIANTS["flatany"] == ["-DYRT_ANY_NESTED=0"]
    assert names.index("flatany") < names.index("flatwalk") == len(names) - 1


def _same_frame(got, base, m, bm, pixels, spp):
    np.testing.assert_array_equal(got.view(np.uint32), base.view(np.uint32))
    st, bst = m["stats"], bm["stats"]
    print({k: st[k] for k in STATS}, m["launches"])
    assert {k: st[k] for k in STATS} == {k: bst[k] for k in STATS}
    assert st["camera_samples"] == pixels * spp
    for x in (bm, m):  # under either library, the flat one alone included
        # the persistent any-hit grid ran, its waves started with some lanes answered and some walking
        assert x["launches"]["shadow"] >= 1, x
        assert 0 < x["stats"]["shadow_rays_culled"] < x["stats"]["shadow_rays"], x["stats"]
    assert np.isfinite(got).all() and got[..., :3].max() > 0.1  # (the ambient term alone is below)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_nested_any_hit_renders_the_flat_walk_s_bits(cid, tmp_path_factory):
    base = _child("cases", "flatany", tmp_path_factory)
    got = _child("cases", "default", tmp_path_factory)
    c = CASES[cid]
    m, bm = got["meta"]["cases"][cid], base["meta"]["cases"][cid]
    _same_frame(got["z"][f"{cid}.img"], base["z"][f"{cid}.img"], m, bm, c["width"] * c["resolution"], c["samples"] ** 2)
    for x in (bm, m):
        # bundle lists where the scene has enough instances for them; `lines`: the tree's root
        if c["scene"].startswith("instance"):
            assert x["tile_lists"]["bundles"], x
        elif c["scene"] == "lines":
            assert not x["tile_lists"]["bundles"], x
        # 9 spp does not fuse: the shading is a launch of its own
        if c["samples"] == 3:
            assert x["launches"].get("shade", 0) >= 1, x


@lru_cache(maxsize=None)
def _oracle_render(scene, width, height, samples, max_depth):
    """(ref, lo, hi, rays, truncated): the oracle's frame and its pow envelope"""
    return Oracle(scene).envelope(height, samples, width=width, max_depth=max_depth)


@pytest.mark.gpu
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("cid", ORACLE_CASES)
def test_both_walks_match_the_oracle(cid, lib, tmp_path_factory):
    c = CASES[cid]
    got = _child("cases", lib, tmp_path_factory)
    img, st = got["z"][f"{cid}.img"], got["meta"]["cases"][cid]["stats"]
    ref, lo, hi, nrays, trunc = _oracle_render(c["scene"], c["width"], c["resolution"], c["samples"], c["max_depth"])
    assert img.shape == ref.shape
    assert st["rays"] == nrays and st["depth_truncated"] == trunc
    assert_frame_parity(img, ref, lo, hi, f"any nested {cid} {lib}")


@pytest.mark.gpu
@pytest.mark.parametrize("ns", (2, 8))
def test_rotated_identity_and_signed_zero_frames(ns, tmp_path_factory):
    base = _child("frames", "flatany", tmp_path_factory)
    got = _child("frames", "default", tmp_path_factory)
    m, bm = got["meta"]["frames"][f"s{ns}"], base["meta"]["frames"][f"s{ns}"]
    _same_frame(got["z"][f"s{ns}.img"], base["z"][f"s{ns}.img"], m, bm, WIDTH * HEIGHT, ns * ns)
    for x in (bm, m):
        assert x["tile_lists"]["bundles"], x


def light_occluders(scene_file, camera, light_pos, samples):
    """per camera sample of the 37 x 24 frame that hits a surface: the instance its ray towards
    `light_pos` hits first (-1: none) -- the reference's shadow ray, from the hit point, tmin 0.01,
    tmax the distance less 0.01"""
    o = Oracle(str(scene_file))
    rays = np.zeros((HEIGHT, WIDTH, samples, samples, 8), np.float32)
    ray = (C.c_float * 8)()
    for j in range(HEIGHT):
        for i in range(WIDTH):
            for jj in range(samples):
                for ii in range(samples):
                    assert o.lib.oracle_camera_ray(o.h, camera, HEIGHT, WIDTH, samples, i, j, ii, jj, ray) == 0
                    rays[j, i, jj, ii] = ray[:]
    rays = rays.reshape(-1, 8)
    first = o.trace(rays)
    hit = first["hit"]
    p = rays[hit, :3] + rays[hit, 3:6] * first["dist"][hit, None]
    to = np.asarray(light_pos, np.float32)[None] - p
    r = np.linalg.norm(to, axis=1).astype(np.float32)
    srays = np.concatenate([p, to / r[:, None], np.full((len(p), 1), 0.01, np.float32), (r - 0.01)[:, None]],
                           1).astype(np.float32)
    occ = o.trace(srays)
    return np.where(occ["hit"], occ["inst"], -1), first["inst"][hit]


@pytest.mark.gpu
def test_the_light_s_shadow_rays_cross_every_kind_of_frame_and_leaf(tmp_path_factory):
    got = _child("frames", "flatany", tmp_path_factory)
    meta = got["meta"]
    assert meta["light"] is not None and meta["nlights"] >= 1
    occluders, _ = light_occluders(got["dir"] / "frames.yrtscene", meta["camera"], meta["light_pos"], 2)
    _check_occluders(meta, occluders)


def _check_occluders(meta, occluders):
    seen = set(int(v) for v in np.unique(occluders)) - {-1}
    assert (occluders == -1).any()  # some samples see the light
    for kind, insts in meta["instances"].items():
        assert seen & set(insts), (kind, sorted(seen))
    # row 1 of the added instances holds the line and the point shape, alternating (k % 2)
    row1 = sorted(i for insts in meta["instances"].values() for i in insts)[6:12]
    assert seen & set(row1[0::2]), ("lines", row1, sorted(seen))
    assert seen & set(row1[1::2]), ("points", row1, sorted(seen))
