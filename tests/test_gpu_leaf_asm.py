"""The nested walks' triangle leaves as generated leaf scans (leaf_asm.h, the default: YRT_LEAF_ASM
= 3) against the compiled loops they replace (`cleaf`, tools/build_variants.py TEST_VARIANTS,
-DYRT_LEAF_ASM=0: wavefront.hip's code object is then the one from before the scans). Both
libraries render the same frames, one fresh child per library and one child at a time
(tests/variant_worker.py and tests/leaf_asm_worker.py with YRT_LIB naming the library): the images
are equal as uint32 and the ray, culled and truncated counts are equal.

Frames, a few thousand pixels each, tile lists forced on (camera lists: k_primary_persist's list
mode, the closest hit's scan; level 0's shadow rays on the persistent any-hit grid, the any hit's):

  instance1k 45 x 27, 2 x 2 spp      the fused kernel; bundle lists; partial tiles on both axes
  instance1k 93 x 70, 8 x 8 spp      both kernels in the flagship's 64-spp form
  instance1k 64 x 8, 3 x 3 spp       9 spp does not fuse: k_shadow_persist<0> + k_shade
  instance100k 37 x 24, 2 x 2 spp    many instances per leaf
  lines 37 x 24, 3 x 3 spp           line leaves beside triangle leaves; too few instances for
                                     lists: the walks start at the tree's root (tree mode)
  the leaf scene 37 x 24, 2 x 2 and 8 x 8 spp (tests/leaf_asm_worker.py): one leaf of four
                                     triangles -- den == 0, a denormal den, and two visible ones
                                     met near-then-far and far-then-near -- a leaf of one
                                     triangle, and a light whose shadow rays cross them

test_the_leaf_scene_has_zero_and_denormal_determinants needs no GPU: it reads the leaf scene's
camera rays on the CPU (helpers.Oracle on the scene the worker's builder makes) and computes den
of the two degenerate triangles for the rays that hit the four-triangle leaf's instances, in
float32 and in tri_hit_mask's order.

Two of the cases and the leaf scene are also compared with the oracle's render
(helpers.assert_frame_parity), under both libraries.

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

sys.path.insert(0, str(ROOT / "tests"))
import leaf_asm_worker as W  # noqa: E402

CHILD_TIMEOUT = 300  # seconds: a child loads torch, uploads its scenes and renders tiny frames
STATS = ("rays", "camera_samples", "shadow_rays", "shadow_rays_culled", "depth_truncated")
LIBS = ("cleaf", "default")
WIDTH, HEIGHT = W.WIDTH, W.HEIGHT


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
                              _case("lines", 37, 24, 3))}
ORACLE_CASES = ("instance1k-45x27-s2", "lines-37x24-s3")


def lib_path(lib):
    if lib == "default":
        return ROOT / "yocto_raytracing_amd" / "libyrt.so"
    (path,) = TOOL.main([f"{lib}:{','.join(TOOL.TEST_VARIANTS[lib])}"], default_library=False, verbose=False)
    return path


_results = {}
_dead = None


def _child(kind, lib, tmp_path_factory):
    """the stored output of one worker on one library (kind: "cases" or "leaf")"""
    global _dead
    if (kind, lib) in _results:
        return _results[kind, lib]
    if _dead:
        pytest.fail(f"no child is started after a failed one: {_dead}")
    path = lib_path(lib)
    assert path.exists(), f"{path}: build the library first"
    d = tmp_path_factory.mktemp(f"leaf_asm_{kind}_{lib}")
    out = d / "out.npz"
    if kind == "cases":
        cases = d / "cases.json"
        cases.write_text(json.dumps(list(CASES.values())))
        cmd = [sys.executable, str(ROOT / "tests" / "variant_worker.py"), str(cases), str(out)]
    else:
        cmd = [sys.executable, str(ROOT / "tests" / "leaf_asm_worker.py"), str(out), str(d / "leaf.yrtscene")]
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


def test_cleaf_is_a_suite_variant_between_unfused_and_flatany():
    names = list(TOOL.TEST_VARIANTS)
    assert TOOL.TEST_VARIANTS["cleaf"] == ["-DYRT_LEAF_ASM=0"]
    assert names.index("unfused") + 1 == names.index("cleaf") == names.index("flatany") - 1
    assert names.index("flatany") < names.index("flatwalk") == len(names) - 1


# ---- the leaf scene on the CPU ----

@pytest.fixture(scope="module")
def leaf_scene(tmp_path_factory):
    import yocto_raytracing_amd as yrt

    s, inst, view = W.build_leaf_scene(yrt)
    path = tmp_path_factory.mktemp("leaf_scene") / "leaf.yrtscene"
    s.save(str(path))
    return path, inst, view


def _camera_rays(o, camera, samples):
    rays = np.zeros((HEIGHT, WIDTH, samples, samples, 8), np.float32)
    ray = (C.c_float * 8)()
    for j in range(HEIGHT):
        for i in range(WIDTH):
            for jj in range(samples):
                for ii in range(samples):
                    assert o.lib.oracle_camera_ray(o.h, camera, HEIGHT, WIDTH, samples, i, j, ii, jj, ray) == 0
                    rays[j, i, jj, ii] = ray[:]
    return rays.reshape(-1, 8)


def _den(d, e1, e2):
    """dot(cross(d, e2), e1) in float32, products and sums apart, in tri_hit_mask's order"""
    f = np.float32
    d, e1, e2 = d.astype(f), np.asarray(e1, f), np.asarray(e2, f)
    r = np.stack([d[:, 1] * e2[2] - d[:, 2] * e2[1], d[:, 2] * e2[0] - d[:, 0] * e2[2],
                  d[:, 0] * e2[1] - d[:, 1] * e2[0]], 1)
    return (r[:, 0] * e1[0] + r[:, 1] * e1[1]) + r[:, 2] * e1[2]


def test_the_leaf_scene_has_zero_and_denormal_determinants(leaf_scene):
    path, inst, view = leaf_scene
    o = Oracle(str(path))
    rays = _camera_rays(o, view, 2)
    first = o.trace(rays)
    tiny = np.finfo(np.float32).tiny  # 2^-126: below it rcp_nr_ok fails
    for name, turn in (("near_far", 1.0), ("far_near", -1.0)):
        reach = first["hit"] & (first["inst"] == inst[name])  # these rays' waves reach the leaf
        assert reach.sum() >= 8, (name, int(reach.sum()))
        # the instance's direction: the identity's is the ray's own; the half turn negates x and z
        # (and renormalises: a few ulp, nothing to a denormal's range)
        d = rays[reach, 3:6] * np.array([turn, 1.0, turn], np.float32)
        p = W.QUAD_POS
        zero = _den(d, p[1] - p[0], p[2] - p[0])
        assert (zero == 0).all()
        den = _den(d, p[4] - p[3], p[5] - p[3])
        assert ((den != 0) & (np.abs(den) < tiny)).all(), den
        # and the two visible triangles are normal: the scan's own path
        for k in (6, 9):
            vis = _den(d, p[k + 1] - p[k], p[k + 2] - p[k])
            assert (np.abs(vis) >= tiny).all()
        # some rays cross both visible triangles: the near one is their hit (element 2 under the
        # identity, 3 after the half turn), and from just behind it they hit the other
        near, far = (2, 3) if name == "near_far" else (3, 2)
        front = reach & (first["ei"] == near)
        assert front.sum() >= 8, (name, int(front.sum()))
        behind = rays[front].copy()
        behind[:, 6] = first["dist"][front] + 1e-3  # tmin
        second = o.trace(behind)
        both = second["hit"] & (second["inst"] == inst[name]) & (second["ei"] == far)
        assert both.sum() >= 8, (name, int(both.sum()))
    assert (first["hit"] & (first["inst"] == inst["single"])).sum() >= 4
    for ns in W.SAMPLES:
        img, _, _, nrays, _ = _oracle_render(str(path), WIDTH, HEIGHT, ns, 16, view)
        assert np.isfinite(img).all() and nrays > WIDTH * HEIGHT * ns * ns


# ---- the GPU comparisons ----

def _same_frame(got, base, m, bm, pixels, spp):
    np.testing.assert_array_equal(got.view(np.uint32), base.view(np.uint32))
    st, bst = m["stats"], bm["stats"]
    print({k: st[k] for k in STATS}, m["launches"])
    assert {k: st[k] for k in STATS} == {k: bst[k] for k in STATS}
    assert st["camera_samples"] == pixels * spp
    for x in (bm, m):  # under either library
        assert x["launches"]["shadow"] >= 1, x  # the persistent any-hit grid ran
        assert 0 < x["stats"]["shadow_rays_culled"] < x["stats"]["shadow_rays"], x["stats"]
    assert np.isfinite(got).all() and got[..., :3].max() > 0.1  # (the ambient term alone is below)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_leaf_scans_render_the_compiled_loops_bits(cid, tmp_path_factory):
    base = _child("cases", "cleaf", tmp_path_factory)
    got = _child("cases", "default", tmp_path_factory)
    c = CASES[cid]
    m, bm = got["meta"]["cases"][cid], base["meta"]["cases"][cid]
    _same_frame(got["z"][f"{cid}.img"], base["z"][f"{cid}.img"], m, bm, c["width"] * c["resolution"], c["samples"] ** 2)
    for x in (bm, m):
        # camera lists and bundle lists where the scene has enough instances; `lines`: the tree's root
        if c["scene"].startswith("instance"):
            assert x["tile_lists"]["bundles"], x
        elif c["scene"] == "lines":
            assert not x["tile_lists"]["bundles"], x
        # 9 spp does not fuse: the shading is a launch of its own
        if c["samples"] == 3:
            assert x["launches"].get("shade", 0) >= 1, x


@lru_cache(maxsize=None)
def _oracle_render(scene, width, height, samples, max_depth, camera=0):
    """(ref, lo, hi, rays, truncated): the oracle's frame and its pow envelope"""
    return Oracle(scene).envelope(height, samples, width=width, max_depth=max_depth, camera=camera)


@pytest.mark.gpu
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("cid", ORACLE_CASES)
def test_both_leaf_forms_match_the_oracle(cid, lib, tmp_path_factory):
    c = CASES[cid]
    got = _child("cases", lib, tmp_path_factory)
    img, st = got["z"][f"{cid}.img"], got["meta"]["cases"][cid]["stats"]
    ref, lo, hi, nrays, trunc = _oracle_render(c["scene"], c["width"], c["resolution"], c["samples"], c["max_depth"])
    assert img.shape == ref.shape
    assert st["rays"] == nrays and st["depth_truncated"] == trunc
    assert_frame_parity(img, ref, lo, hi, f"leaf asm {cid} {lib}")


@pytest.mark.gpu
@pytest.mark.parametrize("ns", W.SAMPLES)
def test_degenerate_and_ordered_triangles_in_one_leaf(ns, tmp_path_factory):
    base = _child("leaf", "cleaf", tmp_path_factory)
    got = _child("leaf", "default", tmp_path_factory)
    m, bm = got["meta"]["frames"][f"s{ns}"], base["meta"]["frames"][f"s{ns}"]
    _same_frame(got["z"][f"s{ns}.img"], base["z"][f"s{ns}.img"], m, bm, WIDTH * HEIGHT, ns * ns)
    for x in (bm, m):
        assert x["tile_lists"]["bundles"], x


@pytest.mark.gpu
@pytest.mark.parametrize("lib", LIBS)
@pytest.mark.parametrize("ns", W.SAMPLES)
def test_the_leaf_scene_matches_the_oracle(ns, lib, tmp_path_factory):
    got = _child("leaf", lib, tmp_path_factory)
    meta = got["meta"]
    img, st = got["z"][f"s{ns}.img"], meta["frames"][f"s{ns}"]["stats"]
    ref, lo, hi, nrays, trunc = _oracle_render(str(got["dir"] / "leaf.yrtscene"), WIDTH, HEIGHT, ns, 16, meta["camera"])
    assert img.shape == ref.shape
    assert st["rays"] == nrays and st["depth_truncated"] == trunc
    assert_frame_parity(img, ref, lo, hi, f"leaf scene s{ns} {lib}")
