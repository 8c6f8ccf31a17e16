"""The camera rays' list-mode closest hit as nested loops (packet_trace.h packet_first_list, the
default) against the flat loop it replaces (`flatwalk`, tools/build_variants.py TEST_VARIANTS,
-DYRT_FIRST_NESTED=0: k_primary_persist's list mode calls packet_first as before). Both
libraries render the same frames, one fresh child per library (tests/variant_worker.py and
tests/first_nested_worker.py with YRT_LIB naming the library): the images are compared as
uint32 and the stats are equal.

Frames: instance1k with camera lists at 64 x 8 (3 x 3 spp: the per-lane form, where an item
is not whole pixels), 45 x 27 (2 x 2), 8 x 200 (4 x 4) and 93 x 70 (8 x 8: the
wave-uniform pixel) -- partial tiles on both axes; `lines` at 37 x 24, 3 x 3 spp; instance100k
at 37 x 24, 2 x 2 spp (long lists, skip bits, many instances per leaf); and a scene with rotated,
identity and signed-zero-identity instance frames at 37 x 24, 2 x 2 and 8 x 8 spp, whose camera
rays hit all three kinds. `lines` has seven instances, too few for camera lists, so its frame
runs the primary grid's tree mode (unchanged code) under both libraries; the line and point
leaves of the list-mode walk are in the frames scene, which instances a line and a point shape
(tests/first_nested_worker.py) and whose camera rays hit both.

Waves without a list (ln < 0: the tree walked as the list's one virtual entry): a chunk is whole
tiles and a tile's samples are a multiple of 64, so no item straddles two tiles, and
k_camera_lists gives every tile a list; the one way left is a ray with a zero direction, which only
a camera with no extent produces. No test had one, so tests/first_nested_worker.py adds a camera
with focus 0 inside the instances' row and renders it under both libraries
(test_camera_without_extent_walks_the_tree).

A child that fails ends the module: no later test starts another.
"""
from __future__ import annotations

import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

CHILD_TIMEOUT = 300  # seconds: a child loads torch, uploads its scenes and renders tiny frames
STATS = ("rays", "camera_samples", "shadow_rays", "depth_truncated", "stack_overflow")


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


CASES = {c["id"]: c for c in (_case("instance1k", 64, 8, 3), _case("instance1k", 45, 27, 2),
                              _case("instance1k", 8, 200, 4), _case("instance1k", 93, 70, 8),
                              _case("lines", 37, 24, 3), _case("instance100k", 37, 24, 2))}


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
    d = tmp_path_factory.mktemp(f"nested_{kind}_{lib}")
    out = d / "out.npz"
    if kind == "cases":
        cases = d / "cases.json"
        cases.write_text(json.dumps(list(CASES.values())))
        cmd = [sys.executable, str(ROOT / "tests" / "variant_worker.py"), str(cases), str(out)]
    else:
        cmd = [sys.executable, str(ROOT / "tests" / "first_nested_worker.py"), str(out)]
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
    res = {"meta": json.loads(str(z["meta"])), "z": z}
    assert res["meta"]["library"] == str(path)
    _results[kind, lib] = res
    return res


def test_flatwalk_is_the_last_suite_variant():
    assert list(TOOL.TEST_VARIANTS)[-1] == "flatwalk"
    assert TOOL.TEST_VARIANTS["flatwalk"] == ["-DYRT_FIRST_NESTED=0"]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_nested_walk_renders_the_flat_walk_s_bits(cid, tmp_path_factory):
    base = _child("cases", "flatwalk", tmp_path_factory)
    got = _child("cases", "default", tmp_path_factory)
    np.testing.assert_array_equal(got["z"][f"{cid}.img"].view(np.uint32), base["z"][f"{cid}.img"].view(np.uint32))
    st, bst = got["meta"]["cases"][cid]["stats"], base["meta"]["cases"][cid]["stats"]
    assert {k: st[k] for k in STATS} == {k: bst[k] for k in STATS}
    c = CASES[cid]
    assert st["camera_samples"] == c["width"] * c["resolution"] * c["samples"] ** 2
    for r in (base, got):
        m = r["meta"]["cases"][cid]
        # the persistent primary grid in list mode: the kernel the knob changes (`lines`: too few
        # instances for lists, the module's docstring)
        assert m["launches"]["primary"] == 1 and m["tile_lists"]["camera"] == (c["scene"] != "lines"), m
    assert np.isfinite(got["z"][f"{cid}.img"]).all() and got["z"][f"{cid}.img"][..., :3].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("ns", (2, 8))
def test_rotated_identity_and_signed_zero_frames(ns, tmp_path_factory):
    base = _child("frames", "flatwalk", tmp_path_factory)
    got = _child("frames", "default", tmp_path_factory)
    np.testing.assert_array_equal(got["z"][f"s{ns}.img"].view(np.uint32), base["z"][f"s{ns}.img"].view(np.uint32))
    st, bst = got["meta"]["frames"][f"s{ns}"]["stats"], base["meta"]["frames"][f"s{ns}"]["stats"]
    assert {k: st[k] for k in STATS} == {k: bst[k] for k in STATS}
    assert st["camera_samples"] == 37 * 24 * ns * ns
    for r in (base, got):
        assert r["meta"]["frames"][f"s{ns}"]["tile_lists"]["camera"], r["meta"]["frames"][f"s{ns}"]
        # camera rays reach all three kinds of frame, among them the parity test's six (the
        # first two of each kind), and line and point leaves
        seen = set(r["meta"]["hit_instances"])
        for kind, insts in r["meta"]["instances"].items():
            assert seen & set(insts[:2]), (kind, insts[:2], sorted(seen))
        assert {r["meta"]["shapes"]["lines"], r["meta"]["shapes"]["points"]} <= set(r["meta"]["hit_shapes"]), r["meta"]
    np.testing.assert_array_equal(got["z"]["ids"], base["z"]["ids"])


@pytest.mark.gpu
def test_camera_without_extent_walks_the_tree(tmp_path_factory):
    """every direction is zero: no wave takes a list, each walks the tree from its root -- the
    same bits and counts in both walks"""
    base = _child("frames", "flatwalk", tmp_path_factory)
    got = _child("frames", "default", tmp_path_factory)
    img = got["z"]["nolist.img"]
    np.testing.assert_array_equal(img.view(np.uint32), base["z"]["nolist.img"].view(np.uint32))
    st, bst = got["meta"]["frames"]["nolist"]["stats"], base["meta"]["frames"]["nolist"]["stats"]
    assert {k: st[k] for k in STATS} == {k: bst[k] for k in STATS}
    assert st["camera_samples"] == 37 * 24 * 4
