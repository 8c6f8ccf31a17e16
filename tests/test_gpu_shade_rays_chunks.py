"""Ray batches through the multi-chunk loop of the wavefront pipeline's ray mode.

The `chunks` library of tools/build_variants.py --tests splits a batch into chunks of 2^11 rays,
so the 7 992 rays of a 37 x 24 frame at s = 3 run as 4 chunks (the last one partial: 1 848 rays)
and the 888 rays at s = 1 as one: on the built scene and on `refl` (both reflective: the mirror
levels and the fold's write into the caller's buffer per chunk, at the chunk's offset) and on
`simple`. tests/shade_rays_worker.py shades the same batches in one fresh child process per
library, one child at a time.

Asserted: the colours and the counters of `chunks` equal the default library's bit for bit; the
primary phase (the level-0 closest hit) was launched once per chunk by `chunks` and once by the
default library.

A child that ends by a signal, an abort, a time limit or any error fails its test with the
child's stderr, and the other tests of this module then fail without starting a child.
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

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300  # seconds: the child loads torch, uploads three scenes and shades six tiny batches
STAT_KEYS = ("rays", "camera_samples", "shadow_rays", "shadow_rays_culled", "depth_truncated")
NRAYS = {1: 888, 3: 7992}
CHUNKS = {1: 1, 3: 4}  # of 2^11 rays
CASES = {f"{scene}-s{s}": {"id": f"{scene}-s{s}", "scene": scene, "samples": s, "max_depth": 16}
         for scene in ("built", "refl", "simple") for s in (1, 3)}


def _tool():
    spec = importlib.util.spec_from_file_location("yrt_build_variants", ROOT / "tools" / "build_variants.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def lib_path(lib):
    if lib == "default":
        return ROOT / "yocto_raytracing_amd" / "libyrt.so"
    tool = _tool()
    paths = tool.main(tool.test_specs(), default_library=False, verbose=False)
    return dict(zip(tool.TEST_VARIANTS, paths))[lib]


_results = {}
_dead = None  # why no further child is started


def results(lib, tmp_path_factory):
    global _dead
    if lib in _results:
        return _results[lib]
    if _dead:
        pytest.fail(f"no child is started after a failed one: {_dead}")
    path = lib_path(lib)
    assert path.exists(), f"{path}: build the library first"
    d = tmp_path_factory.mktemp(f"shade_rays_{lib}")
    cases, out = d / "cases.json", d / "out.npz"
    cases.write_text(json.dumps(list(CASES.values())))
    env = dict(os.environ, YRT_LIB=str(path))
    cmd = [sys.executable, str(ROOT / "tests" / "shade_rays_worker.py"), str(cases), str(out)]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _dead = f"the {lib} child ran into its {CHILD_TIMEOUT} s limit"
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"{_dead}\n{err[-4000:]}")
    if r.returncode != 0:
        _dead = f"the {lib} child ended with status {r.returncode}"
        pytest.fail(f"{_dead}\n{r.stderr[-4000:]}")
    z = np.load(out)
    res = {"meta": json.loads(str(z["meta"])), "z": z}
    assert res["meta"]["library"] == str(path)
    _results[lib] = res
    return res


@pytest.mark.parametrize("cid", list(CASES))
def test_chunked_batches_equal_the_whole_batches(cid, tmp_path_factory):
    base = results("default", tmp_path_factory)
    got = results("chunks", tmp_path_factory)
    s = CASES[cid]["samples"]
    a, b = got["z"][f"{cid}.rgba"], base["z"][f"{cid}.rgba"]
    assert a.shape == b.shape == (NRAYS[s], 4)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (b[:, 3] == 1).all() and (b[:, :3] > 0).any()
    m, bm = got["meta"]["cases"][cid], base["meta"]["cases"][cid]
    assert {k: m["stats"][k] for k in STAT_KEYS} == {k: bm["stats"][k] for k in STAT_KEYS}
    assert bm["stats"]["camera_samples"] == NRAYS[s]
    assert bm["launches"]["primary"] == 1, bm["launches"]
    assert m["launches"]["primary"] == CHUNKS[s], m["launches"]
    assert "accumulate" not in m["launches"] and "accumulate" not in bm["launches"]
