"""Light groups through the multi-chunk render loop.

The `chunks` library of tools/build_variants.py --tests splits a frame into chunks of 2^11
samples, so a 37 x 24 frame runs as 2 chunks at 4 spp and 4 at 9 spp: on the five-light scene of
light_groups_scene.py with mirrors (the mirror levels, every plane's fold records and
k_accumulate_groups per chunk, the per-sample planes and records carved behind each chunk's
workspace) and without (fused at 4 spp: the planes' sums in LDS; unfused at 9).
tests/light_groups_worker.py renders the same cases in one fresh child process per library, one
child at a time.

Asserted: the planes of `chunks` equal the default library's bit for bit, with the same
counters; the primary phase was launched more than once (2 to 4 times) by `chunks` and once by
the default library.

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

RES, WIDTH = 24, 37
CHILD_TIMEOUT = 300  # seconds: the child loads torch, uploads two scenes and renders four tiny frames
PLANES = ("group0", "group1", "group2", "ambient", "beauty")
STAT_KEYS = ("rays", "camera_samples", "shadow_rays", "shadow_rays_culled", "depth_truncated")
CASES = {f"{'mirrors' if m else 'flat'}-s{s}": {"id": f"{'mirrors' if m else 'flat'}-s{s}", "mirrors": m, "samples": s,
                                                "resolution": RES, "width": WIDTH, "max_depth": 16}
         for m in (True, False) for s in (2, 3)}


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
    d = tmp_path_factory.mktemp(f"light_groups_{lib}")
    cases, out = d / "cases.json", d / "out.npz"
    cases.write_text(json.dumps(list(CASES.values())))
    env = dict(os.environ, YRT_LIB=str(path))
    cmd = [sys.executable, str(ROOT / "tests" / "light_groups_worker.py"), str(cases), str(out)]
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
def test_chunked_light_groups_equal_the_whole_frames(cid, tmp_path_factory):
    base = results("default", tmp_path_factory)
    got = results("chunks", tmp_path_factory)
    for n in PLANES:
        a, b = got["z"][f"{cid}.{n}"], base["z"][f"{cid}.{n}"]
        assert a.shape == b.shape == (RES, WIDTH, 4)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=n)
        assert (b[..., :3] > 0).any(), n
    mirrors, s = CASES[cid]["mirrors"], CASES[cid]["samples"]
    m, bm = got["meta"]["cases"][cid], base["meta"]["cases"][cid]
    assert {k: m["stats"][k] for k in STAT_KEYS} == {k: bm["stats"][k] for k in STAT_KEYS}
    assert bm["launches"]["primary"] == 1, bm["launches"]
    assert m["launches"]["primary"] == {2: 2, 3: 4}[s], m["launches"]
    assert ("bounce" in bm["launches"]) == mirrors, bm["launches"]
    if mirrors or s == 3:  # unfused: one k_accumulate_groups launch per chunk
        assert m["launches"]["accumulate"] == m["launches"]["primary"], m["launches"]
    else:
        assert "accumulate" not in m["launches"], m["launches"]
