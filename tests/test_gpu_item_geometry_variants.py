"""The item geometry knob, the light-carry knob and the multi-chunk path, through the variant runner
(tests/variant_worker.py with YRT_LIB naming the library, one fresh child per library).

`itemdiv` (tools/build_variants.py KNOB_VARIANTS, -DYRT_ITEM_MAGIC=0) is the old text: the
emulated divisions and the per-item range checks. It and the default library render four of
tests/test_gpu_item_geometry.py's frames with identical bits and equal counts; so does
`nocarry` (-DYRT_LIGHT_CARRY=0), whose fused grid computes every light's direction and distance
again in its shading instead of carrying them from the light step (instance1k has three
lights; scenes with more than the four carried ones run in tests/test_gpu_shadow_shade_fused.py,
fused against unfused). `chunks`
(YRT_CHUNK_LOG2=11) renders 93 x 70 at 8 x 8 spp as 108 chunks of one tile, so every chunk but
the first has pix0 != 0: the same bits as the default library's single chunk.

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

CHILD_TIMEOUT = 300  # seconds: the child loads torch, uploads one scene and renders 8 tiny frames
STATS = ("rays", "camera_samples", "shadow_rays", "depth_truncated", "stack_overflow")


def _tool():
    spec = importlib.util.spec_from_file_location("yrt_build_variants", ROOT / "tools" / "build_variants.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


def _case(width, height, samples):
    return {"id": f"{width}x{height}-s{samples}", "kind": "render", "scene": "instance1k", "resolution": height,
            "width": width, "samples": samples, "max_depth": 16, "lists": "on", "algorithm": "wavefront",
            "count_work": False}


# the per-lane form at 9 spp, the fused shapes at 4 / 16 / 64 spp (64: the wave-uniform pixel)
CASES = {c["id"]: c for c in (_case(64, 8, 3), _case(45, 27, 2), _case(8, 200, 4), _case(93, 70, 8))}
CHUNKED = "93x70-s8"


def lib_path(lib):
    if lib == "default":
        return ROOT / "yocto_raytracing_amd" / "libyrt.so"
    defs = {**TOOL.TEST_VARIANTS, **TOOL.KNOB_VARIANTS}[lib]
    (path,) = TOOL.main([f"{lib}:{','.join(defs)}"], default_library=False, verbose=False)
    return path


_results = {}
_dead = None


def results(lib, tmp_path_factory):
    global _dead
    if lib in _results:
        return _results[lib]
    if _dead:
        pytest.fail(f"no child is started after a failed one: {_dead}")
    path = lib_path(lib)
    assert path.exists(), f"{path}: build the library first"
    d = tmp_path_factory.mktemp(f"item_{lib}")
    cases, out = d / "cases.json", d / "out.npz"
    cases.write_text(json.dumps(list(CASES.values())))
    cmd = [sys.executable, str(ROOT / "tests" / "variant_worker.py"), str(cases), str(out)]
    try:
        r = subprocess.run(cmd, env=dict(os.environ, YRT_LIB=str(path)), capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT)
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


def test_knob_variant_is_the_old_text():
    assert TOOL.KNOB_VARIANTS == {"itemdiv": ["-DYRT_ITEM_MAGIC=0"], "nocarry": ["-DYRT_LIGHT_CARRY=0"]}
    assert not set(TOOL.KNOB_VARIANTS) & set(TOOL.TEST_VARIANTS)
    assert [s.split(":")[0] for s in TOOL.test_specs()] == [*TOOL.TEST_VARIANTS, *TOOL.KNOB_VARIANTS]


def same(got, base, cid):
    np.testing.assert_array_equal(got["z"][f"{cid}.img"].view(np.uint32), base["z"][f"{cid}.img"].view(np.uint32))
    st, bst = got["meta"]["cases"][cid]["stats"], base["meta"]["cases"][cid]["stats"]
    assert {k: st[k] for k in STATS} == {k: bst[k] for k in STATS}
    c = CASES[cid]
    assert st["camera_samples"] == c["width"] * c["resolution"] * c["samples"] ** 2


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
@pytest.mark.parametrize("lib", list(TOOL.KNOB_VARIANTS))
def test_knob_off_renders_the_same_bits(lib, cid, tmp_path_factory):
    base = results("default", tmp_path_factory)
    got = results(lib, tmp_path_factory)
    same(got, base, cid)
    for r in (base, got):
        m = r["meta"]["cases"][cid]
        assert m["launches"]["primary"] == 1 and m["tile_lists"]["camera"] and m["tile_lists"]["bundles"], m
        # the fused any-hit + shading grid where an item is whole pixels; else k_shade and k_accumulate
        assert ("shade" in m["launches"]) == (CASES[cid]["samples"] == 3), m["launches"]


@pytest.mark.gpu
def test_chunks_with_a_nonzero_first_pixel_render_the_same_bits(tmp_path_factory):
    base = results("default", tmp_path_factory)
    got = results("chunks", tmp_path_factory)
    same(got, base, CHUNKED)
    tiles = -(-93 // 8) * -(-70 // 8)
    assert got["meta"]["cases"][CHUNKED]["launches"]["primary"] == tiles  # 2^11 samples: one 64-spp tile per chunk
    assert base["meta"]["cases"][CHUNKED]["launches"]["primary"] == 1
