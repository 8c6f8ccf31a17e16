"""Differently shaped workspaces through one handle (wavefront.hip plan_chunks, carve).

A handle keeps one workspace, which a call regrows when its shape needs more and otherwise carves
anew: the render's slabs, behind them the passes' per-sample planes or the light groups' table,
planes and mirror-level records, for a ray batch the render's slabs alone. The *_chunks tests start
a process per library and run one shape each; here one uploaded handle runs, on 37 x 24 frames,

    raytrace s = 3 (max_depth 16), render_passes s = 2, render_light_groups s = 3,
    shade_rays of the 888 camera rays of s = 1, raytrace s = 1, render_passes s = 3, raytrace s = 3

so that the workspace grows, is reused by smaller shapes, and is carved with and without pass and
group planes. Every result must have the bits, and the call the counters, of the same call on a
freshly uploaded handle. "groups" is tests/light_groups_scene.py's scene (five lights, two
mirrors: the fused shape never runs, every call keeps mirror-level records); "simple" is a golden
fixture.
"""
import numpy as np
import pytest

import light_groups_scene as LS
import passes_scene as PS
import shade_rays_scene as SS
from helpers import scene_path

pytestmark = pytest.mark.gpu

RES, WIDTH = SS.RES, SS.WIDTH
STAT_KEYS = ("rays", "camera_samples", "shadow_rays", "shadow_rays_culled", "depth_truncated")


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    if y.device_count() < 1:
        pytest.fail("no GPU visible: the -m gpu suite must run on the MI355X box")
    return y


def planes_of(result):
    """the arrays of a call's result, in a fixed order"""
    if isinstance(result, np.ndarray):
        return [result]
    if "groups" in result:
        return [*result["groups"], result["ambient"], result["beauty"]]
    return [result[k] for k in sorted(result)]


def calls(yrt, rays, group_of):
    """the sequence: (what, the call on a device scene)"""
    frame = dict(width=WIDTH, max_depth=16)
    return [
        ("raytrace s=3", lambda ds: yrt.raytrace(ds, PS.AMB, RES, 3, **frame)),
        ("render_passes s=2", lambda ds: yrt.render_passes(ds, PS.AMB, RES, 2, **frame)),
        ("render_light_groups s=3", lambda ds: yrt.render_light_groups(ds, PS.AMB, RES, 3, groups=group_of, **frame)),
        ("shade_rays 888", lambda ds: yrt.shade_rays(ds, rays, PS.AMB, max_depth=16)),
        ("raytrace s=1", lambda ds: yrt.raytrace(ds, PS.AMB, RES, 1, **frame)),
        ("render_passes s=3", lambda ds: yrt.render_passes(ds, PS.AMB, RES, 3, **frame)),
        ("raytrace s=3 again", lambda ds: yrt.raytrace(ds, PS.AMB, RES, 3, **frame)),
    ]


@pytest.mark.parametrize("name", ["groups", "simple"])
def test_one_handle_equals_fresh_handles(yrt, tmp_path, name):
    if name == "groups":
        scn = LS.build(yrt)
        path = tmp_path / "groups.yrtscene"
        scn.save(str(path))
    else:
        path = scene_path(name)
        scn = yrt.load_scene(str(path))
    yrt.build_bvh(scn)
    nlights = len(scn.lights())
    if name == "groups":
        assert nlights == len(LS.LIGHTS) == 5
    rays = SS.camera_rays(path, 1)
    assert rays.shape == (888, 8)
    sequence = calls(yrt, rays, [k % 2 for k in range(nlights)])

    def run_on(ds, call):
        planes = planes_of(call(ds))
        stats = ds.last_stats()
        return planes, {k: stats[k] for k in STAT_KEYS}

    fresh = {}
    for what, call in sequence:
        key = what.replace(" again", "")  # (the same call: one reference)
        if key not in fresh:
            ds = yrt.DeviceScene(scn, 0)
            try:
                fresh[key] = run_on(ds, call)
            finally:
                ds.close()
    assert (fresh["raytrace s=3"][0][0][..., :3] > 0).any()
    assert fresh["raytrace s=3"][1]["camera_samples"] == RES * WIDTH * 9
    assert fresh["shade_rays 888"][1]["camera_samples"] == 888

    one = yrt.DeviceScene(scn, 0)
    try:
        for what, call in sequence:
            got, stats = run_on(one, call)
            want, wstats = fresh[what.replace(" again", "")]
            assert len(got) == len(want), what
            for k, (g, w) in enumerate(zip(got, want)):
                assert g.shape == w.shape and g.dtype == w.dtype == np.float32, (what, k)
                np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=f"{what}, plane {k}")
            assert stats == wstats, what
    finally:
        one.close()
