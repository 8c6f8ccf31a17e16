"""yrt_render_adaptive without a GPU (include/yrt.h): the exports, the argument checks that return
before anything touches a device, the numpy model of the contrast rule (tests/adaptive_model.py)
against a brute-force double loop, and the new kernels' register budgets from the shipped
library's gfx950 code object."""
import ctypes as C
import re

import numpy as np
import pytest

import adaptive_model as AM
from helpers import ROOT

LIB = ROOT / "yocto_raytracing_amd" / "libyrt.so"
YRT_ERR_INVALID_ARG = 1


@pytest.fixture(scope="module")
def yrt():
    import yocto_raytracing_amd as y

    return y


def test_the_symbols_are_declared_exported_and_bound():
    from yocto_raytracing_amd import _native as N

    header = (ROOT / "include" / "yrt.h").read_text()
    assert re.search(r"typedef struct yrt_adaptive_params \{\s*int\s+base_samples;[^}]*float\s+threshold;[^}]*"
                     r"int\s+chunk_pixels;[^}]*\} yrt_adaptive_params;", header)
    assert re.search(r"\bint yrt_render_adaptive\(yrt_scene\* ds, const yrt_render_params\* p, "
                     r"const yrt_adaptive_params\* a,\s*float\* out, unsigned char\* refined[^,]*, int mem, "
                     r"void\* stream\);", header)
    assert re.search(r"\bint yrt_scene_adaptive_refined\(yrt_scene\* ds, unsigned long long\* pixels\);", header)
    lib = C.CDLL(str(LIB))
    for name in ("yrt_render_adaptive", "yrt_scene_adaptive_refined"):
        assert hasattr(lib, name), name
        assert name in N.EXPORTS, name
    y = __import__("yocto_raytracing_amd")
    assert "raytrace_adaptive" in y.__all__ and callable(y.raytrace_adaptive)
    assert callable(y.DeviceScene.render_adaptive_into)
    mirror = (ROOT / "include" / "yrt_raytrace.hpp").read_text()
    assert "yrt_render_adaptive(" in mirror and re.search(r"inline image4f raytrace_adaptive\(", mirror)


def test_invalid_arguments_are_refused_before_any_device_call(yrt):
    from yocto_raytracing_amd import _native as N

    handle = C.cast(C.create_string_buffer(256), C.c_void_p)  # never looked at: the checks come first
    out = (C.c_float * 16)(*([77.0] * 16))
    mask = (C.c_ubyte * 4)(*([7] * 4))

    def call(h=handle, samples=3, base=1, threshold=0.25, chunk=0, o=out, mem=N.YRT_MEM_HOST, camera=0,
             params=True, adaptive=True):
        p = yrt.render_params(resolution=2, samples=samples, width=2, camera=camera)
        a = N.AdaptiveParams(base, threshold, chunk)
        return N.lib.yrt_render_adaptive(h, C.byref(p) if params else None, C.byref(a) if adaptive else None, o, mask,
                                         mem, None)

    cases = {
        "null handle": dict(h=None), "null params": dict(params=False), "null adaptive params": dict(adaptive=False),
        "null out": dict(o=None), "NaN threshold": dict(threshold=float("nan")),
        "base above samples": dict(base=4), "negative base": dict(base=-1), "no samples": dict(samples=0),
        "base defaults to 1, above samples 0": dict(samples=0, base=0), "negative chunk": dict(chunk=-1),
        "mem -1": dict(mem=-1), "mem 2": dict(mem=2), "negative camera": dict(camera=-1),
    }
    for what, kw in cases.items():
        assert call(**kw) == YRT_ERR_INVALID_ARG, what
        assert b"yrt_render_adaptive" in N.lib.yrt_last_error(), what
    assert list(out) == [77.0] * 16 and list(mask) == [7] * 4
    n = C.c_ulonglong(5)
    assert N.lib.yrt_scene_adaptive_refined(None, C.byref(n)) == YRT_ERR_INVALID_ARG
    assert N.lib.yrt_scene_adaptive_refined(handle, None) == YRT_ERR_INVALID_ARG
    assert n.value == 5


def frames():
    """1x1, 1x5, 5x1 and 6x7 frames (rows x columns) with a NaN channel, an infinity, and
    differences below, at and above the threshold 0.25 (every value a multiple of 1/8: exact)"""
    rng = np.random.default_rng(3)
    out = []
    for h, w in ((1, 1), (1, 5), (5, 1), (6, 7)):
        b = (rng.integers(0, 4, (h, w, 4)) / 8).astype(np.float32)  # differences 0, 1/8, 1/4, 3/8
        b[..., 3] = 1
        out.append(b)
    out[3][2, 3, 1] = np.nan
    out[3][4, 5, 0] = np.inf
    return out


@pytest.mark.parametrize("threshold", [0.25, 0.125, 0.0, -1.0, np.inf])
def test_the_model_equals_the_brute_force_rule(threshold):
    for b in frames():
        np.testing.assert_array_equal(AM.flags(b, threshold), AM.flags_brute(b, threshold), err_msg=str(b.shape))


def test_the_models_edge_cases():
    t = np.float32(0.25)
    # a frame of one pixel has no neighbour; a negative threshold flags every pixel that has one
    assert not AM.flags(np.zeros((1, 1, 4), np.float32), -1.0).any()
    for shape in ((1, 5), (5, 1), (6, 7)):
        assert AM.flags(np.zeros(shape + (4,), np.float32), -1.0).all()
        assert not AM.flags(np.zeros(shape + (4,), np.float32), 0.0).any()
    # a difference exactly equal to the threshold is not flagged, the next float above it is
    b = np.zeros((1, 2, 4), np.float32)
    b[0, 1, 2] = t
    assert not AM.flags(b, t).any()
    b[0, 1, 2] = np.nextafter(t, np.float32(1))
    assert AM.flags(b, t).all()
    # alpha is not a channel of the rule
    b = np.zeros((1, 2, 4), np.float32)
    b[0, 1, 3] = 9
    assert not AM.flags(b, t).any()
    # a NaN channel flags nothing by itself: neither the pixel nor its neighbours ...
    b = np.zeros((3, 3, 4), np.float32)
    b[1, 1, 0] = np.nan
    assert not AM.flags(b, t).any()
    # ... but its other channels still count
    b[1, 1, 1] = 1
    assert AM.flags(b, t).all()
    # the diagonal neighbour counts, the pixel two away does not
    b = np.zeros((3, 4, 4), np.float32)
    b[0, 0, 0] = 1
    want = np.zeros((3, 4), bool)
    want[:2, :2] = True
    np.testing.assert_array_equal(AM.flags(b, t), want)
    # compose takes the full render where flagged and the base elsewhere, bit for bit
    full, base = np.full((3, 4, 4), 2, np.float32), np.full((3, 4, 4), -0.0, np.float32)
    got = AM.compose(want, full, base)
    assert (got[want] == 2).all() and np.signbit(got[~want]).all()


def test_adaptive_kernels_code_object_budget():
    """the flag kernel and the pixel-batch kernels the refinement runs on (camera.hip: a
    k_camera_rays per camera model and k_camera_resolve, each once, with the list argument) keep
    everything in registers; the kernels that the shared ones replaced are gone"""
    from yocto_raytracing_amd.codeid import kernel_resources

    res = kernel_resources(LIB)
    new = {k: v for k, v in res.items() if "k_adaptive_" in k or "k_camera_rays" in k or "k_camera_resolve" in k}
    for name, count in (("k_adaptive_flag", 1), ("k_camera_rays", 3), ("k_camera_resolve", 1),
                        ("k_adaptive_rays", 0), ("k_adaptive_resolve", 0), ("k_adaptive_add_counters", 0)):
        assert len([k for k in new if name in k]) == count, (name, sorted(new))
    assert len(new) == 5, sorted(new)
    for name, r in new.items():
        print(f"{name[:48]}: {r['vgpr']} VGPRs, {r['sgpr']} SGPRs, {r['lds']} B LDS, block {r['block']}")
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["private"] == 0, (name, r)
        # streaming kernels: full occupancy (8 waves per SIMD) needs at most 64 VGPRs
        assert r["vgpr"] <= 64 and r["lds"] <= 64, (name, r)
