"""ctypes binding of include/yrt.h (libyrt.so, built in-tree).

The library is the product: nothing here falls back to Python or to the CPU. If
libyrt.so is missing or fails to load, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("YRT_LIB", _PKG / "libyrt.so"))

if not LIB_PATH.exists():
    raise ImportError(
        f"{LIB_PATH} not found: build it with `python yocto_raytracing_amd/build.py` "
        "(or __graft_entry__.build()); there is no fallback path")

# One HIP runtime per process. PyTorch-ROCm bundles its own libamdhip64 (SONAME
# libamdhip64.so.7, but torch asks for it as "libamdhip64.so"): if libyrt.so is loaded
# first, /opt/rocm's runtime is mapped, torch then maps its bundled copy on top of the
# same HSA runtime and finds no GPU ("No HIP GPUs are available"). With torch loaded
# first, libyrt.so's libamdhip64.so.7 resolves to torch's copy and both share it. torch
# is plumbing here (device buffers, streams, torch.distributed), so when it is installed
# it is imported before the library; YRT_NO_TORCH_PRELOAD=1 skips this for processes
# that never import torch.
if os.environ.get("YRT_NO_TORCH_PRELOAD") != "1":
    try:
        import torch  # noqa: F401
    except ImportError:
        pass

lib = C.CDLL(str(LIB_PATH))

YRT_OK = 0
YRT_MEM_HOST = 0
YRT_MEM_DEVICE = 1
YRT_TRANSPORT_COPY = 0
YRT_TRANSPORT_RCCL = 1


class RenderParams(C.Structure):
    _fields_ = [
        ("ambient", C.c_float * 3),
        ("resolution", C.c_int),
        ("width", C.c_int),
        ("samples", C.c_int),
        ("max_depth", C.c_int),
        ("camera", C.c_int),
        ("x0", C.c_int),
        ("y0", C.c_int),
        ("tile_w", C.c_int),
        ("tile_h", C.c_int),
        ("band", C.c_int),
        ("band_stride", C.c_int),
        ("band_offset", C.c_int),
        ("out_stride", C.c_int),
        ("count_work", C.c_int),
        ("algorithm", C.c_int),
        ("timing", C.c_int),
    ]


class Stats(C.Structure):
    _fields_ = [(n, C.c_ulonglong) for n in (
        "rays", "camera_samples", "depth_truncated", "stack_overflow", "box_tests",
        "instance_entries", "prim_tests", "shaded_hits", "texture_lookups", "shadow_rays",
        "shadow_box_tests", "shadow_instance_entries", "shadow_prim_tests", "wave_node_visits",
        "wave_prim_visits", "shadow_wave_node_visits", "shadow_rays_culled")]


PHASES = ("primary", "shadow", "shade", "bounce", "fold", "accumulate", "megakernel", "lists")


class Timings(C.Structure):
    _fields_ = [("ms", C.c_float * 8), ("launches", C.c_int * 8)]


class MaterialDesc(C.Structure):
    _fields_ = [("ke", C.c_float * 3), ("kd", C.c_float * 3), ("ks", C.c_float * 3), ("kr", C.c_float * 3),
                ("rs", C.c_float), ("kd_txt", C.c_int), ("ks_txt", C.c_int)]


class ShapeDesc(C.Structure):
    _fields_ = [("npos", C.c_int), ("pos", C.c_void_p), ("norm", C.c_void_p), ("texcoord", C.c_void_p),
                ("radius", C.c_void_p), ("npoints", C.c_int), ("points", C.c_void_p), ("nlines", C.c_int),
                ("lines", C.c_void_p), ("ntriangles", C.c_int), ("triangles", C.c_void_p)]


# YRT_AOV_*: name -> plane index (bit of the mask); every plane is 16 bytes per pixel
AOVS = {"depth": 0, "position": 1, "normal": 2, "texcoord": 3, "albedo": 4, "ids": 5}
YRT_AOV_COUNT = 6


class AovPlanes(C.Structure):
    _fields_ = [("plane", C.c_void_p * YRT_AOV_COUNT)]


# YRT_PASS_*: name -> plane index (bit of the mask); every plane is RGBA float32
PASSES = {"direct": 0, "diffuse": 1, "specular": 2, "reflection": 3, "ambient": 4}
YRT_PASS_COUNT = 5


class PassPlanes(C.Structure):
    _fields_ = [("plane", C.c_void_p * YRT_PASS_COUNT)]


# yrt_render_light_groups: one plane per group of lights, the ambient plane, the beauty
YRT_LIGHT_GROUPS_MAX = 8


class LightGroupPlanes(C.Structure):
    _fields_ = [("group", C.c_void_p * YRT_LIGHT_GROUPS_MAX), ("ambient", C.c_void_p), ("beauty", C.c_void_p)]


# YRT_MATTE_*: key name -> index (bit of the key mask); per key and layer an int4 plane of ids
# and a float4 plane of coverages, ranks 4 * layer .. 4 * layer + 3
MATTE_KEYS = {"instance": 0, "material": 1, "shape": 2}
YRT_MATTE_KEY_COUNT = 3
YRT_MATTE_LAYERS_MAX = 2


class MattePlanes(C.Structure):
    _fields_ = [("ids", C.c_void_p * YRT_MATTE_LAYERS_MAX * YRT_MATTE_KEY_COUNT),
                ("coverage", C.c_void_p * YRT_MATTE_LAYERS_MAX * YRT_MATTE_KEY_COUNT)]


# yrt_render_adaptive: the base frame's samples per axis (0: 1), the contrast threshold, the
# refined pixels per shading batch (0: sized by the library)
class AdaptiveParams(C.Structure):
    _fields_ = [("base_samples", C.c_int), ("threshold", C.c_float), ("chunk_pixels", C.c_int)]


# yrt_render_ao: occlusion rays per camera sample that hits a triangle (0: 16), their tmax and tmin
YRT_AO_RAYS_MAX = 64


class AoParams(C.Structure):
    _fields_ = [("rays", C.c_int), ("distance", C.c_float), ("bias", C.c_float)]


# yrt_render_camera / yrt_camera_rays: YRT_CAMERA_* by name; the lens diameter (< 0: the scene
# camera's, 0: pinhole), the focus distance (<= 0: the scene camera's), the pixels per shading
# batch (0: sized by the library)
CAMERA_MODELS = {"perspective": 0, "orthographic": 1, "equirect": 2}


class CameraModel(C.Structure):
    _fields_ = [("model", C.c_int), ("aperture", C.c_float), ("focus", C.c_float), ("chunk_pixels", C.c_int)]


# yrt_shade_rays_soft / yrt_render_soft_shadows: K shadow rays per light (0: 16), one radius for
# every light or light_radius[nlights] (host memory)
YRT_SOFT_SHADOW_RAYS_MAX = 64


class SoftShadowParams(C.Structure):
    _fields_ = [("rays", C.c_int), ("radius", C.c_float), ("light_radius", C.POINTER(C.c_float)), ("nlights", C.c_int)]


_vp = C.c_void_p
_ip =C.POINTER(C.c_int)
_fp = C.POINTER(C.c_float)
_sig = {
    "yrt_abi_version": (C.c_int, []),
    "yrt_status_string": (C.c_char_p, [C.c_int]),
    "yrt_last_error": (C.c_char_p, []),
    "yrt_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "yrt_scene_load": (C.c_int, [C.c_char_p, C.POINTER(_vp)]),
    "yrt_scene_save": (C.c_int, [_vp, C.c_char_p]),
    "yrt_host_scene_build_bvh": (C.c_int, [_vp, C.c_int]),
    "yrt_host_scene_build_bvh_gpu": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "yrt_host_scene_save_bvh": (C.c_int, [_vp, C.c_char_p]),
    "yrt_host_scene_info": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "yrt_host_image_size": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "yrt_host_scene_free": (None, [_vp]),
    "yrt_host_scene_create": (C.c_int, [C.POINTER(_vp)]),
    "yrt_host_scene_add_camera": (C.c_int, [_vp, _vp, C.c_float, C.c_float, C.c_float, C.c_float, _ip]),
    "yrt_host_scene_add_texture": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _ip]),
    "yrt_host_scene_add_material": (C.c_int, [_vp, C.POINTER(MaterialDesc), _ip]),
    "yrt_host_scene_add_shape": (C.c_int, [_vp, C.POINTER(ShapeDesc), _ip]),
    "yrt_host_scene_add_instance": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _ip]),
    "yrt_scene_upload": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "yrt_scene_device_bytes": (C.c_size_t, [_vp]),
    "yrt_scene_free": (None, [_vp]),
    "yrt_render_params_default": (None, [C.POINTER(RenderParams)]),
    "yrt_image_size": (C.c_int, [_vp, C.POINTER(RenderParams), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "yrt_render": (C.c_int, [_vp, C.POINTER(RenderParams), _vp, C.c_int, _vp]),
    "yrt_trace_first": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp]),
    "yrt_trace_any": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp]),
    "yrt_scene_set_trace_algorithm": (C.c_int, [_vp, C.c_int]),
    "yrt_scene_set_tile_lists": (C.c_int, [_vp, C.c_int]),
    "yrt_scene_tile_lists": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]),
    "yrt_scene_tile_list_masks": (C.c_int, [_vp, C.POINTER(C.c_ulonglong)]),
    "yrt_scene_set_lds_staging": (C.c_int, [_vp, C.c_int]),
    "yrt_scene_lds_staging": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "yrt_last_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "yrt_last_timings": (C.c_int, [_vp, C.POINTER(Timings)]),
    "yrt_tonemap": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp]),
    "yrt_save_image": (C.c_int, [C.c_char_p, _vp, C.c_int, C.c_int]),
    "yrt_save_image_mem": (C.c_int, [C.c_char_p, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    "yrt_multi_create": (C.c_int, [_vp, _ip, C.c_int, C.POINTER(_vp)]),
    "yrt_multi_free": (None, [_vp]),
    "yrt_multi_info": (C.c_int, [_vp, _ip, _ip]),
    "yrt_multi_render": (C.c_int, [_vp, C.POINTER(RenderParams), _vp, C.c_int]),
    "yrt_multi_last_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "yrt_multi_last_timings": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "yrt_render_multi": (C.c_int, [_vp, _ip, C.c_int, C.POINTER(RenderParams), _vp, C.c_int]),
    "yrt_render_aovs": (C.c_int, [_vp, C.POINTER(RenderParams), C.c_uint, C.POINTER(AovPlanes), C.c_int, _vp]),
    "yrt_render_passes": (C.c_int, [_vp, C.POINTER(RenderParams), C.c_uint, C.POINTER(PassPlanes), _vp, C.c_int, _vp]),
    "yrt_shade_rays": (C.c_int, [_vp, C.POINTER(RenderParams), _vp, C.c_int, _vp, C.c_int, _vp]),
    "yrt_host_scene_lights": (C.c_int, [_vp, _ip, C.c_int, _ip]),
    "yrt_render_light_groups": (C.c_int, [_vp, C.POINTER(RenderParams), _ip, C.c_int, C.c_int,
                                          C.POINTER(LightGroupPlanes), C.c_int, _vp]),
    "yrt_render_mattes": (C.c_int, [_vp, C.POINTER(RenderParams), C.c_uint, C.c_int, C.POINTER(MattePlanes), C.c_int,
                                    _vp]),
    "yrt_scene_matte_dropped": (C.c_int, [_vp, C.POINTER(C.c_ulonglong)]),
    "yrt_host_scene_instances": (C.c_int, [_vp, _ip, _ip, C.c_int, _ip]),
    "yrt_render_adaptive": (C.c_int, [_vp, C.POINTER(RenderParams), C.POINTER(AdaptiveParams), _vp, _vp, C.c_int, _vp]),
    "yrt_scene_adaptive_refined": (C.c_int, [_vp, C.POINTER(C.c_ulonglong)]),
    "yrt_ao_params_default": (None, [C.POINTER(AoParams)]),
    "yrt_ao_tables": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "yrt_render_ao": (C.c_int, [_vp, C.POINTER(RenderParams), C.POINTER(AoParams), _vp, C.c_int, _vp]),
    "yrt_host_scene_shape_kinds": (C.c_int, [_vp, _ip, C.c_int, _ip]),
    "yrt_camera_model_default": (None, [C.POINTER(CameraModel)]),
    "yrt_render_camera": (C.c_int, [_vp, C.POINTER(RenderParams), C.POINTER(CameraModel), _vp, C.c_int, _vp]),
    "yrt_camera_rays": (C.c_int, [_vp, C.POINTER(RenderParams), C.POINTER(CameraModel), _vp, C.c_int, _vp]),
    "yrt_host_scene_camera": (C.c_int, [_vp, C.c_int, _fp, _fp, _fp, _fp, _fp]),
    "yrt_soft_shadow_params_default": (None, [C.POINTER(SoftShadowParams)]),
    "yrt_shade_rays_soft": (C.c_int, [_vp, C.POINTER(RenderParams), C.POINTER(SoftShadowParams), _vp, C.c_int, _vp,
                                      C.c_int, _vp]),
    "yrt_render_soft_shadows": (C.c_int, [_vp, C.POINTER(RenderParams), C.POINTER(CameraModel),
                                          C.POINTER(SoftShadowParams), _vp, C.c_int, _vp]),
}
EXPORTS = tuple(_sig)

for _name, (_res, _args) in _sig.items():
    try:
        _f = getattr(lib, _name)
    except AttributeError as e:
        raise ImportError(f"{LIB_PATH} is stale (missing {_name}): rebuild it") from e
    _f.restype = _res
    _f.argtypes = _args


class YrtError(RuntimeError):
    def __init__(self, status: int, what: str):
        msg = lib.yrt_last_error().decode() or lib.yrt_status_string(status).decode()
        super().__init__(f"{what}: {lib.yrt_status_string(status).decode()}: {msg}")
        self.status = status


def check(status: int, what: str) -> None:
    if status != YRT_OK:
        raise YrtError(status, what)
