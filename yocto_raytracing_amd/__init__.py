"""yocto_raytracing_amd -- MI355X-native renderer for the yocto_raytracing hot path.

Python mirror of the reference's host interface (names, argument meaning and
error behaviour of src/scene.h and src/raytrace.cpp), over the C-ABI of
include/yrt.h implemented by libyrt.so (C++ host code + gfx950 HIP kernels):

    scn = load_scene("in/basic_pointlight/basic_pointlight.obj")   # scene.cpp:113
    build_bvh(scn, False)                                          # scene.cpp:554
    img = raytrace(scn, (0.1, 0.1, 0.1), 720, 1)                   # raytrace.cpp:213
    save_hdr_or_ldr("out.png", img)                                # image.cpp:81

`img` is the reference's image4f: float32 RGBA, shape (H, W, 4), pixels[j][i].
There is no CPU fallback: without a GPU the render calls raise.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _native as N
from ._native import RenderParams, Stats, YrtError, check

__all__ = [
    "Scene", "DeviceScene", "load_scene", "build_bvh", "raytrace", "raytrace_adaptive", "render_aovs", "render_passes", "render_light_groups",
    "render_mattes", "matte", "render_ao", "ao_tables", "raytrace_camera", "camera_rays", "raytrace_soft",
    "shade_rays_soft", "intersect_first",
    "intersect_any", "shade_rays", "tonemap", "save_hdr_or_ldr", "render_params", "device_count", "YrtError",
]

ALGORITHMS = {"wavefront": 0, "megakernel": 1, "wavefront_lane": 2}
TILE_LISTS = {"auto": 0, "on": 1, "off": 2}
INFO_FIELDS = ("cameras", "textures", "materials", "shapes", "instances", "lights",
               "bvh_nodes", "bvh_depth", "shape_bvh_depth", "triangles", "lines", "points")


class Scene:
    """Host scene (the reference's `scene*`), owned by libyrt."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)
        self._device_scenes = {}

    @property
    def handle(self):
        return self._h

    def __del__(self):
        try:
            for ds in self._device_scenes.values():
                ds.close()
            if self._h:
                N.lib.yrt_host_scene_free(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    # ---- building a scene in memory (yrt_host_scene_add_*: the reference's scene*
    # filled field by field, scene.h:26-155) ----
    @classmethod
    def create(cls) -> "Scene":
        h = C.c_void_p()
        check(N.lib.yrt_host_scene_create(C.byref(h)), "yrt_host_scene_create")
        return cls(h.value)

    @staticmethod
    def _frame(frame) -> np.ndarray:
        f = np.ascontiguousarray(frame, np.float32).reshape(-1)
        if f.size != 12:
            raise ValueError("frame must be 12 floats: x.xyz, y.xyz, z.xyz, o.xyz")
        return f

    def _added(self, status, what, idx) -> int:
        check(status, what)
        for ds in self._device_scenes.values():
            ds.close()
        self._device_scenes.clear()
        return idx.value

    def add_camera(self, frame, fovy: float, aspect: float, focus: float, aperture: float = 0.0) -> int:
        f, idx = self._frame(frame), C.c_int()
        return self._added(N.lib.yrt_host_scene_add_camera(self._h, f.ctypes.data, fovy, aspect, aperture, focus,
                                                           C.byref(idx)), "add_camera", idx)

    def add_texture(self, rgba8: np.ndarray) -> int:
        t = np.ascontiguousarray(rgba8, np.uint8)
        if t.ndim != 3 or t.shape[2] != 4:
            raise ValueError("texture must be (h, w, 4) uint8")
        idx = C.c_int()
        return self._added(N.lib.yrt_host_scene_add_texture(self._h, t.shape[1], t.shape[0], t.ctypes.data,
                                                            C.byref(idx)), "add_texture", idx)

    def add_material(self, kd=(0, 0, 0), ks=(0, 0, 0), kr=(0, 0, 0), ke=(0, 0, 0), rs: float = 0.0,
                     kd_txt: int = -1, ks_txt: int = -1) -> int:
        m = N.MaterialDesc()
        for name, v in (("ke", ke), ("kd", kd), ("ks", ks), ("kr", kr)):
            getattr(m, name)[:] = [float(x) for x in v]
        m.rs, m.kd_txt, m.ks_txt = float(rs), int(kd_txt), int(ks_txt)
        idx = C.c_int()
        return self._added(N.lib.yrt_host_scene_add_material(self._h, C.byref(m), C.byref(idx)), "add_material", idx)

    def add_shape(self, pos, norm=None, texcoord=None, radius=None, points=None, lines=None, triangles=None) -> int:
        keep = []

        def arr(a, dtype, cols):
            if a is None:
                return None, 0
            x = np.ascontiguousarray(a, dtype)
            x = x.reshape(-1, cols) if cols > 1 else x.reshape(-1)
            keep.append(x)
            return x.ctypes.data, x.shape[0]

        d = N.ShapeDesc()
        d.pos, d.npos = arr(pos, np.float32, 3)
        d.norm, _ = arr(norm, np.float32, 3)
        d.texcoord, _ = arr(texcoord, np.float32, 2)
        d.radius, _ = arr(radius, np.float32, 1)
        d.points, d.npoints = arr(points, np.int32, 1)
        d.lines, d.nlines = arr(lines, np.int32, 2)
        d.triangles, d.ntriangles = arr(triangles, np.int32, 3)
        for name, n in (("norm", 3), ("texcoord", 2), ("radius", 1)):
            a = locals()[name]
            if a is not None and np.asarray(a).size != d.npos * n:
                raise ValueError(f"{name} must have one entry per vertex")
        idx = C.c_int()
        return self._added(N.lib.yrt_host_scene_add_shape(self._h, C.byref(d), C.byref(idx)), "add_shape", idx)

    def add_instance(self, frame, shape: int, material: int) -> int:
        f, idx = self._frame(frame), C.c_int()
        return self._added(N.lib.yrt_host_scene_add_instance(self._h, f.ctypes.data, shape, material, C.byref(idx)),
                           "add_instance", idx)

    def info(self) -> dict:
        buf = (C.c_longlong * 12)()
        check(N.lib.yrt_host_scene_info(self._h, buf), "yrt_host_scene_info")
        return dict(zip(INFO_FIELDS, list(buf)))

    def lights(self) -> list:
        """the instance index (scene order) of each light, in light order: the instances whose
        material has ke > 0 in every component (raytrace.cpp:126)"""
        n = C.c_int()
        check(N.lib.yrt_host_scene_lights(self._h, None, 0, C.byref(n)), "yrt_host_scene_lights")
        inst = (C.c_int * max(n.value, 1))()
        check(N.lib.yrt_host_scene_lights(self._h, inst, n.value, C.byref(n)), "yrt_host_scene_lights")
        return list(inst[:n.value])

    def instances(self) -> list:
        """(shape, material) of each instance, in scene order: what turns a material or shape
        id of a matte (render_mattes) back into a set of instances"""
        n = C.c_int()
        check(N.lib.yrt_host_scene_instances(self._h, None, None, 0, C.byref(n)), "yrt_host_scene_instances")
        shp, mat = (C.c_int * max(n.value, 1))(), (C.c_int * max(n.value, 1))()
        check(N.lib.yrt_host_scene_instances(self._h, shp, mat, n.value, C.byref(n)), "yrt_host_scene_instances")
        return list(zip(shp[:n.value], mat[:n.value]))

    def shape_kinds(self) -> list:
        """the primitive kind of each shape, in scene order: 0 triangles, 1 lines, 2 points, 3
        empty (the .w of render_aovs' "ids" indexes it; render_ao casts rays from triangles only)"""
        n = C.c_int()
        check(N.lib.yrt_host_scene_shape_kinds(self._h, None, 0, C.byref(n)), "yrt_host_scene_shape_kinds")
        kind = (C.c_int * max(n.value, 1))()
        check(N.lib.yrt_host_scene_shape_kinds(self._h, kind, n.value, C.byref(n)), "yrt_host_scene_shape_kinds")
        return list(kind[:n.value])

    def camera(self, index: int = 0) -> dict:
        """camera `index` as add_camera takes it: {"frame": (12,) float32 x, y, z, o; "fovy",
        "aspect", "aperture" (the lens diameter), "focus"}"""
        frame = np.zeros(12, np.float32)
        v = [C.c_float() for _ in range(4)]
        check(N.lib.yrt_host_scene_camera(self._h, int(index), frame.ctypes.data_as(C.POINTER(C.c_float)),
                                          *[C.byref(x) for x in v]), "yrt_host_scene_camera")
        return dict(zip(("fovy", "aspect", "aperture", "focus"), (x.value for x in v)), frame=frame)

    def image_size(self, resolution: int, camera: int = 0):
        w, h = C.c_int(), C.c_int()
        check(N.lib.yrt_host_image_size(self._h, camera, resolution, C.byref(w), C.byref(h)),
              "yrt_host_image_size")
        return w.value, h.value

    def save(self, path: str) -> None:
        check(N.lib.yrt_scene_save(self._h, str(path).encode()), "yrt_scene_save")

    def save_bvh(self, path: str) -> None:
        check(N.lib.yrt_host_scene_save_bvh(self._h, str(path).encode()), "yrt_host_scene_save_bvh")

    def upload(self, device: int = 0) -> "DeviceScene":
        if device not in self._device_scenes:
            self._device_scenes[device] = DeviceScene(self, device)
        return self._device_scenes[device]


class DeviceScene:
    """A scene resident in one GPU's HBM (yrt_scene*)."""

    def __init__(self, scene: Scene, device: int = 0):
        h = C.c_void_p()
        check(N.lib.yrt_scene_upload(scene.handle, device, C.byref(h)), "yrt_scene_upload")
        self._h = h
        self.device = device
        self.host = scene

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            N.lib.yrt_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_trace_algorithm(self, algorithm: str) -> None:
        """walks used by intersect_first/intersect_any on this scene (identical results)"""
        check(N.lib.yrt_scene_set_trace_algorithm(self._h, ALGORITHMS[algorithm]), "set_trace_algorithm")

    def set_tile_lists(self, mode: str) -> None:
        """per-tile candidate lists of render_into: "on" builds them whenever the scene allows,
        "auto" (default) the same from 9 samples per pixel, "off" never -- identical images
        either way"""
        check(N.lib.yrt_scene_set_tile_lists(self._h, TILE_LISTS[mode]), "set_tile_lists")

    def tile_lists(self) -> dict:
        """the lists the last render used, and the sums of the last render that built any"""
        cam, bun, sums = C.c_int(), C.c_int(), (C.c_ulonglong * 4)()
        check(N.lib.yrt_scene_tile_lists(self._h, C.byref(cam), C.byref(bun), sums), "tile_lists")
        ex = (C.c_ulonglong * 2)()
        check(N.lib.yrt_scene_tile_list_masks(self._h, ex), "tile_list_masks")
        return {"camera": bool(cam.value), "bundles": bool(bun.value), "camera_entries": int(sums[0]),
                "camera_lists": int(sums[1]), "bundle_entries": int(sums[2]), "bundle_lists": int(sums[3]),
                "camera_instances_masked": int(ex[0]), "bundle_instances_masked": int(ex[1])}

    def set_lds_staging(self, on: bool) -> None:
        """LDS staging of the instance tree's top in render_into's persistent walks (the tile
        lists are not built while it is on; identical images; off by default, measured slower:
        DESIGN.md §5)"""
        check(N.lib.yrt_scene_set_lds_staging(self._h, 1 if on else 0), "set_lds_staging")

    def lds_staging(self) -> dict:
        """which walks of the last render read the staged records"""
        v = C.c_int()
        check(N.lib.yrt_scene_lds_staging(self._h, C.byref(v)), "lds_staging")
        return {"closest_hit": bool(v.value & 1), "any_hit": bool(v.value & 2)}

    @property
    def device_bytes(self) -> int:
        return int(N.lib.yrt_scene_device_bytes(self._h))

    def image_size(self, params: RenderParams):
        w, h = C.c_int(), C.c_int()
        check(N.lib.yrt_image_size(self._h, C.byref(params), C.byref(w), C.byref(h)), "yrt_image_size")
        return w.value, h.value

    def render_into(self, params: RenderParams, out_ptr: int, device_memory: bool = True,
                    stream: Optional[int] = None) -> None:
        """Launch raytrace() into a caller buffer (device pointer by default), stream ordered."""
        check(N.lib.yrt_render(self._h, C.byref(params), C.c_void_p(out_ptr), _mem(device_memory),
                               C.c_void_p(stream or 0)), "yrt_render")

    def render_aovs_into(self, params: RenderParams, planes: dict, device_memory: bool = True,
                         stream: Optional[int] = None) -> None:
        """Launch the AOV pass (yrt_render_aovs) into caller planes {name: pointer}, 16 bytes
        per pixel each in render_into's layout; only the named AOVs are computed."""
        mask, ap = _name_mask(planes, N.AOVS, "AOV"), N.AovPlanes()
        for name, ptr in planes.items():
            ap.plane[N.AOVS[name]] = ptr
        check(N.lib.yrt_render_aovs(self._h, C.byref(params), mask, C.byref(ap), _mem(device_memory),
                                    C.c_void_p(stream or 0)), "yrt_render_aovs")

    def render_mattes_into(self, params: RenderParams, planes: dict, layers: int, device_memory: bool = True,
                           stream: Optional[int] = None) -> None:
        """Launch the ID-matte pass (yrt_render_mattes) into caller planes {key: {"ids": [pointer
        per layer], "coverage": [pointer per layer]}}, 16 bytes per pixel each in render_into's
        layout (int32 x 4 and float32 x 4: ranks 4 * layer .. 4 * layer + 3); only the named keys
        are computed, all from one walk."""
        mask, mp = _name_mask(planes, N.MATTE_KEYS, "matte key"), N.MattePlanes()
        for key, kp in planes.items():
            for what, dst in (("ids", mp.ids), ("coverage", mp.coverage)):
                ptrs = list(kp[what])
                if len(ptrs) > N.YRT_MATTE_LAYERS_MAX:
                    raise ValueError(f"at most {N.YRT_MATTE_LAYERS_MAX} layers per matte key")
                for l, ptr in enumerate(ptrs):
                    dst[N.MATTE_KEYS[key]][l] = ptr
        check(N.lib.yrt_render_mattes(self._h, C.byref(params), mask, int(layers), C.byref(mp), _mem(device_memory),
                                      C.c_void_p(stream or 0)), "yrt_render_mattes")

    def matte_dropped(self) -> dict:
        """the samples the last render_mattes_into dropped per key (their id found the key's
        table full), 0 for a key it did not compute; waits for that pass"""
        d = (C.c_ulonglong * N.YRT_MATTE_KEY_COUNT)()
        check(N.lib.yrt_scene_matte_dropped(self._h, d), "yrt_scene_matte_dropped")
        return {key: int(d[k]) for key, k in N.MATTE_KEYS.items()}

    def render_passes_into(self, params: RenderParams, planes: dict, beauty_ptr: Optional[int] = None,
                           device_memory: bool = True, stream: Optional[int] = None) -> None:
        """Launch raytrace() with its shading passes (yrt_render_passes) into caller planes
        {name: pointer}, RGBA float32 each in render_into's layout; only the named passes are
        written. `beauty_ptr`, when given, receives render_into's image from the same walk."""
        mask, pp = _name_mask(planes, N.PASSES, "pass"), N.PassPlanes()
        for name, ptr in planes.items():
            pp.plane[N.PASSES[name]] = ptr
        check(N.lib.yrt_render_passes(self._h, C.byref(params), mask, C.byref(pp), C.c_void_p(beauty_ptr or 0),
                                      _mem(device_memory), C.c_void_p(stream or 0)), "yrt_render_passes")

    def render_light_groups_into(self, params: RenderParams, groups: Sequence[int], group_ptrs: Sequence[int],
                                 ambient_ptr: Optional[int] = None, beauty_ptr: Optional[int] = None,
                                 device_memory: bool = True, stream: Optional[int] = None) -> None:
        """Launch raytrace() split by light group (yrt_render_light_groups): `groups` gives each of
        the scene's lights (Scene.lights() order) its group, -1 for none; `group_ptrs` one plane
        per group, RGBA float32 in render_into's layout; `ambient_ptr` and `beauty_ptr`, when
        given, receive the ambient term's plane and render_into's image from the same walk."""
        ngroups = _light_groups(groups, len(group_ptrs))
        lp = N.LightGroupPlanes()
        for g, ptr in enumerate(group_ptrs):
            lp.group[g] = ptr
        lp.ambient, lp.beauty = ambient_ptr or None, beauty_ptr or None
        gof = (C.c_int * max(len(groups), 1))(*[int(g) for g in groups])
        check(N.lib.yrt_render_light_groups(self._h, C.byref(params), gof, len(groups), ngroups, C.byref(lp),
                                            _mem(device_memory), C.c_void_p(stream or 0)), "yrt_render_light_groups")

    def shade_rays_into(self, params: RenderParams, rays_ptr: int, n: int, out_ptr: int, device_memory: bool = True,
                        stream: Optional[int] = None) -> None:
        """Launch shade() for n caller rays (yrt_shade_rays): `rays_ptr` n x 8 float32 {o.xyz,
        d.xyz, tmin, tmax}, `out_ptr` n x RGBA float32, both device pointers by default, stream
        ordered. Of `params`, ambient, max_depth, algorithm and timing are used."""
        check(N.lib.yrt_shade_rays(self._h, C.byref(params), C.c_void_p(rays_ptr), int(n), C.c_void_p(out_ptr),
                                   _mem(device_memory), C.c_void_p(stream or 0)), "yrt_shade_rays")

    def render_adaptive_into(self, params: RenderParams, out_ptr: int, threshold: float, base_samples: int = 1,
                             refined_ptr: Optional[int] = None, chunk_pixels: int = 0, device_memory: bool = True,
                             stream: Optional[int] = None) -> None:
        """Launch raytrace() with adaptive supersampling (yrt_render_adaptive) into a caller buffer
        in render_into's layout: `base_samples` per axis in every pixel, `params.samples` per axis
        in the pixels whose base colour differs from a neighbour's by more than `threshold` in a
        channel. `refined_ptr`, when given, receives one byte per pixel, 1 where refined."""
        ap = N.AdaptiveParams(int(base_samples), float(threshold), int(chunk_pixels))
        check(N.lib.yrt_render_adaptive(self._h, C.byref(params), C.byref(ap), C.c_void_p(out_ptr),
                                        C.c_void_p(refined_ptr or 0), _mem(device_memory), C.c_void_p(stream or 0)),
              "yrt_render_adaptive")

    def adaptive_refined(self) -> int:
        """the pixels the last render_adaptive_into refined; waits for that call"""
        n = C.c_ulonglong()
        check(N.lib.yrt_scene_adaptive_refined(self._h, C.byref(n)), "yrt_scene_adaptive_refined")
        return int(n.value)

    def render_ao_into(self, params: RenderParams, out_ptr: int, rays: int = 16, distance: float = float("inf"),
                       bias: float = 0.01, device_memory: bool = True, stream: Optional[int] = None) -> None:
        """Launch the ambient occlusion pass (yrt_render_ao) into a caller buffer in render_into's
        layout: per pixel {a, a, a, w}, a the unoccluded share of `rays` cosine-weighted rays
        ([bias, distance]) per camera sample, premultiplied by the coverage w."""
        ap = N.AoParams(int(rays), float(distance), float(bias))
        check(N.lib.yrt_render_ao(self._h, C.byref(params), C.byref(ap), C.c_void_p(out_ptr), _mem(device_memory),
                                  C.c_void_p(stream or 0)), "yrt_render_ao")

    def render_camera_into(self, params: RenderParams, out_ptr: int, model: str = "perspective",
                           aperture: Optional[float] = None, focus: Optional[float] = None, chunk_pixels: int = 0,
                           device_memory: bool = True, stream: Optional[int] = None) -> None:
        """Launch raytrace() under a camera model (yrt_render_camera) into a caller buffer in
        render_into's layout: "perspective" (a thin lens of diameter `aperture`, None: the scene
        camera's, 0: the pinhole, focused at `focus`, None: the scene camera's), "orthographic" or
        "equirect". The camera rays are generated on the device and shaded as ray batches."""
        cm = _camera_model(model, aperture, focus, chunk_pixels)
        check(N.lib.yrt_render_camera(self._h, C.byref(params), C.byref(cm), C.c_void_p(out_ptr), _mem(device_memory),
                                      C.c_void_p(stream or 0)), "yrt_render_camera")

    def camera_rays_into(self, params: RenderParams, rays_ptr: int, model: str = "perspective",
                         aperture: Optional[float] = None, focus: Optional[float] = None, device_memory: bool = True,
                         stream: Optional[int] = None) -> None:
        """Write the camera rays of render_camera_into's frame (yrt_camera_rays): window pixels x
        samples^2 records of 8 float32 {o.xyz, d.xyz, tmin, tmax}, ordered (row, column, jj, ii)."""
        cm = _camera_model(model, aperture, focus, 0)
        check(N.lib.yrt_camera_rays(self._h, C.byref(params), C.byref(cm), C.c_void_p(rays_ptr), _mem(device_memory),
                                    C.c_void_p(stream or 0)), "yrt_camera_rays")

    def render_soft_shadows_into(self, params: RenderParams, out_ptr: int, radius: float = 0.0, light_radii=None,
                                 shadow_rays: int = 16, model: str = "perspective", aperture: Optional[float] = 0.0,
                                 focus: Optional[float] = None, chunk_pixels: int = 0, device_memory: bool = True,
                                 stream: Optional[int] = None) -> None:
        """Launch raytrace() with soft shadows (yrt_render_soft_shadows) into a caller buffer in
        render_into's layout: every light is a disk of `radius` (or light_radii[li], Scene.lights()
        order) facing the shading point, sampled by `shadow_rays` any-hit rays per hit and light;
        radius 0 is the point light. The camera is render_camera_into's (the pinhole by default)."""
        cm = _camera_model(model, aperture, focus, chunk_pixels)
        sp, _keep = _soft_params(radius, light_radii, shadow_rays)
        check(N.lib.yrt_render_soft_shadows(self._h, C.byref(params), C.byref(cm), C.byref(sp), C.c_void_p(out_ptr),
                                            _mem(device_memory), C.c_void_p(stream or 0)), "yrt_render_soft_shadows")

    def shade_rays_soft_into(self, params: RenderParams, rays_ptr: int, n: int, out_ptr: int, radius: float = 0.0,
                             light_radii=None, shadow_rays: int = 16, device_memory: bool = True,
                             stream: Optional[int] = None) -> None:
        """shade_rays_into with render_soft_shadows_into's lights (yrt_shade_rays_soft)."""
        sp, _keep = _soft_params(radius, light_radii, shadow_rays)
        check(N.lib.yrt_shade_rays_soft(self._h, C.byref(params), C.byref(sp), C.c_void_p(rays_ptr), int(n),
                                        C.c_void_p(out_ptr), _mem(device_memory), C.c_void_p(stream or 0)),
              "yrt_shade_rays_soft")

    def last_timings(self) -> dict:
        """per-phase GPU ms of the last render with timing=True: {phase: (ms, launches)}"""
        t = N.Timings()
        check(N.lib.yrt_last_timings(self._h, C.byref(t)), "yrt_last_timings")
        return {name: (float(t.ms[k]), int(t.launches[k])) for k, name in enumerate(N.PHASES)
                if t.launches[k]}

    def last_stats(self) -> dict:
        s = Stats()
        check(N.lib.yrt_last_stats(self._h, C.byref(s)), "yrt_last_stats")
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}


def _camera_model(model: str, aperture, focus, chunk_pixels: int) -> "N.CameraModel":
    """yrt_camera_model of a model's name; None is the scene camera's aperture or focus. An
    unknown name raises before any native call."""
    if model not in N.CAMERA_MODELS:
        raise ValueError(f"unknown camera model {model!r} (one of {', '.join(N.CAMERA_MODELS)})")
    cm = N.CameraModel()
    N.lib.yrt_camera_model_default(C.byref(cm))
    cm.model = N.CAMERA_MODELS[model]
    if aperture is not None:
        cm.aperture = float(aperture)
    if focus is not None:
        cm.focus = float(focus)
    cm.chunk_pixels = int(chunk_pixels)
    return cm


def _soft_params(radius: float, light_radii, shadow_rays: int) -> tuple:
    """(yrt_soft_shadow_params, the array its light_radius points into)"""
    sp = N.SoftShadowParams()
    N.lib.yrt_soft_shadow_params_default(C.byref(sp))
    sp.rays, sp.radius = int(shadow_rays), float(radius)
    radii = None
    if light_radii is not None:
        radii = np.ascontiguousarray(light_radii, dtype=np.float32).reshape(-1)
        keep = radii if radii.size else np.zeros(1, np.float32)  # (no lights: a pointer that is not null)
        sp.light_radius, sp.nlights, radii = keep.ctypes.data_as(C.POINTER(C.c_float)), int(radii.size), keep
    return sp, radii


class MultiScene:
    """A scene replicated on several GPUs of this node (yrt_multi*): raytrace() of a
    whole frame split into interleaved 8-row bands, gathered to devices[0] over RCCL
    (or plain copies when a device is listed twice -- a rehearsal on one GPU)."""

    def __init__(self, scene: "Scene", devices: Sequence[int]):
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        check(N.lib.yrt_multi_create(scene.handle, ids, len(devices), C.byref(h)), "yrt_multi_create")
        self._h = h
        self.devices = tuple(int(d) for d in devices)
        n, tr = C.c_int(), C.c_int()
        check(N.lib.yrt_multi_info(self._h, C.byref(n), C.byref(tr)), "yrt_multi_info")
        self.transport = "rccl" if tr.value == N.YRT_TRANSPORT_RCCL else "copy"

    def close(self):
        if self._h:
            N.lib.yrt_multi_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def render_into(self, params: RenderParams, out_ptr: int, device_memory: bool = False) -> None:
        """raytrace() of the whole frame into a host buffer, or a device buffer on devices[0]"""
        check(N.lib.yrt_multi_render(self._h, C.byref(params), C.c_void_p(out_ptr), _mem(device_memory)),
              "yrt_multi_render")

    def last_stats(self) -> dict:
        s = Stats()
        check(N.lib.yrt_multi_last_stats(self._h, C.byref(s)), "yrt_multi_last_stats")
        return {name: int(getattr(s, name)) for name, _ in Stats._fields_}

    def last_timings(self) -> dict:
        r, g = C.c_float(), C.c_float()
        check(N.lib.yrt_multi_last_timings(self._h, C.byref(r), C.byref(g)), "yrt_multi_last_timings")
        return {"render_ms": r.value, "gather_ms": g.value}


def device_count() -> int:
    n = C.c_int(0)
    N.lib.yrt_device_count(C.byref(n))
    return n.value


def load_scene(filename: str) -> Scene:
    """load_scene (src/scene.cpp:113): Yocto OBJ or .yrtscene. Raises on failure
    (the reference prints "could not load scene" and exits)."""
    h = C.c_void_p()
    check(N.lib.yrt_scene_load(str(filename).encode(), C.byref(h)), f"load_scene({filename})")
    return Scene(h.value)


def build_bvh(scn: Scene, equal_num: bool = False, device: Optional[int] = None) -> Optional[float]:
    """build_bvh (src/scene.cpp:554): per-shape BVHs, then the instance BVH. With
    `device`, the tree construction runs on that GPU (the same nodes byte for byte) and
    the GPU milliseconds of its level passes are returned."""
    if device is None:
        check(N.lib.yrt_host_scene_build_bvh(scn.handle, 1 if equal_num else 0), "build_bvh")
        return None
    ms = C.c_float(0)
    check(N.lib.yrt_host_scene_build_bvh_gpu(scn.handle, 1 if equal_num else 0, int(device), C.byref(ms)),
          "build_bvh(device)")
    return float(ms.value)


def render_params(amb=(0.1, 0.1, 0.1), resolution: int = 720, samples: int = 1, *,
                  width: int = 0, max_depth: int = 16, camera: int = 0, window=None,
                  band=(1, 1, 0), count_work: bool = False, algorithm: str = "wavefront",
                  timing: int = 0) -> RenderParams:
    p = RenderParams()
    N.lib.yrt_render_params_default(C.byref(p))
    if np.isscalar(amb):
        amb = (amb, amb, amb)
    for k in range(3):
        p.ambient[k] = float(amb[k])
    p.resolution, p.samples, p.width = int(resolution), int(samples), int(width)
    p.max_depth, p.camera = int(max_depth), int(camera)
    if window is not None:
        p.x0, p.y0, p.tile_w, p.tile_h = (int(v) for v in window)
    p.band, p.band_stride, p.band_offset = (int(v) for v in band)
    p.count_work = 1 if count_work else 0
    p.algorithm = ALGORITHMS[algorithm]
    p.timing = int(timing)
    return p


def _device_scene(scn, device: int = 0) -> DeviceScene:
    if isinstance(scn, DeviceScene):
        return scn
    return scn.upload(device)


def _mem(device_memory: bool) -> int:
    return N.YRT_MEM_DEVICE if device_memory else N.YRT_MEM_HOST


def _name_mask(names, table: dict, noun: str) -> int:
    """the bit mask of `names` in `table` (N.AOVS, N.MATTE_KEYS or N.PASSES: name -> bit); an
    unknown name, or no name at all, raises before any native call"""
    names = list(names)
    bad = [n for n in names if n not in table]
    if bad or not names:
        raise ValueError((f"unknown {noun} {bad[0]!r}" if bad else f"no {noun} named") + f" (one of {', '.join(table)})")
    mask = 0
    for n in names:
        mask |= 1 << table[n]
    return mask


def _window_shape(ds: DeviceScene, p: RenderParams, window) -> tuple:
    """(h, w) of the arrays a render of `p` fills: the window's, or the whole image's"""
    W, H = ds.image_size(p)
    if window is None:
        return H, W
    return window[3] or H - window[1], window[2] or W - window[0]


def raytrace(scn, amb: Sequence[float] = (0.1, 0.1, 0.1), resolution: int = 720, samples: int = 1,
             *, width: int = 0, max_depth: int = 16, camera: int = 0, window=None,
             count_work: bool = False, return_stats: bool = False, algorithm: str = "wavefront",
             devices: Optional[Sequence[int]] = None):
    """raytrace (src/raytrace.cpp:213): RGBA float32 image (H, W, 4), row-major.

    `samples` is per axis (s*s samples per pixel), `resolution` the vertical size.
    `window` = (x0, y0, w, h) renders a sub-rectangle only. `devices` (a Scene, whole
    frames) splits the frame over those GPUs (MultiScene)."""
    if devices is not None:
        if window is not None or isinstance(scn, DeviceScene):
            raise ValueError("devices= renders whole frames of a host Scene")
        ms = MultiScene(scn, devices)
        try:
            p = render_params(amb, resolution, samples, width=width, max_depth=max_depth, camera=camera,
                              count_work=count_work, algorithm=algorithm)
            W, H = scn.image_size(resolution, camera)  # host-side: no extra replica on devices[0]
            W = int(width) or W
            img = np.zeros((H, W, 4), np.float32)
            ms.render_into(p, img.ctypes.data)
            stats = ms.last_stats()
        finally:
            ms.close()
        return (img, stats) if return_stats else img
    ds = _device_scene(scn)
    p = render_params(amb, resolution, samples, width=width, max_depth=max_depth, camera=camera,
                      window=window, count_work=count_work, algorithm=algorithm)
    h, w = _window_shape(ds, p, window)
    img = np.zeros((h, w, 4), np.float32)
    ds.render_into(p, img.ctypes.data, device_memory=False)
    if return_stats:
        return img, ds.last_stats()
    return img


def raytrace_adaptive(scn, amb: Sequence[float] = (0.1, 0.1, 0.1), resolution: int = 720, samples: int = 1, *,
                      threshold: float, base_samples: int = 1, width: int = 0, window=None, max_depth: int = 16,
                      algorithm: str = "wavefront", chunk_pixels: int = 0, return_mask: bool = False,
                      return_stats: bool = False):
    """raytrace with adaptive supersampling: every pixel gets base_samples x base_samples camera
    samples, and a pixel whose base colour differs from one of its eight neighbours' by more than
    `threshold` in r, g or b gets raytrace's value at samples x samples instead, bit for bit.
    Returns the (H, W, 4) float32 image; with `return_mask` also the (H, W) uint8 mask of the
    refined pixels, with `return_stats` also last_stats() plus "refined_pixels". `chunk_pixels`
    (0: chosen by the library) sizes the shading batches and never changes a bit. `scn` is a
    Scene or a DeviceScene, as for raytrace."""
    ds = _device_scene(scn)
    p = render_params(amb, resolution, samples, width=width, max_depth=max_depth, window=window, algorithm=algorithm)
    h, w = _window_shape(ds, p, window)
    img = np.zeros((h, w, 4), np.float32)
    mask = np.zeros((h, w), np.uint8) if return_mask else None
    ds.render_adaptive_into(p, img.ctypes.data, threshold, base_samples,
                            refined_ptr=mask.ctypes.data if return_mask else None, chunk_pixels=chunk_pixels,
                            device_memory=False)
    out = (img,) + ((mask,) if return_mask else ())
    if return_stats:
        out += (dict(ds.last_stats(), refined_pixels=ds.adaptive_refined()),)
    return out if len(out) > 1 else img


def raytrace_camera(scn, amb: Sequence[float] = (0.1, 0.1, 0.1), resolution: int = 720, samples: int = 1, *,
                    model: str = "perspective", aperture: Optional[float] = None, focus: Optional[float] = None,
                    width: int = 0, window=None, max_depth: int = 16, camera: int = 0, algorithm: str = "wavefront",
                    chunk_pixels: int = 0, return_stats: bool = False):
    """raytrace under another camera model: "perspective" is a thin lens of diameter `aperture`
    (None: the scene camera's own, 0: the pinhole, which gives raytrace's image bit for bit)
    focused at the distance `focus` (None: the scene camera's), "orthographic" a film of the
    perspective view's size at the focus distance, "equirect" the 360 x 180 degree panorama
    (pass width = 2 * resolution for pixels that are square in angle). The camera rays are
    generated on the GPU, shaded as ray batches and box filtered there: the image equals the box
    filter of shade_rays(camera_rays(...)) bit for bit. `chunk_pixels` (0: chosen by the library)
    sizes the batches and never changes a bit. Returns the (H, W, 4) float32 image, with
    `return_stats` also last_stats(). `scn` is a Scene or a DeviceScene, as for raytrace."""
    ds = _device_scene(scn)
    p = render_params(amb, resolution, samples, width=width, max_depth=max_depth, camera=camera, window=window,
                      algorithm=algorithm)
    h, w = _window_shape(ds, p, window)
    img = np.zeros((h, w, 4), np.float32)
    ds.render_camera_into(p, img.ctypes.data, model, aperture, focus, chunk_pixels, device_memory=False)
    if return_stats:
        return img, ds.last_stats()
    return img


def raytrace_soft(scn, amb: Sequence[float] = (0.1, 0.1, 0.1), resolution: int = 720, samples: int = 1, *,
                  radius: float = 0.0, light_radii=None, shadow_rays: int = 16, model: str = "perspective",
                  aperture: Optional[float] = 0.0, focus: Optional[float] = None, width: int = 0, window=None,
                  max_depth: int = 16, camera: int = 0, algorithm: str = "wavefront", chunk_pixels: int = 0,
                  device_memory: bool = False, return_stats: bool = False):
    """raytrace with soft shadows: every light is a disk of `radius` (or light_radii[li], in
    Scene.lights() order) that faces the shading point, and every hit, at every mirror level,
    casts `shadow_rays` (1..64) any-hit rays per light at it; a light's term is scaled by the
    share that arrives. Radius 0 is the point light: with every radius 0 the image is raytrace's
    bit for bit. The camera is raytrace_camera's (by default the pinhole, aperture 0), so soft
    shadows and a thin lens combine. `device_memory` renders into device memory (a torch tensor)
    and copies the plane back. Returns the (H, W, 4) float32 image, with `return_stats` also
    last_stats()."""
    ds = _device_scene(scn)
    p = render_params(amb, resolution, samples, width=width, max_depth=max_depth, camera=camera, window=window,
                      algorithm=algorithm)
    h, w = _window_shape(ds, p, window)
    args = (radius, light_radii, shadow_rays, model, aperture, focus, chunk_pixels)
    if device_memory:
        import torch

        dev = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        ds.render_soft_shadows_into(p, dev.data_ptr(), *args, device_memory=True,
                                    stream=torch.cuda.current_stream().cuda_stream)
        img = dev.cpu().numpy()
    else:
        img = np.zeros((h, w, 4), np.float32)
        ds.render_soft_shadows_into(p, img.ctypes.data, *args, device_memory=False)
    if return_stats:
        return img, ds.last_stats()
    return img


def camera_rays(scn, resolution: int = 720, samples: int = 1, *, model: str = "perspective",
                aperture: Optional[float] = None, focus: Optional[float] = None, width: int = 0, window=None,
                camera: int = 0) -> np.ndarray:
    """The camera rays raytrace_camera shades, (n, 8) float32 {o.xyz, d.xyz, tmin, tmax} in the
    order (row, column, jj, ii) of the window (or the whole image): shade_rays' input."""
    ds = _device_scene(scn)
    p = render_params(resolution=resolution, samples=samples, width=width, camera=camera, window=window)
    h, w = _window_shape(ds, p, window)
    rays = np.zeros((h * w * int(samples) ** 2, 8), np.float32)
    ds.camera_rays_into(p, rays.ctypes.data, model, aperture, focus, device_memory=False)
    return rays


def render_aovs(scn, resolution: int = 720, samples: int = 1, *, aovs: Sequence[str] = tuple(N.AOVS),
                width: int = 0, camera: int = 0, window=None, device: int = 0) -> dict:
    """The camera hit's geometry buffers on raytrace's sample grid: {name: (H, W, 4)}, float32
    {value.xyz premultiplied by coverage, coverage} for "depth", "position", "normal",
    "texcoord" and "albedo", int32 {instance, element, material, shape} of the pixel's first
    sample for "ids" (-1 on a miss). `scn` is a Scene or a DeviceScene, as for raytrace."""
    _name_mask(aovs, N.AOVS, "AOV")
    ds = _device_scene(scn, device)
    p = render_params(resolution=resolution, samples=samples, width=width, camera=camera, window=window)
    h, w = _window_shape(ds, p, window)
    out = {n: np.zeros((h, w, 4), np.int32 if n == "ids" else np.float32) for n in aovs}
    ds.render_aovs_into(p, {n: a.ctypes.data for n, a in out.items()}, device_memory=False)
    return out


def render_mattes(scn, resolution: int = 720, samples: int = 1, *, keys: Sequence[str] = ("instance",),
                  ranks: int = 4, width: int = 0, window=None, camera: int = 0, device: int = 0) -> dict:
    """ID mattes on raytrace's sample grid, every key from one pass: {key: {"ids": (H, W, ranks)
    int32, "coverage": (H, W, ranks) float32}, ..., "dropped": {key: int}} for the keys
    "instance", "material" and "shape" (the .x, .z and .w of render_aovs' "ids"). Per pixel the
    ids covering it, ranked by their share of the pixel's s*s samples (ties by id), -1 and +0
    in unused ranks; `ranks` is 4 or 8, and a sample whose id finds all ranks taken is dropped
    and counted under "dropped". matte() turns a key's arrays and a set of ids into a mask that
    is box filtered as the beauty is. `scn` is a Scene or a DeviceScene, as for raytrace."""
    keys = list(keys)
    _name_mask(keys, N.MATTE_KEYS, "matte key")
    if isinstance(ranks, bool) or ranks not in (4, 8):
        raise ValueError(f"ranks must be 4 or 8, not {ranks!r}")
    layers = int(ranks) // 4
    ds = _device_scene(scn, device)
    p = render_params(resolution=resolution, samples=samples, width=width, camera=camera, window=window)
    h, w = _window_shape(ds, p, window)
    planes = {k: {"ids": [np.zeros((h, w, 4), np.int32) for _ in range(layers)],
                  "coverage": [np.zeros((h, w, 4), np.float32) for _ in range(layers)]} for k in keys}
    ds.render_mattes_into(p, {k: {n: [a.ctypes.data for a in v] for n, v in kp.items()} for k, kp in planes.items()},
                          layers, device_memory=False)
    out = {k: {n: np.concatenate(v, axis=-1) for n, v in kp.items()} for k, kp in planes.items()}
    dropped = ds.matte_dropped()
    out["dropped"] = {k: dropped[k] for k in keys}
    return out


def render_ao(scn, resolution: int = 720, samples: int = 1, *, rays: int = 16, distance: float = float("inf"),
              bias: float = 0.01, width: int = 0, window=None, camera: int = 0, device: int = 0,
              return_stats: bool = False):
    """Ambient occlusion on raytrace's sample grid: (H, W, 4) float32 {a, a, a, w}. Every camera
    sample that hits a triangle casts `rays` (1..64) cosine-weighted rays over [bias, distance]
    about its face-forward shading normal (the directions of ao_tables()); a hit on a line or a
    point counts as unoccluded. a is the unoccluded share of the pixel's rays times the coverage
    w (render_aovs' .w), so a / w is the ambient occlusion in [0, 1]. A count, so the same bits on
    every run. `scn` is a Scene or a DeviceScene, as for raytrace."""
    ds = _device_scene(scn, device)
    p = render_params(resolution=resolution, samples=samples, width=width, camera=camera, window=window)
    h, w = _window_shape(ds, p, window)
    img = np.zeros((h, w, 4), np.float32)
    ds.render_ao_into(p, img.ctypes.data, rays, distance, bias, device_memory=False)
    if return_stats:
        return img, ds.last_stats()
    return img


def ao_tables() -> tuple:
    """the tables render_ao's kernel reads: dirs (64, 3) float32, the cosine-weighted directions
    about +z of which a call uses the first `rays`, and rots (16, 2) float32, (cos, sin) of the
    rotation about the normal that a camera sample applies to them"""
    dirs, rots = np.zeros((64, 3), np.float32), np.zeros((16, 2), np.float32)
    fp = C.POINTER(C.c_float)
    check(N.lib.yrt_ao_tables(dirs.ctypes.data_as(fp), rots.ctypes.data_as(fp)), "yrt_ao_tables")
    return dirs, rots


def matte(m: dict, ids) -> np.ndarray:
    """The (H, W) float32 matte of the ids in `ids` from one key's arrays m = {"ids", "coverage"}
    (render_mattes): from +0, in rank order, acc = acc + where(m["ids"][..., r] in ids,
    m["coverage"][..., r], +0) in float32 -- a fixed order, so the same bits every time."""
    mi, mc = np.asarray(m["ids"]), np.asarray(m["coverage"], np.float32)
    if mi.shape != mc.shape or mi.ndim < 1:
        raise ValueError("matte: ids and coverage must have the same shape (..., ranks)")
    wanted = np.asarray(list(ids), np.int64).reshape(-1)
    acc = np.zeros(mi.shape[:-1], np.float32)
    for r in range(mi.shape[-1]):
        acc = (acc + np.where(np.isin(mi[..., r], wanted), mc[..., r], np.float32(0))).astype(np.float32)
    return acc


def render_passes(scn, amb: Sequence[float] = (0.1, 0.1, 0.1), resolution: int = 720, samples: int = 1, *,
                  passes: Sequence[str] = tuple(N.PASSES), beauty: bool = True, width: int = 0, max_depth: int = 16,
                  camera: int = 0, window=None, algorithm: str = "wavefront", devices=None, device: int = 0) -> dict:
    """raytrace with its lighting split: {name: (H, W, 4) float32} for "direct" (diffuse +
    specular per light), "diffuse", "specular", "reflection" (the mirror ray's colour times
    kr) and "ambient", each the box filter of that term of shade() (raytrace.cpp:88-211), and
    with `beauty` the image raytrace gives, under "beauty", from the same render. At one sample
    per pixel beauty == (direct + reflection) + ambient in float32. One GPU: `devices` is not
    supported (shard with a window or bands instead)."""
    _name_mask(passes, N.PASSES, "pass")
    if devices is not None:
        raise ValueError("render_passes renders on one GPU: devices= is not supported")
    ds = _device_scene(scn, device)
    p = render_params(amb, resolution, samples, width=width, max_depth=max_depth, camera=camera, window=window,
                      algorithm=algorithm)
    h, w = _window_shape(ds, p, window)
    out = {n: np.zeros((h, w, 4), np.float32) for n in passes}
    img = np.zeros((h, w, 4), np.float32) if beauty else None
    ds.render_passes_into(p, {n: a.ctypes.data for n, a in out.items()},
                          beauty_ptr=img.ctypes.data if beauty else None, device_memory=False)
    if beauty:
        out["beauty"] = img
    return out


def _light_groups(groups, ngroups: Optional[int] = None) -> int:
    """the number of groups `groups` names (each entry a group in [0, YRT_LIGHT_GROUPS_MAX) or
    -1; at least one group); a bad entry raises before any native call"""
    gs = list(groups)
    for g in gs:
        if not isinstance(g, (int, np.integer)) or isinstance(g, bool) or g < -1 or g >= N.YRT_LIGHT_GROUPS_MAX:
            raise ValueError(f"light group {g!r}: an integer from -1 (no plane) to {N.YRT_LIGHT_GROUPS_MAX - 1}")
    need = max([int(g) for g in gs] + [0]) + 1
    if ngroups is None:
        return need
    if not need <= ngroups <= N.YRT_LIGHT_GROUPS_MAX:
        raise ValueError(f"{ngroups} planes for light groups 0..{need - 1} (at most {N.YRT_LIGHT_GROUPS_MAX})")
    return ngroups


def render_light_groups(scn, amb: Sequence[float] = (0.1, 0.1, 0.1), resolution: int = 720, samples: int = 1, *,
                        groups: Sequence[int], ambient: bool = True, beauty: bool = True, width: int = 0,
                        max_depth: int = 16, camera: int = 0, window=None, algorithm: str = "wavefront",
                        devices=None, device: int = 0) -> dict:
    """raytrace split by light: `groups` gives each light of the scene (Scene.lights() order) its
    group, 0 to 7, or -1 for a light that is in no plane. Returns {"groups": [(H, W, 4) float32 per
    group], "ambient": ..., "beauty": ...} from one render: a group's plane is the image its lights
    alone produce (mirror reflections included, ambient 0), "ambient" the image of the ambient term
    alone, "beauty" the image raytrace gives. The image is linear in each light's ke and in the
    ambient, so the beauty is the sum of the planes up to float32 rounding and a light can be
    rescaled or recoloured without tracing a ray. One GPU: `devices` is not supported."""
    ngroups = _light_groups(groups)
    if devices is not None:
        raise ValueError("render_light_groups renders on one GPU: devices= is not supported")
    host = scn.host if isinstance(scn, DeviceScene) else scn
    if len(list(groups)) != len(host.lights()):
        raise ValueError(f"groups names {len(list(groups))} lights, the scene has {len(host.lights())}")
    ds = _device_scene(scn, device)
    p = render_params(amb, resolution, samples, width=width, max_depth=max_depth, camera=camera, window=window,
                      algorithm=algorithm)
    h, w = _window_shape(ds, p, window)
    out = {"groups": [np.zeros((h, w, 4), np.float32) for _ in range(ngroups)]}
    if ambient:
        out["ambient"] = np.zeros((h, w, 4), np.float32)
    if beauty:
        out["beauty"] = np.zeros((h, w, 4), np.float32)
    ds.render_light_groups_into(p, list(groups), [a.ctypes.data for a in out["groups"]],
                                ambient_ptr=out["ambient"].ctypes.data if ambient else None,
                                beauty_ptr=out["beauty"].ctypes.data if beauty else None, device_memory=False)
    return out


def _rays_array(rays) -> np.ndarray:
    r = np.ascontiguousarray(rays, dtype=np.float32)
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError("rays must be (n, 8): o.xyz, d.xyz, tmin, tmax")
    return r


def intersect_first(scn, rays) -> dict:
    """Batch intersect_first (src/scene.cpp:483): per ray hit, instance, ei, ew[4], dist."""
    ds = _device_scene(scn)
    r = _rays_array(rays)
    n = r.shape[0]
    out = {"hit": np.zeros(n, np.uint8), "inst": np.zeros(n, np.int32), "ei": np.zeros(n, np.int32),
           "ew": np.zeros((n, 4), np.float32), "dist": np.zeros(n, np.float32)}
    check(N.lib.yrt_trace_first(ds.handle, r.ctypes.data, n, out["hit"].ctypes.data,
                                out["inst"].ctypes.data, out["ei"].ctypes.data, out["ew"].ctypes.data,
                                out["dist"].ctypes.data, N.YRT_MEM_HOST, None), "intersect_first")
    out["hit"] = out["hit"].astype(bool)
    return out


def intersect_any(scn, rays) -> np.ndarray:
    """Batch intersect_any (src/scene.cpp:489): occluded flag per ray."""
    ds = _device_scene(scn)
    r = _rays_array(rays)
    hit = np.zeros(r.shape[0], np.uint8)
    check(N.lib.yrt_trace_any(ds.handle, r.ctypes.data, r.shape[0], hit.ctypes.data, N.YRT_MEM_HOST,
                              None), "intersect_any")
    return hit.astype(bool)


def shade_rays(scn, rays, amb: Sequence[float] = (0.1, 0.1, 0.1), *, max_depth: int = 16,
               algorithm: str = "wavefront", return_stats: bool = False):
    """Batch shade (src/raytrace.cpp:88): the colour of each caller ray, (n, 4) float32 {c.xyz, 1},
    {0, 0, 0, 1} on a miss. `rays` is (n, 8) {o.xyz, d.xyz, tmin, tmax}, used as given (d is not
    renormalised; the view vector comes from each ray's own origin), so any camera model can be
    written as a ray generator. `scn` is a Scene or a DeviceScene, as for raytrace."""
    r = _rays_array(rays)
    ds = _device_scene(scn)
    p = render_params(amb, max_depth=max_depth, algorithm=algorithm)
    out = np.zeros((r.shape[0], 4), np.float32)
    ds.shade_rays_into(p, r.ctypes.data, r.shape[0], out.ctypes.data, device_memory=False)
    if return_stats:
        return out, ds.last_stats()
    return out


def shade_rays_soft(scn, rays, amb: Sequence[float] = (0.1, 0.1, 0.1), *, radius: float = 0.0, light_radii=None,
                    shadow_rays: int = 16, max_depth: int = 16, algorithm: str = "wavefront",
                    return_stats: bool = False):
    """shade_rays with raytrace_soft's lights: (n, 4) float32 {c.xyz, 1} per caller ray."""
    r = _rays_array(rays)
    ds = _device_scene(scn)
    p = render_params(amb, max_depth=max_depth, algorithm=algorithm)
    out = np.zeros((r.shape[0], 4), np.float32)
    ds.shade_rays_soft_into(p, r.ctypes.data, r.shape[0], out.ctypes.data, radius, light_radii, shadow_rays,
                            device_memory=False)
    if return_stats:
        return out, ds.last_stats()
    return out


def tonemap(img: np.ndarray) -> np.ndarray:
    """tonemap (src/image.cpp:55, exposure 0, srgb): RGBA8 of the same shape."""
    a = np.ascontiguousarray(img, dtype=np.float32)
    out = np.zeros(a.shape, np.uint8)
    check(N.lib.yrt_tonemap(a.ctypes.data, a.size // 4, out.ctypes.data, N.YRT_MEM_HOST, None), "tonemap")
    return out


def save_image_device(filename: str, ptr: int, width: int, height: int, stream: Optional[int] = None) -> None:
    """save_hdr_or_ldr of a frame in device memory: the PNG tonemap runs on the GPU"""
    check(N.lib.yrt_save_image_mem(str(filename).encode(), C.c_void_p(ptr), int(width), int(height),
                                   N.YRT_MEM_DEVICE, C.c_void_p(stream or 0)), "save_image_device")


def tonemap_device(rgba_ptr: int, n: int, out_ptr: int, stream: Optional[int] = None) -> None:
    """tonemap (src/image.cpp:55) of n RGBA f32 pixels in device memory into RGBA8 (device)"""
    check(N.lib.yrt_tonemap(C.c_void_p(rgba_ptr), int(n), C.c_void_p(out_ptr), N.YRT_MEM_DEVICE,
                            C.c_void_p(stream or 0)), "tonemap_device")


def save_hdr_or_ldr(filename: str, img: np.ndarray) -> None:
    """save_hdr_or_ldr (src/image.cpp:81): .hdr -> RGBE, otherwise tonemapped PNG."""
    a = np.ascontiguousarray(img, dtype=np.float32)
    check(N.lib.yrt_save_image(str(filename).encode(), a.ctypes.data, a.shape[1], a.shape[0]),
          "save_hdr_or_ldr")
