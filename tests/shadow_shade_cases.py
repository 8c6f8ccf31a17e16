"""The cases of tests/test_gpu_shadow_shade_fused.py and tests/shadow_shade_worker.py (not a test
module): what is rendered, how, and which of it level 0's fused kernel
(k_shadow_shade_persist, wavefront.hip) must take.

Frames of 37 x 24 pixels (5 x 3 tiles of 8 x 8, partial on both axes) with the tile lists
forced on, which puts level 0's shadow rays on the persistent any-hit grid at this size. The
fused kernel runs where an item of that grid is whole pixels (1, 4, 16 or 64 spp), the render
has one level and the scene has 1 to 32 lights; every other case keeps k_shadow_persist and
k_shade.
"""
import numpy as np

RES, WIDTH = 24, 37
AMB = 0.1
FUSED_SAMPLES = (1, 2, 4, 8)  # per axis: 1, 4, 16, 64 spp
CONTROL_SAMPLES = 3           # 9 spp: an item is not whole pixels
GOLDEN_SCENES = ("simple", "instance1k", "lines", "refl", "edge_unlit", "edge_lightsonly", "edge_sky", "edge_empty")
BUILT_LIGHTS = (5, 33)        # more than OCC4's four; more than the mask's 32
# one level for the scene with mirrors (its reflective hits take the truncated branch) and for
# `lines`, so that neither can have a second one
ONE_LEVEL = ("refl", "lines")
BAND = (8, 3, 1)              # rank 1 of 3: image rows 8..15
BAND_TILE_H = 16              # padded past the frame: local rows 8..15 are image rows 32..39


def built_name(nlights):
    return f"lights{nlights}"


def build_lights(yrt, nlights):
    """a floor, an upright panel that shadows part of it, a glossy rotated panel and `nlights`
    point lights of different colours on an arc above them (scene builder, BVH not built)"""
    s = yrt.Scene.create()
    eye = np.array([0.4, 2.2, 6.5], np.float32)
    z = eye / np.linalg.norm(eye)
    x = np.cross([0, 1, 0], z).astype(np.float32)
    x /= np.linalg.norm(x)
    y = np.cross(z, x).astype(np.float32)
    s.add_camera(np.concatenate([x, y, z, eye]).astype(np.float32), fovy=0.7, aspect=WIDTH / RES,
                 focus=float(np.linalg.norm(eye)))
    floor_m = s.add_material(kd=(0.8, 0.7, 0.6), ks=(0.1, 0.1, 0.1), rs=0.5)
    panel_m = s.add_material(kd=(0.3, 0.4, 0.6), ks=(0.4, 0.4, 0.3), rs=0.25)

    def quad(pos, n):
        return s.add_shape(np.asarray(pos, np.float32), norm=np.tile(np.asarray(n, np.float32), (4, 1)),
                           texcoord=np.asarray(((0, 0), (1, 0), (1, 1), (0, 1)), np.float32),
                           triangles=np.array([[0, 1, 2], [0, 2, 3]], np.int32))

    def frame(rot=None, o=(0, 0, 0)):
        r = np.eye(3, dtype=np.float32) if rot is None else rot
        return np.concatenate([r.reshape(-1), np.asarray(o, np.float32)]).astype(np.float32)

    floor = quad([[-5, 0, 5], [5, 0, 5], [5, 0, -5], [-5, 0, -5]], (0, 1, 0))
    panel = quad([[-0.8, 0, 0], [0.8, 0, 0], [0.8, 1.6, 0], [-0.8, 1.6, 0]], (0, 0, 1))
    c, sn = np.float32(np.cos(0.6)), np.float32(np.sin(0.6))
    rot = np.array([[c, 0, -sn], [0, 1, 0], [sn, 0, c]], np.float32)
    s.add_instance(frame(), floor, floor_m)
    s.add_instance(frame(o=(-0.5, 0.0, 0.6)), panel, panel_m)
    s.add_instance(frame(rot, (1.9, 0.0, 1.2)), panel, panel_m)
    for k in range(nlights):
        a = np.pi * (k + 0.5) / nlights
        pos = (4.0 * np.cos(a), 3.0 + 0.5 * np.sin(3 * a), 2.5 + 2.0 * np.sin(a))
        ke = tuple(float(v) for v in 60.0 / nlights * np.array([1 + k % 3, 1 + (k + 1) % 3, 1 + (k + 2) % 3]))
        m = s.add_material(ke=ke)
        # shade() takes a light's position from its shape's first vertex (raytrace.cpp:129)
        lamp = s.add_shape(np.asarray([pos], np.float32), norm=np.asarray([[0, 1, 0]], np.float32),
                           texcoord=np.asarray([[0.5, 0.5]], np.float32), radius=np.array([0.002], np.float32),
                           points=np.array([0], np.int32))
        s.add_instance(frame(), lamp, m)
    return s


def max_depth_of(scene):
    return 1 if scene in ONE_LEVEL else 16


def case_id(scene, samples, band=False):
    return f"{scene}-s{samples}" + ("-band" if band else "")


def cases():
    """[(id, scene, samples per axis, band render?)]"""
    out = []
    for scene in (*GOLDEN_SCENES, *(built_name(n) for n in BUILT_LIGHTS)):
        for s in (*FUSED_SAMPLES, CONTROL_SAMPLES):
            out.append((case_id(scene, s), scene, s, False))
    for s in (2, CONTROL_SAMPLES):
        out.append((case_id("simple", s, True), "simple", s, True))
    return out


def takes_fused(nlights, samples):
    """run()'s condition for these cases: the lists are on (the persistent grid runs), one level"""
    return 1 <= nlights <= 32 and 64 % (samples * samples) == 0


class Scenes:
    """host and device scenes by name, loaded or built once; `tmp`: where a built scene's
    .yrtscene file (the oracle reads it) goes"""

    def __init__(self, yrt, tmp):
        self.yrt, self.tmp, self.cache = yrt, tmp, {}

    def get(self, name):
        """(host scene, .yrtscene path, device scene)"""
        if name not in self.cache:
            from helpers import SCENES

            if name.startswith("lights"):
                host = build_lights(self.yrt, int(name[len("lights"):]))
                path = self.tmp / f"{name}.yrtscene"
                host.save(str(path))
            else:
                path = SCENES / f"{name}.yrtscene"
                host = self.yrt.load_scene(str(path))
            self.yrt.build_bvh(host)
            self.cache[name] = (host, path, host.upload(0))
        return self.cache[name]


def render(yrt, ds, scene, samples, band):
    """one timed render with the lists forced on: (frame, last_stats(), {phase: launches})"""
    kw = dict(width=WIDTH, max_depth=max_depth_of(scene), timing=1)
    if band:
        kw.update(band=BAND, window=(0, 0, WIDTH, BAND_TILE_H))
    rows = BAND_TILE_H if band else RES
    img = np.full((rows, WIDTH, 4), np.nan, np.float32)
    ds.set_tile_lists("on")
    try:
        ds.render_into(yrt.render_params(AMB, RES, samples, **kw), img.ctypes.data, device_memory=False)
        stats = ds.last_stats()
        launches = {phase: n for phase, (_, n) in ds.last_timings().items() if n}
    finally:
        ds.set_tile_lists("auto")
    return img, stats, launches
