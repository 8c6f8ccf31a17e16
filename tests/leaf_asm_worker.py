"""Renders a scene made for the triangle leaves' scans (leaf_asm.h) on whatever library YRT_LIB
names and stores what came out, for tests/test_gpu_leaf_asm.py (which starts it as a fresh child
process, one library at a time; not a test module itself).

    YRT_LIB=yocto_raytracing_amd/variants/libyrt_cleaf.so python tests/leaf_asm_worker.py out.npz scene.yrtscene

The scene is first_nested_worker.build_scene's (enough instances for camera lists and shadow
bundles) plus, in front of its rows and facing the view camera:

  `quad`    one shape of exactly four triangles -- one leaf, its triangles in this slot order:
              0  three equal vertices: e1 = e2 = 0, so den == 0 on every lane;
              1  edges of 1e-20: den = -d.z * 1e-40, a denormal, so the scan leaves for the
                 compiled triangle test (rcp_nr_ok fails; so it does at triangle 0);
              2  a visible triangle at local z = +0.3;
              3  a visible triangle behind it at local z = -0.3, a little larger.
            Instance `near_far` has the identity frame: the camera meets triangle 2 first and
            triangle 3 is rejected by the tmax it left. Instance `far_near` is turned half round y:
            triangle 2 is now the far one, so one scan has two hits with a tmax update between.
  `single`  a one-triangle shape (a leaf of count 1), one instance.
  a light   an emissive point above and in front, so that the shadows of all three fall on the
            floor in view: the floor's shadow rays meet the same leaves in the any-hit scan.

out.npz holds the float32 frames at 37 x 24, 2 x 2 and 8 x 8 spp ("s2.img", "s8.img"), tile lists
forced on, and in "meta" (JSON) each frame's last_stats(), tile_lists() and per-phase launch
counts (of a second, timing=1 render, which must give the same bits), the added instances, the
light's position and the view camera. The scene is saved to the second argument for the test's
CPU-side reading (tests/helpers.py Oracle).

Only tests/golden and the package are read.
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from first_nested_worker import HEIGHT, SAMPLES, WIDTH, build_scene  # noqa: E402

TINY = 1e-20
QUAD_POS = np.array([[0.1, 0.1, 0.0], [0.1, 0.1, 0.0], [0.1, 0.1, 0.0],            # 0: no area
                     [0.0, 0.0, 0.0], [TINY, 0.0, 0.0], [0.0, TINY, 0.0],          # 1: edges of 1e-20
                     [-0.4, -0.4, 0.3], [0.4, -0.4, 0.3], [0.0, 0.4, 0.3],         # 2
                     [-0.5, -0.5, -0.3], [0.5, -0.5, -0.3], [0.0, 0.5, -0.3]],     # 3
                    np.float32)
QUAD_TRIANGLES = np.arange(12).reshape(4, 3)
SINGLE_POS = np.array([[-0.35, -0.3, 0.0], [0.35, -0.3, 0.0], [0.0, 0.35, 0.0]], np.float32)
ORIGINS = {"near_far": (-0.8, 1.2, 2.0), "far_near": (0.8, 1.2, 2.0), "single": (0.0, 2.1, 2.0)}
HALF_TURN_Y = (-1, 0, 0, 0, 1, 0, 0, 0, -1)
LIGHT_POS = (0.0, 4.5, 3.5)


def build_leaf_scene(yrt):
    """-> scene, {"near_far", "far_near", "single", "light": instance indices}, the view camera"""
    s, _, view, _, _ = build_scene(yrt)
    m = s.add_material(kd=(0.6, 0.4, 0.3))
    facing = lambda n: np.tile([0.0, 0.0, 1.0], (n, 1))  # noqa: E731
    quad = s.add_shape(QUAD_POS, norm=facing(12), triangles=QUAD_TRIANGLES)
    single = s.add_shape(SINGLE_POS, norm=facing(3), triangles=np.arange(3).reshape(1, 3))
    ident = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    inst = {"near_far": s.add_instance(np.r_[ident, ORIGINS["near_far"]].astype(np.float32), quad, m),
            "far_near": s.add_instance(np.r_[HALF_TURN_Y, ORIGINS["far_near"]].astype(np.float32), quad, m),
            "single": s.add_instance(np.r_[ident, ORIGINS["single"]].astype(np.float32), single, m)}
    glow = s.add_material(ke=(30.0, 30.0, 30.0))
    bulb = s.add_shape(np.zeros((1, 3), np.float32), radius=np.full(1, 0.001), points=np.arange(1))
    inst["light"] = s.add_instance(np.r_[ident, LIGHT_POS].astype(np.float32), bulb, glow)
    if inst["light"] not in s.lights():
        raise RuntimeError("the added point instance is not a light")
    return s, inst, view


def main(argv):
    out_path, scene_path = argv
    import yocto_raytracing_amd as yrt
    from yocto_raytracing_amd import _native as N

    if yrt.device_count() < 1:
        raise RuntimeError("no GPU visible")
    s, inst, view = build_leaf_scene(yrt)
    s.save(scene_path)
    yrt.build_bvh(s)
    ds = s.upload(0)
    ds.set_tile_lists("on")
    arrays = {}
    meta = {"library": str(N.LIB_PATH), "instances": inst, "frames": {}, "light_pos": list(LIGHT_POS), "camera": view}
    for ns in SAMPLES:
        kw = dict(width=WIDTH, max_depth=16, camera=view, algorithm="wavefront")
        img, stats = yrt.raytrace(ds, (0.1, 0.1, 0.1), HEIGHT, ns, return_stats=True, **kw)
        lists = ds.tile_lists()
        timed = np.zeros_like(img)
        ds.render_into(yrt.render_params(0.1, HEIGHT, ns, timing=1, **kw), timed.ctypes.data, device_memory=False)
        launches = {phase: n for phase, (_, n) in ds.last_timings().items()}
        if not np.array_equal(img.view(np.uint32), timed.view(np.uint32)):
            raise RuntimeError(f"s{ns}: the timing=1 render differs from the plain one")
        arrays[f"s{ns}.img"] = img
        meta["frames"][f"s{ns}"] = {"stats": stats, "tile_lists": lists, "launches": launches}
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
