"""Renders the frames scene of tests/first_nested_worker.py, with a light of its own, on whatever
library YRT_LIB names and stores what came out, for tests/test_gpu_any_nested.py (which starts
it as a fresh child process, one library at a time; not a test module itself).

    YRT_LIB=yocto_raytracing_amd/variants/libyrt_flatany.so python tests/any_nested_worker.py out.npz scene.yrtscene

The scene is first_nested_worker.build_scene's (`basic` plus sixteen rows of six instances whose
frames are the identity, rotated about y, and the identity with -0.0 entries; row 1 instances a
line shape and a point shape) plus one emissive point instance, made here, in front of and above
the first two rows on the camera's side: the shadow rays of what the view camera sees behind and
below those rows -- the floor, the rows further back -- cross them, so the any-hit walk enters all
three kinds of frame and reaches line and point leaves, and the rows' own back faces are culled
(their light term is zero). With the tile lists forced on, level 0's shadow rays run on the
persistent any-hit grid at any frame size. out.npz holds the float32 frames at 37 x 24, 2 x 2 and 8 x 8 spp ("s2.img", "s8.img") and in
"meta" (JSON) each frame's last_stats(), tile_lists() and per-phase launch counts (of a second,
timing=1 render, which must give the same bits), the added instances by kind of frame, the two
shapes, the light's instance and position and the view camera. The scene is saved to the second
argument for the test's CPU-side reading of the shadow rays (tests/helpers.py Oracle).

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

LIGHT_POS = (0.4, 4.5, 5.0)  # in front of rows 0 and 1 (z -1.5 .. -0.5, y 0.6 .. 2.1), above the camera


def main(argv):
    out_path, scene_path = argv
    import yocto_raytracing_amd as yrt
    from yocto_raytracing_amd import _native as N

    if yrt.device_count() < 1:
        raise RuntimeError("no GPU visible")
    s, added, view, cam, shapes = build_scene(yrt)
    glow = s.add_material(ke=(30.0, 30.0, 30.0))
    bulb = s.add_shape(np.zeros((1, 3), np.float32), radius=np.full(1, 0.001), points=np.arange(1))
    light = s.add_instance(np.r_[1, 0, 0, 0, 1, 0, 0, 0, 1, LIGHT_POS].astype(np.float32), bulb, glow)
    if light not in s.lights():
        raise RuntimeError("the added point instance is not a light")
    s.save(scene_path)
    yrt.build_bvh(s)
    ds = s.upload(0)
    ds.set_tile_lists("on")
    arrays = {}
    meta = {"library": str(N.LIB_PATH), "instances": added, "shapes": shapes, "frames": {}, "light": light,
            "light_pos": list(LIGHT_POS), "camera": view, "nlights": len(s.lights())}
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
