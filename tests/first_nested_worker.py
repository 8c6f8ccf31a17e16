"""Renders a scene whose instance frames are not all the identity on whatever library YRT_LIB
names and stores what came out, for tests/test_gpu_first_nested.py (which starts it as a fresh
child process, one library at a time; not a test module itself).

    YRT_LIB=yocto_raytracing_amd/variants/libyrt_flatwalk.so python tests/first_nested_worker.py out.npz

The scene is tests/golden's `basic` plus the six instances of
tests/test_gpu_parity.py::test_identity_rotation_instances_share_direction: frames whose rotation
is bitwise the identity (instances 5 and 8), rotated about y (6 and 9) and the identity with -0.0
entries (7 and 10: not flagged as identity, so they take the full instance entry). Eleven instances
are too few for camera lists (the instance level's wide tree needs YRT_BUNDLE_MIN_TOP records), and
without lists the primary grid runs its tree mode, which is not the code under test. So fifteen more
rows of six instances with the same three kinds of frame follow, behind and above the first, and
their shapes include a line shape and a point shape made here: the list-mode walk then meets
rotated frames, line leaves and point leaves. out.npz holds the float32 frames at 37 x 24, 2 x 2
and 8 x 8 spp, camera lists on ("s2.img", "s8.img"), from a camera added in front of the first
two rows, and in "meta" (JSON) each frame's last_stats() and tile_lists(), the added instances
by kind of frame, the two shapes, and the instances and shapes that the 8 x 8 spp frame's camera
rays hit ("hit_instances", "hit_shapes": the "ids" AOV at one pixel per sample; "ids" keeps every
eighth pixel of it).

The scene's second camera has focus 0 and therefore no extent: every ray's direction is zero, and a
wave with such a ray takes no tile list but walks the tree from its root as the list's one virtual
entry (wavefront.hip primary_samples: the only way a camera ray of a whole-tile chunk gets no
list). Those rays hit nothing (every triangle test's determinant is 0) but pass every box that
holds the origin, which lies inside the added instances' row: descents, instance entries and
leaves are all run. Its frame, 2 x 2 spp, is "nolist.img".

Only tests/golden and the package are read.
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

WIDTH, HEIGHT, SAMPLES = 37, 24, (2, 8)


ROWS = 16


def build_scene(yrt):
    s = yrt.load_scene(str(GOLDEN / "scenes" / "basic.yrtscene"))
    m = s.add_material(kd=(0.5, 0.5, 0.5))
    # a zigzag of 24 line segments and 30 points, each about one unit across
    t = np.arange(25, dtype=np.float32)
    lpos = np.stack([t / 24 - 0.5, 0.25 * (t % 2) + 0.1 * np.sin(t), 0.3 * np.cos(0.7 * t)], 1)
    lines = s.add_shape(lpos, norm=np.tile([1.0, 0.0, 0.0], (25, 1)), radius=np.full(25, 0.12),
                        lines=np.stack([np.arange(24), np.arange(1, 25)], 1))
    u = np.arange(30, dtype=np.float32)
    ppos = np.stack([0.5 * np.cos(2.4 * u) * u / 30, u / 30 - 0.3, 0.5 * np.sin(2.4 * u) * u / 30], 1)
    points = s.add_shape(ppos, norm=np.tile([0.0, 1.0, 0.0], (30, 1)), radius=np.full(30, 0.15), points=np.arange(30))
    pool = [1, 2, 3, 4, lines, points]
    c, sn = np.cos(0.7), np.sin(0.7)
    added = {"identity": [], "rotated": [], "signed_zero": []}
    for r in range(ROWS):
        for k in range(6):
            if r < 2:  # in front of the view camera: the parity test's six, and a row above them
                o = [-3.0 + 1.2 * k, 0.6 + 1.5 * r, -1.5 + 0.5 * (k % 3)]
            else:  # the rest only make the instance tree large enough for lists
                o = [-3.0 + 1.2 * k, 0.6 + 0.3 * r, -6.0 - 1.5 * r + 0.5 * (k % 3)]
            if k % 3 == 0:  # identity rotation
                fr, kind = np.r_[1, 0, 0, 0, 1, 0, 0, 0, 1, o], "identity"
            elif k % 3 == 1:  # rotated about y
                fr, kind = np.r_[c, 0, -sn, 0, 1, 0, sn, 0, c, o], "rotated"
            else:  # the identity with negative zeros: mathematically the same frame
                fr, kind = np.r_[1, -0.0, -0.0, -0.0, 1, -0.0, -0.0, -0.0, 1, o], "signed_zero"
            # (row 0: the six instances as in the parity test; row 1: lines and points)
            shape = 1 + k % 4 if r == 0 else (lines, points)[k % 2] if r == 1 else pool[(k + r) % 6]
            added[kind].append(s.add_instance(fr.astype(np.float32), shape, m))
    # the frames' camera: in front of the two rows, looking down -z
    view = s.add_camera(np.r_[1, 0, 0, 0, 1, 0, 0, 0, 1, 0.0, 1.3, 6.5].astype(np.float32), 0.62, 37 / 24, 8.0)
    # a camera with no extent among the added instances, looking down -z
    cam = s.add_camera(np.r_[1, 0, 0, 0, 1, 0, 0, 0, 1, -0.6, 0.7, -1.0].astype(np.float32), 0.8, 37 / 24, 0.0)
    return s, added, view, cam, {"lines": lines, "points": points}


def main(argv):
    (out_path,) = argv
    import yocto_raytracing_amd as yrt
    from yocto_raytracing_amd import _native as N

    if yrt.device_count() < 1:
        raise RuntimeError("no GPU visible")
    s, added, view, cam, shapes = build_scene(yrt)
    yrt.build_bvh(s)
    ds = s.upload(0)
    ds.set_tile_lists("on")
    arrays, meta = {}, {"library": str(N.LIB_PATH), "instances": added, "shapes": shapes, "frames": {}}
    for ns in SAMPLES:
        img, stats = yrt.raytrace(ds, (0.1, 0.1, 0.1), HEIGHT, ns, return_stats=True, width=WIDTH, max_depth=16,
                                  camera=view, algorithm="wavefront")
        arrays[f"s{ns}.img"] = img
        meta["frames"][f"s{ns}"] = {"stats": stats, "tile_lists": ds.tile_lists()}
    img, stats = yrt.raytrace(ds, (0.1, 0.1, 0.1), HEIGHT, 2, return_stats=True, width=WIDTH, max_depth=16,
                              camera=cam, algorithm="wavefront")
    arrays["nolist.img"] = img
    meta["frames"]["nolist"] = {"stats": stats, "tile_lists": ds.tile_lists()}
    # what the 8 x 8 spp frame's camera rays hit: one pixel of a 296 x 192 frame per sample of
    # the 37 x 24 one (the same u, v: (8 i + ii + 0.5) / 296; no lens, so the same ray)
    ids = yrt.render_aovs(ds, HEIGHT * 8, 1, aovs=("ids",), width=WIDTH * 8, camera=view)["ids"]
    meta["hit_instances"] = sorted(set(np.unique(ids[..., 0]).tolist()))
    meta["hit_shapes"] = sorted(set(np.unique(ids[..., 3]).tolist()))
    arrays["ids"] = ids[::8, ::8].copy()
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
