"""Shades a list of ray batches on whatever library YRT_LIB names and stores what came out, for
tests/test_gpu_shade_rays_chunks.py (which starts it as a fresh child process, one library at a
time; not a test module itself).

    YRT_LIB=yocto_raytracing_amd/variants/libyrt_chunks.so python tests/shade_rays_worker.py cases.json out.npz

cases.json is a list of {"id", "scene", "samples", "max_depth"}; the scene "built" is
tests/shade_rays_scene.py's, any other name a fixture under tests/golden/scenes; the batch is
camera 0's rays of the 37 x 24 frame at that many samples per axis. out.npz holds per case the
colours of one timing=1 yrt_shade_rays ("<id>.rgba") and in "meta" (JSON) its last_stats() and
per-phase launch counts.
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
for d in (ROOT, ROOT / "tests"):
    if str(d) not in sys.path:
        sys.path.insert(0, str(d))


def main(argv):
    cases_path, out_path = argv
    cases = json.loads(Path(cases_path).read_text())
    import passes_scene as PS
    import shade_rays_scene as SS
    import yocto_raytracing_amd as yrt
    from yocto_raytracing_amd import _native as N

    if yrt.device_count() < 1:
        raise RuntimeError("no GPU visible")
    scenes = {}

    def scene(name):
        if name not in scenes:
            if name == "built":
                s = SS.build(yrt)
                path = Path(out_path).with_name("built3.yrtscene")
                s.save(str(path))
            else:
                path = GOLDEN / "scenes" / f"{name}.yrtscene"
                s = yrt.load_scene(str(path))
            yrt.build_bvh(s)
            scenes[name] = (s, path, s.upload(0))
        return scenes[name][1:]

    arrays, meta = {}, {"library": str(N.LIB_PATH), "cases": {}}
    for c in cases:
        path, ds = scene(c["scene"])
        rays = SS.camera_rays(path, c["samples"])
        out = np.zeros((len(rays), 4), np.float32)
        p = yrt.render_params(PS.AMB, max_depth=c["max_depth"], timing=1)
        ds.shade_rays_into(p, rays.ctypes.data, len(rays), out.ctypes.data, device_memory=False)
        launches = {phase: n for phase, (_, n) in ds.last_timings().items()}
        arrays[f"{c['id']}.rgba"] = out
        meta["cases"][c["id"]] = {"stats": ds.last_stats(), "launches": launches, "rays": len(rays)}
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
