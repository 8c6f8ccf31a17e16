"""Renders the shading passes of a list of cases on whatever library YRT_LIB names and stores
what came out, for tests/test_gpu_passes_chunks.py (which starts it as a fresh child process,
one library at a time; not a test module itself).

    YRT_LIB=yocto_raytracing_amd/variants/libyrt_chunks.so python tests/passes_worker.py cases.json out.npz

cases.json is a list of {"id", "scene", "samples", "resolution", "width", "max_depth"}; the
scene "built" is tests/passes_scene.py's, any other name a fixture under tests/golden/scenes.
out.npz holds per case the five planes and the beauty of one timing=1 yrt_render_passes
("<id>.<name>") and in "meta" (JSON) its last_stats() and per-phase launch counts.
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
    import yocto_raytracing_amd as yrt
    from yocto_raytracing_amd import _native as N

    if yrt.device_count() < 1:
        raise RuntimeError("no GPU visible")
    scenes = {}

    def dev_scene(name):
        if name not in scenes:
            s = PS.build(yrt) if name == "built" else yrt.load_scene(str(GOLDEN / "scenes" / f"{name}.yrtscene"))
            yrt.build_bvh(s)
            scenes[name] = (s, s.upload(0))
        return scenes[name][1]

    arrays, meta = {}, {"library": str(N.LIB_PATH), "cases": {}}
    for c in cases:
        ds = dev_scene(c["scene"])
        p = yrt.render_params(PS.AMB, c["resolution"], c["samples"], width=c["width"], max_depth=c["max_depth"], timing=1)
        W, H = ds.image_size(p)
        planes = {n: np.zeros((H, W, 4), np.float32) for n in (*N.PASSES, "beauty")}
        ds.render_passes_into(p, {n: planes[n].ctypes.data for n in N.PASSES}, beauty_ptr=planes["beauty"].ctypes.data,
                              device_memory=False)
        launches = {phase: n for phase, (_, n) in ds.last_timings().items()}
        for n, a in planes.items():
            arrays[f"{c['id']}.{n}"] = a
        meta["cases"][c["id"]] = {"stats": ds.last_stats(), "launches": launches}
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
