"""Renders the light groups of a list of cases on whatever library YRT_LIB names and stores what
came out, for tests/test_gpu_light_groups_chunks.py (which starts it as a fresh child process,
one library at a time; not a test module itself).

    YRT_LIB=yocto_raytracing_amd/variants/libyrt_chunks.so python tests/light_groups_worker.py cases.json out.npz

cases.json is a list of {"id", "mirrors", "samples", "resolution", "width", "max_depth"} on
tests/light_groups_scene.py's five-light scene with its GROUP_OF. out.npz holds per case the
planes of one timing=1 yrt_render_light_groups ("<id>.group<g>", "<id>.ambient", "<id>.beauty")
and in "meta" (JSON) its last_stats() and per-phase launch counts.
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for d in (ROOT, ROOT / "tests"):
    if str(d) not in sys.path:
        sys.path.insert(0, str(d))


def main(argv):
    cases_path, out_path = argv
    cases = json.loads(Path(cases_path).read_text())
    import light_groups_scene as LS
    import passes_scene as PS
    import yocto_raytracing_amd as yrt
    from yocto_raytracing_amd import _native as N

    if yrt.device_count() < 1:
        raise RuntimeError("no GPU visible")
    scenes = {}

    def dev_scene(mirrors):
        if mirrors not in scenes:
            s = LS.build(yrt, mirrors=mirrors)
            yrt.build_bvh(s)
            scenes[mirrors] = (s, s.upload(0))
        return scenes[mirrors][1]

    arrays, meta = {}, {"library": str(N.LIB_PATH), "cases": {}}
    for c in cases:
        ds = dev_scene(c["mirrors"])
        p = yrt.render_params(PS.AMB, c["resolution"], c["samples"], width=c["width"], max_depth=c["max_depth"], timing=1)
        W, H = ds.image_size(p)
        names = [f"group{g}" for g in range(LS.NGROUPS)] + ["ambient", "beauty"]
        planes = {n: np.zeros((H, W, 4), np.float32) for n in names}
        ds.render_light_groups_into(p, LS.GROUP_OF, [planes[f"group{g}"].ctypes.data for g in range(LS.NGROUPS)],
                                    ambient_ptr=planes["ambient"].ctypes.data, beauty_ptr=planes["beauty"].ctypes.data,
                                    device_memory=False)
        launches = {phase: n for phase, (_, n) in ds.last_timings().items()}
        for n, a in planes.items():
            arrays[f"{c['id']}.{n}"] = a
        meta["cases"][c["id"]] = {"stats": ds.last_stats(), "launches": launches}
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
