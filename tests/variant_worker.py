"""Runs a list of render and trace cases on whatever library YRT_LIB names and stores what
came out, for tests/test_gpu_variants.py (which starts it as a fresh child process, one
library at a time; not a test module itself).

    YRT_LIB=yocto_raytracing_amd/variants/libyrt_masks.so python tests/variant_worker.py cases.json out.npz

cases.json is a list of
    {"id", "kind": "render", "scene", "samples", "max_depth", "lists", "algorithm", "count_work"}
    {"id", "kind": "trace", "scene", "rays": <file under tests/golden>}
with "resolution" and "width" per render case. out.npz holds, per render case, the float32
frame ("<id>.img") and in "meta" (JSON) its last_stats(), tile_lists() and the per-phase
launch counts of a second, timing=1 render of the same frame (which must give the same
bits); per trace case the intersect_first records and the intersect_any flags. Only
tests/golden and the package are read.
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main(argv):
    cases_path, out_path = argv
    cases = json.loads(Path(cases_path).read_text())
    import yocto_raytracing_amd as yrt
    from yocto_raytracing_amd import _native as N

    if yrt.device_count() < 1:
        raise RuntimeError("no GPU visible")
    scenes = {}

    def dev_scene(name):
        if name not in scenes:
            s = yrt.load_scene(str(GOLDEN / "scenes" / f"{name}.yrtscene"))
            yrt.build_bvh(s)
            scenes[name] = (s, s.upload(0))
        return scenes[name][1]

    arrays, meta = {}, {"library": str(N.LIB_PATH), "cases": {}}
    for c in cases:
        ds = dev_scene(c["scene"])
        if c["kind"] == "trace":
            rays = np.load(GOLDEN / c["rays"])["rays"]
            first = yrt.intersect_first(ds, rays)
            for k, v in first.items():
                arrays[f"{c['id']}.first.{k}"] = v
            arrays[f"{c['id']}.any"] = yrt.intersect_any(ds, rays)
            meta["cases"][c["id"]] = {}
            continue
        ds.set_tile_lists(c["lists"])
        kw = dict(width=c["width"], max_depth=c["max_depth"], count_work=c["count_work"], algorithm=c["algorithm"])
        img, stats = yrt.raytrace(ds, (0.1, 0.1, 0.1), c["resolution"], c["samples"], return_stats=True, **kw)
        lists = ds.tile_lists()
        timed = np.zeros_like(img)
        ds.render_into(yrt.render_params(0.1, c["resolution"], c["samples"], timing=1, **kw), timed.ctypes.data,
                       device_memory=False)
        launches = {phase: n for phase, (_, n) in ds.last_timings().items()}
        if not np.array_equal(img.view(np.uint32), timed.view(np.uint32)):
            raise RuntimeError(f"{c['id']}: the timing=1 render differs from the plain one")
        ds.set_tile_lists("auto")
        arrays[f"{c['id']}.img"] = img
        meta["cases"][c["id"]] = {"stats": stats, "tile_lists": lists, "launches": launches}
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
