"""Renders the cases of tests/shadow_shade_cases.py on whatever library YRT_LIB names and stores
the frames, the counts and the launches, for tests/test_gpu_shadow_shade_fused.py (which starts
it as a fresh child process; not a test module itself).

    YRT_LIB=yocto_raytracing_amd/variants/libyrt_unfused.so python tests/shadow_shade_worker.py out.npz
"""
import json
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv):
    (out_path,) = argv
    import shadow_shade_cases as SC
    import yocto_raytracing_amd as yrt
    from yocto_raytracing_amd import _native as N

    if yrt.device_count() < 1:
        raise RuntimeError("no GPU visible")
    arrays, meta = {}, {"library": str(N.LIB_PATH), "cases": {}}
    with tempfile.TemporaryDirectory() as td:
        scenes = SC.Scenes(yrt, Path(td))
        for cid, scene, samples, band in SC.cases():
            img, stats, launches = SC.render(yrt, scenes.get(scene)[2], scene, samples, band)
            arrays[f"{cid}.img"] = img
            meta["cases"][cid] = {"stats": stats, "launches": launches}
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    main(sys.argv[1:])
