"""GPU time of yrt_render_soft_shadows next to yrt_render_camera (the pinhole: the hard batch path
the soft one is built on) of the same frame in the same process, per phase, and the any-hit rays
per second of each.

    python tools/time_soft_shadows.py [--scene S --resolution R --samples N --rays K --radius R] [--calls 5]
                                      [--warmup 2] [--out FILE]

The default is instance10000 at 1920 x 1080, 2 x 2 samples, K = 16, R = 1. Timed on device buffers
and one stream, the two variants alternating in every round: the medians over `--calls` rounds
after `--warmup` of the per-phase GPU ms of yrt_last_timings (timing = 1) and their sum, and
shadow_rays / shadow phase of each. Radius 0 is checked to give the hard image bit for bit.
Prints one JSON line; --out also writes it there. Needs the GPU.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="instance10000")
    ap.add_argument("--resolution", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--rays", type=int, default=16)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--max-depth", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_soft_shadows: no GPU visible")
    torch.cuda.set_device(0)
    import yocto_raytracing_amd as yrt

    scn = yrt.load_scene(str(ROOT / "tests" / "golden" / "scenes" / f"{a.scene}.yrtscene"))
    yrt.build_bvh(scn)
    ds = scn.upload(0)
    p = yrt.render_params(0.1, a.resolution, a.samples, max_depth=a.max_depth, timing=1)
    W, H = ds.image_size(p)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    out = frame.data_ptr()
    variants = {
        "hard": lambda: ds.render_camera_into(p, out, "perspective", aperture=0.0, stream=stream),
        "soft": lambda: ds.render_soft_shadows_into(p, out, a.radius, None, a.rays, stream=stream),
    }
    ds.render_soft_shadows_into(p, out, 0.0, None, a.rays, stream=stream)
    torch.cuda.synchronize()
    zero = frame.cpu().numpy().copy()
    rec = {v: {"phases": {}, "totals": []} for v in variants}
    for k in range(a.warmup + a.calls):
        for v, call in variants.items():
            torch.cuda.synchronize()
            call()
            torch.cuda.synchronize()
            t = ds.last_timings()
            if k == 0:
                rec[v]["stats"] = {n: c for n, c in ds.last_stats().items() if c}
                if v == "hard":
                    assert np.array_equal(frame.cpu().numpy().view(np.uint32), zero.view(np.uint32)), "radius 0 is not the hard image"
            if k < a.warmup:
                continue
            for ph, (ms, _) in t.items():
                rec[v]["phases"].setdefault(ph, []).append(ms)
            rec[v]["totals"].append(sum(ms for ms, _ in t.values()))
    res = {"scene": a.scene, "width": W, "height": H, "samples_per_axis": a.samples, "rays": a.rays, "radius": a.radius,
           "max_depth": a.max_depth, "calls": a.calls, "warmup": a.warmup}
    for v, r in rec.items():
        phases = {ph: round(statistics.median(x), 4) for ph, x in r["phases"].items()}
        res[v] = {"ms": round(statistics.median(r["totals"]), 4), "min_ms": round(min(r["totals"]), 4),
                  "max_ms": round(max(r["totals"]), 4), "phases_ms": phases, "stats": r["stats"],
                  "any_hit_grays_per_s": round(r["stats"]["shadow_rays"] / phases["shadow"] / 1e6, 3)}
    res["soft_over_hard_ms"] = round(res["soft"]["ms"] / res["hard"]["ms"], 4)
    res["per_ray_any_hit_time_soft_over_hard"] = round(res["hard"]["any_hit_grays_per_s"] / res["soft"]["any_hit_grays_per_s"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
