"""GPU time of the AOV pass next to the same build's closest-hit work in yrt_render:

    python tools/time_aovs.py [--scene instance10000] [--resolution 1080] [--samples 8]
                              [--aovs depth,ids] [--out FILE]

Times yrt_render_aovs with all six AOVs (or --aovs) into device planes (stream events around
`--calls` calls after `--warmup` calls) and, on the same frame, yrt_render's camera-ray phases
(YRT_PHASE_PRIMARY + YRT_PHASE_LISTS of yrt_last_timings, averaged over the same number of
renders). Prints one JSON line; --out also writes it to a file. Needs the GPU: without one it
fails.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="instance10000")
    ap.add_argument("--resolution", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--aovs", help="comma-separated AOV names [all six]")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import yocto_raytracing_amd as yrt
    from yocto_raytracing_amd import _native as N

    if yrt.device_count() < 1:
        raise SystemExit("time_aovs: no GPU visible")
    torch.cuda.set_device(0)
    scn = yrt.load_scene(str(ROOT / "tests" / "golden" / "scenes" / f"{a.scene}.yrtscene"))
    yrt.build_bvh(scn)
    ds = scn.upload(0)
    p = yrt.render_params(resolution=a.resolution, samples=a.samples)
    W, H = ds.image_size(p)
    names = a.aovs.split(",") if a.aovs else list(N.AOVS)
    planes = {n: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for n in names}
    ptrs = {n: t.data_ptr() for n, t in planes.items()}
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        ds.render_aovs_into(p, ptrs, device_memory=True, stream=stream)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.calls):
        ds.render_aovs_into(p, ptrs, device_memory=True, stream=stream)
    t1.record()
    torch.cuda.synchronize()
    aov_ms = t0.elapsed_time(t1) / a.calls
    stats = ds.last_stats()
    hit_share = None if names[0] == "ids" else float(planes[names[0]][..., 3].mean().item())

    # the yardstick: the beauty render's camera rays on the same frame
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    pt = yrt.render_params(resolution=a.resolution, samples=a.samples, timing=1)
    torch.cuda.synchronize()
    primary = lists = total = 0.0
    for k in range(a.warmup + a.calls):
        ds.render_into(pt, frame.data_ptr(), device_memory=True, stream=stream)
        t = ds.last_timings()
        if k >= a.warmup:
            primary += t.get("primary", (0.0, 0))[0]
            lists += t.get("lists", (0.0, 0))[0]
            total += sum(ms for ms, _ in t.values())
    primary, lists, total = primary / a.calls, lists / a.calls, total / a.calls
    res = {"scene": a.scene, "width": W, "height": H, "samples_per_axis": a.samples, "calls": a.calls,
           "warmup": a.warmup, "aovs": names, "aov_ms_per_call": round(aov_ms, 4),
           "aov_rays": stats["rays"], "aov_grays_per_s": round(stats["rays"] / aov_ms / 1e6, 3),
           "coverage_mean": hit_share,
           "render_primary_ms": round(primary, 4), "render_lists_ms": round(lists, 4),
           "render_primary_plus_lists_ms": round(primary + lists, 4), "render_all_phases_ms": round(total, 4),
           "aov_over_primary_plus_lists": round(aov_ms / (primary + lists), 4),
           "tile_lists": ds.tile_lists()["camera"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
