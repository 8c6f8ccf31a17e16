"""GPU time of the ambient occlusion pass:

    python tools/time_ao.py [--scene instance10000] [--resolution 1080] [--samples 1,2]
                            [--rays 4,16,64] [--distance inf,1.0] [--runs 3] [--out FILE]

Times yrt_render_ao into a device plane for every combination of --samples (per axis), --rays (K)
and --distance: stream events around `--calls` calls after `--warmup` calls, `--runs` times over,
and reports the median ms per call with the runs' minimum and maximum and the occlusion rays per
second. Per --samples it also times yrt_render_aovs with the depth plane alone, the cost of the
pass's camera half (the same walk and the same tile geometry). Prints one JSON line per timing;
--out also writes them to a file. Needs the GPU: without one it fails.
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
    ap.add_argument("--samples", default="1,2", help="comma-separated samples per axis [1,2]")
    ap.add_argument("--rays", default="4,16,64", help="comma-separated K [4,16,64]")
    ap.add_argument("--distance", default="inf,1.0", help="comma-separated distances [inf,1.0]")
    ap.add_argument("--bias", type=float, default=0.01)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import yocto_raytracing_amd as yrt

    if yrt.device_count() < 1:
        raise SystemExit("time_ao: no GPU visible")
    torch.cuda.set_device(0)
    scn = yrt.load_scene(str(ROOT / "tests" / "golden" / "scenes" / f"{a.scene}.yrtscene"))
    yrt.build_bvh(scn)
    ds = scn.upload(0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = []

    def timed(call):
        """median, min and max over the runs of the ms per call"""
        ms = []
        for _ in range(a.runs):
            for _ in range(a.warmup):
                call()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                call()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1) / a.calls)
        return statistics.median(ms), min(ms), max(ms)

    def emit(res):
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)

    for s in (int(v) for v in a.samples.split(",")):
        p = yrt.render_params(resolution=a.resolution, samples=s)
        W, H = ds.image_size(p)
        plane = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        base = {"scene": a.scene, "width": W, "height": H, "samples_per_axis": s, "calls": a.calls, "warmup": a.warmup,
                "runs": a.runs}
        med, lo, hi = timed(lambda: ds.render_aovs_into(p, {"depth": plane.data_ptr()}, device_memory=True, stream=stream))
        camera_ms = med
        emit(dict(base, what="aov_depth", ms_per_call=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                  camera_samples=ds.last_stats()["camera_samples"]))
        for K in (int(v) for v in a.rays.split(",")):
            for distance in (float(v) for v in a.distance.split(",")):
                med, lo, hi = timed(lambda: ds.render_ao_into(p, plane.data_ptr(), K, distance, a.bias, device_memory=True,
                                                              stream=stream))
                st = ds.last_stats()
                emit(dict(base, what="ao", rays=K, distance=str(distance), bias=a.bias, ms_per_call=round(med, 4),
                          ms_min=round(lo, 4), ms_max=round(hi, 4), camera_samples=st["camera_samples"],
                          occlusion_rays=st["shadow_rays"],
                          occlusion_grays_per_s=round(st["shadow_rays"] / med / 1e6, 3),
                          occlusion_grays_per_s_less_camera=round(st["shadow_rays"] / max(med - camera_ms, 1e-6) / 1e6, 3),
                          camera_share=round(camera_ms / med, 4),
                          mean_a=round(float(plane[..., 0].mean().item()), 6), mean_w=round(float(plane[..., 3].mean().item()), 6)))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
