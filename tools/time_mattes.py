"""GPU time of the ID-matte pass:

    python tools/time_mattes.py [--scene instance10000] [--resolution 1080] [--samples 8]
                                [--keys instance] [--ranks 4] [--out FILE]

Times yrt_render_mattes for --keys (comma-separated, of instance,material,shape) at --ranks
(4 or 8) into device planes: stream events around `--calls` calls after `--warmup` calls.
Prints one JSON line; --out also writes it to a file. tools/time_aovs.py --aovs depth,ids on
the same frame is the yardstick: the same walk with sums instead of tables. Needs the GPU:
without one it fails.
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
    ap.add_argument("--keys", default="instance", help="comma-separated matte keys [instance]")
    ap.add_argument("--ranks", type=int, default=4, choices=(4, 8))
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import yocto_raytracing_amd as yrt
    from yocto_raytracing_amd import _native as N

    keys = a.keys.split(",")
    if not keys or any(k not in N.MATTE_KEYS for k in keys):
        raise SystemExit(f"time_mattes: --keys takes names of {', '.join(N.MATTE_KEYS)}")
    if yrt.device_count() < 1:
        raise SystemExit("time_mattes: no GPU visible")
    torch.cuda.set_device(0)
    scn = yrt.load_scene(str(ROOT / "tests" / "golden" / "scenes" / f"{a.scene}.yrtscene"))
    yrt.build_bvh(scn)
    ds = scn.upload(0)
    p = yrt.render_params(resolution=a.resolution, samples=a.samples)
    W, H = ds.image_size(p)
    layers = a.ranks // 4
    planes = {k: {n: [torch.zeros((H, W, 4), dtype=torch.int32 if n == "ids" else torch.float32, device="cuda:0")
                      for _ in range(layers)] for n in ("ids", "coverage")} for k in keys}
    ptrs = {k: {n: [t.data_ptr() for t in v] for n, v in kp.items()} for k, kp in planes.items()}
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        ds.render_mattes_into(p, ptrs, layers, device_memory=True, stream=stream)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.calls):
        ds.render_mattes_into(p, ptrs, layers, device_memory=True, stream=stream)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.calls
    stats, dropped = ds.last_stats(), ds.matte_dropped()
    first = planes[keys[0]]
    res = {"scene": a.scene, "width": W, "height": H, "samples_per_axis": a.samples, "calls": a.calls,
           "warmup": a.warmup, "keys": keys, "ranks": a.ranks, "matte_ms_per_call": round(ms, 4),
           "matte_rays": stats["rays"], "matte_grays_per_s": round(stats["rays"] / ms / 1e6, 3),
           "dropped": {k: dropped[k] for k in keys},
           "coverage_mean": float(sum(t.sum(-1) for t in first["coverage"]).mean().item()),
           "ranks_used_max": int(sum((t >= 0).sum(-1) for t in first["ids"]).max().item())}
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
