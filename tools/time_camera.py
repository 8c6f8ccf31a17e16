"""GPU time of yrt_render_camera next to yrt_render of the same frame in the same process, per
phase: what the camera models cost, and what they save over building the rays on the host.

    python tools/time_camera.py [--scene S --resolution R --samples N --max-depth D] [--calls 10] [--warmup 2]
                                [--host-calls 2] [--out-dir DIR]

The default is bench.py's flagship frame: instance10000 at 1920 x 1080, 8 x 8 samples. Timed, on
device buffers and one stream, alternating over the variants in every round so that they share
the machine's state: the medians over `--calls` rounds after `--warmup` of the per-phase GPU ms
of yrt_last_timings (timing = 1) and their sum, and of the wall time of a call up to its
stream's end, for
  render          yrt_render
  pinhole         yrt_render_camera, perspective, aperture 0: the same image, so the difference
                  is the cost of the batch route (rays written and read back, colours summed)
  lens            perspective, aperture 0.05 x the camera's focus
  orthographic
  equirect        at 2 * resolution x resolution
and, `--host-calls` times (0 skips it), the route this replaces:
  host_rays       yrt.shade_rays on the frame's rays in host memory (32 B up and 16 B down per
                  ray; the rays come from yrt.camera_rays once, outside the timed part, and the
                  box filter on the host is not timed either): wall time only.
Prints one JSON line per variant with its ratio to `render`; --out-dir also writes each to
DIR/time_camera_<scene>_<variant>.json. Needs the GPU.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="instance10000")
    ap.add_argument("--resolution", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--max-depth", type=int, default=16)
    ap.add_argument("--chunk-pixels", type=int, default=0, help="pixels per batch (0: the library's choice)")
    ap.add_argument("--algorithm", default="wavefront")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--out-dir")
    a = ap.parse_args()
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_camera: no GPU visible")
    torch.cuda.set_device(0)
    import yocto_raytracing_amd as yrt

    scn = yrt.load_scene(str(ROOT / "tests" / "golden" / "scenes" / f"{a.scene}.yrtscene"))
    yrt.build_bvh(scn)
    ds = scn.upload(0)
    s = a.samples
    focus = scn.camera(0)["focus"]
    p = yrt.render_params(0.1, a.resolution, s, max_depth=a.max_depth, algorithm=a.algorithm, timing=1)
    pp = yrt.render_params(0.1, a.resolution, s, width=2 * a.resolution, max_depth=a.max_depth, algorithm=a.algorithm,
                           timing=1)
    W, H = ds.image_size(p)
    frame = torch.zeros((H, max(W, 2 * H), 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    out = frame.data_ptr()
    cam = dict(chunk_pixels=a.chunk_pixels, stream=stream)
    variants = {
        "render": (W, lambda: ds.render_into(p, out, stream=stream)),
        "pinhole": (W, lambda: ds.render_camera_into(p, out, "perspective", aperture=0.0, **cam)),
        "lens": (W, lambda: ds.render_camera_into(p, out, "perspective", aperture=0.05 * focus, **cam)),
        "orthographic": (W, lambda: ds.render_camera_into(p, out, "orthographic", **cam)),
        "equirect": (2 * H, lambda: ds.render_camera_into(pp, out, "equirect", **cam)),
    }
    rec = {v: {"phases": {}, "totals": [], "walls": []} for v in variants}
    images = {}
    for k in range(a.warmup + a.calls):
        for v, (width, call) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            t = ds.last_timings()
            if k == 0:
                rec[v]["stats"] = {n: c for n, c in ds.last_stats().items() if c}
                if v in ("render", "pinhole"):
                    images[v] = frame.view(-1, 4)[:H * width].cpu().numpy().copy()
            if k < a.warmup:
                continue
            for ph, (ms, _) in t.items():
                rec[v]["phases"].setdefault(ph, []).append(ms)
            rec[v]["totals"].append(sum(ms for ms, _ in t.values()))
            rec[v]["walls"].append(wall)
    assert np.array_equal(images["render"].view(np.uint32), images["pinhole"].view(np.uint32)), "the pinhole is not yrt_render's image"
    common = {"scene": a.scene, "height": H, "samples_per_axis": s, "max_depth": a.max_depth, "algorithm": a.algorithm,
              "chunk_pixels": a.chunk_pixels, "calls": a.calls, "warmup": a.warmup}
    results = {}
    for v, r in rec.items():
        results[v] = dict(common, variant=v, width=variants[v][0], ms=round(statistics.median(r["totals"]), 4),
                          min_ms=round(min(r["totals"]), 4), max_ms=round(max(r["totals"]), 4),
                          wall_ms=round(statistics.median(r["walls"]), 4), min_wall_ms=round(min(r["walls"]), 4),
                          phases_ms={ph: round(statistics.median(x), 4) for ph, x in r["phases"].items()}, stats=r["stats"])
    if a.host_calls > 0:
        rays = yrt.camera_rays(ds, a.resolution, s, aperture=0.0)  # the pinhole's rays, in host memory
        walls = []
        for k in range(a.host_calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            colours = yrt.shade_rays(ds, rays, 0.1, max_depth=a.max_depth, algorithm=a.algorithm)
            walls.append((time.perf_counter() - t0) * 1e3)
        results["host_rays"] = dict(common, variant="host_rays", width=W, calls=a.host_calls, warmup=0, rays=int(rays.shape[0]),
                                    bytes_up=int(rays.nbytes), bytes_down=int(colours.nbytes),
                                    wall_ms=round(statistics.median(walls), 4), min_wall_ms=round(min(walls), 4))
    for v, r in results.items():
        r["wall_ratio_to_render"] = round(r["wall_ms"] / results["render"]["wall_ms"], 4)
        if "ms" in r:
            r["ratio_to_render"] = round(r["ms"] / results["render"]["ms"], 4)
        line = json.dumps(r)
        print(line)
        if a.out_dir:
            Path(a.out_dir).mkdir(parents=True, exist_ok=True)
            (Path(a.out_dir) / f"time_camera_{a.scene}_{v}.json").write_text(line + "\n")


if __name__ == "__main__":
    main()
