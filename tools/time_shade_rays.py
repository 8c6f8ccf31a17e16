"""GPU time of yrt_shade_rays on a frame's camera rays next to yrt_render of the same frame, per
phase: what leaving the camera path costs (no camera-relative records, no tile lists, no
persistent grids, 32 B of input per ray).

    python tools/time_shade_rays.py [--config c3|c4] [--scene S --resolution R --samples N --max-depth D]
                                    [--algorithm wavefront] [--calls 10] [--warmup 2] [--out FILE]

c3 is refl at 1920 x 1080, 4 x 4 samples, depth 8; c4 is instance10000 at 1920 x 1080, 8 x 8
samples (bench.py's flagship frame). The rays are camera 0's eval_camera rays (raytrace.cpp:6-37),
generated on the device with torch from the camera record of the .yrtscene file, in the order
(j, i, jj, ii): a pixel's samples are consecutive, as in the render. Only the calls are timed,
on device buffers and one stream: the medians over `--calls` calls after `--warmup` of the
per-phase GPU ms of yrt_last_timings (timing = 1) and their sum, for yrt_shade_rays and for
yrt_render with the tile lists on auto, their ratio, and the phase that carries most of the
difference. The box filter of the batch's colours is compared with the render's frame (torch's
float32 rays are not bit for bit camera_ray's, so the largest difference is reported, not
asserted). Prints one JSON line; --out also writes it to a file. Needs the GPU.
"""
from __future__ import annotations

import argparse
import gzip
import json
import math
import statistics
import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CONFIGS = {"c3": ("refl", 1080, 4, 8), "c4": ("instance10000", 1080, 8, 16)}


def camera_of(path, index=0):
    """camera `index` of a .yrtscene file (scene_io.cpp): frame x, y, z, o, then fovy, aspect,
    aperture, focus"""
    with gzip.open(path, "rb") as f:
        assert f.read(8) == b"YRTSCN1\0", path
        n, = struct.unpack("<I", f.read(4))
        assert index < n
        f.read(64 * index)
        v = struct.unpack("<16f", f.read(64))
    return {"x": v[0:3], "y": v[3:6], "z": v[6:9], "o": v[9:12], "fovy": v[12], "aspect": v[13], "focus": v[15]}


def camera_rays(torch, cam, W, H, s, rows_per_step=32):
    """(H * W * s * s, 8) float32 on the device: eval_camera with the sample positions of
    raytrace.cpp:235-238"""
    dev = "cuda:0"
    f32 = torch.float32
    rays = torch.empty((H, W, s, s, 8), dtype=f32, device=dev)
    x, y, z, o = (torch.tensor(cam[k], dtype=f32, device=dev) for k in ("x", "y", "z", "o"))
    h = 2.0 * cam["focus"] * math.tan(cam["fovy"] / 2.0)
    w = h * cam["aspect"]
    sub = (torch.arange(s, dtype=f32, device=dev) + 0.5) / s
    for j0 in range(0, H, rows_per_step):
        j1 = min(H, j0 + rows_per_step)
        jj = torch.arange(j0, j1, dtype=f32, device=dev)
        ii = torch.arange(W, dtype=f32, device=dev)
        u = (ii[None, :, None, None] + sub[None, None, None, :]) / W
        v = (jj[:, None, None, None] + sub[None, None, :, None]) / H
        u, v = torch.broadcast_tensors(u, v)
        d = ((u - 0.5) * w)[..., None] * x - ((v - 0.5) * h)[..., None] * y - cam["focus"] * z
        d = d / torch.linalg.vector_norm(d, dim=-1, keepdim=True)
        blk = rays[j0:j1]
        blk[..., 0:3] = o
        blk[..., 3:6] = d
        blk[..., 6] = 1e-4
        blk[..., 7] = torch.finfo(f32).max
    return rays.reshape(-1, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--scene", default="instance10000")
    ap.add_argument("--resolution", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--max-depth", type=int, default=16)
    ap.add_argument("--algorithm", default="wavefront")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.config:
        a.scene, a.resolution, a.samples, a.max_depth = CONFIGS[a.config]
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_shade_rays: no GPU visible")
    torch.cuda.set_device(0)
    import yocto_raytracing_amd as yrt

    path = ROOT / "tests" / "golden" / "scenes" / f"{a.scene}.yrtscene"
    scn = yrt.load_scene(str(path))
    yrt.build_bvh(scn)
    ds = scn.upload(0)
    p = yrt.render_params(0.1, a.resolution, a.samples, max_depth=a.max_depth, algorithm=a.algorithm, timing=1)
    W, H = ds.image_size(p)
    s = a.samples
    rays = camera_rays(torch, camera_of(path), W, H, s)
    n = rays.shape[0]
    colours = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    def measure(call):
        phases, totals = {}, []
        for k in range(a.warmup + a.calls):
            call()
            t = ds.last_timings()  # (synchronises)
            if k < a.warmup:
                continue
            for ph, (ms, _) in t.items():
                phases.setdefault(ph, []).append(ms)
            totals.append(sum(ms for ms, _ in t.values()))
        return {"ms": round(statistics.median(totals), 4), "min_ms": round(min(totals), 4),
                "max_ms": round(max(totals), 4),
                "phases_ms": {ph: round(statistics.median(v), 4) for ph, v in phases.items()}}

    res = {"scene": a.scene, "width": W, "height": H, "samples_per_axis": s, "max_depth": a.max_depth,
           "algorithm": a.algorithm, "rays": n, "calls": a.calls, "warmup": a.warmup}
    res["shade_rays"] = measure(lambda: ds.shade_rays_into(p, rays.data_ptr(), n, colours.data_ptr(), stream=stream))
    res["shade_rays"]["stats"] = {k: v for k, v in ds.last_stats().items() if v}
    res["render"] = measure(lambda: ds.render_into(p, frame.data_ptr(), stream=stream))
    res["render"]["stats"] = {k: v for k, v in ds.last_stats().items() if v}
    res["render"]["tile_lists"] = {k: v for k, v in ds.tile_lists().items() if k in ("camera", "bundles")}
    res["ratio"] = round(res["shade_rays"]["ms"] / res["render"]["ms"], 4)
    phases = set(res["shade_rays"]["phases_ms"]) | set(res["render"]["phases_ms"])
    res["phase_difference_ms"] = {ph: round(res["shade_rays"]["phases_ms"].get(ph, 0.0) -
                                            res["render"]["phases_ms"].get(ph, 0.0), 4) for ph in sorted(phases)}
    res["largest_difference"] = max(res["phase_difference_ms"], key=lambda ph: res["phase_difference_ms"][ph])
    # the batch's box filter against the frame (jj outer, ii inner, as raytrace.cpp:232-249)
    acc = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    c = colours.reshape(H, W, s, s, 4)
    for jj in range(s):
        for ii in range(s):
            acc = acc + c[:, :, jj, ii, :3]
    acc = acc / float(s * s)
    torch.cuda.synchronize()
    res["max_abs_difference_from_frame"] = float((acc - frame[..., :3]).abs().max().item())
    res["pixels_with_the_frames_bits"] = float((acc == frame[..., :3]).all(dim=-1).float().mean().item())
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
