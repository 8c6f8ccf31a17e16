"""GPU time of yrt_render_adaptive next to yrt_render of the same frame in the same process, per
phase, with the flagged share and the image quality: what adaptive supersampling saves.

    python tools/time_adaptive.py [--config c3|c4] [--scene S --resolution R --samples N --max-depth D]
                                  [--thresholds 0.05,0.1,0.25] [--base-samples 1] [--chunk-pixels 0] [--calls 10]
                                  [--warmup 2] [--out-dir DIR]

c3 is refl at 1920 x 1080, 4 x 4 samples, depth 8; c4 is instance10000 at 1920 x 1080, 8 x 8
samples (bench.py's flagship frame). Only the calls are timed, on device buffers and one stream:
the medians over `--calls` calls after `--warmup` of the per-phase GPU ms of yrt_last_timings
(timing = 1) and their sum, and of the wall time of a call up to its stream's end (the adaptive
call waits once, for the flagged count, which no phase shows). Per threshold: the flagged share,
the ratio to the full render, the prediction 1 / (s*s / (b*b)) + share * 1.43 (a
ray batch costs 1.43 x the render per ray at c4), and the 8-bit PSNR (tests/helpers.py
tonemap_ref, psnr_u8) of the adaptive frame and of the base frame against the full render.
Prints one JSON line per threshold; --out-dir also writes each to
DIR/time_adaptive_<scene>_t<threshold>.json. Needs the GPU.
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
sys.path.insert(0, str(ROOT / "tests"))

CONFIGS = {"c3": ("refl", 1080, 4, 8), "c4": ("instance10000", 1080, 8, 16)}
BATCH_COST_PER_RAY = 1.43  # DESIGN.md §5 "Ray batches": yrt_shade_rays / yrt_render per ray at c4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS))
    ap.add_argument("--scene", default="instance10000")
    ap.add_argument("--resolution", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--max-depth", type=int, default=16)
    ap.add_argument("--thresholds", default="0.05,0.1,0.25")
    ap.add_argument("--base-samples", type=int, default=1)
    ap.add_argument("--chunk-pixels", type=int, default=0, help="refined pixels per batch (0: the library's choice)")
    ap.add_argument("--algorithm", default="wavefront")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out-dir")
    a = ap.parse_args()
    if a.config:
        a.scene, a.resolution, a.samples, a.max_depth = CONFIGS[a.config]
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_adaptive: no GPU visible")
    torch.cuda.set_device(0)
    import yocto_raytracing_amd as yrt
    from helpers import psnr_u8, tonemap_ref

    scn = yrt.load_scene(str(ROOT / "tests" / "golden" / "scenes" / f"{a.scene}.yrtscene"))
    yrt.build_bvh(scn)
    ds = scn.upload(0)
    s, b = a.samples, a.base_samples
    p = yrt.render_params(0.1, a.resolution, s, max_depth=a.max_depth, algorithm=a.algorithm, timing=1)
    pb = yrt.render_params(0.1, a.resolution, b, max_depth=a.max_depth, algorithm=a.algorithm, timing=1)
    W, H = ds.image_size(p)
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream

    def measure(call):
        phases, totals, walls = {}, [], []
        for k in range(a.warmup + a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            t = ds.last_timings()
            if k < a.warmup:
                continue
            for ph, (ms, _) in t.items():
                phases.setdefault(ph, []).append(ms)
            totals.append(sum(ms for ms, _ in t.values()))
            walls.append(wall)
        return {"ms": round(statistics.median(totals), 4), "min_ms": round(min(totals), 4),
                "max_ms": round(max(totals), 4), "wall_ms": round(statistics.median(walls), 4),
                "phases_ms": {ph: round(statistics.median(v), 4) for ph, v in phases.items()}}

    common = {"scene": a.scene, "width": W, "height": H, "samples_per_axis": s, "base_samples_per_axis": b,
              "max_depth": a.max_depth, "algorithm": a.algorithm, "chunk_pixels": a.chunk_pixels, "calls": a.calls,
              "warmup": a.warmup}
    full = measure(lambda: ds.render_into(p, frame.data_ptr(), stream=stream))
    full["stats"] = {k: v for k, v in ds.last_stats().items() if v}
    full_u8 = tonemap_ref(frame.cpu().numpy())
    base = measure(lambda: ds.render_into(pb, frame.data_ptr(), stream=stream))
    base_psnr = psnr_u8(tonemap_ref(frame.cpu().numpy()), full_u8)
    for text in a.thresholds.split(","):
        thr = float(text)
        res = dict(common, threshold=thr, render=full, base_render=base)
        res["adaptive"] = measure(lambda: ds.render_adaptive_into(p, frame.data_ptr(), thr, b,
                                                                  refined_ptr=mask.data_ptr(),
                                                                  chunk_pixels=a.chunk_pixels, stream=stream))
        res["adaptive"]["stats"] = {k: v for k, v in ds.last_stats().items() if v}
        flagged = ds.adaptive_refined()
        assert flagged == int(mask.sum().item())
        share = flagged / (W * H)
        res["flagged_pixels"], res["flagged_share"] = flagged, round(share, 4)
        res["ratio"] = round(res["adaptive"]["ms"] / full["ms"], 4)
        res["wall_ratio"] = round(res["adaptive"]["wall_ms"] / full["wall_ms"], 4)
        res["predicted_ratio"] = round(b * b / (s * s) + share * BATCH_COST_PER_RAY, 4)
        phases = set(res["adaptive"]["phases_ms"]) | set(full["phases_ms"])
        res["phase_difference_ms"] = {ph: round(res["adaptive"]["phases_ms"].get(ph, 0.0) -
                                                full["phases_ms"].get(ph, 0.0), 4) for ph in sorted(phases)}
        # (identical 8-bit frames have no finite PSNR: null)
        psnr = psnr_u8(tonemap_ref(frame.cpu().numpy()), full_u8)
        res["psnr_u8_adaptive_vs_full"] = round(psnr, 2) if psnr != float("inf") else None
        res["psnr_u8_base_vs_full"] = round(base_psnr, 2) if base_psnr != float("inf") else None
        line = json.dumps(res)
        print(line)
        if a.out_dir:
            Path(a.out_dir).mkdir(parents=True, exist_ok=True)
            (Path(a.out_dir) / f"time_adaptive_{a.scene}_t{text.strip()}.json").write_text(line + "\n")


if __name__ == "__main__":
    main()
