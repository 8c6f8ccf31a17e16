"""GPU time of yrt_render_passes next to the same build's yrt_render, per phase:

    python tools/time_passes.py [--scene instance10000] [--resolution 1080] [--samples 8]
                                [--max-depth 16] [--passes reflection] [--lib LIB.so] [--out FILE]

Renders the frame into device planes on one stream and reports, as medians over `--calls`
calls after `--warmup` calls, the per-phase GPU ms of yrt_last_timings (timing = 1) and their
sum for yrt_render, for yrt_render_passes with all five passes and the beauty, and for
yrt_render_passes with `--passes` alone and no beauty; the passes' sums over yrt_render's; the
sha256 of yrt_render's frame (profiles/frame_digests.json), of the six planes of the call with
all passes (passes_sha256: the five passes and the beauty) and whether that beauty has the
frame's bits. --lib times another build of the library (tools/build_rev.py); one that has no
yrt_render_passes gives the yrt_render part alone. Prints one JSON line; --out also writes it
to a file. Needs the GPU: without one it fails.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def bind(path):
    from yocto_raytracing_amd import _native as N  # struct layouts only

    lib = C.CDLL(str(path), mode=os.RTLD_LOCAL)
    vp = C.c_void_p
    lib.yrt_scene_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.yrt_host_scene_build_bvh.argtypes = [vp, C.c_int]
    lib.yrt_scene_upload.argtypes = [vp, C.c_int, C.POINTER(vp)]
    lib.yrt_render_params_default.argtypes = [C.POINTER(N.RenderParams)]
    lib.yrt_image_size.argtypes = [vp, C.POINTER(N.RenderParams), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.yrt_render.argtypes = [vp, C.POINTER(N.RenderParams), vp, C.c_int, vp]
    lib.yrt_last_timings.argtypes = [vp, C.POINTER(N.Timings)]
    lib.yrt_last_error.restype = C.c_char_p
    if hasattr(lib, "yrt_render_passes"):
        lib.yrt_render_passes.argtypes = [vp, C.POINTER(N.RenderParams), C.c_uint, C.POINTER(N.PassPlanes), vp, C.c_int, vp]
    return lib, N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="instance10000")
    ap.add_argument("--resolution", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--max-depth", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--passes", default="reflection", help="comma-separated passes of the second, partial call")
    ap.add_argument("--lib", default=str(ROOT / "yocto_raytracing_amd" / "libyrt.so"))
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_passes: no GPU visible")
    torch.cuda.set_device(0)
    lib, N = bind(a.lib)
    hs, ds = C.c_void_p(), C.c_void_p()
    scene = str(ROOT / "tests" / "golden" / "scenes" / f"{a.scene}.yrtscene").encode()
    assert lib.yrt_scene_load(scene, C.byref(hs)) == 0, lib.yrt_last_error()
    assert lib.yrt_host_scene_build_bvh(hs, 0) == 0, lib.yrt_last_error()
    assert lib.yrt_scene_upload(hs, 0, C.byref(ds)) == 0, lib.yrt_last_error()
    p = N.RenderParams()
    lib.yrt_render_params_default(C.byref(p))
    p.resolution, p.samples, p.max_depth, p.timing = a.resolution, a.samples, a.max_depth, 1
    w, h = C.c_int(), C.c_int()
    assert lib.yrt_image_size(ds, C.byref(p), C.byref(w), C.byref(h)) == 0
    W, H = w.value, h.value
    stream = torch.cuda.current_stream().cuda_stream
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    planes = {n: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for n in N.PASSES}
    torch.cuda.synchronize()

    def measure(call):
        phases, totals = {}, []
        for k in range(a.warmup + a.calls):
            assert call() == 0, lib.yrt_last_error()
            t = N.Timings()
            assert lib.yrt_last_timings(ds, C.byref(t)) == 0  # (synchronises)
            if k < a.warmup:
                continue
            for q, ph in enumerate(N.PHASES):
                if t.launches[q]:
                    phases.setdefault(ph, []).append(t.ms[q])
            totals.append(sum(t.ms[q] for q in range(len(N.PHASES)) if t.launches[q]))
        return {"ms": round(statistics.median(totals), 4), "min_ms": round(min(totals), 4),
                "max_ms": round(max(totals), 4),
                "phases_ms": {ph: round(statistics.median(v), 4) for ph, v in phases.items()}}

    def digest(t):
        torch.cuda.synchronize()
        return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()

    res = {"scene": a.scene, "width": W, "height": H, "samples_per_axis": a.samples, "max_depth": a.max_depth,
           "calls": a.calls, "warmup": a.warmup, "library": Path(a.lib).name}
    res["render"] = measure(lambda: lib.yrt_render(ds, C.byref(p), C.c_void_p(frame.data_ptr()), 1, C.c_void_p(stream)))
    res["frame_sha256"] = digest(frame)
    if hasattr(lib, "yrt_render_passes"):
        def passes_call(names, beauty):
            pp, mask = N.PassPlanes(), 0
            for n in names:
                pp.plane[N.PASSES[n]] = planes[n].data_ptr()
                mask |= 1 << N.PASSES[n]
            return lambda: lib.yrt_render_passes(ds, C.byref(p), mask, C.byref(pp),
                                                 C.c_void_p(beauty.data_ptr() if beauty is not None else 0), 1,
                                                 C.c_void_p(stream))

        beauty = torch.zeros_like(frame)
        res["passes_all"] = measure(passes_call(list(N.PASSES), beauty))
        res["passes_all"]["over_render"] = round(res["passes_all"]["ms"] / res["render"]["ms"], 4)
        res["passes_sha256"] = dict({n: digest(planes[n]) for n in N.PASSES}, beauty=digest(beauty))
        res["passes_beauty_same_bits"] = res["passes_sha256"]["beauty"] == res["frame_sha256"]
        names = a.passes.split(",")
        res["passes_partial"] = dict(measure(passes_call(names, None)), passes=names)
        res["passes_partial"]["over_render"] = round(res["passes_partial"]["ms"] / res["render"]["ms"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
