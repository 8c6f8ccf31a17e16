"""GPU time of yrt_render_light_groups next to the same build's yrt_render, per phase:

    python tools/time_light_groups.py [--scene instance10000] [--resolution 1080] [--samples 8]
                                      [--max-depth 16] [--lib LIB.so] [--out FILE]

Renders the frame into device planes on one stream and reports, as medians over `--calls`
calls after `--warmup` calls, the per-phase GPU ms of yrt_last_timings (timing = 1) and their
sum for yrt_render and for yrt_render_light_groups with one group per light (light k in group
k % 8), the ambient plane and the beauty; the groups call's sum over yrt_render's; what the
planes cost without the call, G + 1 renders, bounded from below by the same process's
yrt_render phases as (G + 1) x (lists + primary) + shadow (every render repeats the lists and
the camera rays; together they walk each shadow ray once); the sha256 of yrt_render's frame
(profiles/frame_digests.json), of every plane, and whether the call's beauty has the frame's
bits. --lib times another build of the library (tools/build_rev.py); one that has no
yrt_render_light_groups gives the yrt_render part alone. Prints one JSON line; --out also writes
it to a file. Needs the GPU: without one it fails.
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
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    lib.yrt_scene_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.yrt_host_scene_build_bvh.argtypes = [vp, C.c_int]
    lib.yrt_host_scene_info.argtypes = [vp, C.POINTER(C.c_longlong)]
    lib.yrt_scene_upload.argtypes = [vp, C.c_int, C.POINTER(vp)]
    lib.yrt_render_params_default.argtypes = [C.POINTER(N.RenderParams)]
    lib.yrt_image_size.argtypes = [vp, C.POINTER(N.RenderParams), ip, ip]
    lib.yrt_render.argtypes = [vp, C.POINTER(N.RenderParams), vp, C.c_int, vp]
    lib.yrt_last_timings.argtypes = [vp, C.POINTER(N.Timings)]
    lib.yrt_last_error.restype = C.c_char_p
    if hasattr(lib, "yrt_render_light_groups"):
        lib.yrt_render_light_groups.argtypes = [vp, C.POINTER(N.RenderParams), ip, C.c_int, C.c_int,
                                                C.POINTER(N.LightGroupPlanes), C.c_int, vp]
    return lib, N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="instance10000")
    ap.add_argument("--resolution", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--max-depth", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--lib", default=str(ROOT / "yocto_raytracing_amd" / "libyrt.so"))
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("time_light_groups: no GPU visible")
    torch.cuda.set_device(0)
    lib, N = bind(a.lib)
    hs, ds = C.c_void_p(), C.c_void_p()
    scene = str(ROOT / "tests" / "golden" / "scenes" / f"{a.scene}.yrtscene").encode()
    assert lib.yrt_scene_load(scene, C.byref(hs)) == 0, lib.yrt_last_error()
    assert lib.yrt_host_scene_build_bvh(hs, 0) == 0, lib.yrt_last_error()
    assert lib.yrt_scene_upload(hs, 0, C.byref(ds)) == 0, lib.yrt_last_error()
    info = (C.c_longlong * 12)()
    assert lib.yrt_host_scene_info(hs, info) == 0
    nlights = int(info[5])
    p = N.RenderParams()
    lib.yrt_render_params_default(C.byref(p))
    p.resolution, p.samples, p.max_depth, p.timing = a.resolution, a.samples, a.max_depth, 1
    w, h = C.c_int(), C.c_int()
    assert lib.yrt_image_size(ds, C.byref(p), C.byref(w), C.byref(h)) == 0
    W, H = w.value, h.value
    stream = torch.cuda.current_stream().cuda_stream
    frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
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
           "calls": a.calls, "warmup": a.warmup, "library": Path(a.lib).name, "lights": nlights}
    res["render"] = measure(lambda: lib.yrt_render(ds, C.byref(p), C.c_void_p(frame.data_ptr()), 1, C.c_void_p(stream)))
    res["frame_sha256"] = digest(frame)
    if hasattr(lib, "yrt_render_light_groups"):
        ngroups = max(1, min(nlights, N.YRT_LIGHT_GROUPS_MAX))
        group_of = (C.c_int * max(nlights, 1))(*[k % N.YRT_LIGHT_GROUPS_MAX for k in range(nlights)])
        planes = [torch.zeros_like(frame) for _ in range(ngroups + 2)]
        lp = N.LightGroupPlanes()
        for g in range(ngroups):
            lp.group[g] = planes[g].data_ptr()
        lp.ambient, lp.beauty = planes[-2].data_ptr(), planes[-1].data_ptr()
        torch.cuda.synchronize()
        g = measure(lambda: lib.yrt_render_light_groups(ds, C.byref(p), group_of, nlights, ngroups, C.byref(lp), 1,
                                                        C.c_void_p(stream)))
        ph = res["render"]["phases_ms"]
        g["groups"] = ngroups
        g["over_render"] = round(g["ms"] / res["render"]["ms"], 4)
        g["separate_renders_lower_bound_ms"] = round(
            (ngroups + 1) * (ph.get("lists", 0.0) + ph.get("primary", 0.0)) + ph.get("shadow", 0.0), 4)
        g["over_lower_bound"] = round(g["ms"] / g["separate_renders_lower_bound_ms"], 4)
        res["light_groups"] = g
        names = [f"group{k}" for k in range(ngroups)] + ["ambient", "beauty"]
        res["planes_sha256"] = {n: digest(t) for n, t in zip(names, planes)}
        res["beauty_same_bits"] = res["planes_sha256"]["beauty"] == res["frame_sha256"]
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
