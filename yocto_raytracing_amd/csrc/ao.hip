// ao.hip -- the ambient occlusion pass (yrt_render_ao): per pixel the share of the
// cosine-weighted hemisphere above the camera hit that no geometry closes within a distance. A
// pass of its own beside yrt_render and yrt_render_aovs, on the beauty's sample grid
// (raytrace(), src/raytrace.cpp:228-250). render.hip includes this file after aov.hip: the pass
// is a part of that translation unit and of its gfx950 code object, and runs on aov.hip's tile
// frame (tile_pixel_of, tile_camera_sample, tile_count_camera_samples, tile_grid).
//
// The tile passes' geometry: one lane owns one pixel, a wave an 8 x 8 tile, the lane loops over the s*s
// sub-samples in the reference's order. Per sample the wave walks its 64 camera rays together
// (packet_first), evaluates the hits, and then walks K times more: iteration k carries
// direction k of every lane whose sample hit a triangle, through the any-hit walk of
// trace_packet_kernel<true>. The camera walk's state is dead during the K rays; what stays live
// across them is the hit point, the normal, the two tangents, the rotation and three counts.
//
// The contract (include/yrt.h): directions come from the two tables of
// ao_tables.h, every step is float32 without contraction, and the result per pixel is a count of
// unoccluded rays and one IEEE division: the same bits on every run and under any schedule.
#include <hip/hip_runtime.h>

#include "ao_tables.h"
#include "packet_trace.h"
#include "trace_common.h"
#include "yrt_render.h"

namespace yrt {
namespace {

__constant__ float ao_dirs[ao_dir_count * 3] = {YRT_AO_DIRS};
__constant__ float ao_rots[ao_rot_count * 2] = {YRT_AO_ROTS};

// `rays` (K), `bias` and `distance` are kernel arguments, the same in every lane: the loop over
// k is a scalar loop and dirs[k] a scalar load.
__global__ __launch_bounds__(AOV_BLOCK) void k_ao(dev_scene_view S, dev_render_args A, int rays, float bias,
                                                  float distance, float4* __restrict__ out,
                                                  unsigned long long* counters) {
    const tile_pixel P = tile_pixel_of(A);
    if (!__ballot(P.in_window)) return;  // a tile outside the window: nothing to trace or write

    const int ns = A.samples;
    const int rot0 = (P.i & 3) | (P.j & 3) << 2;
    int open = 0, hits = 0, cast = 0;  // unoccluded rays (K per line or point hit), hits, triangle hits
    if (__ballot(P.valid)) {
        for (int jj = 0; jj < ns; jj++) {
            for (int ii = 0; ii < ns; ii++) {
                // every lane reaches the K walks too, a lane without a triangle hit with tri = false
                work_counts wc;
                const tile_sample cs = tile_camera_sample(S, A, P, ii, jj, wc);
                const bool hit = cs.hit && P.valid;
                bool tri = false;
                vec3f p = {0, 0, 0}, n = {0, 0, 1}, b1 = {1, 0, 0}, b2 = {0, 1, 0};
                if (hit) {
                    hits++;
                    const surface sf = eval_surface(S, cs.hr.slot, cs.hr.ei, cs.hr.ew);
                    tri = sf.kind == kind_triangles;
                    if (!tri) open += rays;  // lines and points: no hemisphere, K unoccluded rays
                    p = sf.p;
                    n = sf.n;
                    if (dot(n, cs.ray.d) > 0.0f) n = {-n.x, -n.y, -n.z};
                    // the basis about n (Duff et al.), the sign of n.z taken so that +0 and -0 agree
                    const float sg = n.z >= 0.0f ? 1.0f : -1.0f;
                    const float a = -1.0f / (sg + n.z);
                    const float bb = n.x * n.y * a;
                    b1 = {1.0f + sg * n.x * n.x * a, sg * bb, -sg * n.x};
                    b2 = {bb, sg + n.y * n.y * a, -n.y};
                }
                if (!__ballot(tri)) continue;  // no lane of the wave casts a ray for this sample
                cast += tri ? 1 : 0;
                const int rot = rot0 ^ ((jj * ns + ii) & 15);
                const float c = ao_rots[2 * rot], sn = ao_rots[2 * rot + 1];
                for (int k = 0; k < rays; k++) {
                    const float tx = ao_dirs[3 * k], ty = ao_dirs[3 * k + 1], tz = ao_dirs[3 * k + 2];
                    const float x = c * tx - sn * ty;
                    const float y = sn * tx + c * ty;
                    const ray3 oray = {p, (b1 * x + b2 * y) + n * tz, bias, distance};
                    const bool occ = S.wide ? packet_occluded_wide2(S, oray, tri) : packet_any<false>(S, oray, tri, wc);
                    open += tri && !occ ? 1 : 0;
                }
            }
        }
    }
    if (P.in_window) {
        const float a = float(open) / float(rays * ns * ns);
        out[P.at(A)] = make_float4(a, a, a, float(hits) / float(ns * ns));
    }
    // the camera samples under rays and samples, the occlusion rays under the shadow rays:
    // yrt_last_stats adds the two into its rays
    tile_count_camera_samples(counters, P, ns);
    const unsigned long long o = wave_sum((unsigned long long)cast) * (unsigned long long)rays;
    if (P.lane == 0 && o) atomicAdd(counter_line(counters) + cnt_shadow_rays, o);
}

}  // namespace

hipError_t launch_ao(const device_scene& ds, const dev_render_args& args, int rays, float bias, float distance,
                     void* out_rgba, unsigned long long* counters, hipStream_t stream) {
    if (args.tile_w <= 0 || args.tile_h <= 0) return hipSuccess;
    if (rays < 1 || rays > ao_dir_count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ao, tile_grid(args), dim3(AOV_BLOCK), 0, stream, ds.view, args, rays, bias, distance,
                       reinterpret_cast<float4*>(out_rgba), counters);
    return hipGetLastError();
}

}  // namespace yrt
