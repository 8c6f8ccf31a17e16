// ao.hip -- the ambient occlusion pass (yrt_render_ao): per pixel the share of the
// cosine-weighted hemisphere above the camera hit that no geometry closes within a distance. A
// pass of its own beside yrt_render and yrt_render_aovs, on the beauty's sample grid
// (raytrace(), src/raytrace.cpp:228-250). render.hip includes this file after aov.hip: the pass
// is a part of that translation unit and of its gfx950 code object, and uses aov.hip's tile
// geometry.
//
// k_aov's geometry: one lane owns one pixel, a wave an 8 x 8 tile, the lane loops over the s*s
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lx = (blockIdx.x * AOV_BLOCK_TILES + (wave % AOV_BLOCK_TILES)) * AOV_TILE + (lane % AOV_TILE);
    const int ly = (blockIdx.y * AOV_BLOCK_TILES + (wave / AOV_BLOCK_TILES)) * AOV_TILE + (lane / AOV_TILE);
    const bool in_window = lx < A.tile_w && ly < A.tile_h;
    // this lane's image row under the band interleave, as in k_aov
    const int i = A.x0 + lx;
    const int b = ly / A.band, r = ly % A.band;
    const int j = A.y0 + (b * A.band_stride + A.band_offset) * A.band + r;
    // local rows past the image edge read as zeros
    const bool valid = in_window && i < A.width && j < A.height;
    if (!__ballot(in_window)) return;  // a tile outside the window: nothing to trace or write

    const int ns = A.samples;
    const int rot0 = (i & 3) | (j & 3) << 2;
    int open = 0, hits = 0, cast = 0;  // unoccluded rays (K per line or point hit), hits, triangle hits
    if (__ballot(valid)) {
        for (int jj = 0; jj < ns; jj++) {
            for (int ii = 0; ii < ns; ii++) {
                // every lane reaches the walks; lanes without a pixel pass valid = false
                ray3 ray = {{0, 0, 0}, {0, 0, 1}, 0, 0};
                if (valid) ray = camera_ray(A.cam, A.width, A.height, ns, i, j, ii, jj);
                hit_record hr = {-1, -1, {0, 0, 0, 0}, 0};
                work_counts wc;
                const bool hit = packet_first<false>(S, ray, valid, hr, wc) && valid;
                bool tri = false;
                vec3f p = {0, 0, 0}, n = {0, 0, 1}, b1 = {1, 0, 0}, b2 = {0, 1, 0};
                if (hit) {
                    hits++;
                    const surface sf = eval_surface(S, hr.slot, hr.ei, hr.ew);
                    tri = sf.kind == kind_triangles;
                    if (!tri) open += rays;  // lines and points: no hemisphere, K unoccluded rays
                    p = sf.p;
                    n = sf.n;
                    if (dot(n, ray.d) > 0.0f) n = {-n.x, -n.y, -n.z};
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
    if (in_window) {
        const float a = float(open) / float(rays * ns * ns);
        out[(size_t)ly * A.out_stride + lx] = make_float4(a, a, a, float(hits) / float(ns * ns));
    }
    // the camera samples under rays and samples (k_aov: lanes 0 and 1 of the wave's line), the
    // occlusion rays under the shadow rays: yrt_last_stats adds the two into its rays
    static_assert(cnt_rays == 0 && cnt_samples == 1, "lanes 0 and 1 add to the line's first two counters");
    const unsigned long long s = wave_sum(valid ? (unsigned long long)(ns * ns) : 0ull);
    if (lane < 2 && s) atomicAdd(counter_line(counters) + lane, s);
    const unsigned long long o = wave_sum((unsigned long long)cast) * (unsigned long long)rays;
    if (lane == 0 && o) atomicAdd(counter_line(counters) + cnt_shadow_rays, o);
}

}  // namespace

hipError_t launch_ao(const device_scene& ds, const dev_render_args& args, int rays, float bias, float distance,
                     void* out_rgba, unsigned long long* counters, hipStream_t stream) {
    if (args.tile_w <= 0 || args.tile_h <= 0) return hipSuccess;
    if (rays < 1 || rays > ao_dir_count) return hipErrorInvalidValue;
    constexpr int side = AOV_TILE * AOV_BLOCK_TILES;
    dim3 grid((args.tile_w + side - 1) / side, (args.tile_h + side - 1) / side);
    hipLaunchKernelGGL(k_ao, grid, dim3(AOV_BLOCK), 0, stream, ds.view, args, rays, bias, distance,
                       reinterpret_cast<float4*>(out_rgba), counters);
    return hipGetLastError();
}

}  // namespace yrt
