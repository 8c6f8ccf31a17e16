// aov.hip -- the AOV pass (yrt_render_aovs): per pixel the camera hit's depth, world
// position, shading normal, texture coordinate, albedo and ids, on the beauty's sample
// grid and box filter (raytrace(), src/raytrace.cpp:228-250). A pass of its own beside
// yrt_render: it shares no kernel, workspace or state with it. render.hip includes this file at
// its end: the pass is a part of that translation unit and of its gfx950 code object (the
// library keeps one code object per device source that build.py lists).
//
// One lane owns one pixel for the whole kernel, a wave an 8 x 8 pixel tile of the window,
// a 256-thread block 16 x 16 pixels. The wave loops over the s*s sub-samples: in each
// iteration its 64 rays are the same sub-sample of 64 neighbouring pixels, walked together
// by packet_first (packet_trace.h), and every lane adds its hit's values into its own
// registers in the reference's jj-major / ii-minor order. The per-pixel sums therefore need
// no LDS, no atomics and no second pass, and are the same bits on every run.
//
// Parity contract: see trace_common.h. A miss adds nothing (the beauty's
// shade() returns zero for it), so every float AOV is premultiplied by its .w, the coverage.
#include <hip/hip_runtime.h>

#include "packet_trace.h"
#include "trace_common.h"
#include "yrt_render.h"

namespace yrt {
namespace {

constexpr int AOV_BLOCK = packet_block;  // packet_first's LDS slots are sized for it
constexpr int AOV_TILE = 8;              // a wave's tile: lane = 8 * row + column
constexpr int AOV_BLOCK_TILES = 2;       // a block's 2 x 2 waves
static_assert(AOV_TILE * AOV_TILE == 64 && AOV_BLOCK_TILES * AOV_BLOCK_TILES * 64 == AOV_BLOCK, "one wave per tile");

constexpr unsigned aov_bit(int aov) { return 1u << aov; }
constexpr unsigned AOV_NEEDS_SURFACE = aov_bit(aov_position) | aov_bit(aov_normal) | aov_bit(aov_texcoord) | aov_bit(aov_albedo);

__device__ __forceinline__ void store_plane(void* plane, size_t at, vec3f v, float w) {
    reinterpret_cast<float4*>(plane)[at] = make_float4(v.x, v.y, v.z, w);
}

// `mask` (the requested AOVs) is a kernel argument, the same in every lane: every branch on
// it is a scalar branch, and the stores of an absent plane are never issued.
__global__ __launch_bounds__(AOV_BLOCK) void k_aov(dev_scene_view S, dev_render_args A, unsigned mask,
                                                   dev_aov_planes O, unsigned long long* counters) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lx = (blockIdx.x * AOV_BLOCK_TILES + (wave % AOV_BLOCK_TILES)) * AOV_TILE + (lane % AOV_TILE);
    const int ly = (blockIdx.y * AOV_BLOCK_TILES + (wave / AOV_BLOCK_TILES)) * AOV_TILE + (lane / AOV_TILE);
    const bool in_window = lx < A.tile_w && ly < A.tile_h;
    // this lane's image row under the band interleave (any band height: a tile may span bands)
    const int i = A.x0 + lx;
    const int b = ly / A.band, r = ly % A.band;
    const int j = A.y0 + (b * A.band_stride + A.band_offset) * A.band + r;
    // local rows past the image edge (the last partial band of a shard) read as zeros, as in yrt_render
    const bool valid = in_window && i < A.width && j < A.height;
    if (!__ballot(in_window)) return;  // a tile outside the window: nothing to trace or write

    const int ns = A.samples;
    float depth = 0.0f, cover = 0.0f;
    vec3f pos = {0, 0, 0}, nrm = {0, 0, 0}, alb = {0, 0, 0};
    vec2f tuv = {0, 0};
    int id_inst = -1, id_ei = -1, id_mat = -1, id_shape = -1;
    if (__ballot(valid)) {
        for (int jj = 0; jj < ns; jj++) {
            for (int ii = 0; ii < ns; ii++) {
                // every lane reaches the walk; lanes without a pixel pass valid = false
                ray3 ray = {{0, 0, 0}, {0, 0, 1}, 0, 0};
                if (valid) ray = camera_ray(A.cam, A.width, A.height, ns, i, j, ii, jj);
                hit_record hr = {-1, -1, {0, 0, 0, 0}, 0};
                work_counts wc;
                const bool h = packet_first<false>(S, ray, valid, hr, wc);
                if (!(valid && h)) continue;
                cover += 1.0f;
                depth += hr.dist;
                if ((mask & aov_bit(aov_ids)) && jj == 0 && ii == 0) {
                    const f4* ti = S.tinst + 4 * hr.slot;
                    id_inst = S.tinst_id[hr.slot];
                    id_ei = hr.ei;
                    id_mat = (int)((uint32_t)ibits(ti[2].w) & mat_index_mask);
                    id_shape = ibits(ti[0].w) & (int)inst_shape_mask;
                }
                if (mask & AOV_NEEDS_SURFACE) {
                    const surface sf = eval_surface(S, hr.slot, hr.ei, hr.ew);
                    pos = pos + sf.p;
                    nrm = nrm + sf.n;
                    tuv = tuv + sf.uv;
                    if (mask & aov_bit(aov_albedo)) {
                        // kd of shade() (raytrace.cpp:150-154)
                        const float4 m0 = ld4(S.mats + 4 * sf.mat), m1 = ld4(S.mats + 4 * sf.mat + 1);
                        vec3f kd = xyz(m0);
                        const int kd_txt = ibits(m1.w);
                        if (kd_txt >= 0) kd = kd * eval_texture<false>(S, kd_txt, sf.uv, wc, S.srgb);
                        alb = alb + kd;
                    }
                }
            }
        }
    }
    if (in_window) {
        const size_t at = (size_t)ly * A.out_stride + lx;
        const float d = float(ns * ns);
        const float w = cover / d;
        if (mask & aov_bit(aov_depth)) store_plane(O.plane[aov_depth], at, {depth / d, 0.0f, 0.0f}, w);
        if (mask & aov_bit(aov_position)) store_plane(O.plane[aov_position], at, pos / d, w);
        if (mask & aov_bit(aov_normal)) store_plane(O.plane[aov_normal], at, nrm / d, w);
        if (mask & aov_bit(aov_texcoord)) store_plane(O.plane[aov_texcoord], at, {tuv.x / d, tuv.y / d, 0.0f}, w);
        if (mask & aov_bit(aov_albedo)) store_plane(O.plane[aov_albedo], at, alb / d, w);
        if (mask & aov_bit(aov_ids))
            reinterpret_cast<int4*>(O.plane[aov_ids])[at] = make_int4(id_inst, id_ei, id_mat, id_shape);
    }
    // rays == camera samples: one wave sum, added to the two neighbouring counters of the
    // wave's line by its lanes 0 and 1 (one atomic instruction per wave)
    static_assert(cnt_rays == 0 && cnt_samples == 1, "lanes 0 and 1 add to the line's first two counters");
    const unsigned long long s = wave_sum(valid ? (unsigned long long)(ns * ns) : 0ull);
    if (lane < 2 && s) atomicAdd(counter_line(counters) + lane, s);
}

}  // namespace

hipError_t launch_aovs(const device_scene& ds, const dev_render_args& args, unsigned mask, const dev_aov_planes& out,
                       unsigned long long* counters, hipStream_t stream) {
    if (args.tile_w <= 0 || args.tile_h <= 0) return hipSuccess;
    constexpr int side = AOV_TILE * AOV_BLOCK_TILES;
    dim3 grid((args.tile_w + side - 1) / side, (args.tile_h + side - 1) / side);
    hipLaunchKernelGGL(k_aov, grid, dim3(AOV_BLOCK), 0, stream, ds.view, args, mask, out, counters);
    return hipGetLastError();
}

}  // namespace yrt
