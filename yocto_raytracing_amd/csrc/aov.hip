// aov.hip -- the AOV pass (yrt_render_aovs): per pixel the camera hit's depth, world
// position, shading normal, texture coordinate, albedo and ids, on the beauty's sample
// grid and box filter (raytrace(), src/raytrace.cpp:228-250). A pass of its own beside
// yrt_render: it shares no kernel, workspace or state with it. render.hip includes this file at
// its end: the pass is a part of that translation unit and of its gfx950 code object (the
// library keeps one code object per device source that build.py lists).
//
// This file also holds the frame of every tile pass (k_aov, mattes.hip k_matte, ao.hip k_ao): a
// lane's pixel, a camera sample of it, the count of the camera samples, a hit's ids and the
// launch grid of a window. A pass's kernel holds only what it makes of the hits.
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

// A lane's pixel: lane = 8 * row + column of its wave's tile, (lx, ly) in the window, (i, j) in
// the image, the row under the band interleave (any band height: a tile may span bands). Local
// rows past the image edge (the last partial band of a shard) are in the window but not valid:
// they read as zeros, as in yrt_render, and trace nothing.
struct tile_pixel {
    int lane, lx, ly, i, j;
    bool in_window, valid;
    // its place in a plane of the window's layout; a function, so that the 64-bit index is
    // formed behind the sample loop where it is used and not kept live through it
    __device__ __forceinline__ size_t at(const dev_render_args& A) const { return (size_t)ly * A.out_stride + lx; }
};

__device__ __forceinline__ tile_pixel tile_pixel_of(const dev_render_args& A) {
    tile_pixel P;
    P.lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    P.lx = (blockIdx.x * AOV_BLOCK_TILES + (wave % AOV_BLOCK_TILES)) * AOV_TILE + (P.lane % AOV_TILE);
    P.ly = (blockIdx.y * AOV_BLOCK_TILES + (wave / AOV_BLOCK_TILES)) * AOV_TILE + (P.lane / AOV_TILE);
    P.in_window = P.lx < A.tile_w && P.ly < A.tile_h;
    P.i = A.x0 + P.lx;
    const int b = P.ly / A.band, r = P.ly % A.band;
    P.j = A.y0 + (b * A.band_stride + A.band_offset) * A.band + r;
    P.valid = P.in_window && P.i < A.width && P.j < A.height;
    return P;
}

// Sub-sample (ii, jj) of the lane's pixel: the wave's 64 rays are the same sub-sample of 64
// neighbouring pixels, walked together by packet_first. Every lane reaches the walk; a lane
// without a valid pixel passes a null ray and valid = false. `hit` is the walk's own flag: a
// kernel reads it together with P.valid.
struct tile_sample {
    bool hit;
    hit_record hr;
    ray3 ray;
};

__device__ __forceinline__ tile_sample tile_camera_sample(const dev_scene_view& S, const dev_render_args& A,
                                                          const tile_pixel& P, int ii, int jj, work_counts& wc) {
    tile_sample s = {false, {-1, -1, {0, 0, 0, 0}, 0}, {{0, 0, 0}, {0, 0, 1}, 0, 0}};
    if (P.valid) s.ray = camera_ray(A.cam, A.width, A.height, A.samples, P.i, P.j, ii, jj);
    s.hit = packet_first<false>(S, s.ray, P.valid, s.hr, wc);
    return s;
}

// rays == camera samples: one wave sum, added to the two neighbouring counters of the wave's
// line by its lanes 0 and 1 (one atomic instruction per wave)
__device__ __forceinline__ void tile_count_camera_samples(unsigned long long* counters, const tile_pixel& P, int ns) {
    static_assert(cnt_rays == 0 && cnt_samples == 1, "lanes 0 and 1 add to the line's first two counters");
    const unsigned long long s = wave_sum(P.valid ? (unsigned long long)(ns * ns) : 0ull);
    if (P.lane < 2 && s) atomicAdd(counter_line(counters) + P.lane, s);
}

// the ids of YRT_AOV_IDS and of the matte keys: the hit's instance in scene order, its
// material and its shape
struct hit_ids {
    int inst, mat, shape;
};

__device__ __forceinline__ hit_ids hit_ids_of(const dev_scene_view& S, const hit_record& hr) {
    const f4* ti = S.tinst + 4 * hr.slot;
    return {S.tinst_id[hr.slot], (int)((uint32_t)ibits(ti[2].w) & mat_index_mask), ibits(ti[0].w) & (int)inst_shape_mask};
}

// a block's 2 x 2 tiles over the window
dim3 tile_grid(const dev_render_args& args) {
    constexpr int side = AOV_TILE * AOV_BLOCK_TILES;
    return dim3((args.tile_w + side - 1) / side, (args.tile_h + side - 1) / side);
}

__device__ __forceinline__ void store_plane(void* plane, size_t at, vec3f v, float w) {
    reinterpret_cast<float4*>(plane)[at] = make_float4(v.x, v.y, v.z, w);
}

// `mask` (the requested AOVs) is a kernel argument, the same in every lane: every branch on
// it is a scalar branch, and the stores of an absent plane are never issued.
__global__ __launch_bounds__(AOV_BLOCK) void k_aov(dev_scene_view S, dev_render_args A, unsigned mask,
                                                   dev_aov_planes O, unsigned long long* counters) {
    const tile_pixel P = tile_pixel_of(A);
    if (!__ballot(P.in_window)) return;  // a tile outside the window: nothing to trace or write

    const int ns = A.samples;
    float depth = 0.0f, cover = 0.0f;
    vec3f pos = {0, 0, 0}, nrm = {0, 0, 0}, alb = {0, 0, 0};
    vec2f tuv = {0, 0};
    hit_ids ids = {-1, -1, -1};
    int id_ei = -1;
    if (__ballot(P.valid)) {
        for (int jj = 0; jj < ns; jj++) {
            for (int ii = 0; ii < ns; ii++) {
                work_counts wc;
                const tile_sample cs = tile_camera_sample(S, A, P, ii, jj, wc);
                if (!(P.valid && cs.hit)) continue;
                cover += 1.0f;
                depth += cs.hr.dist;
                if ((mask & aov_bit(aov_ids)) && jj == 0 && ii == 0) {
                    ids = hit_ids_of(S, cs.hr);
                    id_ei = cs.hr.ei;
                }
                if (mask & AOV_NEEDS_SURFACE) {
                    const surface sf = eval_surface(S, cs.hr.slot, cs.hr.ei, cs.hr.ew);
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
    if (P.in_window) {
        const size_t at = P.at(A);
        const float d = float(ns * ns);
        const float w = cover / d;
        if (mask & aov_bit(aov_depth)) store_plane(O.plane[aov_depth], at, {depth / d, 0.0f, 0.0f}, w);
        if (mask & aov_bit(aov_position)) store_plane(O.plane[aov_position], at, pos / d, w);
        if (mask & aov_bit(aov_normal)) store_plane(O.plane[aov_normal], at, nrm / d, w);
        if (mask & aov_bit(aov_texcoord)) store_plane(O.plane[aov_texcoord], at, {tuv.x / d, tuv.y / d, 0.0f}, w);
        if (mask & aov_bit(aov_albedo)) store_plane(O.plane[aov_albedo], at, alb / d, w);
        if (mask & aov_bit(aov_ids))
            reinterpret_cast<int4*>(O.plane[aov_ids])[at] = make_int4(ids.inst, id_ei, ids.mat, ids.shape);
    }
    tile_count_camera_samples(counters, P, ns);
}

}  // namespace

hipError_t launch_aovs(const device_scene& ds, const dev_render_args& args, unsigned mask, const dev_aov_planes& out,
                       unsigned long long* counters, hipStream_t stream) {
    if (args.tile_w <= 0 || args.tile_h <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_aov, tile_grid(args), dim3(AOV_BLOCK), 0, stream, ds.view, args, mask, out, counters);
    return hipGetLastError();
}

}  // namespace yrt
