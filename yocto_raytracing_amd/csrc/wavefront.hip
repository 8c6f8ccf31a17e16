// wavefront.hip -- the default render path: raytrace() (src/raytrace.cpp:213-254)
// as a wavefront pipeline of small gfx950 kernels over one lane per CAMERA SAMPLE.
//
// Per chunk of camera samples (a whole 1080p x 64 spp frame is one chunk; the
// per-sample state, ~70 B, lives in HBM -- 9 GB at c4 -- rather than in registers):
//   k_primary   eval_camera (:6-37) + closest hit (intersect_first, scene.cpp:483)
//               + eval_pos/eval_norm/eval_texcoord (scene.h:159-218) -> surface SoA
//   k_shadow    per light: the shadow ray of shade() (raytrace.cpp:129-133),
//               intersect_any (scene.cpp:489) -> occlusion byte
//   k_shade     the rest of shade() (:99-206): ambient, textures, Blinn-Phong or
//               lines lighting per unoccluded light, and for reflective hits the
//               mirror ray, compacted into the next level with one ballot + one
//               atomic per wave
//   (levels 1..max_depth-1: k_bounce (closest hit of the compacted rays), k_shadow,
//    k_shade; a sample whose value is final folds it up its chain of parents at once:
//    R_k = (D_k + R_{k+1}*kr_k) + la_k)
//   k_accumulate  the ordered per-pixel sum of raytrace.cpp:232-249
// A ray batch (yrt_shade_rays, run_rays) is the same pipeline with its level 0 from the caller:
// k_rays_first (the rays as given, the generic closest-hit walk), k_rays_shadow and k_rays_shade
// (the view point per sample from the ray's own origin), then the levels above; one RGBA per ray.
// A soft batch (yrt_shade_rays_soft, yrt_render_soft_shadows) is a ray batch whose lights are
// disks: k_soft_shadow casts K any-hit rays per (hit, light) at every level and leaves the count
// of open ones, k_soft_shade scales the light's term by the open share.
//
// Why: every traversal kernel carries only its ray and stack (few VGPRs, high
// occupancy), lanes of one wave are 64 samples of one pixel (s=8) or an 8x8 pixel
// tile (s=1), so their rays are nearly identical and stay converged through both
// BVH levels, and shadow rays of one light are traced together.
//
// Parity: each sample's arithmetic is shade()'s, in its order (trace_common.h);
// samples are summed per pixel in the reference's jj-major / ii-minor order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <type_traits>

#include "item_magic.h"
#include "packet_trace.h"
#include "soft_shadow_rays.h"
#include "trace_common.h"
#include "wf_workspace.h"
#include "yrt_render.h"

namespace yrt {
namespace {

constexpr int WF_BLOCK = 256;
#ifndef YRT_PRIMARY_BLOCK
#define YRT_PRIMARY_BLOCK 64  // threads per k_primary block (<= packet_block; a multiple of 64). A/B at c4: 256 -> 64 is -3 %
#endif
#ifndef YRT_SHADOW_BLOCK
#define YRT_SHADOW_BLOCK 64
#endif
// threads per block of the packet shadow kernel: one wave. Walks of very different
// lengths share a CU; a block's slots are only refilled once all its waves are done, so
// the smallest block keeps the CU fullest (A/B at c4: 256 -> 64 is -5 % on k_shadow;
// 1024 is +22 %). k_primary stays at WF_BLOCK: its LDS (the parked world 1/d) and the
// per-block counter flush would cap the blocks per CU. The per-lane walks keep WF_BLOCK
// (their stacks are in LDS).
template <bool PACKET>
constexpr int shadow_block() { return PACKET ? YRT_SHADOW_BLOCK : WF_BLOCK; }
#ifndef YRT_TRACE_WAVES
#define YRT_TRACE_WAVES 8  // waves per SIMD the traversal kernels are register-budgeted for (A/B at c4 with the structured walks: 7 -> 8 is -3.5 %)
#endif
#ifndef YRT_SHADOW_WAVES
#define YRT_SHADOW_WAVES YRT_TRACE_WAVES  // the same for k_shadow
#endif
#ifndef YRT_SHADOW_BLOCK_CHUNK
// k_shadow_persist: queue positions per block chunk (A/B at c4 against per-wave grabs of 8:
// 8 / 16 / 32 / 64 / 128 / 256 / 512: -2.8 / -2.7 / -2.6 / -2.7 / -2.2 / -1.0 / 0 %)
#define YRT_SHADOW_BLOCK_CHUNK 16
#endif
// samples per chunk (host side only: run() splits a frame by them). Small values are for the
// tests, which run frames of a few tiles as several chunks (tests/test_gpu_variants.py)
#ifndef YRT_CHUNK_LOG2
#define YRT_CHUNK_LOG2 29  // non-reflective scenes (~70 B of HBM per sample)
#endif
#ifndef YRT_MIRROR_CHUNK_LOG2
#define YRT_MIRROR_CHUNK_LOG2 25  // reflective scenes (64 B more per sample and mirror level)
#endif
constexpr int CHUNK_LOG2 = YRT_CHUNK_LOG2;
constexpr int MIRROR_CHUNK_LOG2 = YRT_MIRROR_CHUNK_LOG2;
static_assert(CHUNK_LOG2 >= 0 && CHUNK_LOG2 <= 29 && MIRROR_CHUNK_LOG2 >= 0 && MIRROR_CHUNK_LOG2 <= 29,
              "a chunk's samples are counted in an int");

struct wf_buffers {
    f4* surf0;          // {p.xyz, info}: info = mat*4+kind, -1 miss, -2 not a sample
    f4* surf1;          // {n.xyz, u}
    float* surfv;       // v
    unsigned char* occl;  // [light][sample]
    f4* rad;            // level-0 radiance per sample
    // bounce levels (reflective scenes only)
    // mirror levels (reflective scenes): one slab per record kind, `capacity` records per
    // level, so any number of levels is plain indexing (the reference recursion has no cap)
    f4* ray_o_;  // level k >= 1 at (k - 1) * capacity: {o.xyz, parent index}
    f4* ray_d_;  // level k >= 1: {d.xyz, -}
    f4* rec0_;   // level k < nlevels - 1 at k * capacity: {D.xyz, material index}
    f4* rec1_;   // {la.xyz, -}; kr is the material's, re-read where the fold needs it
    __device__ __forceinline__ f4* ray_o(int k) const { return ray_o_ + (size_t)(k - 1) * capacity; }
    __device__ __forceinline__ f4* ray_d(int k) const { return ray_d_ + (size_t)(k - 1) * capacity; }
    __device__ __forceinline__ f4* rec0(int k) const { return rec0_ + (size_t)k * capacity; }
    __device__ __forceinline__ f4* rec1(int k) const { return rec1_ + (size_t)k * capacity; }
    int* count;             // level k >= 1, segment g: rays at count[(k * level_segments + g) * count_stride]
    int seg;                // slots per segment of a mirror level (seg_count)
    unsigned* queue;        // work counters of the persistent grids: shadow [0, 8) per XCD + [8] shared, primary [16, 24) + [24]
    // a render's instance-level spine records relative to the camera origin -- or, in ray mode
    // (yrt_shade_rays, run_rays), where no kernel reads those: this chunk's rays in the
    // caller's buffer, 8 floats {o.xyz, d.xyz, tmin, tmax} per sample
    union {
        const f4* trel;
        const float* rays;
    };
    int capacity;           // samples per chunk
    int nlevels;            // levels allocated
    int need_v;             // the scene has textures: the surface's v (surfv) is stored and read
    // shadow bundles (level 0 of the persistent any-hit grid, k_bundle_lists)
    int bundles;            // 1: this chunk's k_primary writes pbox and its shadow items walk lists
    f4* pbox;               // per 64-sample item: {lo.xyz, -1 if a hit point is not finite} {hi.xyz, -}
    int* lcount;            // per (bundle, light): candidate leaves, -1 = walk the tree
    int* lskip;             // per (bundle, light): instances of its listed leaves its hull excludes
    f4* lists;              // per (bundle, light): bundle_recs wide records (wide_record_bytes each)
    f4* slists;             // per (super-bundle, light): its bundles' common leaf list (k_bundle_super)
    // camera lists (the closest hit of the camera rays, k_camera_lists)
    int cam_lists;          // 1: this chunk's camera rays walk their tile's list
    int* ccount;            // per 8x8-pixel tile of the chunk: listed leaves, -1 = walk the tree
    int* cskip;             // per tile: instances of its listed leaves its cone excludes
    f4* clist;              // per tile: camera_list_max entries of 2 f4 {lo - o, first} {hi - o, count}
    unsigned long long* lstats;  // the render's list sums (k_list_stats, list_sums of them)
};

// the counter of segment g of a mirror level (level_segments, count_stride: wf_workspace.h)
__device__ __forceinline__ int* seg_counter(int* count, int level, int g) {
    return count + (level * level_segments + g) * count_stride;
}

#if !defined(YRT_ITEM_MAGIC)  // (its non-default build is the `itemdiv` library of tools/build_variants.py)
// the item paths' divisions by spp, samples, tiles_x and band as a multiply-high and shifts
// (item_magic.h, the pairs made once per frame by run()), the item's tile on the scalar unit
// where an item lies in one tile, and camera_ray_w's range checks decided once per frame
// (DESIGN.md §5); 0: the emulated divisions and the per-item ballots
#define YRT_ITEM_MAGIC 1
#endif

struct chunk_args {
    long long pix0;  // first pixel (in tile enumeration order) of this chunk
    int npix;        // pixels in this chunk
    int spp;
    int tiles_x;     // 8x8 tiles across the window
    item_magic M;    // (YRT_ITEM_MAGIC) the frame's division pairs; all zero: the general code
};

// pixel enumeration: 8x8 tiles across the local window, row-major tiles, row-major
// pixels inside a tile; samples of a pixel consecutive in jj-major / ii-minor order
__device__ __forceinline__ bool pixel_of(const dev_render_args& A, int tiles_x, long long p, int& lx, int& ly,
                                         int& i, int& j) {
    long long t = p / (TILE * TILE);
    int w = (int)(p % (TILE * TILE));
    lx = (int)(t % tiles_x) * TILE + (w % TILE);
    ly = (int)(t / tiles_x) * TILE + (w / TILE);
    if (lx >= A.tile_w || ly >= A.tile_h) return false;
    i = A.x0 + lx;
    int b = ly / A.band, r = ly % A.band;
    j = A.y0 + (b * A.band_stride + A.band_offset) * A.band + r;
    return i < A.width && j < A.height;
}

// pixel w of tile t, with the frame's pairs (C.M.on). t and w may be wave-uniform: the
// caller hands the pairs' words over as it holds them (scalars there, lanes elsewhere)
struct tile_magic {
    uint32_t tx_mul, tx_shift, tiles_x, band_mul, band_shift, band;
};
__device__ __forceinline__ bool pixel_of_tile(const dev_render_args& A, const tile_magic& G, uint32_t t, uint32_t w,
                                              int& lx, int& ly, int& i, int& j) {
    const uint32_t ty = magic_div(t, G.tx_mul, G.tx_shift), tx = t - ty * G.tiles_x;
    lx = (int)(tx * TILE + (w % TILE));
    ly = (int)(ty * TILE + (w / TILE));
    if (lx >= A.tile_w || ly >= A.tile_h) return false;
    i = A.x0 + lx;
    const uint32_t b = magic_div((uint32_t)ly, G.band_mul, G.band_shift), r = (uint32_t)ly - b * G.band;
    j = A.y0 + ((int)b * A.band_stride + A.band_offset) * A.band + (int)r;
    return i < A.width && j < A.height;
}
__device__ __forceinline__ tile_magic tile_magic_of(const chunk_args& C) {
    return {C.M.tiles_x.mul, C.M.tiles_x.shift, C.M.tiles_x.d, C.M.band.mul, C.M.band.shift, C.M.band.d};
}
// pixel_of for the callers that hold the chunk's arguments: the pairs where the frame has them
__device__ __forceinline__ bool pixel_of(const dev_render_args& A, const chunk_args& C, long long p, int& lx,
                                         int& ly, int& i, int& j) {
    if (YRT_ITEM_MAGIC && C.M.on) {  // (uniform over the grid)
        const uint32_t p32 = (uint32_t)p;
        return pixel_of_tile(A, tile_magic_of(C), p32 / (TILE * TILE), p32 % (TILE * TILE), lx, ly, i, j);
    }
    return pixel_of(A, C.tiles_x, p, lx, ly, i, j);
}

__device__ __forceinline__ void flush(unsigned long long* counters, int idx, unsigned long long v) {
    unsigned long long s = wave_sum(v);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(counter_line(counters) + idx, s);
}

// the timed kernels' counters: wave sums combined per block in LDS, then ONE device
// atomic per counter per block into the block's counter line (a per-wave atomic
// costs ~4x as many fabric atomics; the c4 shadow pass has 1.5 M blocks)
// (tid: the thread's index in its block, threadIdx.x however the caller has it; index_of(k):
// the counter of v[k])
template <int N, int BS, class F>
__device__ __forceinline__ void flush_block_at(unsigned long long* counters, const unsigned long long (&v)[N],
                                               unsigned tid, F index_of) {
    __shared__ unsigned long long part[BS / 64][N];
    const int w = tid >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const unsigned long long s = wave_sum(v[k]);
        if ((tid & 63) == 0) part[w][k] = s;
    }
    __syncthreads();
    if (tid < N) {
        unsigned long long t = 0;
#pragma unroll
        for (int q = 0; q < BS / 64; q++) t += part[q][tid];
        const unsigned b = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        if (t) atomicAdd(counters + (size_t)(b % cnt_slots) * cnt_count + index_of(tid), t);
    }
}
template <int N, int BS = WF_BLOCK>
__device__ __forceinline__ void flush_block(unsigned long long* counters, const int (&idx)[N],
                                            const unsigned long long (&v)[N]) {
    flush_block_at<N, BS>(counters, v, threadIdx.x, [&](unsigned k) { return idx[k]; });
}

__device__ __forceinline__ void flush_work(unsigned long long* counters, const work_counts& wc) {
    flush(counters, cnt_box_tests, wc.box);
    flush(counters, cnt_inst_entries, wc.inst);
    flush(counters, cnt_prim_tests, wc.prim);
    flush(counters, cnt_shaded_hits, wc.hits);
    flush(counters, cnt_tex_lookups, wc.tex);
    flush(counters, cnt_wave_node_visits, wc.wnode);
    flush(counters, cnt_wave_prim_visits, wc.wprim);
}

// A workspace pointer as a global-memory pointer. k_primary_persist reads its buffer
// arguments back from an LDS copy, and a pointer loaded from memory is generic to the
// compiler: its stores would be FLAT, which count against LGKM_CNT as well, so the walk's
// next s_waitcnt lgkmcnt(0) (every record fetch) would wait for them to reach memory.
typedef float gvec4 __attribute__((ext_vector_type(4)));
// a constant made where it is used: v_mov of the immediate in volatile asm, which the compiler
// does not hoist out of a persistent kernel's item loop (a hoisted {0, 0, 0, -1} register
// tuple is held across the walk and spilled: the tuple is not rematerialised)
template <int IMM>
__device__ __forceinline__ float vconst() {
    float r;
    asm volatile("v_mov_b32 %0, %1" : "=v"(r) : "n"(IMM));
    return r;
}
// The per-sample workspace streams (surface records, occlusion bytes) are written and read
// with the non-temporal hint, so that they pass through L2 without evicting the scene
// (A/B in one process, profiles/r4/ab_nt: c4 24.77 -> 24.62 ms, rank 0 of 8 / 4 and c3
// -0.6 to -0.8 %, identical images)
__device__ __forceinline__ void gstore(f4* p, int idx, float x, float y, float z, float w) {
    __builtin_nontemporal_store(gvec4{x, y, z, w}, (__attribute__((address_space(1))) gvec4*)p + idx);
}
__device__ __forceinline__ void gstore(float* p, int idx, float x) {
    __builtin_nontemporal_store(x, (__attribute__((address_space(1))) float*)p + idx);
}
// a workspace stream's record / float / byte
__device__ __forceinline__ float4 ld4s(const f4* p) {
    const gvec4 v = __builtin_nontemporal_load((const __attribute__((address_space(1))) gvec4*)p);
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float lds1(const float* p) {
    return __builtin_nontemporal_load((const __attribute__((address_space(1))) float*)p);
}
__device__ __forceinline__ unsigned char ldb(const unsigned char* p) {
    return __builtin_nontemporal_load((const __attribute__((address_space(1))) unsigned char*)p);
}
__device__ __forceinline__ void stb(unsigned char* p, unsigned char v) {
    __builtin_nontemporal_store(v, (__attribute__((address_space(1))) unsigned char*)p);
}

// the sample's record in surf0: {p, info (mat*4+kind, -1 miss, -2 not a sample)}; the info field
__device__ __forceinline__ int sample_state(float4 s0) { return ibits(s0.w); }
__device__ __forceinline__ void store_not_sample(const wf_buffers& B, int idx) {
    gstore(B.surf0, idx, vconst<0>(), vconst<0>(), vconst<0>(), vconst<-2>());
}

// The surface record of a sample: the hit's surface is evaluated and stored on the hit lanes
// only, and a miss stores its marker. (Written as `surface sf = {}; if (hit) sf = ...;` the
// conditional aggregate copy kept the first 28 bytes of sf in a private array, which the
// backend promoted to 28 KB of LDS per 1024-thread block; its 64-bit address then took
// VGPRs the closest-hit walk spilled to scratch.)
// the surface record's info word: shadow class << 26 | material << 2 | kind (material < 2^24,
// so a hit's info is >= 0; -1 miss, -2 not a sample)
__device__ __forceinline__ int surf_info(const surface& sf) { return sf.mcls << 26 | sf.mat << 2 | sf.kind; }
__device__ __forceinline__ int info_mat(int info) { return (info >> 2) & (int)mat_index_mask; }

__device__ __forceinline__ vec3f store_hit_surface(const dev_scene_view& S, const wf_buffers& B, int idx, bool hit,
                                                   const hit_record& hr) {
    if (!hit) {
        gstore(B.surf0, idx, vconst<0>(), vconst<0>(), vconst<0>(), vconst<-1>());
        return {0, 0, 0};
    }
    const surface sf = eval_surface(S, hr.slot, hr.ei, hr.ew);
    gstore(B.surf0, idx, sf.p.x, sf.p.y, sf.p.z, __int_as_float(surf_info(sf)));
    gstore(B.surf1, idx, sf.n.x, sf.n.y, sf.n.z, sf.uv.x);
    // uv is read only by texture lookups: a scene without textures never needs it
    if (B.need_v) gstore(B.surfv, idx, sf.uv.y);
    return sf.p;
}

// the two traversal schedules behind one call: PACKET = wave-coherent walk
// (packet_trace.h, default), otherwise one independent walk per lane
// (trace_common.h). Both are called in wave-uniform control flow.
template <bool ANY, bool COUNT, bool PACKET, typename SE, int BS = packet_block>
struct tracer {
    SE* lane_stk;
    __device__ __forceinline__ bool trace(const dev_scene_view& S, const ray3& ray, bool valid, hit_record& hr,
                                          work_counts& wc) {
        if (PACKET) {
            if constexpr (ANY)
                return packet_any<COUNT>(S, ray, valid, wc);
            else
                return packet_first<COUNT, BS>(S, ray, valid, hr, wc);
        }
        if (!valid) return false;
        if (ANY) return occluded<COUNT, WF_BLOCK>(S, ray, lane_stk, wc);
        return traverse<false, COUNT, WF_BLOCK>(S, ray, hr, lane_stk, wc);
    }
};

// LDS for either schedule: per-lane stack columns; the packet walk keeps its stack
// in VGPR lanes and needs none
template <bool PACKET, typename SE>
struct traversal_lds;
template <typename SE>
struct traversal_lds<false, SE> {
    SE lane[traversal_stack_cap * WF_BLOCK];
};
template <typename SE>
struct traversal_lds<true, SE> {
    int unused;
};

template <bool ANY, bool COUNT, bool PACKET, typename SE>
__device__ __forceinline__ tracer<ANY, COUNT, PACKET, SE> make_tracer(traversal_lds<PACKET, SE>& L) {
    tracer<ANY, COUNT, PACKET, SE> t;
    if constexpr (PACKET)
        t.lane_stk = nullptr;
    else
        t.lane_stk = L.lane + threadIdx.x;
    return t;
}

// Workgroups are dealt round-robin to the 8 XCDs (linear block b runs on XCD b % 8).
// xcd_runs keeps the round-robin sweep over the image but hands each XCD runs of C
// consecutive blocks: the grid is cut into super-chunks of 8 runs, XCD x takes run x of
// each (a bijection; a ragged last super-chunk keeps its blocks). Each XCD then traces
// neighbouring pixels (its L2 and its CUs' scalar caches see one region) while all eight
// still sweep the image together. (Contiguous block ranges per XCD lose: +10 % primary,
// +7.5 % shadow -- image regions differ in cost and the slowest XCD sets the launch time.)
template <unsigned C>
__device__ __forceinline__ unsigned xcd_runs(unsigned b, unsigned n) {
    constexpr unsigned G = 8u * C;
    if (b >= n / G * G) return b;
    const unsigned w = b % G;
    return b - w + (w % 8u) * C + w / 8u;
}

#ifndef YRT_SHADOW_LIGHT_MINOR
#define YRT_SHADOW_LIGHT_MINOR 24  // k_shadow: XCD run length with the light index minor (A/B: shadow -1.1 %)
#endif
#ifndef YRT_XCD_CHUNK_PRIMARY
#define YRT_XCD_CHUNK_PRIMARY 256  // k_primary: XCD runs of this many blocks (A/B: -1.5 %)
#endif

// ke / rr (vec3f / float: three divisions) with fast_div.h's div_nr when every active
// lane's operands are in its range
__device__ __forceinline__ vec3f div3(vec3f ke, float rr) {
    if (!__ballot(!(div_nr_ok(ke.x, rr) && div_nr_ok(ke.y, rr) && div_nr_ok(ke.z, rr)))) {
        const float y = rcp_nr(rr);
        return {div_nr(ke.x, rr, y), div_nr(ke.y, rr, y), div_nr(ke.z, rr, y)};
    }
    return ke / rr;
}

// ---- shadow rays whose light term is exactly zero are not traced ----
// shade() (raytrace.cpp:133-183) adds a light's term c += ld + ls only when intersect_any
// finds no occluder; skipping it and adding it are the same when the term is +-0 in every
// component (c starts at +0 and a sum never turns into -0 under round-to-nearest, so c + +-0
// is c bit for bit). From the hit's material class (yrt_device.h mat_class_shift, set at
// upload) and the geometry alone, the term is +-0 when max(0, n.l) is +-0 and ker = ke / r^2
// is below 2^100 in every component -- then ld = (kd0 * tkd) * ker * max(0, n.l) is a finite
// product (|kd0| <= 2^20, the texture factor in [0, 1]) times +-0 -- and ls is +-0:
//   class 1 (Ks == 0, ns in [0, FLT_MAX]): ks * ker is +-0, and with x = max(0, n.h) in
//     [0, 1] spec_pow takes its shortcut (factor 1), so ls = +-0;
//   class c >= 2 (ns >= mat_class_ns(c) > 0, |Ks| <= 2^20): powf_cr(x, ns) is exactly 0 when
//     x == 0, or when x in [2^-126, 1) and ns * log2(x) < -151 by v_log_f32 -- which
//     mat_class_ns(c) * log2(x) < -151 implies (log2(x) < 0, and rounding is monotone) --, so
//     ls = finite * 0; where spec_pow takes its shortcut instead, ls = +-0 * 1.
// n, l, r, v, h and ker are computed with the functions k_shade uses (normalize_len, div3),
// so the test sees k_shade's values.
// Lines (their sin-based lighting) are always traced. A culled ray is recorded as occluded:
// k_shade skips the light, which leaves c as adding +-0 would. The ray counters keep the
// reference's counts (a culled ray is counted); the instrumented COUNT pass traces every ray.
// n is the surface record's second row, loaded beside the first: no dependent load.
// Called in uniform control flow; a wave in which no lane can pass the cheap first tests
// (class, kind, max(0, n.l) == 0) skips the rest.
__device__ __forceinline__ bool light_term_zero(int info, vec3f nrm, vec3f p, vec3f ro, vec3f l, float r, vec3f ke) {
    const int cls = (info >> 26) & 15;
    const float sd = smax(0.0f, dot(nrm, l));
    const bool first = info >= 0 && cls != 0 && (info & 3) != kind_lines && sd == 0.0f;
    if (!ballot(first)) return false;
    vec3f v, h, ker;
    float vlen, hlen;
    normalize_len(ro - p, v, vlen);
    normalize_len(v + l, h, hlen);
    ker = div3(ke, r * r);
    const float x = smax(0.0f, dot(nrm, h));
    const bool ker_ok = fabsf(ker.x) < 0x1p100f && fabsf(ker.y) < 0x1p100f && fabsf(ker.z) < 0x1p100f;
    const bool ls_zero =
        cls == 1 ? x >= 0.0f && x <= 1.0f
                 : x == 0.0f || (x >= 0x1p-126f && x < 1.0f &&
                                 (float)(16 << ((cls - 2) & 15)) * __builtin_amdgcn_logf(x) < -151.0f);
    return first && ker_ok && ls_zero;
}

// camera_ray (trace_common.h, raytrace.cpp:6-37 with the uv of :235-238) with its four
// divisions and normalize through fast_div.h where every active lane is in range (the
// same bits); called per lane in divergent code (the checks ballot the active lanes).
// in_range (wave-uniform): run() has decided for the whole frame that every division is in
// range (item_magic::div_ok), so the checks are not made
__device__ __forceinline__ ray3 camera_ray_w(const dev_camera& cam, int W, int H, int ns, int i, int j, int ii,
                                             int jj, bool in_range = false) {
    const float fns = (float)ns, fw = (float)W, fh = (float)H;
    const float a = ii + 0.5f, b = jj + 0.5f;
    float u, v;
    if (in_range || !__ballot(!(div_nr_ok(a, fns) && div_nr_ok(b, fns)))) {
        const float y = rcp_nr(fns);
        u = i + div_nr(a, fns, y), v = j + div_nr(b, fns, y);
    } else {
        u = i + a / fns, v = j + b / fns;
    }
    if (in_range || !__ballot(!(div_nr_ok(u, fw) && div_nr_ok(v, fh)))) {
        u = div_nr(u, fw, rcp_nr(fw)), v = div_nr(v, fh, rcp_nr(fh));
    } else {
        u = u / fw, v = v / fh;
    }
    vec3f q;
    q.x = cam.ox + (u - 0.5f) * cam.w * cam.xx + (v - 0.5f) * cam.h * cam.yx - cam.focus * cam.zx;
    q.y = cam.oy + (u - 0.5f) * cam.w * cam.xy + (v - 0.5f) * cam.h * cam.yy - cam.focus * cam.zy;
    q.z = cam.oz + (u - 0.5f) * cam.w * cam.xz + (v - 0.5f) * cam.h * cam.yz - cam.focus * cam.zz;
    const vec3f o = {cam.ox, cam.oy, cam.oz};
    vec3f d;
    float len;
    normalize_len(q - o, d, len);
    return {o, d, ray_eps, flt_max};
}

// ---- shadow bundles ----
// The shadow rays of one light from the samples of a bundle (bundle_g consecutive 64-sample
// items: an 8x8-pixel tile at 8x8 spp) all run from points inside the box P of the bundle's
// hit points towards one point, the light's position Lp (raytrace.cpp:129-133; the light
// frame's rotation is the identity, so its ray is p -> transform_point(frame, pos0 - p) =
// pos0 - p + o). Every such segment lies in the convex hull of P and Lp. k_bundle_lists
// collects, per (bundle, light), the instance-level leaves of the any-hit tree whose box no
// bounding plane of that hull separates by more than a margin far above the slab test's
// rounding (its t values carry a few ulps of |t| <= |P - Lp|, the 1.00000024 fudge another
// 2.4e-7): a leaf outside that list fails the exact box test of every ray of the bundle.
// The walk then starts from the list (at most bundle_max leaves as a chain of wide records)
// instead of the tree's root. It tests each listed leaf's own box,
// exactly as the tree walk does, and reaches every leaf the tree walk reaches -- the
// any-hit answer does not depend on which inner boxes were tested.
// A bundle whose light is rotated, whose hit points are not finite or whose list would be
// longer walks the tree.
// (bundle_g items per bundle, bundle_recs, bundle_max_lights, camera_list_max: wf_workspace.h)
#ifndef YRT_BUNDLE_MIN_TOP
#define YRT_BUNDLE_MIN_TOP 8  // bundles only when the instance level's wide tree has this many records
#endif
#ifndef YRT_LISTS_MIN_SPP
// the lists' cost is per 8x8-pixel tile (~0.2 ms at 1080p), their gain per sample: in one
// process (profiles/r5/ab/r5t_*) instance10000 at 1080p with lists on / off -- 1 spp 1.79 /
// 1.54 ms, 4 spp 3.00 / 3.06, 16 spp 6.84 / 7.93, 64 spp 19.41 / 24.18; instance100k at 4 spp
// 4.21 / 3.99, instance1k 1.50 / 1.65. YRT_LISTS_AUTO builds them from this many samples per
// pixel (a 3x3 grid)
#define YRT_LISTS_MIN_SPP 9
#endif
// (the list builders also mark the instances of a listed leaf that their cone / hull excludes,
// and the walks skip them: k_camera_lists, k_bundle_lists; dev_scene_view ibox)
constexpr int bundle_max = 16;        // candidate leaves per list

// wave-wide min / max with DPP row rotations and row broadcasts (VALU only, no LDS round
// trips): every row of 16 lanes folds itself, rows 1 and 3 take rows 0 and 2 (row_bcast:15),
// rows 2 and 3 take row 1 (row_bcast:31); lane 63 then holds the result. The floats (no NaN
// here) are folded as integers whose signed order is theirs (b ^ (b >> 31 & 0x7fffffff)), so
// that each step is one v_min_i32 / v_max_i32 with the DPP source and no canonicalisation.
// (the lanes of rows outside ROWS are left undefined: only row 3's lanes, which every step
// writes, reach the result)
template <int CTRL, int ROWS>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_mov_dpp(v, CTRL, ROWS, 0xf, false);
}
__device__ __forceinline__ int fkey(int b) { return b ^ ((b >> 31) & 0x7fffffff); }  // (its own inverse)
template <bool MAX>
__device__ __forceinline__ float wave_fold(float f) {
    auto op = [](int a, int b) { return MAX ? max(a, b) : min(a, b); };
    int v = fkey(__float_as_int(f));
    v = op(v, dpp_i<0x121, 0xf>(v));  // row_ror:1
    v = op(v, dpp_i<0x122, 0xf>(v));  // row_ror:2
    v = op(v, dpp_i<0x124, 0xf>(v));  // row_ror:4
    v = op(v, dpp_i<0x128, 0xf>(v));  // row_ror:8
    v = op(v, dpp_i<0x142, 0xa>(v));  // row_bcast:15 into rows 1, 3
    v = op(v, dpp_i<0x143, 0xc>(v));  // row_bcast:31 into rows 2, 3
    return __int_as_float(fkey(__builtin_amdgcn_readlane(v, 63)));
}
__device__ __forceinline__ float wave_fmin(float v) { return wave_fold<false>(v); }
__device__ __forceinline__ float wave_fmax(float v) { return wave_fold<true>(v); }
// a box's six folds in lock step (their DPP steps interleave: no wait states between them)
__device__ __forceinline__ void wave_box(float (&lo)[3], float (&hi)[3]) {
    int v[6];
    for (int a = 0; a < 3; a++) v[a] = fkey(__float_as_int(lo[a])), v[3 + a] = fkey(__float_as_int(hi[a]));
#define YRT_BOX_STEP(CTRL, ROWS)                                                  \
    {                                                                             \
        int t[6];                                                                 \
        for (int a = 0; a < 6; a++) t[a] = dpp_i<CTRL, ROWS>(v[a]);               \
        for (int a = 0; a < 6; a++) v[a] = a < 3 ? min(v[a], t[a]) : max(v[a], t[a]); \
    }
    YRT_BOX_STEP(0x121, 0xf)
    YRT_BOX_STEP(0x122, 0xf)
    YRT_BOX_STEP(0x124, 0xf)
    YRT_BOX_STEP(0x128, 0xf)
    YRT_BOX_STEP(0x142, 0xa)
    YRT_BOX_STEP(0x143, 0xc)
#undef YRT_BOX_STEP
    for (int a = 0; a < 3; a++) {
        lo[a] = __int_as_float(fkey(__builtin_amdgcn_readlane(v[a], 63)));
        hi[a] = __int_as_float(fkey(__builtin_amdgcn_readlane(v[3 + a], 63)));
    }
}

// the box of this wave's hit points (the item idx / 64), for k_bundle_lists; called by
// every lane of the wave
__device__ __forceinline__ void store_item_box(const wf_buffers& B, int idx, bool has_p, vec3f p) {
    const bool fin = has_p && __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z);
    const bool bad = has_p && !fin;
    float lo[3] = {fin ? p.x : INFINITY, fin ? p.y : INFINITY, fin ? p.z : INFINITY};
    float hi[3] = {fin ? p.x : -INFINITY, fin ? p.y : -INFINITY, fin ? p.z : -INFINITY};
    wave_box(lo, hi);
    const bool any_bad = ballot(bad) != 0;
    if ((threadIdx.x & 63) == 0) {
        const int item = idx >> 6;
        gstore(B.pbox, 2 * item, lo[0], lo[1], lo[2], any_bad ? -1.0f : 0.0f);
        gstore(B.pbox, 2 * item + 1, hi[0], hi[1], hi[2], 0.0f);
    }
}

// ---- level 0: camera rays + closest hit + surface ----
// the camera samples idx of one wave: eval_camera, closest hit, surface record
template <bool COUNT, bool PACKET, typename SE, int BS = packet_block, int LDSN = 0, bool LIST = false,
          bool NESTED = false>
__device__ __forceinline__ bool primary_samples(const dev_scene_view& S, const dev_render_args& A, const chunk_args& C,
                                                const wf_buffers& B, tracer<false, COUNT, PACKET, SE, BS>& T, int idx,
                                                work_counts& wc, const float4* lds = nullptr) {
    const int nsamp = C.npix * C.spp;
    bool valid = false;
    ray3 ray = {{0, 0, 0}, {0, 0, 1}, ray_eps, flt_max};
    const bool magic = YRT_ITEM_MAGIC && uniform(C.M.on) != 0;
    int list_tile = -1;  // (magic) wave-uniform: the chunk's tile all of the wave's samples lie in
    if (magic) {
        const bool in_range = uniform(C.M.div_ok) != 0;
        const int ns = A.samples;
        int lx, ly, i, j, ii, jj;
        if (uniform(C.M.pow2)) {
            // an item is 64 / spp whole pixels of one tile (pix0 is whole tiles): the tile, and
            // at 64 spp the pixel, from the item index on the scalar unit; the lane's pixel and
            // sample are bits of its index
            const uint32_t item = (uint32_t)uniform(idx) >> 6;
            const uint32_t sl = (uint32_t)uniform(C.M.spp_log2), lane = (uint32_t)idx & 63u;
            const uint32_t ct = item >> sl;  // the tile of the chunk
            const uint32_t t = (uint32_t)uniform((int)(uint32_t)(C.pix0 >> 6)) + ct;
            const tile_magic G = {(uint32_t)uniform((int)C.M.tiles_x.mul), (uint32_t)uniform((int)C.M.tiles_x.shift),
                                  (uint32_t)uniform((int)C.M.tiles_x.d),  (uint32_t)uniform((int)C.M.band.mul),
                                  (uint32_t)uniform((int)C.M.band.shift), (uint32_t)uniform((int)C.M.band.d)};
            const uint32_t w0 = (item & ((1u << sl) - 1u)) << (6u - sl);  // the item's first pixel in the tile
            if (sl == 6u)
                valid = pixel_of_tile(A, G, t, w0, lx, ly, i, j);
            else
                valid = pixel_of_tile(A, G, t, w0 + (lane >> sl), lx, ly, i, j);
            const uint32_t q = lane & ((1u << sl) - 1u), nl = sl >> 1;
            ii = (int)(q & ((1u << nl) - 1u)), jj = (int)(q >> nl);
            valid = valid && idx < nsamp;
            if ((int)(item * 64u) < nsamp) list_tile = (int)ct;
        } else {
            const uint32_t pl = magic_div((uint32_t)idx, C.M.spp), q = (uint32_t)idx - pl * (uint32_t)C.spp;
            const uint32_t p = (uint32_t)C.pix0 + pl;
            valid = idx < nsamp && pixel_of_tile(A, tile_magic_of(C), p / (TILE * TILE), p % (TILE * TILE), lx, ly, i, j);
            jj = (int)magic_div(q, C.M.samples), ii = (int)q - jj * ns;
        }
        if (valid)
            ray = camera_ray_w(A.cam, A.width, A.height, ns, i, j, ii, jj, in_range);
        else if (idx < nsamp)
            store_not_sample(B, idx);
    } else if (idx < nsamp) {
        const long long p = C.pix0 + idx / C.spp;
        const int q = idx % C.spp;
        int lx, ly, i, j;
        valid = pixel_of(A, C.tiles_x, p, lx, ly, i, j);
        if (valid) {
            const int ns = A.samples;
            ray = camera_ray_w(A.cam, A.width, A.height, ns, i, j, q % ns, q / ns);
        } else {
            store_not_sample(B, idx);
        }
    }
    hit_record hr = {-1, -1, {0, 0, 0, 0}, 0};
    // every camera ray starts at the camera origin (camera_ray): the packet walk tests the
    // instance level on the records relative to it -- or, with camera lists, walks the list
    // of the 8x8-pixel tile this wave's samples lie in (a wave straddling two tiles walks
    // the tree)
    bool hit;
    if constexpr (PACKET) {
        const f4* lbase = nullptr;
        int ln = -1;
        if (LIST && !COUNT) {
            const int nsamp = C.npix * C.spp;
            const int i0 = uniform(idx) & ~63, i1 = min(i0 + 63, nsamp - 1);
            int t0, t1;
            if (magic && list_tile >= 0) {
                t0 = t1 = list_tile;
            } else if (magic) {  // (scalar: the sample indices and the pair are wave-uniform)
                const uint32_t mul = (uint32_t)uniform((int)C.M.spp.mul), sh = (uint32_t)uniform((int)C.M.spp.shift);
                t0 = (int)(magic_div((uint32_t)i0, mul, sh) / (TILE * TILE));
                t1 = (int)(magic_div((uint32_t)max(i1, 0), mul, sh) / (TILE * TILE));
            } else {
                t0 = i0 / C.spp / (TILE * TILE), t1 = i1 / C.spp / (TILE * TILE);
            }
            // (a zero direction -- a camera with no extent -- walks the tree)
            const bool zero_dir = valid && ray.d.x == 0.0f && ray.d.y == 0.0f && ray.d.z == 0.0f;
            if (t0 == t1 && i0 < nsamp && !ballot(zero_dir)) {
                ln = uniform(B.ccount[t0]);
                lbase = B.clist + (size_t)t0 * camera_list_max * 2;
            }
        }
        // the list mode's walk as nested loops (packet_first_list; YRT_FIRST_NESTED=0: the flat one)
        if constexpr (NESTED && LIST && !COUNT && LDSN == 0)
            hit = packet_first_list<BS>(S, ray, valid, hr, wc, B.trel, lbase, ln);
        else
            hit = packet_first<COUNT, BS, true, LDSN, LIST>(S, ray, valid, hr, wc, B.trel, lds, lbase, ln);
    } else {
        hit = T.trace(S, ray, valid, hr, wc);
    }
    vec3f hp = {0, 0, 0};
    if (valid) {
        if (COUNT && hit) wc.hits++;
        hp = store_hit_surface(S, B, idx, hit, hr);
    }
    if (!COUNT && B.bundles) store_item_box(B, idx, valid && hit, hp);
    return valid;
}

// The instance-level spine records with the camera origin subtracted from every bound, in
// fp32 as the reference's slab test does it ((bbox.min - ray.o), scene.cpp:373-374), are what
// the primary rays' REL walk reads (packet_first); k_chunk_setup writes them once per render.

// ---- per-chunk setup: one launch instead of a kernel and three to five fills ----
// the camera-relative spine records (the first chunk of a packet render: tpair != nullptr),
// and zeros for the persistent grids' work counters (queue), the list sums (lstats, the first
// chunk that builds lists), the mirror levels' ray counts (count_ints) and the render's counter
// lines (counters, the first chunk). Each fill was its own hipMemsetAsync launch of ~4 us of
// GPU time; at a rank's share of an 8-way split a frame is ~2.6 ms.
__global__ __launch_bounds__(WF_BLOCK) void k_chunk_setup(const f4* __restrict__ tpair, int nrec, float ox, float oy,
                                                          float oz, f4* __restrict__ trel, unsigned* queue,
                                                          unsigned long long* lstats, int* count, int count_ints,
                                                          unsigned long long* counters, int counter_words) {
    const int i = blockIdx.x * WF_BLOCK + threadIdx.x;
    const int stride = gridDim.x * WF_BLOCK;
    if (tpair)
        for (int k = i; k < nrec; k += stride) {
            const float4 r = ld4(tpair + k);
            trel[k] = {r.x - ox, r.y - oy, r.z - oz, r.w};
        }
    if (i < 32) queue[i] = 0u;
    if (lstats && i < list_sums) lstats[i] = 0ull;
    for (int k = i; k < count_ints; k += stride) count[k] = 0;
    if (counters)
        for (int k = i; k < counter_words; k += stride) counters[k] = 0ull;
}

// ---- work distribution of the persistent any-hit grid: block chunks ----
// The waves of an XCD share one agent-scope counter over its item sequence, which keeps
// the chip's working window as tight as the hardware's block dealing does (a fixed
// interleave, wave j taking j, j + W, ..., lets the waves drift apart: +21 %). A block
// takes CS consecutive positions per atomic and its waves take them one at a time from
// an LDS counter, so the waves of a CU trace neighbouring items together (per-wave grabs
// of 8 consecutive positions: +2.7 % on the any-hit grid). Chunk g's base sits in ring
// entry g % R behind a tag; the wave taking chunk g's middle slot fetches chunk g + 1,
// once every slot of the entry's previous chunk has been read (each taker reads its base
// right after taking its slot, before it looks at the item, and slots are taken in
// order, so every wait ends). All atomics are vector (lane 0) or LDS operations.
#ifndef YRT_SHARED_TAIL
// the persistent grids' last 1/YRT_SHARED_TAIL items come from one queue that every XCD
// takes from once its own share is done (the XCDs' shares otherwise end up to 2 % of a
// c4 launch apart, 6 % at a rank's share of an 8-way split: tools/tail_stats.py); 0: each
// XCD keeps its static share to the end. A/B in one process (profiles/r4/ab_shared_tail):
// 1/32 / 1/16 / 1/8 -- c4 24.67 -> 24.43 / 24.43 / 24.42 ms, rank 0 of 4 6.42 -> 6.34 /
// 6.37 / 6.35, instance100k 32.92 -> 32.70 / 32.87 / 33.14 (its short any-hit grid pays
// for a larger shared tail), rank 0 of 8 and c3 within 0.3 %
#define YRT_SHARED_TAIL 32
#endif
constexpr unsigned tail_flag = 0x80000000u;  // a position in the shared tail
constexpr unsigned gcd_u(unsigned a, unsigned b) { return b ? gcd_u(b, a % b) : a; }
// items of the per-XCD head: whole super-runs of 8 x lcm(RUN, CS) (so that every XCD's
// share is whole runs and whole block chunks); the rest is the shared tail
template <unsigned RUN, unsigned CS>
__device__ __forceinline__ unsigned head_items(unsigned n_items) {
    constexpr unsigned G = 8u * (RUN / gcd_u(RUN, CS) * CS);
    return YRT_SHARED_TAIL ? (n_items - n_items / YRT_SHARED_TAIL) / G * G : 0u;
}
// a block chunk's first position: from the XCD's own counter while its share lasts
// (limit = positions per XCD), then from the shared one (flagged)
template <unsigned CS>
__device__ __forceinline__ unsigned chunk_fetch(unsigned* counter, unsigned* gcounter, unsigned limit) {
    const unsigned k = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!YRT_SHARED_TAIL || k * CS + CS <= limit) return k * CS;
    return tail_flag | __hip_atomic_fetch_add(gcounter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * CS;
}

struct chunk_ring {
    static constexpr unsigned R = 4;
    unsigned base[R], tag[R], reads[R], taken;
};

template <unsigned CS>
__device__ __forceinline__ void chunk_ring_init(chunk_ring& ring, unsigned* counter, unsigned* gcounter = nullptr,
                                                unsigned limit = ~0u) {
    static_assert(CS >= 2, "a chunk's middle slot fetches the next chunk");
    if (threadIdx.x < chunk_ring::R) {
        ring.tag[threadIdx.x] = threadIdx.x == 0 ? 0u : ~0u;
        ring.reads[threadIdx.x] = threadIdx.x == 0 ? 0u : CS;
    }
    if (threadIdx.x == 0) {
        ring.base[0] = chunk_fetch<CS>(counter, gcounter, limit);
        ring.taken = 0;
    }
    __syncthreads();
}

// the calling wave's next position in its XCD's item sequence (wave-uniform)
template <unsigned CS>
__device__ __forceinline__ unsigned chunk_ring_next(chunk_ring& ring, unsigned* counter, unsigned lane,
                                                    unsigned* gcounter = nullptr, unsigned limit = ~0u) {
    constexpr unsigned R = chunk_ring::R;
    unsigned t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(&ring.taken, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    t = (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    const unsigned g = t / CS, o = t % CS;
    if (o == CS / 2) {  // publish chunk g + 1
        const unsigned e1 = (g + 1) % R;
        unsigned nbase = 0;
        if (lane == 0) nbase = chunk_fetch<CS>(counter, gcounter, limit);
        nbase = (unsigned)__builtin_amdgcn_readfirstlane((int)nbase);
        while (__hip_atomic_load(&ring.reads[e1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != CS)
            __builtin_amdgcn_s_sleep(1);
        if (lane == 0) {
            ring.base[e1] = nbase;
            __hip_atomic_store(&ring.reads[e1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(&ring.tag[e1], g + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    const unsigned e = g % R;
    while (__hip_atomic_load(&ring.tag[e], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != g)
        __builtin_amdgcn_s_sleep(1);
    const unsigned q = (unsigned)__builtin_amdgcn_readfirstlane((int)ring.base[e]) + o;
    if (lane == 0) __hip_atomic_fetch_add(&ring.reads[e], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    return q;
}

// position q of XCD xcd's sequence -> item: runs of RUN consecutive items per XCD (XCD x
// takes runs x, x + 8, ...), then the items past the last whole super-run round-robin
template <unsigned RUN>
__device__ __forceinline__ unsigned xcd_item(unsigned q, unsigned xcd, unsigned n_items) {
    const unsigned full = n_items / (8u * RUN) * (8u * RUN);
    const unsigned per_xcd = full / 8u;
    return q < per_xcd ? ((q / RUN) * 8u + xcd) * RUN + q % RUN : full + (q - per_xcd) * 8u + xcd;
}
// the same with a shared tail (YRT_SHARED_TAIL): an XCD's own positions cover whole runs of
// the head, a flagged position is the tail's (head + its index; >= n_items: done)
template <unsigned RUN>
__device__ __forceinline__ unsigned split_item(unsigned q, unsigned xcd, unsigned n_items, unsigned head) {
    if (!YRT_SHARED_TAIL) return xcd_item<RUN>(q, xcd, n_items);
    if (q & tail_flag) return head + (q & ~tail_flag);
    return ((q / RUN) * 8u + xcd) * RUN + q % RUN;
}

#ifdef YRT_TAIL_STATS
// diagnostic build only (tools/tail_stats.py): per wave of the persistent grids, its start
// and end on the 100 MHz constant clock, the items it took and its XCD (vector stores)
static __device__ unsigned long long g_tail[2][8192][4];
__device__ __forceinline__ void tail_record(int k, unsigned long long t0, unsigned items) {
    const unsigned gw = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u;
    if ((threadIdx.x & 63) == 0 && gw < 8192u) {
        unsigned long long* e = g_tail[k][gw];
        e[0] = t0, e[1] = __builtin_amdgcn_s_memrealtime(), e[2] = items, e[3] = blockIdx.x % 8u;
    }
}
#endif

// (LIST: the camera rays walk their tiles' lists, k_camera_lists)
template <bool COUNT, bool PACKET, typename SE, bool LIST = false>
__global__ __launch_bounds__(YRT_PRIMARY_BLOCK, YRT_TRACE_WAVES) void k_primary(dev_scene_view S, dev_render_args A,
                                                               chunk_args C, wf_buffers B,
                                                               unsigned long long* counters) {
    constexpr int BS = YRT_PRIMARY_BLOCK;
    __shared__ traversal_lds<PACKET, SE> lds;
    auto T = make_tracer<false, COUNT, PACKET, SE>(lds);
    const int idx = (int)xcd_runs<YRT_XCD_CHUNK_PRIMARY>(blockIdx.x, gridDim.x) * BS + threadIdx.x;
    work_counts wc;
    const bool valid = primary_samples<COUNT, PACKET, SE, packet_block, 0, LIST>(S, A, C, B, T, idx, wc);
    flush_block<2, BS>(counters, {cnt_rays, cnt_samples}, {valid ? 1ull : 0ull, valid ? 1ull : 0ull});
    if (COUNT) flush_work(counters, wc);
}

// ---- level 0, persistent: k_primary's work on a grid that fills the chip once (two
// SP_BLOCK-thread blocks per CU), each wave taking 64-sample items through its block's
// chunk ring (counters B.queue[8..15]). The render, chunk and buffer arguments are read
// from LDS copies for each item (a compiler barrier per item), so they are not held in
// registers across the walk.
constexpr int SP_BLOCK = 1024;  // threads per persistent block (two blocks per CU at 8 waves/SIMD)
#ifndef YRT_PRIMARY_WAVES
#define YRT_PRIMARY_WAVES YRT_TRACE_WAVES  // k_primary_persist: waves per SIMD (register budget and grid)
#endif
#ifndef YRT_PRIMARY_SP_BLOCK
// k_primary_persist: threads per block, whole blocks filling YRT_PRIMARY_WAVES per SIMD
#define YRT_PRIMARY_SP_BLOCK \
    (YRT_PRIMARY_WAVES == 7 ? 448 : YRT_PRIMARY_WAVES == 6 ? 768 : YRT_PRIMARY_WAVES == 5 ? 640 : SP_BLOCK)
#endif
static_assert((YRT_PRIMARY_WAVES * 4 * 64) % YRT_PRIMARY_SP_BLOCK == 0, "whole blocks per CU");
#ifndef YRT_PRIMARY_LDS_RECORDS
// k_primary_persist with LDS staging on (yrt_scene_set_lds_staging): the first records of the
// camera-relative instance level (breadth first, device_scene.cpp) staged in LDS per block and
// read by the walk instead of through the scalar cache (A/B, DESIGN.md §5: 1 023 / 511 / 255
// records +4.1 / +3.7 / +4.3 %; the handle's default is off)
#define YRT_PRIMARY_LDS_RECORDS 511
#endif
#ifndef YRT_PRIMARY_PERSIST_MIN_ITEMS
// A/B against k_primary (items = 64-sample blocks; profiles/r3/ab_primary_persist): 2.07 M
// (c4) primary 11.55 -> 11.37 ms; instance100k 27.16 -> 27.01. Round 4
// (profiles/r4/ab_persist): the band shares of an N-rank split, which the old 1 M threshold
// sent to k_primary, lose most: c4 rank 0 of 8 / 4 primary 2.89 -> 1.52 / 4.60 -> 2.89 ms,
// instance100k rank 0 of 8 13.91 -> 3.74; c3 1.14 -> 1.10, 640x360 c4 1.49 -> 0.98; c1/c2
// equal. The timed path is persistent at every size. (Holding the arguments in registers
// instead: 62 SGPR and 12 VGPR spills, c4 unchanged.)
#define YRT_PRIMARY_PERSIST_MIN_ITEMS 0
#endif
#ifndef YRT_PRIMARY_BLOCK_CHUNK
#define YRT_PRIMARY_BLOCK_CHUNK 16  // (64: the same)
#endif
template <typename SE, int LDSN, bool LIST = false>
__global__ __launch_bounds__(YRT_PRIMARY_SP_BLOCK, YRT_PRIMARY_WAVES) void k_primary_persist(dev_scene_view S,
                                                                                dev_render_args A, chunk_args C,
                                                                                wf_buffers B,
                                                                                unsigned long long* counters) {
    constexpr unsigned CS = YRT_PRIMARY_BLOCK_CHUNK;
    constexpr int SPB = YRT_PRIMARY_SP_BLOCK;
    __shared__ chunk_ring ring;
    __shared__ dev_render_args A_lds;
    __shared__ chunk_args C_lds;
    __shared__ wf_buffers B_lds;
    __shared__ float4 lds_rec[LDSN > 0 ? LDSN * spine_record_f4 : 1];
    if constexpr (LDSN > 0) {
        // (the instance level may have fewer records: the walk never addresses past them)
        const int n = min(LDSN, S.ntnodes) * spine_record_f4;
        const float4* src = reinterpret_cast<const float4*>(B.trel);
        for (int i = (int)threadIdx.x; i < n; i += SPB) lds_rec[i] = src[i];
    }
    if (threadIdx.x == 0) A_lds = A, C_lds = C, B_lds = B;
    const unsigned lane = threadIdx.x & 63;
    const unsigned xcd = blockIdx.x % 8u;
    unsigned* counter = B.queue + 16 + xcd;
    unsigned* gcounter = B.queue + 24;
    const unsigned n_items = (unsigned)((C.npix * C.spp + 63) / 64);
    const unsigned head = head_items<YRT_XCD_CHUNK_PRIMARY, CS>(n_items);
    chunk_ring_init<CS>(ring, counter, gcounter, head / 8u);  // (its barrier also publishes the copies)
    tracer<false, false, true, SE, SPB> T;
    T.lane_stk = nullptr;
    work_counts wc;
    unsigned valid_n = 0;  // wave-uniform: camera samples of this wave
#ifdef YRT_TAIL_STATS
    const unsigned long long tail_t0 = __builtin_amdgcn_s_memrealtime();
    unsigned tail_items = 0;
#endif
    for (;;) {
        const unsigned q = chunk_ring_next<CS>(ring, counter, lane, gcounter, head / 8u);
        const unsigned it = split_item<YRT_XCD_CHUNK_PRIMARY>(q, xcd, n_items, head);
        if (it >= n_items) break;
#ifdef YRT_TAIL_STATS
        tail_items++;
#endif
        asm volatile("" ::: "memory");
        // (lane_now(), not `lane`: a lane index held across the walk would be spilled)
        const bool valid = primary_samples<false, true, SE, SPB, LDSN, LIST, YRT_FIRST_NESTED != 0>(S, A_lds, C_lds, B_lds, T,
                                                                            (int)(it * 64) + lane_now(), wc, lds_rec);
        valid_n += (unsigned)__popcll(ballot(valid));
    }
#ifdef YRT_TAIL_STATS
    tail_record(0, tail_t0, tail_items);
#endif
    const unsigned long long mine = lane == 0 ? (unsigned long long)valid_n : 0ull;
    flush_block<2, SPB>(counters, {cnt_rays, cnt_samples}, {mine, mine});
}

// ---- level 0 of a ray batch (yrt_shade_rays): the caller's rays instead of eval_camera ----
// Sample idx of the chunk is ray idx of B.rays, used as given: o, d (not renormalised), tmin and
// tmax all reach the closest-hit query, as shade() hands its ray to intersect_first
// (raytrace.cpp:91). The rays share no origin, so the walk is the mirror levels' generic one
// (k_bounce's: world-space records from the root, no camera-relative records, no camera lists),
// and the hit and surface records go where k_primary stores them. A partial block's idle lanes
// reach the walk as invalid lanes, as in k_bounce.
// The level-0 view point (raytrace.cpp:147,196: normalize(ray.o - p)) is re-read from B.rays by
// the kernels that need it (ray_origin): 12 of the 32 bytes k_rays_first has just streamed,
// against a per-sample origin record that would cost 16 B of workspace per sample and one more
// store here for the same loads there.
__device__ __forceinline__ vec3f ray_origin(const wf_buffers& B, int idx) {
    const float* r = B.rays + (size_t)idx * 8;
    return {r[0], r[1], r[2]};
}

template <bool PACKET, typename SE>
__global__ __launch_bounds__(WF_BLOCK, YRT_TRACE_WAVES) void k_rays_first(dev_scene_view S, int n, wf_buffers B,
                                                                          unsigned long long* counters) {
    __shared__ traversal_lds<PACKET, SE> lds;
    auto T = make_tracer<false, false, PACKET, SE>(lds);
    work_counts wc;
    const int idx = blockIdx.x * WF_BLOCK + threadIdx.x;
    const bool valid = idx < n;
    ray3 ray = {{0, 0, 0}, {0, 0, 1}, ray_eps, flt_max};
    if (valid) {
        const float* r = B.rays + (size_t)idx * 8;
        ray = {{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, r[6], r[7]};
    }
    hit_record hr = {-1, -1, {0, 0, 0, 0}, 0};
    const bool hit = T.trace(S, ray, valid, hr, wc);
    if (valid) store_hit_surface(S, B, idx, hit, hr);
    // one intersect_first and one level-0 shade() call per ray
    flush_block<2>(counters, {cnt_rays, cnt_samples}, {valid ? 1ull : 0ull, valid ? 1ull : 0ull});
}

// ---- levels >= 1: closest hit of the compacted mirror rays (grid-stride) ----
template <bool COUNT, bool PACKET, typename SE>
__global__ __launch_bounds__(WF_BLOCK, YRT_TRACE_WAVES) void k_bounce(dev_scene_view S, int level, wf_buffers B,
                                                     unsigned long long* counters) {
    __shared__ traversal_lds<PACKET, SE> lds;
    auto T = make_tracer<false, COUNT, PACKET, SE>(lds);
    work_counts wc;
    unsigned long long rays = 0;
    const int stride = gridDim.x * WF_BLOCK;
    for (int g = 0; g < level_segments; g++) {
    const int n = *seg_counter(B.count, level, g);
    const int nround = (n + stride - 1) / stride;  // uniform: every lane reaches the traversal
    for (int round = 0; round < nround; round++) {
        const int j = round * stride + blockIdx.x * WF_BLOCK + threadIdx.x;
        const bool valid = j < n;
        const int idx = g * B.seg + j;
        ray3 ray = {{0, 0, 0}, {0, 0, 1}, ray_eps, flt_max};
        if (valid) {
            float4 o = ld4(B.ray_o(level) + idx), d = ld4(B.ray_d(level) + idx);
            ray = {xyz(o), xyz(d), ray_eps, flt_max};
            rays++;
        }
        hit_record hr = {-1, -1, {0, 0, 0, 0}, 0};
        const bool hit = T.trace(S, ray, valid, hr, wc);
        if (valid) {
            if (COUNT && hit) wc.hits++;
            store_hit_surface(S, B, idx, hit, hr);
        }
    }
    }
    flush_block<1>(counters, {cnt_rays}, {rays});
    if (COUNT) flush_work(counters, wc);
}

// ---- shadow rays (raytrace.cpp:128-133): one light per blockIdx.y ----
// WIDE: the 4-wide any-hit walk (timed kernels on scenes whose wide stack fits);
// otherwise the tracer's binary walk (and always for the instrumented COUNT pass)
template <bool COUNT, bool PACKET, typename SE, bool WIDE>
__global__ __launch_bounds__(shadow_block<PACKET>(), YRT_SHADOW_WAVES) void k_shadow(dev_scene_view S, int level,
                                                                     int nsamp_level0, wf_buffers B,
                                                                     unsigned long long* counters, float4 cam4) {
    const vec3f cam_o = xyz(cam4);  // the camera rays' origin (level 0's view point)
    constexpr int BS = shadow_block<PACKET>();
    __shared__ traversal_lds<PACKET, SE> lds;
    auto T = make_tracer<true, COUNT, PACKET, SE>(lds);
    // level 0 (one block per 256 samples and light): the remap runs over the whole
    // (x, light) grid; levels >= 1 are grid-stride and keep their blocks
    // a pixel block's lights in neighbouring blocks (light index minor), dealt in XCD runs
    const unsigned lin = level ? blockIdx.x
                               : xcd_runs<YRT_SHADOW_LIGHT_MINOR>(blockIdx.y * gridDim.x + blockIdx.x,
                                                                  gridDim.x * gridDim.y);
    const int li = level ? (int)blockIdx.y : (int)(lin % gridDim.y);
    const int bx = level ? (int)blockIdx.x : (int)(lin / gridDim.y);
    const f4* lr = S.lights + 6 * li;
    const frame3f lf = {xyz(ld4(lr)), xyz(ld4(lr + 1)), xyz(ld4(lr + 2)), xyz(ld4(lr + 3))};
    const vec3f lp0 = xyz(ld4(lr + 4)), ke = xyz(ld4(lr + 5));
    work_counts wc;
    unsigned long long rays = 0, culled = 0;  // culled: counted in rays, answered without a walk
    const int stride = gridDim.x * BS;
    for (int g = 0; g < (level ? level_segments : 1); g++) {
    const int n = level ? *seg_counter(B.count, level, g) : nsamp_level0;
    const int nround = (n + stride - 1) / stride;
    for (int round = 0; round < nround; round++) {
        const int j = round * stride + bx * BS + threadIdx.x;
        const int idx = g * B.seg + j;
        bool valid = false;
        int info = -1;
        float r = 1.0f;
        float4 s1 = {0, 0, 0, 0}, ro4 = make_float4(cam_o.x, cam_o.y, cam_o.z, 0.0f);
        ray3 sr = {{0, 0, 0}, {0, 0, 1}, 0.01f, 1.0f};
        constexpr bool CULL = !COUNT;  // (the instrumented pass traces every ray)
        if (j < n) {
            float4 s0 = ld4s(B.surf0 + idx);
            if (CULL) {  // n and the view point, for light_term_zero
                s1 = ld4s(B.surf1 + idx);
                if (level) ro4 = ld4(B.ray_o(level) + idx);
            }
            info = sample_state(s0);
            if (info >= 0) {
                const vec3f p = xyz(s0);
                vec3f tp = transform_point(lf, lp0 - p);
                vec3f l;
                normalize_len(tp, l, r);
                sr = {p, l, 0.01f, r - 0.01f};
                valid = true;
                rays++;
            }
        }
        if (CULL) {  // (uniform control flow; a lane that is not a hit has info < 0)
            if (light_term_zero(info, xyz(s1), sr.o, xyz(ro4), sr.d, r, ke)) {
                stb(B.occl + (size_t)li * B.capacity + idx, 1);
                valid = false;
                culled++;
            }
        }
        hit_record hr;
        bool occ;
        if constexpr (WIDE)
            occ = packet_occluded_wide2(S, sr, valid);
        else
            occ = T.trace(S, sr, valid, hr, wc);
        if (valid) stb(B.occl + (size_t)li * B.capacity + idx, occ ? 1 : 0);
    }
    }
    // shadow rays are counted once, here; yrt_last_stats reports rays = cnt_rays + this
    flush_block<2, BS>(counters, {cnt_shadow_rays, cnt_shadow_culled}, {rays, culled});
    if (COUNT) {
        flush_work(counters, wc);
        flush(counters, cnt_shadow_box_tests, wc.box);
        flush(counters, cnt_shadow_inst_entries, wc.inst);
        flush(counters, cnt_shadow_prim_tests, wc.prim);
        flush(counters, cnt_shadow_wave_node_visits, wc.wnode);
    }
}

// level 0 of a ray batch (run_rays): k_shadow's level-0 work again -- the same grid (one block
// per BS samples and light, the light index minor, dealt in XCD runs), shadow ray, cull and walk
// -- with the view point of the zero-light-term cull taken per sample from the ray's own origin
// (ray_origin) instead of the camera's. A kernel of its own, not a flag of k_shadow: the
// render's kernels keep the code they have. Every lane of a partial block reaches the walk.
// (Not a device function shared with k_shadow, neither for the sample's body nor for the whole
// kernel body: either changes the instructions of every k_shadow, a timed kernel of the frame.)
template <bool PACKET, typename SE, bool WIDE>
__global__ __launch_bounds__(shadow_block<PACKET>(), YRT_SHADOW_WAVES) void k_rays_shadow(dev_scene_view S, int nsamp,
                                                                                          wf_buffers B,
                                                                                          unsigned long long* counters) {
    constexpr int BS = shadow_block<PACKET>();
    __shared__ traversal_lds<PACKET, SE> lds;
    auto T = make_tracer<true, false, PACKET, SE>(lds);
    const unsigned lin = xcd_runs<YRT_SHADOW_LIGHT_MINOR>(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
    const int li = (int)(lin % gridDim.y);
    const int idx = (int)(lin / gridDim.y) * BS + (int)threadIdx.x;
    const f4* lr = S.lights + 6 * li;
    const frame3f lf = {xyz(ld4(lr)), xyz(ld4(lr + 1)), xyz(ld4(lr + 2)), xyz(ld4(lr + 3))};
    const vec3f lp0 = xyz(ld4(lr + 4)), ke = xyz(ld4(lr + 5));
    work_counts wc;
    unsigned long long rays = 0, culled = 0;  // culled: counted in rays, answered without a walk
    bool valid = false;
    int info = -1;
    float r = 1.0f;
    float4 s1 = {0, 0, 0, 0};
    vec3f ro = {0, 0, 0};
    ray3 sr = {{0, 0, 0}, {0, 0, 1}, 0.01f, 1.0f};
    if (idx < nsamp) {
        float4 s0 = ld4s(B.surf0 + idx);
        s1 = ld4s(B.surf1 + idx);  // n and the view point, for light_term_zero
        ro = ray_origin(B, idx);
        info = sample_state(s0);
        if (info >= 0) {
            const vec3f p = xyz(s0);
            vec3f tp = transform_point(lf, lp0 - p);
            vec3f l;
            normalize_len(tp, l, r);
            sr = {p, l, 0.01f, r - 0.01f};
            valid = true;
            rays++;
        }
    }
    // (uniform control flow; a lane that is not a hit has info < 0)
    if (light_term_zero(info, xyz(s1), sr.o, ro, sr.d, r, ke)) {
        stb(B.occl + (size_t)li * B.capacity + idx, 1);
        valid = false;
        culled++;
    }
    hit_record hr;
    bool occ;
    if constexpr (WIDE)
        occ = packet_occluded_wide2(S, sr, valid);
    else
        occ = T.trace(S, sr, valid, hr, wc);
    if (valid) stb(B.occl + (size_t)li * B.capacity + idx, occ ? 1 : 0);
    flush_block<2, BS>(counters, {cnt_shadow_rays, cnt_shadow_culled}, {rays, culled});
}

// ---- soft shadows (yrt_shade_rays_soft, yrt_render_soft_shadows): K any-hit rays per light ----
// Every level of a soft ray batch (run_rays with soft_shadow_args). Light li is a disk of radius
// radius[li] about its point, facing the shading point; a sample that hit casts K rays from its
// hit point at the disk's points soft_shadow_rays.h gives (the text the host twin
// tools/check_soft_shadow_rays.cpp evaluates), and the byte of (light, sample) in the occlusion
// slab receives the number of unoccluded ones, 0..K, instead of k_shadow's flag. A light of radius
// 0 casts the hard shadow ray itself -- no basis, no offset -- and records K or 0.
// Level 0 has k_rays_shadow's grid (one block per BS samples and light, the light index minor,
// dealt in XCD runs) and takes the view point of the zero-term cull from the ray's own origin;
// levels >= 1 have k_shadow's grid-stride form over the level's segments and take it from the
// mirror ray's record. K and the light's radius are the same in every lane: the loop over k is a
// scalar loop and dirs[k] a scalar load (k_ao's), and a wave's 64 rays of one k start at
// neighbouring hit points and aim at one neighbourhood of the disk, so they walk together.
// Every lane of a partial wave reaches every walk (valid = false).
// What stays live across the K walks: p, tp, the two tangents, the rotation and the count -- 17
// VGPRs beside the walk's own.
__constant__ float soft_dirs[ao_dir_count * 3] = {YRT_AO_DIRS};
__constant__ float soft_rots[ao_rot_count * 2] = {YRT_AO_ROTS};

// Six waves per SIMD (80 VGPRs) where k_shadow has eight (64): at 64 the wide walk's own registers
// leave no room for the 17 and the kernel spilled 9 VGPRs to scratch; at 80 it takes 68 and spills
// none. The per-lane walk (YRT_ALGO_WAVEFRONT_LANE) needs 110: four waves (128).
template <bool PACKET>
constexpr int soft_shadow_waves() { return PACKET ? 6 : 4; }
template <bool PACKET, typename SE, bool WIDE>
__global__ __launch_bounds__(shadow_block<PACKET>(), soft_shadow_waves<PACKET>()) void k_soft_shadow(
    dev_scene_view S, int level, int nsamp_level0, wf_buffers B, unsigned long long* counters, int K,
    const float* __restrict__ radius) {
    constexpr int BS = shadow_block<PACKET>();
    __shared__ traversal_lds<PACKET, SE> lds;
    auto T = make_tracer<true, false, PACKET, SE>(lds);
    const unsigned lin = level ? blockIdx.x
                               : xcd_runs<YRT_SHADOW_LIGHT_MINOR>(blockIdx.y * gridDim.x + blockIdx.x,
                                                                  gridDim.x * gridDim.y);
    const int li = level ? (int)blockIdx.y : (int)(lin % gridDim.y);
    const int bx = level ? (int)blockIdx.x : (int)(lin / gridDim.y);
    const f4* lr = S.lights + 6 * li;
    const frame3f lf = {xyz(ld4(lr)), xyz(ld4(lr + 1)), xyz(ld4(lr + 2)), xyz(ld4(lr + 3))};
    const vec3f lp0 = xyz(ld4(lr + 4)), ke = xyz(ld4(lr + 5));
    const float R = radius[li];
    const bool hard = R == 0.0f;
    const unsigned long long per_pair = hard ? 1ull : (unsigned long long)K;  // rays a (hit sample, light) pair counts
    work_counts wc;
    unsigned long long rays = 0, culled = 0;  // culled: counted in rays, answered without a walk
    const int stride = gridDim.x * BS;
    for (int g = 0; g < (level ? level_segments : 1); g++) {
    const int n = level ? *seg_counter(B.count, level, g) : nsamp_level0;
    const int nround = (n + stride - 1) / stride;
    for (int round = 0; round < nround; round++) {
        const int j = round * stride + bx * BS + (int)threadIdx.x;
        const int idx = g * B.seg + j;
        bool valid = false;
        int info = -1;
        float r = 1.0f;
        float4 s1 = {0, 0, 0, 0};
        vec3f ro = {0, 0, 0}, p = {0, 0, 0}, tp = {0, 0, 1}, l = {0, 0, 1};
        if (j < n) {
            const float4 s0 = ld4s(B.surf0 + idx);
            s1 = ld4s(B.surf1 + idx);  // n and the view point, for light_term_zero
            ro = level ? xyz(ld4(B.ray_o(level) + idx)) : ray_origin(B, idx);
            info = sample_state(s0);
            if (info >= 0) {
                p = xyz(s0);
                tp = transform_point(lf, lp0 - p);
                normalize_len(tp, l, r);
                valid = true;
                rays += per_pair;
            }
        }
        // (uniform control flow; a lane that is not a hit has info < 0)
        if (light_term_zero(info, xyz(s1), p, ro, l, r, ke)) {
            stb(B.occl + (size_t)li * B.capacity + idx, 0);
            valid = false;
            culled += per_pair;
        }
        hit_record hr;
        int open = 0;
        if (hard) {  // (uniform over the block) the hard shadow ray, bit for bit
            const ray3 sr = {p, l, 0.01f, r - 0.01f};
            bool occ;
            if constexpr (WIDE)
                occ = packet_occluded_wide2(S, sr, valid);
            else
                occ = T.trace(S, sr, valid, hr, wc);
            open = occ ? 0 : K;
        } else {
            const int rot = soft_shadow_rot(p, li);
            const float c = soft_rots[2 * rot], sn = soft_rots[2 * rot + 1];
            vec3f b1, b2;
            soft_shadow_basis(l, b1, b2);
            for (int k = 0; k < K; k++) {
                const vec3f tq = soft_shadow_target(tp, b1, b2, c, sn, soft_dirs, k, R);
                vec3f lq;
                float rq;
                normalize_len(tq, lq, rq);
                const ray3 sr = {p, lq, 0.01f, rq - 0.01f};
                bool occ;
                if constexpr (WIDE)
                    occ = packet_occluded_wide2(S, sr, valid);
                else
                    occ = T.trace(S, sr, valid, hr, wc);
                open += valid && !occ ? 1 : 0;
            }
        }
        if (valid) stb(B.occl + (size_t)li * B.capacity + idx, (unsigned char)open);
    }
    }
    flush_block<2, BS>(counters, {cnt_shadow_rays, cnt_shadow_culled}, {rays, culled});
}

// The hull of box P = [P0, P1] and the point Lp, as the 16 lanes of a slot group hold it:
// lane j = lane % 16, j == 0 the hull's box (P's box with Lp), j = 1..12 the plane through
// Lp and box edge j - 1 of P when that edge is on P's silhouette seen from Lp (one adjacent
// face turned towards Lp, the other away). A box is dropped only when some lane finds it
// entirely outside its plane by more than the margin -- a conservative test (the hull's
// other separating axes are not tried); every plane bounds the hull, so a hull holding more
// rays (a super-bundle's) keeps everything a smaller one does.
struct hull_t {
    float bxl, bxh, byl, byh, bzl, bzh;   // j == 0
    float nx, ny, nz, nd, nmargin;        // j >= 1 (nmargin infinite: no plane)
    int j;
};
__device__ __forceinline__ hull_t make_hull(float plx, float ply, float plz, float phx, float phy, float phz, vec3f Lp,
                                            int lane) {
    hull_t H;
    const float M = fmaxf(fmaxf(fmaxf(fabsf(plx), fabsf(ply)), fmaxf(fabsf(plz), fabsf(phx))),
                          fmaxf(fmaxf(fabsf(phy), fabsf(phz)), fmaxf(fmaxf(fabsf(Lp.x), fabsf(Lp.y)), fabsf(Lp.z))));
    const float eps = 1e-3f + 3e-5f * M;
    H.j = lane & 15;
    const float P0[3] = {plx, ply, plz}, P1[3] = {phx, phy, phz}, L3[3] = {Lp.x, Lp.y, Lp.z};
    H.bxl = fminf(plx, Lp.x) - eps, H.bxh = fmaxf(phx, Lp.x) + eps;
    H.byl = fminf(ply, Lp.y) - eps, H.byh = fmaxf(phy, Lp.y) + eps;
    H.bzl = fminf(plz, Lp.z) - eps, H.bzh = fmaxf(phz, Lp.z) + eps;
    H.nx = 0.0f, H.ny = 0.0f, H.nz = 0.0f, H.nd = 0.0f, H.nmargin = INFINITY;
    if (H.j >= 1 && H.j <= 12) {
        const int e = H.j - 1, a = e >> 2, b = (a + 1) % 3, c = (a + 2) % 3;
        const bool bh = e & 1, ch = (e >> 1) & 1;  // the edge's sides on axes b and c
        // a face faces Lp when Lp lies strictly outside the box on that face's side
        const bool fb = bh ? L3[b] > P1[b] : L3[b] < P0[b];
        const bool fc = ch ? L3[c] > P1[c] : L3[c] < P0[c];
        if (fb != fc) {
            float e0[3], e1[3];
            e0[a] = P0[a], e1[a] = P1[a];
            e0[b] = e1[b] = bh ? P1[b] : P0[b];
            e0[c] = e1[c] = ch ? P1[c] : P0[c];
            const float ux = e1[0] - e0[0], uy = e1[1] - e0[1], uz = e1[2] - e0[2];
            const float vx = L3[0] - e0[0], vy = L3[1] - e0[1], vz = L3[2] - e0[2];
            float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            // the box centre on the inner (negative) side
            const float cx = 0.5f * (P0[0] + P1[0]) - e0[0], cy = 0.5f * (P0[1] + P1[1]) - e0[1],
                        cz = 0.5f * (P0[2] + P1[2]) - e0[2];
            if (nx * cx + ny * cy + nz * cz > 0.0f) nx = -nx, ny = -ny, nz = -nz;
            H.nx = nx, H.ny = ny, H.nz = nz;
            H.nd = nx * e0[0] + ny * e0[1] + nz * e0[2];
            H.nmargin = (fabsf(nx) + fabsf(ny) + fabsf(nz)) * (eps + 1e-5f * M);
        }
    }
    return H;
}
// this lane's plane has the box entirely outside (a NaN bound never separates: the
// reference's select-based slab test can pass a box with a NaN plane)
__device__ __forceinline__ bool hull_sep(const hull_t& H, float clx, float cly, float clz, float chx, float chy,
                                         float chz) {
    if (H.j == 0) return clx > H.bxh || chx < H.bxl || cly > H.byh || chy < H.byl || clz > H.bzh || chz < H.bzl;
    const float mn = H.nx * (H.nx > 0.0f ? clx : chx) + H.ny * (H.ny > 0.0f ? cly : chy) +
                     H.nz * (H.nz > 0.0f ? clz : chz);
    return mn - H.nd > H.nmargin;
}
// the instance-level leaves the hull does not exclude, from a walk of the any-hit tree (lane
// 16 s + j tests slot s of the current wide record against plane j; a lane-indexed stack):
// up to CAP of them into cand (lane 0 writes), else overflow
// only_slot >= 0: of the root record, only that slot's subtree (k_bundle_lists<FUSED> splits a
// super-bundle's walk over a block's four waves by root slot)
template <int CAP>
__device__ __forceinline__ void hull_walk(const dev_scene_view& S, const hull_t& H, int lane, float (*cand)[8], int& nc,
                                          bool& overflow, int only_slot = -1) {
    const int s = lane >> 4;  // the slot this lane tests
    const f4* wbase = sgpr_ptr(S.wnodes);
    int stk = 0, sp = 0;
    nc = 0, overflow = false;
    uint32_t cur = (uint32_t)S.wtop_root;
    bool root = true;
    for (;;) {
        float4 r[7];
        ld_wide_record(wbase, cur, r);
        const float4 rs[7] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
        auto comp = [&](float4 v) { return s == 0 ? v.x : s == 1 ? v.y : s == 2 ? v.z : v.w; };
        const bool sep = hull_sep(H, comp(rs[0]), comp(rs[1]), comp(rs[2]), comp(rs[3]), comp(rs[4]), comp(rs[5]));
        const unsigned long long sm = ballot(sep);
        unsigned long long m = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t wq = ubits(q == 0 ? r[6].x : q == 1 ? r[6].y : q == 2 ? r[6].z : r[6].w);
            if (wq != wide_leaf && !((sm >> (16 * q)) & 0xffffull)) m |= 0xffffull << (16 * q);
        }
        if (root && only_slot >= 0) m &= 0xffffull << (16 * only_slot);
        root = false;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (!((m >> (16 * q)) & 0xffffull)) continue;
            const uint32_t word = ubits(q == 0 ? r[6].x : q == 1 ? r[6].y : q == 2 ? r[6].z : r[6].w);
            if (word & wide_leaf) {
                if (nc == CAP) {
                    overflow = true;
                    continue;
                }
                if (lane == 0) {
                    float* e = cand[nc];
                    e[0] = q == 0 ? r[0].x : q == 1 ? r[0].y : q == 2 ? r[0].z : r[0].w;
                    e[1] = q == 0 ? r[1].x : q == 1 ? r[1].y : q == 2 ? r[1].z : r[1].w;
                    e[2] = q == 0 ? r[2].x : q == 1 ? r[2].y : q == 2 ? r[2].z : r[2].w;
                    e[3] = q == 0 ? r[3].x : q == 1 ? r[3].y : q == 2 ? r[3].z : r[3].w;
                    e[4] = q == 0 ? r[4].x : q == 1 ? r[4].y : q == 2 ? r[4].z : r[4].w;
                    e[5] = q == 0 ? r[5].x : q == 1 ? r[5].y : q == 2 ? r[5].z : r[5].w;
                    e[6] = __uint_as_float(word);
                }
                nc++;
            } else {
                stk = writelane(stk, (int)word, sp);
                sp++;
            }
        }
        if (overflow || sp == 0) break;
        sp--;
        cur = (uint32_t)__builtin_amdgcn_readlane(stk, sp);
    }
}

// the box of the hit points of items [i0, i0 + n) (n <= 4 * 64: each lane takes up to four),
// whether any is not finite, and the light's position if its frame is the identity
__device__ __forceinline__ void bundle_box(const wf_buffers& B, int i0, int n, int n_items, int lane, float& plx,
                                           float& ply, float& plz, float& phx, float& phy, float& phz, bool& bad) {
    plx = ply = plz = INFINITY, phx = phy = phz = -INFINITY;
    bad = false;
    for (int k = 0; k < 4; k++) {
        const int o = k * 64 + lane, it = i0 + o;
        if (o < n && it < n_items) {
            const float4 a = ld4(B.pbox + 2 * it), b = ld4(B.pbox + 2 * it + 1);
            plx = fminf(plx, a.x), ply = fminf(ply, a.y), plz = fminf(plz, a.z);
            phx = fmaxf(phx, b.x), phy = fmaxf(phy, b.y), phz = fmaxf(phz, b.z);
            bad = bad || a.w < 0.0f;
        }
    }
    float lo[3] = {plx, ply, plz}, hi[3] = {phx, phy, phz};
    wave_box(lo, hi);
    plx = lo[0], ply = lo[1], plz = lo[2], phx = hi[0], phy = hi[1], phz = hi[2];
}
__device__ __forceinline__ bool light_position(const dev_scene_view& S, int li, vec3f& Lp) {
    float4 lrec[5];
    ld_records_at<5>(S.lights, (unsigned)(6 * li), lrec);
    const bool ident = ubits(lrec[0].x) == 0x3f800000u && ubits(lrec[0].y) == 0 && ubits(lrec[0].z) == 0 &&
                       ubits(lrec[1].x) == 0 && ubits(lrec[1].y) == 0x3f800000u && ubits(lrec[1].z) == 0 &&
                       ubits(lrec[2].x) == 0 && ubits(lrec[2].y) == 0 && ubits(lrec[2].z) == 0x3f800000u;
    Lp = xyz(lrec[4]) + xyz(lrec[3]);
    return ident && __builtin_isfinite(Lp.x) && __builtin_isfinite(Lp.y) && __builtin_isfinite(Lp.z);
}

#ifdef YRT_LIST_TIMING
// diagnostic build only (tools/list_timing.py): per wave of the list builders, phase times
// on the 100 MHz constant clock and a size (vector stores by lane 0)
static __device__ unsigned long long g_list_time[3][65536][4];
#define YRT_LT_STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memrealtime()
#define YRT_LT_WRITE(k, i, a, b, c, d)                                                          \
    do {                                                                                        \
        if (lane == 0 && (unsigned)(i) < 65536u) {                                              \
            unsigned long long* e_ = g_list_time[k][i];                                         \
            e_[0] = (a), e_[1] = (b), e_[2] = (c), e_[3] = (d);                                 \
        }                                                                                       \
    } while (0)
#else
#define YRT_LT_STAMP(v)
#define YRT_LT_WRITE(k, i, a, b, c, d)
#endif

// Two-level build: one tree walk per (super-bundle of 4 consecutive bundles, light) into a
// list of up to super_max leaves (k_bundle_super), which each bundle then filters with its own
// planes instead of walking the tree (a super list that overflows: the bundles walk). A/B in
// one process (profiles/r4/ab_bundle_super): the lists phase at c4 0.28 -> 0.24 ms, c5 rank 0
// of 8 0.82 -> 0.67 ms; identical images
#ifndef YRT_BUNDLE_FUSED
// the super lists and the bundle lists in one launch (k_bundle_lists<true>). A/B in one process
// (profiles/r6/ab/r6e_*): lists phase c4 0.31 -> 0.37 ms, instance100k 0.47 -> 0.60, c5 rank 0
// of 8 0.82 -> 1.00, rank 0 of 8 0.10 -> 0.09; the block's four waves wait at its barrier for
// the longest root slot's walk. Off.
// (Kept although nothing launches it: run() names k_bundle_lists<true> in a plain `if`, so the
// default build still instantiates it, and with that second caller of hull_walk<super_max>
// passing a variable only_slot the compiler peels the walk's first iteration in k_bundle_super
// too. Without the instantiation k_bundle_super comes out as another kernel, 890 instructions
// for 1147; no other kernel changes. Taking the switch out is a change of a timed kernel, to
// be measured on its own.)
#define YRT_BUNDLE_FUSED 0
#endif
// (super_bundles, super_max, super_list_f4: wf_workspace.h)

// one wave per (super-bundle, light): its list at B.slists
__global__ __launch_bounds__(256) void k_bundle_super(dev_scene_view S, wf_buffers B, int n_items) {
    __shared__ float cand[4][super_max][8];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nl = S.nlights;
    const int nsuper = (n_items + super_bundles * bundle_g - 1) / (super_bundles * bundle_g);
    const int sl = blockIdx.x * 4 + w;
    if (sl >= nsuper * nl) return;  // (whole waves)
    YRT_LT_STAMP(lt0);
    const int sg = sl / nl, li = sl - sg * nl;
    f4* out = B.slists + (size_t)sl * super_list_f4;
    float plx, ply, plz, phx, phy, phz;
    bool bad;
    bundle_box(B, sg * super_bundles * bundle_g, super_bundles * bundle_g, n_items, lane, plx, ply, plz, phx, phy, phz,
               bad);
    vec3f Lp;
    const bool lok = light_position(S, li, Lp);
    int nc = -1;
    YRT_LT_STAMP(lt1);
    if (!ballot(bad) && lok) {
        if (!(plx <= phx)) {
            nc = 0;
        } else {
            const hull_t H = make_hull(plx, ply, plz, phx, phy, phz, Lp, lane);
            bool overflow;
            hull_walk<super_max>(S, H, lane, cand[w], nc, overflow);
            if (overflow) nc = -1;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // lane 0's candidate stores
    if (lane < 2 * max(nc, 0)) {
        const float* e = cand[w][lane >> 1];
        reinterpret_cast<float4*>(out)[1 + lane] =
            (lane & 1) ? float4{e[3], e[4], e[5], 0.0f} : float4{e[0], e[1], e[2], e[6]};
    }
    if (lane == 0) reinterpret_cast<float4*>(out)[0] = float4{__int_as_float(nc), 0.0f, 0.0f, 0.0f};
    YRT_LT_STAMP(lt2);
    YRT_LT_WRITE(1, sl, lt1 - lt0, lt2 - lt1, 0ull, (unsigned long long)(unsigned)nc);
}

// one wave per (bundle, light): the candidate list (see above) -- from the super-bundle's
// list, or a walk of the tree where that list overflowed -- as a chain of wide records.
// FUSED (YRT_BUNDLE_FUSED): one block per (super-bundle, light), wave w its bundle w, and the
// super-bundle's list is built in the same launch: the four waves write their bundles' boxes to
// LDS, each walks one root slot's subtree with the super-bundle's hull (the union box), and the
// four shares, in slot order, are the super list every wave then filters -- k_bundle_super's
// list, one launch and one wave's walk fewer
template <bool FUSED>
__global__ __launch_bounds__(256) void k_bundle_lists(dev_scene_view S, wf_buffers B, int n_items) {
    __shared__ float cand[4][bundle_max][8];  // per wave: lo.xyz, hi.xyz, word
    __shared__ float scand[FUSED ? 4 : 1][super_max][8];  // FUSED: root slot w's share of the super list
    __shared__ float sbox[FUSED ? 4 : 1][8];             // FUSED: bundle w's box, and whether it is bad
    __shared__ int scount[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nl = S.nlights;
    const int ngroups = (n_items + bundle_g - 1) / bundle_g;
    int g, li;
    if constexpr (FUSED) {
        const int nsuper = (ngroups + super_bundles - 1) / super_bundles;
        if ((int)blockIdx.x >= nsuper * nl) return;  // (whole blocks)
        const int sg = (int)blockIdx.x / nl;
        li = (int)blockIdx.x - sg * nl, g = sg * super_bundles + w;
    } else {
        const int gl0 = blockIdx.x * 4 + w;
        if (gl0 >= ngroups * nl) return;  // (whole waves)
        g = gl0 / nl, li = gl0 - g * nl;
    }
    const int gl = g * nl + li;
    YRT_LT_STAMP(lt0);
    float plx, ply, plz, phx, phy, phz;
    bool bad;
    // (a bundle past the last, FUSED's padding: no items, an empty box)
    bundle_box(B, g * bundle_g, bundle_g, n_items, lane, plx, ply, plz, phx, phy, phz, bad);
    int sc = -1;  // the super-bundle's list length, -1: walk the tree
    const f4* sup = nullptr;
    if constexpr (FUSED) {
        const bool wbad = ballot(bad) != 0;
        if (lane == 0) {
            float* b = sbox[w];
            b[0] = plx, b[1] = ply, b[2] = plz, b[3] = phx, b[4] = phy, b[5] = phz, b[6] = wbad ? 1.0f : 0.0f;
        }
        __syncthreads();
        // the super-bundle's box: the union of its bundles' (bundle_box's fminf / fmaxf fold)
        float Plx = INFINITY, Ply = INFINITY, Plz = INFINITY, Phx = -INFINITY, Phy = -INFINITY, Phz = -INFINITY;
        bool sbad = false;
        for (int q = 0; q < super_bundles; q++) {
            const float* b = sbox[q];
            Plx = fminf(Plx, b[0]), Ply = fminf(Ply, b[1]), Plz = fminf(Plz, b[2]);
            Phx = fmaxf(Phx, b[3]), Phy = fmaxf(Phy, b[4]), Phz = fmaxf(Phz, b[5]);
            sbad = sbad || b[6] != 0.0f;
        }
        vec3f Ls;
        const bool lok = light_position(S, li, Ls);
        int nq = -1;
        if (!sbad && lok) {
            if (!(Plx <= Phx)) {
                nq = 0;
            } else {
                const hull_t Hs = make_hull(Plx, Ply, Plz, Phx, Phy, Phz, Ls, lane);
                bool of;
                hull_walk<super_max>(S, Hs, lane, scand[w], nq, of, w);
                if (of) nq = -1;
            }
        }
        if (lane == 0) scount[w] = nq;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // lane 0's candidate stores
        __syncthreads();
        const int c0 = scount[0], c1 = scount[1], c2 = scount[2], c3 = scount[3];
        sc = (c0 < 0 || c1 < 0 || c2 < 0 || c3 < 0 || c0 + c1 + c2 + c3 > super_max) ? -1 : c0 + c1 + c2 + c3;
        if (g >= ngroups) return;  // (after the block's barriers)
    }
    vec3f Lp;
    if (ballot(bad) || !light_position(S, li, Lp)) {
        if (lane == 0) B.lcount[gl] = -1, B.lskip[gl] = 0;
        return;
    }
    if (!(plx <= phx)) {  // no hit point in the bundle: no shadow ray
        if (lane == 0) B.lcount[gl] = 0, B.lskip[gl] = 0;
        return;
    }
    const hull_t H = make_hull(plx, ply, plz, phx, phy, phz, Lp, lane);
    int nc = 0;
    bool overflow = false;
    if (!FUSED) {
        sup = B.slists + (size_t)((g / super_bundles) * nl + li) * super_list_f4;
        sc = __builtin_amdgcn_readfirstlane(__float_as_int(ld4(sup).x));
    }
    if (sc >= 0) {
        // the super list's leaves that this bundle's own planes do not exclude: lane 16 s + j
        // tests leaf c0 + s against plane j, four leaves a pass
        for (int c0 = 0; c0 < sc && !overflow; c0 += 4) {
            const int e = c0 + (lane >> 4);
            float4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
            if (e < sc) {
                if constexpr (FUSED) {  // entry e of the four shares, in slot order
                    int q = 0, k = e;
                    while (k >= scount[q]) k -= scount[q], q++;
                    const float* d = scand[q][k];
                    a = {d[0], d[1], d[2], d[6]}, b = {d[3], d[4], d[5], 0.0f};
                } else {
                    a = ld4(sup + 1 + 2 * e), b = ld4(sup + 2 + 2 * e);
                }
            }
            const bool sep = e >= sc || hull_sep(H, a.x, a.y, a.z, b.x, b.y, b.z);
            const unsigned long long sm = ballot(sep);
            unsigned keep = 0;  // bit q: leaf c0 + q stays
            for (int q = 0; q < 4; q++) keep |= ((sm >> (16 * q)) & 0xffffull) ? 0u : 1u << q;
            const int k = __popc(keep);
            if (nc + k > bundle_max) {
                overflow = true;
                break;
            }
            const int q = lane >> 4;
            if ((lane & 15) == 0 && ((keep >> q) & 1u)) {
                float* d = cand[w][nc + __popc(keep & ((1u << q) - 1u))];
                d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = b.x, d[4] = b.y, d[5] = b.z, d[6] = a.w;
            }
            nc += k;
        }
    } else {
        hull_walk<bundle_max>(S, H, lane, cand[w], nc, overflow);
    }
    if (overflow) {
        if (lane == 0) B.lcount[gl] = -1, B.lskip[gl] = 0;
        return;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the candidate stores, before any lane reads them
    YRT_LT_STAMP(lt1);
    if (nc > 1) {
        // the leaves in the order the bundle's rays meet them, from the light towards the hit
        // points (box centres projected on that direction), so that the chain's later records
        // are compact boxes the rays can pass by and an occluded bundle meets its occluder
        // sooner. The any-hit answer does not depend on the order. A/B in one process
        // (profiles/r4/ab_bundle_sort), tree order -> from the hit points / from the light: c4
        // shadow 11.82 -> 11.72 / 11.62 ms, instance1k 7.42 -> 7.30 / 7.39, instance100k (lists
        // off) unchanged; the leaf that holds the hit points' centre last: 11.71 / 7.39
        const float cx = 0.5f * (plx + phx), cy = 0.5f * (ply + phy), cz = 0.5f * (plz + phz);
        const float dx = Lp.x - cx, dy = Lp.y - cy, dz = Lp.z - cz;
        float e[7] = {};
        float key = INFINITY;
        if (lane < nc) {
            for (int q = 0; q < 7; q++) e[q] = cand[w][lane][q];
            key = -((0.5f * (e[0] + e[3]) - cx) * dx + (0.5f * (e[1] + e[4]) - cy) * dy + (0.5f * (e[2] + e[5]) - cz) * dz);
            if (!(key == key)) key = INFINITY;  // (a NaN bound: last)
        }
        int rank = 0;  // a permutation of 0 .. nc - 1: ties go by index
        for (int j = 0; j < nc; j++) {
            const float kj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(key), j));
            rank += (kj < key || (kj == key && j < (int)lane)) ? 1 : 0;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every lane's reads, before the writes
        if (lane < nc)
            for (int q = 0; q < 7; q++) cand[w][rank][q] = e[q];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    // the instances of each listed leaf that the hull excludes: their world boxes
    // (dev_scene_view ibox) outside a hull plane by more than the margin fail every ray's
    // root box test in the instance's space, so the walk skips them (skip bits in the leaf's
    // word: the bundle records' format, bundle_leaf_word)
    int nskip = 0;  // (wave-uniform) instances the hull excludes, over the listed leaves
    if (S.inst_masks) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int e = 0; e < nc; e++) {
            const uint32_t wu = (uint32_t)__builtin_amdgcn_readfirstlane(__float_as_int(cand[w][e][6]));
            const int first = (int)(wu & wide_index_mask), count = (int)((wu >> wide_count_shift) & 7u);
            uint32_t skip = 0;
            for (int i0 = 0; count > 1 && i0 < count; i0 += 4) {
                const int i = i0 + (lane >> 4);  // lane 16 s + j: instance i0 + s against plane j
                bool sep = false;
                if (i < count) {
                    const float4 a = ld4(S.ibox + 2 * (first + i)), b = ld4(S.ibox + 2 * (first + i) + 1);
                    sep = hull_sep(H, a.x, a.y, a.z, b.x, b.y, b.z);
                }
                const unsigned long long sm = ballot(sep);
                for (int q = 0; q < 4; q++)
                    if (i0 + q < count && ((sm >> (16 * q)) & 0xffffull)) skip |= 1u << (i0 + q);
            }
            if (lane == 0) cand[w][e][6] = __uint_as_float(bundle_leaf_word(first, count, skip));
            nskip += __popc(skip);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // a leaf whose every instance is excluded leaves the list (the walk would test its box
        // and enter nothing); the others keep their order
        float e[7] = {};
        bool keep = false;
        if (lane < nc) {
            for (int q = 0; q < 7; q++) e[q] = cand[w][lane][q];
            const uint32_t wu = ubits(e[6]);
            const int count = (int)((wu >> wide_count_shift) & 7u);
            const uint32_t all = (1u << count) - 1u;
            keep = count == 0 || ((wu >> bundle_skip_shift) & 0x7fu) != all;
        }
        const unsigned long long km = ballot(keep);
        const int pos = __popcll(km & ((1ull << lane) - 1ull));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every lane's reads, before the writes
        if (keep)
            for (int q = 0; q < 7; q++) cand[w][pos][q] = e[q];
        nc = __popcll(km);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    YRT_LT_STAMP(lt2);
    // the list as wide records at B.lists + gl * bundle_recs: up to 4 leaves in the root;
    // more in up to 4 child records of 4, the root's slot c holding child c's box (the union
    // of its leaves' boxes) and its byte offset from B.lists
    // a chain: record r holds leaves 3r, 3r + 1, 3r + 2 and, in slot 3, record r + 1 (its box
    // the union of every leaf after them) -- the last record holds the last <= 4 leaves
    const int nrec = nc <= 4 ? 1 : 1 + (nc - 4 + 2) / 3;
    const uint32_t rec0 = (uint32_t)gl * bundle_recs;
    // lane q (< nrec * 4) builds slot q % 4 of record q / 4 -- then lanes write the rows
    __shared__ float slot[4][bundle_recs * 4][8];
    if (lane < nrec * 4) {
        const int rq = lane / 4, c = lane % 4;
        float v[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, __uint_as_float(wide_leaf)};
        if (rq == nrec - 1 || c < 3) {  // a leaf
            const int e = 3 * rq + c;
            if (e < nc)
                for (int q = 0; q < 7; q++) v[q] = cand[w][e][q];
        } else {  // the rest of the chain
            // the union of the later leaves' boxes, a NaN bound sticking: the walk's slab test
            // ignores a NaN plane, so a leaf with one passes more rays than its finite bounds
            // say, and the chain box must let all of those through too (fminf / fmaxf alone
            // would drop the NaN and could narrow the box below that leaf's reach)
            for (int e = 3 * rq + 3; e < nc; e++)
                for (int q = 0; q < 3; q++) {
                    const float lo = cand[w][e][q], hi = cand[w][e][q + 3];
                    v[q] = (lo != lo || v[q] != v[q]) ? __builtin_nanf("") : fminf(v[q], lo);
                    v[q + 3] = (hi != hi || v[q + 3] != v[q + 3]) ? __builtin_nanf("") : fmaxf(v[q + 3], hi);
                }
            v[6] = __uint_as_float((rec0 + rq + 1) * (uint32_t)wide_record_bytes);
        }
        for (int q = 0; q < 7; q++) slot[w][lane][q] = v[q];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane < nrec * 8) {
        const int rq = lane / 8, row = lane % 8;
        const float* a = slot[w][4 * rq];
        float4 o = row < 7 ? make_float4(a[row], a[8 + row], a[16 + row], a[24 + row]) : make_float4(0, 0, 0, 0);
        reinterpret_cast<float4*>(B.lists)[(size_t)(rec0 + rq) * 8 + row] = o;
    }
    if (lane == 0) B.lcount[gl] = nc, B.lskip[gl] = nskip;
    YRT_LT_STAMP(lt3);
    YRT_LT_WRITE(2, gl, lt1 - lt0, lt2 - lt1, lt3 - lt2, (unsigned long long)(unsigned)nc);
}

// ---- camera lists: per 8x8-pixel tile of the chunk, a frontier of the reference's instance
// tree for packet_first's list mode. The tile's rays start at the camera origin O and run
// through its pixels' rectangle [i0, i1 + 1] x [j0, j1 + 1] of the image plane (the samples lie
// strictly inside it, raytrace.cpp:236-239), so they lie in the cone from O through the
// rectangle's four corners; a box that lies outside a cone plane by more than a margin above
// the slab test's rounding fails every such ray's exact test (intersect_check_bbox,
// scene.cpp:371-382) at any tmax.
//
// The list is a frontier: disjoint subtrees of the reference's tree (inner nodes or leaves)
// that together hold every leaf the cone reaches, in the reference's DFS order (child start+1
// before start, scene.cpp:446-479). One wave per tile grows it from the root, a round per tree
// level, lane q holding entry q: an inner entry whose children the cone reaches one or none of
// is replaced by that child (or dropped) -- that never lengthens the list --, and one whose
// children both stay is replaced by them while the list has room (camera_list_max entries, the
// earlier entries first), so a small frontier ends as the tile's leaf list and a large one
// keeps subtrees where the cone splits. Entries are the first 32 bytes of the node's
// camera-relative spine record (trel: {lo - o, child record offset or first slot}
// {hi - o, count | leaf}), exactly what the walk reads for that node.
__global__ __launch_bounds__(256) void k_camera_lists(dev_scene_view S, dev_render_args A, chunk_args C, wf_buffers B) {
    constexpr int K = camera_list_max;
    static_assert(K <= 64, "one list entry per lane");
    __shared__ float4 fr[4][2][K][2];  // per wave: the frontier, double-buffered
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ntiles = C.npix / (TILE * TILE);
    const int t = blockIdx.x * 4 + w;
    if (t >= ntiles) return;  // (whole waves)
    YRT_LT_STAMP(lt0);
    const long long T = C.pix0 / (TILE * TILE) + t;
    const int lx0 = (int)(T % C.tiles_x) * TILE, ly0 = (int)(T / C.tiles_x) * TILE;
    // the tile's image columns and rows (bands interleave the rows: take their range)
    const int i0 = A.x0 + lx0, i1 = A.x0 + lx0 + TILE - 1;
    int jr;
    {
        const int ly = ly0 + (lane < TILE ? lane : 0);
        const int b = ly / A.band, r = ly % A.band;
        jr = A.y0 + (b * A.band_stride + A.band_offset) * A.band + r;
    }
    int j0 = jr, j1 = jr;
    for (int off = 1; off < 64; off <<= 1) j0 = min(j0, __shfl_xor(j0, off, 64)), j1 = max(j1, __shfl_xor(j1, off, 64));
    j0 = uniform(j0), j1 = uniform(j1);
    const float u0 = (float)i0 / (float)A.width, u1 = (float)(i1 + 1) / (float)A.width;
    const float v0 = (float)j0 / (float)A.height, v1 = (float)(j1 + 1) / (float)A.height;
    const dev_camera& Kc = A.cam;
    auto dir = [&](float u, float v) {
        return vec3f{(u - 0.5f) * Kc.w * Kc.xx + (v - 0.5f) * Kc.h * Kc.yx - Kc.focus * Kc.zx,
                     (u - 0.5f) * Kc.w * Kc.xy + (v - 0.5f) * Kc.h * Kc.yy - Kc.focus * Kc.zy,
                     (u - 0.5f) * Kc.w * Kc.xz + (v - 0.5f) * Kc.h * Kc.yz - Kc.focus * Kc.zz};
    };
    const vec3f O = {Kc.ox, Kc.oy, Kc.oz};
    // the margin of a box: 1e-3 + 3e-5 x the magnitude of its coordinates and the origin's, far
    // above the slab test's rounding at that magnitude. Per box, not the scene's: the root box's
    // magnitude made it huge for every box once one instance was (an instance of an empty shape
    // is bounded by +-FLT_MAX), and every list became the whole tree.
    const float Om = fmaxf(fmaxf(fabsf(O.x), fabsf(O.y)), fabsf(O.z));
    // cone plane k (through O and corners k, k + 1; the cone on its negative side), computed by
    // lane k < 4 and read by every lane
    vec3f n = {0, 0, 0};
    if (lane < 4) {
        const float cu[4] = {u0, u1, u1, u0}, cv[4] = {v0, v0, v1, v1};
        const vec3f a = dir(cu[lane], cv[lane]), b = dir(cu[(lane + 1) & 3], cv[(lane + 1) & 3]);
        n = cross(a, b);
        const vec3f c = dir(0.5f * (u0 + u1), 0.5f * (v0 + v1));
        if (dot(n, c) > 0.0f) n = n * -1.0f;
    }
    float pn[4][3], pl1[4];
    for (int k = 0; k < 4; k++) {
        pn[k][0] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(n.x), k));
        pn[k][1] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(n.y), k));
        pn[k][2] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(n.z), k));
        pl1[k] = fabsf(pn[k][0]) + fabsf(pn[k][1]) + fabsf(pn[k][2]);
    }
    // a camera-relative box outside some cone plane by more than its margin (a NaN bound never
    // separates; neither does an infinite one, whose margin is infinite)
    auto outside = [&](float4 lo, float4 hi) {
        const float Mb = Om + fmaxf(fmaxf(fmaxf(fabsf(lo.x), fabsf(lo.y)), fmaxf(fabsf(lo.z), fabsf(hi.x))),
                                    fmaxf(fabsf(hi.y), fabsf(hi.z)));
        const float eps = 1e-3f + 3e-5f * Mb;
        bool o = false;
        for (int k = 0; k < 4; k++) {
            const float mn = pn[k][0] * (pn[k][0] > 0.0f ? lo.x : hi.x) + pn[k][1] * (pn[k][1] > 0.0f ? lo.y : hi.y) +
                             pn[k][2] * (pn[k][2] > 0.0f ? lo.z : hi.z);
            o = o || mn > pl1[k] * eps;
        }
        return o;
    };
    const f4* trel = B.trel;
    const unsigned long long below = (1ull << lane) - 1ull;
    // the frontier starts as the tree's top cut (S.tcut: the nodes at depth camera_cut_depth
    // and the leaves above it, in DFS order) less the nodes the cone excludes -- one round of
    // parallel loads instead of camera_cut_depth dependent ones from the root. A node whose
    // ancestor the cone excludes is excluded too (its box lies inside the ancestor's), and an
    // entry kept needlessly only costs its box test in the walk: the list stays exact.
    static_assert((1 << camera_cut_depth) <= K, "the top cut fits one list");
    int nf, cur = 0;
    {
        float4 rl = {0, 0, 0, 0}, rh = {0, 0, 0, 0};
        bool in = false;
        if (lane < S.ntcut) {
            const f4* r = trel + (size_t)((unsigned)S.tcut[lane] / 16u);
            rl = ld4(r), rh = ld4(r + 1);
            in = !outside(rl, rh);
        }
        const unsigned long long km0 = ballot(in);
        if (in) {
            const int q = __popcll(km0 & below);
            fr[w][0][q][0] = rl, fr[w][0][q][1] = rh;
        }
        nf = __popcll(km0);
    }
#ifdef YRT_LIST_TIMING
    int nrounds = 0;
#endif
    YRT_LT_STAMP(lt1);
    for (int round = 0; round < 64 && nf > 0; round++) {
#ifdef YRT_LIST_TIMING
        nrounds++;
#endif
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        float4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0}, alo = lo, ahi = lo, blo = lo, bhi = lo;
        bool inner = false, ka = false, kb = false;
        if (lane < nf) {
            lo = fr[w][cur][lane][0], hi = fr[w][cur][lane][1];
            inner = !(ubits(hi.w) & leaf_bit);
            if (inner) {
                // children start (B) and start + 1 (A): adjacent records, start's at byte offset lo.w
                const f4* rb = trel + (size_t)((unsigned)ibits(lo.w) / 16u);
                blo = ld4(rb), bhi = ld4(rb + 1), alo = ld4(rb + spine_record_f4), ahi = ld4(rb + spine_record_f4 + 1);
                ka = !outside(alo, ahi), kb = !outside(blo, bhi);
            }
        }
        const int c = (int)ka + (int)kb;
        const bool both = inner && c == 2;  // expanding it lengthens the list by one
        const bool shrink = inner && c < 2;
        // the list's length with no two-child expansion, then the two-child ones that fit, in order
        const int size0 = lane < nf ? (shrink ? c : 1) : 0;
        const unsigned long long b1 = ballot(size0 & 1), b2 = ballot(size0 & 2);
        const int len0 = __popcll(b1) + 2 * __popcll(b2);
        const unsigned long long bb = ballot(both);
        const bool grow = both && __popcll(bb & below) < K - len0;
        if (!ballot(shrink || grow)) break;
        const int size = grow ? 2 : size0;
        const unsigned long long s1 = ballot(size & 1), s2 = ballot(size & 2);
        const int pos = __popcll(s1 & below) + 2 * __popcll(s2 & below);
        float4(*dst)[2] = fr[w][cur ^ 1];
        if (shrink || grow) {
            int q = pos;
            if (ka) dst[q][0] = alo, dst[q][1] = ahi, q++;  // the reference visits start+1 first
            if (kb) dst[q][0] = blo, dst[q][1] = bhi;
        } else if (lane < nf) {
            dst[pos][0] = lo, dst[pos][1] = hi;
        }
        nf = __popcll(s1) + 2 * __popcll(s2);
        cur ^= 1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    YRT_LT_STAMP(lt2);
    float4 elo = {0, 0, 0, 0}, ehi = {0, 0, 0, 0};
    bool keep = false;
    int nskip = 0;  // this lane's entry: the instances the cone excludes
    if (lane < nf) {
        const float4 lo = fr[w][cur][lane][0];
        float4 hi = fr[w][cur][lane][1];
        // a listed leaf's instances that the cone excludes (their world boxes, dev_scene_view
        // ibox, relative to O and outside a cone plane by more than the margin: every ray of
        // the tile fails their root box test in the instance's space): skip bits 16-30 of the
        // entry's count word, which packet_first's list mode honours (a tree leaf's are 0)
        const uint32_t cw = ubits(hi.w);
        const int count = (int)(cw & 0xffffu);
        if (S.ibox && (cw & leaf_bit) && count > 1 && count <= 15) {
            const int first = ibits(lo.w);
            uint32_t skip = 0;
            for (int i = 0; i < count; i++) {
                const float4 a = ld4(S.ibox + 2 * (first + i)), b = ld4(S.ibox + 2 * (first + i) + 1);
                const float4 ar = {a.x - O.x, a.y - O.y, a.z - O.z, 0.0f}, br = {b.x - O.x, b.y - O.y, b.z - O.z, 0.0f};
                if (outside(ar, br)) skip |= 1u << i;
            }
            hi.w = __uint_as_float(cw | skip << 16);
            nskip = __popc(skip);
            // a leaf whose every instance is excluded leaves the list
            keep = skip != (1u << count) - 1u;
        } else {
            keep = true;
        }
        elo = lo, ehi = hi;
    }
    // the kept entries, in order
    const unsigned long long km = ballot(keep);
    if (keep) {
        f4* out = B.clist + ((size_t)t * camera_list_max + __popcll(km & below)) * 2;
        out[0] = {elo.x, elo.y, elo.z, elo.w};
        out[1] = {ehi.x, ehi.y, ehi.z, ehi.w};
    }
    nf = __popcll(km);
    nskip = (int)wave_sum((unsigned long long)nskip);
    if (lane == 0) B.ccount[t] = nf, B.cskip[t] = nskip;
    YRT_LT_STAMP(lt3);
    YRT_LT_WRITE(0, t, lt1 - lt0, lt2 - lt1, lt3 - lt2, (unsigned long long)nrounds << 32 | (unsigned)nf);
}

// the sums of one chunk's list lengths into B.lstats (a list that fell back to the tree counts
// as camera_list_max + 1 / bundle_max + 1 entries) and of the instances the lists' masks
// exclude, added to the render's totals: a grid-stride sum per block, list_sums atomics per block
__global__ __launch_bounds__(256) void k_list_stats(wf_buffers B, int ntiles, int nlists) {
    __shared__ unsigned long long part[list_sums][256 / 64];
    unsigned long long v[list_sums] = {};
    const int stride = gridDim.x * 256;
    if (B.cam_lists)
        for (int i = blockIdx.x * 256 + (int)threadIdx.x; i < ntiles; i += stride) {
            const int n = B.ccount[i];
            v[0] += n < 0 ? camera_list_max + 1 : n, v[1]++, v[4] += (unsigned)B.cskip[i];
        }
    if (B.bundles)
        for (int i = blockIdx.x * 256 + (int)threadIdx.x; i < nlists; i += stride) {
            const int n = B.lcount[i];
            v[2] += n < 0 ? bundle_max + 1 : n, v[3]++, v[5] += (unsigned)B.lskip[i];
        }
    for (int q = 0; q < list_sums; q++) {
        const unsigned long long t = wave_sum(v[q]);
        if ((threadIdx.x & 63) == 0) part[q][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < list_sums) {
        const unsigned long long t = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
        if (t) atomicAdd(B.lstats + threadIdx.x, t);
    }
}

// ---- shadow rays, persistent: a grid of SP_BLOCK-thread blocks that fills the chip once;
// every wave walks its own share of the (64-sample block, light) items, so no block
// launch, block retirement or per-block counter flush happens per item (level 0 with
// enough items; the kernel also takes a mirror level's sample count from the device). LDSN > 0: each block first stages the first LDSN 4-wide records --
// the breadth-first top of the instance tree (device_scene.cpp emit_bfs) -- in LDS, and
// the walk reads those with ds_read_b128 instead of through the scalar cache (the
// north_star's "hot node tiles staged in LDS").
//
// Item order: item = bx * nlights + light (the light index minor, as k_shadow). The
// hardware deals workgroup b to XCD b % 8; XCD x takes runs x, x + 8, x + 16, ... of C
// consecutive items (k_shadow's XCD runs), its blocks taking chunks of them in order, so
// all eight XCDs sweep the image together while each traces neighbouring pixels. Items
// past the last whole super-run are dealt round-robin to the XCDs.
#ifndef YRT_SHADOW_PERSIST_MIN_ITEMS
// the persistent grid saves the hardware dealing's per-block cost and, with block chunks,
// keeps a CU's waves on neighbouring items; it needs enough items per wave to amortise its
// start and tail (A/B against k_shadow, items = 64-sample blocks x lights: 6.2 M (a c4
// frame) -6 % before block chunks, which take another 2.7 % off; 1.55 M (rank 0 of 4) -10 %; 1.04 M (c3's level 0) -9 %; 0.78 M (rank 0 of
// 8) -9.5 %; 43 K (instance10000 at 720p, 1 spp) +1 %; 29 K (c2) +20 %)
#define YRT_SHADOW_PERSIST_MIN_ITEMS 262144
#endif
#ifndef YRT_SHADOW_ITEM_LIGHTS
// an item is a 64-sample block with all its lights, looped inside the item, instead of one
// (block, light) pair: one queue position, item split, index arithmetic and bundle-list
// prologue per block (A/B, one process: c4 shadow 8.14 -> 7.79 ms, instance100k 4.69 -> 3.01,
// instance1k 5.30 -> 4.77, c3 1.54 -> 1.46, rank 0 of 8 equal)
#define YRT_SHADOW_ITEM_LIGHTS 1
#endif
#ifndef YRT_SHADOW_ITEM_RUN
#define YRT_SHADOW_ITEM_RUN 48  // (YRT_SHADOW_ITEM_LIGHTS) XCD run length in 64-sample blocks (12 / 24 / 48: within 1 %)
#endif
#ifndef YRT_SHADOW_LDS_RECORDS
// k_shadow_persist with LDS staging on (yrt_scene_set_lds_staging): the 4-wide records staged
// in LDS per block (A/B: 21 / 85 / 341 records +2 / +2 / +3 %; the handle's default is off)
#define YRT_SHADOW_LDS_RECORDS 85
#endif

// the any hit of the persistent any-hit grids' items: the walk as nested loops
// (packet_occluded_nested) where the records come through the scalar cache; the LDS-staged
// opt-in (LDSN > 0) and YRT_ANY_NESTED=0 keep the flat loop (packet_occluded_wide2)
template <int LDSN>
__device__ __forceinline__ bool item_any_hit(const dev_scene_view& S, const ray3& sr, bool valid, const float4* lds_nodes,
                                             const f4* tbase, uint32_t troot, unsigned long long culled) {
    if constexpr (YRT_ANY_NESTED != 0 && LDSN == 0)
        return packet_occluded_nested<0, true>(S, sr, valid, lds_nodes, tbase, troot, culled);
    else
        return packet_occluded_wide2<LDSN, true>(S, sr, valid, lds_nodes, tbase, troot, culled);
}

// one light of a 64-sample item of the persistent any-hit grids (k_shadow_persist and
// k_shadow_shade_persist): the shadow ray of lane's sample idx = bx * 64 + lane towards light
// li, and whether it is occluded (a culled ray counts as occluded). valid: the lane has a ray.
// IL: the item holds every light (its surface loads are the cached ones)
// WCULL: `culled_n` counts the wave's culled rays (wave-uniform) instead of the lane's
// carry: where this lane's {l, r} goes for the item's shading, or null
template <int LDSN, bool IL, bool WCULL = false>
__device__ __forceinline__ bool shadow_item_light(const dev_scene_view& S, const wf_buffers& B, int nsamp, int bx,
                                                  int li, int nl, unsigned lane, const vec3f& cam_o,
                                                  const float4* lds_nodes, unsigned& rays, unsigned& culled_n,
                                                  bool& valid, float4* carry = nullptr) {
    // the light's frame and position: one wave-uniform record, through the scalar cache
    float4 lrec[6];
    ld_records_at<6>(S.lights, (unsigned)(6 * li), lrec);
    const frame3f lf = {xyz(lrec[0]), xyz(lrec[1]), xyz(lrec[2]), xyz(lrec[3])};
    const vec3f lp0 = xyz(lrec[4]);
    const int idx = bx * 64 + (int)lane;
    valid = false;
    int info = -1;
    float r = 1.0f;
    float4 s1 = {0, 0, 0, 0};
    ray3 sr = {{0, 0, 0}, {0, 0, 1}, 0.01f, 1.0f};
    if (idx < nsamp) {
        // (every light of the item reads the sample's surface again: cached loads, not the
        // streaming ones; holding it across the walks instead spills 5 VGPRs: +0.5 %)
        float4 s0 = IL ? ld4(B.surf0 + idx) : ld4s(B.surf0 + idx);
        s1 = IL ? ld4(B.surf1 + idx) : ld4s(B.surf1 + idx);  // n, for light_term_zero
        info = sample_state(s0);
        if (info >= 0) {
            const vec3f p = xyz(s0);
            vec3f tp = transform_point(lf, lp0 - p);
            vec3f l;
            normalize_len(tp, l, r);
            sr = {p, l, 0.01f, r - 0.01f};
            valid = true;
            // (YRT_LIGHT_CARRY) for the item's shading, which would compute both again
            if (carry) carry[lane] = make_float4(l.x, l.y, l.z, r);
        }
    }
    rays += (unsigned)__popcll(ballot(valid));
    // the rays whose light term is zero (light_term_zero, called by every lane in uniform
    // control flow: its loads and ballots see the whole wave; it is false on a lane that is
    // not a hit, info < 0, so it implies valid) start the walk as done -- recorded as
    // occluded -- and a wave whose every ray is culled skips it. (Taking them out of `valid`
    // instead trips the compiler inside this loop: "illegal VGPR to SGPR copy".)
    const bool zero_term = light_term_zero(info, xyz(s1), sr.o, cam_o, sr.d, r, xyz(lrec[5]));
    const unsigned long long culled = ballot(zero_term);
    culled_n += WCULL ? (unsigned)__popcll(culled) : zero_term ? 1u : 0u;
    const bool all_culled = culled == ballot(valid);
    int lc = -1;  // the bundle's list: its leaf count, -1 = walk the tree
    if (LDSN == 0 && B.bundles) {
        const int gl = (bx / bundle_g) * nl + li;
        lc = __builtin_amdgcn_readfirstlane(B.lcount[gl]);
    }
    const f4* tbase = S.wnodes;
    uint32_t troot = (uint32_t)S.wtop_root;
    if (lc > 0) {  // (the host turns bundles off with LDS-staged records: LDSN == 0 here)
        tbase = B.lists;
        troot = (uint32_t)(((bx / bundle_g) * nl + li) * bundle_recs * wide_record_bytes);
    }
    // lc == 0: no leaf can be passed by these rays, none is occluded; all_culled: recorded
    // as occluded, k_shade skips the light
    return all_culled ? true
                     : lc == 0 ? ((culled >> lane) & 1ull) != 0
                               : item_any_hit<LDSN>(S, sr, valid, lds_nodes, tbase, troot, culled);
}

template <int LDSN>
__global__ __launch_bounds__(SP_BLOCK, YRT_SHADOW_WAVES) void k_shadow_persist(dev_scene_view S, int nsamp,
                                                                                int nx, wf_buffers B,
                                                                                unsigned long long* counters,
                                                                                float4 cam4) {
    const vec3f cam_o = xyz(cam4);  // the camera rays' origin: the view point of level 0's shading
    constexpr int WPB = SP_BLOCK / 64;  // waves per block
    constexpr unsigned C = (YRT_SHADOW_ITEM_LIGHTS && LDSN == 0) ? YRT_SHADOW_ITEM_RUN : YRT_SHADOW_LIGHT_MINOR;
    __shared__ float4 lds_nodes[LDSN > 0 ? LDSN * 8 : 1];
    if constexpr (LDSN > 0) {
        const int nrec = LDSN * 8;
        const float4* src = reinterpret_cast<const float4*>(S.wnodes);
        for (int i = threadIdx.x; i < nrec; i += SP_BLOCK) lds_nodes[i] = src[i];
        __syncthreads();
    }
    const int nl = S.nlights;
    // YRT_SHADOW_ITEM_LIGHTS: an item is a 64-sample block with every light (the lights looped
    // inside it: one queue position, one item split, per block instead of per (block, light))
    // (not with LDS-staged records: that copy keeps its registers for the staged walk)
    constexpr bool IL = YRT_SHADOW_ITEM_LIGHTS && LDSN == 0;
    const unsigned n_items = IL ? (unsigned)nx : (unsigned)nx * (unsigned)nl;
    const unsigned lane = threadIdx.x & 63;
    const unsigned xcd = blockIdx.x % 8u;
    unsigned rays = 0;  // wave-uniform (an SGPR): shadow rays of this wave (the reference's count)
    // per lane (a VGPR: one more SGPR would spill): this lane's rays answered without a walk
    unsigned culled_l = 0;
    // positions from the block's chunk ring (chunk_ring_next), YRT_SHADOW_BLOCK_CHUNK at a time
    constexpr unsigned CS = YRT_SHADOW_BLOCK_CHUNK;
    __shared__ chunk_ring ring;
    const unsigned head = head_items<C, CS>(n_items);
    chunk_ring_init<CS>(ring, B.queue + xcd, B.queue + 8, head / 8u);
#ifdef YRT_TAIL_STATS
    const unsigned long long tail_t0 = __builtin_amdgcn_s_memrealtime();
    unsigned tail_items = 0;
#endif
    for (;;) {
        const unsigned q = chunk_ring_next<CS>(ring, B.queue + xcd, lane, B.queue + 8, head / 8u);
        const unsigned it = split_item<C>(q, xcd, n_items, head);
        if (it >= n_items) break;
#ifdef YRT_TAIL_STATS
        tail_items++;
#endif
        const int bx = IL ? (int)it : (int)(it / (unsigned)nl);
        for (int lq = 0; lq < (IL ? nl : 1); lq++) {
            const int li = IL ? lq : (int)(it % (unsigned)nl);
            bool valid;  // (idx < nsamp on a valid lane)
            const bool occ =
                shadow_item_light<LDSN, IL>(S, B, nsamp, bx, li, nl, lane, cam_o, lds_nodes, rays, culled_l, valid);
            // (the byte's address in this form, idx an int of its own: with bx * 64 + lane written
            // into the sum the kernel spills 2 VGPRs)
            const int idx = bx * 64 + (int)lane;
            if (valid) stb(B.occl + (size_t)li * B.capacity + idx, occ ? 1 : 0);
        }
    }
#ifdef YRT_TAIL_STATS
    tail_record(1, tail_t0, tail_items);
#endif
    const unsigned long long mine = lane == 0 ? (unsigned long long)rays : 0ull;
    flush_block<2, SP_BLOCK>(counters, {cnt_shadow_rays, cnt_shadow_culled}, {mine, (unsigned long long)culled_l});
}

// ---- shade() after the queries (raytrace.cpp:99-206) ----
// FUSE (level 0 of a scene without mirrors, s*s dividing the block): the block's
// samples are whole pixels, so the ordered per-pixel sum of k_accumulate is done here
// from LDS and the per-sample radiance never goes to HBM.
#ifndef YRT_SHADE_WAVES
#define YRT_SHADE_WAVES 7  // k_shade register budget: 65-73 VGPRs with the f64 pow called (A/B at c4: 5 -> 7 waves -4 %; with the pow inlined it needed 96)
#endif
// OCC4 (scenes with at most four lights): the occlusion bytes are loaded together with the
// surface, one memory round trip instead of one per light inside the light loop.
#ifndef YRT_SHADE_LEVEL_WAVES
// the same for the unfused k_shade (reflective scenes: per-level shading, mirror-ray
// compaction, the fold). Its waits are dependent loads (SQ_WAIT_ANY 76 % at 7 waves); more
// registers per wave shorten them (A/B at c3: shade 1.55 -> 1.35 / 1.34 ms at 6 / 5 waves)
#define YRT_SHADE_LEVEL_WAVES 5
#endif
// shade() for one sample that hit (info >= 0), raytrace.cpp:99-206: the surface rows, the
// material, the textures, the lights that are not occluded, the mirror branch. Every kernel
// that shades calls this one body (k_shade, k_rays_shade, k_shade_passes and
// k_shadow_shade_persist's epilogue): the image, the ray batches and the passes are bit-exact
// because they run the same operations in the same order. Two kernels keep a body of their own:
// the fused k_shade_passes, and k_shade_groups, whose light loop runs once per plane over the
// plane's lights. The three bodies call one light_reach, one light_term and (the two with
// mirror levels) one compact_mirror_rays. What still stands in each of them, and is to be
// changed in all three together: the surface and material block ahead of the light loop (s1, uv,
// the material rows, the texels, la), v, the light's occlusion test, `c = c + (ld + ls)`, and
// the `!reflective` / depth-cap / spawn arithmetic after the loop. (As one function that block
// gave the unfused k_shade three more VGPRs and every k_shade_groups other instructions.)
// OCC4: the lights' occlusion is the mask occ_bits, else the bytes B.occl.
// LATE (k_shadow_shade_persist, at the any-hit grid's 64 VGPRs): what only the end needs, la and
// kr and the reflective flag, is computed or loaded again after the light loop instead of held
// across it; the same operations on the same values, 7 VGPR spills fewer.
// TERMS (the shading passes, k_shade_passes): *terms collects the terms the beauty adds up, as
// they are computed; with the default, an empty type, nothing of it is compiled.
// The straight-line pieces the three shading bodies share (shade_hit, the fused k_shade_passes,
// k_shade_groups). Inlined, they leave every shading kernel its count of instructions per
// mnemonic and its registers, spills and LDS; a few instructions stand elsewhere or have a
// commutative operation's operands swapped ("Shared shading pieces", and
// `tools/isa_dump.py --compare` for the check).
// light_reach: light record `lr` (six rows, the same for every lane: one scalar fetch instead of
// six 64-lane vector loads of one address) seen from p: direction l, distance r, emission ke
__device__ __forceinline__ void light_reach(const f4* lr, vec3f p, vec3f& l, float& r, vec3f& ke) {
    float4 lrec[6];
    ld_scalar<6>(lr, lrec);
    frame3f lf = {xyz(lrec[0]), xyz(lrec[1]), xyz(lrec[2]), xyz(lrec[3])};
    vec3f lp0 = xyz(lrec[4]);
    ke = xyz(lrec[5]);
    vec3f tp = transform_point(lf, lp0 - p);
    normalize_len(tp, l, r);
}
// light_term: one light's diffuse and specular terms ld, ls (raytrace.cpp:147-185) from the
// view direction v, the light's {l, r, ke} and the material's kd, ks, ns
__device__ __forceinline__ void light_term(int kind, vec3f nrm, vec3f v, vec3f l, float r, vec3f ke, vec3f kd,
                                           vec3f ks, float ns, vec3f& ld, vec3f& ls) {
    vec3f h;
    float hlen;
    normalize_len(v + l, h, hlen);
    const vec3f ker = div3(ke, r * r);
    ld = kd * ker;
    ls = ks * ker;
    if (kind == kind_lines) {
        float prodnl = dot(nrm, l);
        float prodnh = dot(nrm, h);
        if (prodnl < 0.0f) prodnl *= -1;
        if (prodnh < 0.0f) prodnh *= -1;
        float sinnl = __builtin_sqrtf(1.0f - prodnl);
        float sinnh = __builtin_sqrtf(1.0f - prodnh);
        ld = ld * sinnl;
        ls = ls * spec_pow(sinnh, ns, ls);
    } else {
        ld = ld * smax(0.0f, dot(nrm, l));
        ls = ls * spec_pow(smax(0.0f, dot(nrm, h)), ns, ls);
    }
}
// compact_mirror_rays: the block's mirror rays (spawn; mask its wave's ballot) take consecutive
// slots of segment gout of level + 1 (waves in wave order, lanes in lane order) behind one
// atomic per block. (One atomic per wave: c3 shade 1.99 -> 5.81 ms.) The fold follows parent
// indices, so the order is free. Every lane of the block calls it: two barriers.
template <int SB>
__device__ __forceinline__ void compact_mirror_rays(const wf_buffers& B, int level, int gout, int idx, bool spawn,
                                                    unsigned long long mask, vec3f p, vec3f dr,
                                                    int (&cmp_count)[SB / 64], int (&cmp_base)[SB / 64]) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) cmp_count[w] = __popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int q = 0; q < SB / 64; q++) tot += cmp_count[q];
        int acc = tot ? atomicAdd(seg_counter(B.count, level + 1, gout), tot) : 0;
        for (int q = 0; q < SB / 64; q++) cmp_base[q] = acc, acc += cmp_count[q];
    }
    __syncthreads();
    if (spawn) {
        const int slot = gout * B.seg + cmp_base[w] + __popcll(mask & ((1ull << lane) - 1));
        B.ray_o(level + 1)[slot] = {p.x, p.y, p.z, __int_as_float(idx)};
        B.ray_d(level + 1)[slot] = {dr.x, dr.y, dr.z, 0};
    }
}

struct no_terms {};
struct pass_terms {
    // c after the light loop, its ld and ls parts, the vector added for the mirror ray where
    // max_depth cuts it (0 * kr), la. A sample that never gets here keeps +0 in each.
    vec3f c = {0, 0, 0}, d = {0, 0, 0}, s = {0, 0, 0}, r = {0, 0, 0}, la = {0, 0, 0};
};
// SOFT (soft shadows, k_soft_shade): a light's occlusion record is its count of unoccluded rays
// out of soft->rays (k_soft_shadow; OCC4: byte li of occ_bits), a light with none is skipped and
// every other term is scaled by float(open) / float(rays); with the default, an empty type,
// nothing of it is compiled.
struct no_soft {};
struct soft_factor {
    int rays;  // K
};
__device__ __forceinline__ vec3f amb_of(const vec3f& a) { return a; }
__device__ __forceinline__ vec3f amb_of(const float* a) { return {a[0], a[1], a[2]}; }  // (LATE: read where it is used)
template <bool COUNT, bool FUSE, bool OCC4, bool LATE = false, class AMB = vec3f, class TERMS = no_terms,
          class SOFT = no_soft>
__device__ __forceinline__ void shade_hit(const dev_scene_view& S, const wf_buffers& B, int idx, int info,
                                          const float4& s0, const float4& ro4, uint32_t occ_bits, int level,
                                          int max_depth, const AMB& amb, const float* lut, work_counts& wc,
                                          unsigned long long& truncated, vec3f& R, vec3f& p, bool& spawn, vec3f& dr,
                                          vec3f& rec_d, vec3f& rec_la, int& rec_mat, bool& write_r,
                                          TERMS* terms = nullptr, const float4* carried = nullptr,
                                          int ncarried = 0, const SOFT* soft = nullptr) {
    // carried (k_shadow_shade_persist, YRT_LIGHT_CARRY): this lane's {l, r} of light li at
    // carried[li * 64], for li < ncarried -- the values the light loop computes, from the same
    // statements on the same p (shadow_item_light)
    constexpr bool SPLIT = !std::is_same<TERMS, no_terms>::value;
    constexpr bool AREA = !std::is_same<SOFT, no_soft>::value;
    vec3f nrm;
    vec2f uv;
    int mat, kind;
    {
        const float4 s1 = ld4s(B.surf1 + idx);
        // (v is read only by texture lookups: a scene without textures neither writes nor reads it)
        p = xyz(s0), nrm = xyz(s1), uv = {s1.w, B.need_v ? lds1(B.surfv + idx) : 0.0f};
        mat = info_mat(info), kind = info & 3;
    }
    const vec3f ro = xyz(ro4);
    float4 m0, m1, m2, m3;
    {
        m0 = ld4(S.mats + 4 * mat), m1 = ld4(S.mats + 4 * mat + 1);
        m2 = ld4(S.mats + 4 * mat + 2), m3 = ld4(S.mats + 4 * mat + 3);
    }
    const vec3f kd0 = xyz(m0), ks0 = xyz(m1);
    vec3f kr = xyz(m2);
    const float ns = m0.w;
    const int kd_txt = ibits(m1.w), ks_txt = ibits(m2.w);
    bool reflective = !LATE && (ibits(m3.w) & mat_reflective);
    vec3f la = {0, 0, 0};
    if (!LATE) la = amb_of(amb) * kd0;
    vec3f tkd = {1, 1, 1}, tks = {1, 1, 1};
    if (kd_txt >= 0) {
        tkd = eval_texture<COUNT>(S, kd_txt, uv, wc, lut);
        if (!LATE) la = la * tkd;
    }
    if (ks_txt >= 0) tks = eval_texture<COUNT>(S, ks_txt, uv, wc, lut);
    vec3f c = {0.0f, 0.0f, 0.0f};
    // raytrace.cpp:147 (per light) and :196 (mirror): the same value each time
    vec3f v;
    float vlen;
    normalize_len(ro - p, v, vlen);
    for (int li = 0; li < S.nlights; li++) {
        uint32_t open = 0;  // (AREA) the light's unoccluded rays
        if constexpr (AREA) {
            open = OCC4 ? (occ_bits >> (8 * li)) & 0xffu : (uint32_t)ldb(B.occl + (size_t)li * B.capacity + idx);
            if (open == 0u) continue;
        } else {
            if (OCC4 ? ((occ_bits >> li) & 1u) != 0u : ldb(B.occl + (size_t)li * B.capacity + idx) != 0) continue;
        }
        const f4* lr = S.lights + 6 * li;
        vec3f l, ke;
        float r;
        if (carried && li < ncarried) {
            // (YRT_LIGHT_CARRY) the light step of this item left the sample's {l, r} in LDS
            float4 lrec[2];
            ld_scalar_at<2>(S.lights, (unsigned)(6 * li + 4), lrec);
            ke = xyz(lrec[1]);
            const float4 c4 = carried[li * 64];
            l = xyz(c4), r = c4.w;
        } else {
            light_reach(lr, p, l, r, ke);
        }
        vec3f kd = kd0, ks = ks0;
        if (kd_txt >= 0) kd = kd * tkd;
        if (ks_txt >= 0) ks = ks * tks;
        vec3f ld, ls;
        light_term(kind, nrm, v, l, r, ke, kd, ks, ns, ld, ls);
        if constexpr (AREA)
            c = c + (ld + ls) * (float(open) / float(soft->rays));
        else
            c = c + (ld + ls);
        if constexpr (SPLIT) terms->d = terms->d + ld, terms->s = terms->s + ls;
    }
    if (LATE) {
        la = amb_of(amb) * kd0;
        if (kd_txt >= 0) la = la * tkd;
        // (the material's address from the sample's info again, not a pointer kept in registers)
        int matl = info_mat(info);
        asm volatile("" : "+v"(matl));
        const f4* ml = S.mats + 4 * matl;
        reflective = ibits(ld4(ml + 3).w) & mat_reflective;
        if (reflective) kr = xyz(ld4(ml + 2));
    }
    if constexpr (SPLIT) terms->c = c, terms->la = la;
    if (!reflective) {
        R = c + la;
    } else if (FUSE || level + 1 >= max_depth || level + 1 >= B.nlevels) {
        // (FUSE runs one-level renders: B.nlevels == 1, no mirror ray is spawned)
        // depth cap: the reflected contribution counts as a miss (col = 0)
        truncated++;
        vec3f t = {0.0f * kr.x, 0.0f * kr.y, 0.0f * kr.z};
        if constexpr (SPLIT) terms->r = t;
        R = (c + t) + la;
    } else {
        spawn = true;
        dr = (nrm * 2.0f * dot(nrm, v)) - v;
        rec_d = c;
        rec_la = la;
        rec_mat = mat;
        write_r = false;
    }
    if (COUNT) wc.hits++;
}

// the fused shapes' per-pixel sums: `ppb` pixels from chunk pixel pl0 on, their samples
// consecutive in `rad` (LDS); lane t0 of STRIDE takes every STRIDE-th (pixel, component).
// SPP: C.spp where the caller knows it at compile time (the chain of adds is unrolled, its
// LDS reads issued ahead of it), else 0
template <int STRIDE, int SPP = 0>
__device__ __forceinline__ void sum_pixels(const dev_render_args& A, const chunk_args& C, float4* __restrict__ out,
                                           const float4* rad, int pl0, int ppb, int t0) {
    for (int t = t0; t < 3 * ppb; t += STRIDE) {
        const int px = t / 3, comp = t - 3 * px;
        const int pl = pl0 + px;
        int lx, ly, i, j;
        const bool valid = pl < C.npix && pixel_of(A, C, C.pix0 + pl, lx, ly, i, j);
        if (pl < C.npix && lx < A.tile_w && ly < A.tile_h) {
            float v = 0.0f;
            if (valid) {
                const int spp = SPP ? SPP : C.spp;
                const float* r = reinterpret_cast<const float*>(rad + px * spp) + comp;
                float acc = 0.0f;
                if constexpr (SPP > 0) {
#pragma unroll
                    for (int q = 0; q < SPP; q++) acc = acc + r[4 * q];
                } else {
                    for (int q = 0; q < spp; q++) acc = acc + r[4 * q];
                }
                v = acc / float(spp);
            }
            float* o = reinterpret_cast<float*>(out + (size_t)ly * A.out_stride + lx);
            o[comp] = v;
            if (comp == 0) o[3] = valid ? 1.0f : 0.0f;
        }
    }
}

// the fused shapes' per-pixel sums over several planes: the block's per-sample values stand in
// LDS rows of SB + 1 floats per (plane, component), a pixel's samples consecutive; one lane per
// (pixel, plane, colour component), each lane's sum the reference's ordered chain of adds for
// that component. NP: the plane count, an int or (its divisions by a constant)
// std::integral_constant; plane k is summed into out(k) where wanted(k). Both are callables that
// read the kernel's argument where it is used, as accumulate_plane's are: with the mask by value
// and the planes as a pointer the fused k_shade_passes came out two and three instructions longer
template <int SB, class NP, class WANTED, class OUT>
__device__ __forceinline__ void sum_plane_rows(const dev_render_args& A, const chunk_args& C, const float* rows,
                                               NP nplanes, WANTED&& wanted, OUT&& out) {
    constexpr int ROW = SB + 1;
    const int ppb = SB / C.spp;
    for (int t = (int)threadIdx.x; t < 3 * nplanes * ppb; t += SB) {
        const int px = t / (3 * nplanes), r = t - 3 * nplanes * px;
        const int k = r / 3, comp = r - 3 * k;
        if (!wanted(k)) continue;
        const int pl = (int)(blockIdx.x * SB / C.spp) + px;
        int lx, ly, i, j;
        const bool valid = pl < C.npix && pixel_of(A, C, C.pix0 + pl, lx, ly, i, j);
        if (pl < C.npix && lx < A.tile_w && ly < A.tile_h) {
            float v = 0.0f;
            if (valid) {
                const float* row = rows + (k * 3 + comp) * ROW + px * C.spp;
                float acc = 0.0f;
                for (int q = 0; q < C.spp; q++) acc = acc + row[q];
                v = acc / float(C.spp);
            }
            float* o = reinterpret_cast<float*>(out(k) + (size_t)ly * A.out_stride + lx);
            o[comp] = v;
            if (comp == 0) o[3] = valid ? 1.0f : 0.0f;
        }
    }
}

// the table a texture lookup ends in: the block's LDS copy of the srgb table (1 KiB), staged
// here by its BS threads, so that the last link of a lookup's chain of dependent loads
// (material -> texel -> table) is an LDS read. A scene without textures never looks the table
// up: it is not staged.
// BARRIER: the copy is followed by its barrier here; otherwise by one of the caller's
using srgb_table = float[256];
template <int BS, bool BARRIER>
__device__ __forceinline__ const float* stage_srgb(const dev_scene_view& S, srgb_table& srgb_lds) {
    if (S.ntextures > 0) {  // uniform over the grid
        for (int q = (int)threadIdx.x; q < 256; q += BS) srgb_lds[q] = S.srgb[q];
        if (BARRIER) __syncthreads();
    }
    return srgb_lds;
}

// ---- shading passes (yrt_render_passes): the beauty split into the terms shade() adds up ----
// Per camera sample: DIRECT is c after the light loop (raytrace.cpp:121-185), DIFFUSE and
// SPECULAR the same chain of adds over the same lights with ld or ls alone, REFLECTION the
// vector added at raytrace.cpp:203 (col * kr; 0 * kr where max_depth cuts the mirror ray, +0
// on a material that does not reflect), AMBIENT la. A miss adds +0 to every pass. Each plane
// is the beauty's box filter of its value: the ordered sum over jj/ii divided by float(s*s).
// The beauty is plane pass_count of the same kernels. The unfused k_shade_passes is
// shade_samples, the body of k_shade, with PASSES set: the same statements shade (shade_hit),
// fold and compact, and what the passes add stands under `if constexpr (PASSES)`, of which the
// beauty's kernels compile nothing. The fused k_shade_passes keeps a body of its own (there).
constexpr int pass_planes = pass_count + 1;  // the five passes and the beauty
struct pass_buffers {
    unsigned mask;            // bit k: plane k is wanted (bit pass_count: the beauty)
    float4* out[pass_planes];  // the caller's planes (window layout, out_stride); null when not wanted
    f4* smp[pass_count];      // per-sample values of a wanted pass (unfused and mirror shapes only)
};

// The body of every kernel that shades after the queries: k_shade, k_rays_shade and
// k_shade_passes keep their own names, arguments and launch bounds.
// RAYS (a ray batch, unfused, k_rays_shade): level 0's view point -- shading and the mirror-ray
// spawn -- is the sample's own ray origin (ray_origin), and B.rad is the caller's output, one
// RGBA per ray
// PASSES (the unfused k_shade_passes; P its planes): the terms of each camera sample go to
// P.smp, the reflection term of a sample with a mirror ray where the fold reaches it
// SOFT (a soft ray batch, k_soft_shade; soft_rays its K): the occlusion bytes are counts of
// unoccluded rays, with OCC4 four of them in occ_bits, and shade_hit scales each light's term
template <bool COUNT, bool FUSE, int SB, bool OCC4, bool RAYS, bool PASSES = false, bool SOFT = false>
__device__ __forceinline__ void shade_samples(dev_scene_view S, dev_render_args A, int level, int nsamp_level0,
                                              int max_depth, wf_buffers B, unsigned long long* counters, chunk_args C,
                                              float4* __restrict__ out, const pass_buffers* P = nullptr,
                                              int soft_rays = 0) {
    static_assert(!(PASSES && FUSE), "the fused passes kernel has its own body");
    static_assert(!SOFT || (RAYS && !PASSES && !FUSE && !COUNT), "soft shadows shade ray batches");
    __shared__ float4 fused_rad[FUSE ? SB : 1];
    __shared__ int cmp_count[SB / 64], cmp_base[SB / 64];
    __shared__ srgb_table srgb_lds;
    const float* lut = stage_srgb<SB, true>(S, srgb_lds);
    work_counts wc;
    unsigned long long truncated = 0;
    const vec3f amb = {A.amb[0], A.amb[1], A.amb[2]};
    const vec3f cam_o = {A.cam.ox, A.cam.oy, A.cam.oz};
    // the loop bounds are uniform per block so every lane reaches the ballot and the
    // barriers below
    const int stride = gridDim.x * SB;
    // this block's mirror rays go to segment blockIdx.x % level_segments of the next level
    const int gout = (int)(blockIdx.x % (unsigned)level_segments);
    // (FUSE runs level 0 only: one segment, no loop)
    const int nseg = FUSE ? 1 : level ? level_segments : 1;
    for (int g = 0; g < nseg; g++) {
    const int n = (!FUSE && level) ? *seg_counter(B.count, level, g) : nsamp_level0;
    const int nround = (n + stride - 1) / stride;
    for (int round = 0; round < nround; round++) {
        const int j = round * stride + blockIdx.x * SB + threadIdx.x;
        const int idx = FUSE ? j : g * B.seg + j;
        bool spawn = false;
        vec3f p = {0, 0, 0}, dr = {0, 0, 0}, rec_d = {0, 0, 0}, rec_la = {0, 0, 0};
        int rec_mat = 0;
        if (j < n) {
            float4 s0 = ld4s(B.surf0 + idx);
            uint32_t occ_bits = 0;
            if constexpr (OCC4) {
                // (the same text in the fused k_shade_passes; as a function it gave every OCC4
                // kernel other instructions)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int lq = q < S.nlights ? q : 0;  // an unconditional load, masked after
                    const uint32_t ob = ldb(B.occl + (size_t)lq * B.capacity + idx);
                    if constexpr (SOFT)
                        occ_bits |= q < S.nlights ? ob << (8 * q) : 0u;
                    else
                        occ_bits |= (q < S.nlights && ob != 0u) ? 1u << q : 0u;
                }
            }
            const int info = sample_state(s0);
            vec3f R = {0, 0, 0};
            bool write_r = info != -2;
            // level >= 1: this sample's ray record {origin, parent index}
            float4 ro4 = (!FUSE && level) ? ld4(B.ray_o(level) + idx) : make_float4(cam_o.x, cam_o.y, cam_o.z, 0.0f);
            if constexpr (RAYS && !FUSE) {
                if (!level) {
                    const vec3f o = ray_origin(B, idx);
                    ro4 = make_float4(o.x, o.y, o.z, 0.0f);
                }
            }
            // this sample's pass values (level 0): a miss keeps +0 in each. (Without PASSES an
            // empty object and a null pointer: with its address k_shade came out differently)
            typename std::conditional<PASSES, pass_terms, no_terms>::type T;
            if (info >= 0) {
                if constexpr (SOFT) {
                    const soft_factor F = {soft_rays};
                    shade_hit<COUNT, FUSE, OCC4, false, vec3f, no_terms, soft_factor>(
                        S, B, idx, info, s0, ro4, occ_bits, level, max_depth, amb, lut, wc, truncated, R, p, spawn, dr,
                        rec_d, rec_la, rec_mat, write_r, nullptr, nullptr, 0, &F);
                } else {
                    shade_hit<COUNT, FUSE, OCC4>(S, B, idx, info, s0, ro4, occ_bits, level, max_depth, amb, lut, wc,
                                                 truncated, R, p, spawn, dr, rec_d, rec_la, rec_mat, write_r,
                                                 PASSES ? &T : nullptr);
                }
            }
            if constexpr (PASSES) {
                if (level == 0 && info != -2) {
                    // level 0's values per sample; a sample that spawns a mirror ray gets its
                    // reflection value where the fold reaches it
                    const unsigned m = P->mask;
                    if (m >> pass_direct & 1) gstore(P->smp[pass_direct], idx, T.c.x, T.c.y, T.c.z, 0.0f);
                    if (m >> pass_diffuse & 1) gstore(P->smp[pass_diffuse], idx, T.d.x, T.d.y, T.d.z, 0.0f);
                    if (m >> pass_specular & 1) gstore(P->smp[pass_specular], idx, T.s.x, T.s.y, T.s.z, 0.0f);
                    if (m >> pass_ambient & 1) gstore(P->smp[pass_ambient], idx, T.la.x, T.la.y, T.la.z, 0.0f);
                    if ((m >> pass_reflection & 1) && !spawn)
                        gstore(P->smp[pass_reflection], idx, T.r.x, T.r.y, T.r.z, 0.0f);
                }
            }
            if (FUSE) {
                fused_rad[threadIdx.x] = make_float4(R.x, R.y, R.z, 1.0f);
            } else if (write_r) {
                // a final value at level k >= 1 folds straight up its chain of parents
                // (raytrace.cpp:201-206, R_k-1 = (D + R_k * kr) + la, in that order) to
                // the camera sample; each parent has this one child, so its value is
                // final now too
                vec3f col = R;
                int lev = level, node = idx;
                while (lev > 0) {
                    const int parent = ibits(B.ray_o(lev)[node].w);
                    const float4 d = ld4(B.rec0(lev - 1) + parent);
                    const float4 la = ld4(B.rec1(lev - 1) + parent);
                    const float4 kr = ld4(S.mats + 4 * ibits(d.w) + 2);  // the parent's material kr
                    vec3f cc = {d.x, d.y, d.z};
                    const vec3f t = {col.x * kr.x, col.y * kr.y, col.z * kr.z};
                    if constexpr (PASSES) {  // the last step, into the camera sample, adds its reflection value
                        if (lev == 1 && (P->mask >> pass_reflection & 1))
                            gstore(P->smp[pass_reflection], parent, t.x, t.y, t.z, 0.0f);
                    }
                    cc = cc + t;
                    cc = cc + xyz(la);
                    col = cc, node = parent, lev--;
                }
                B.rad[node] = {col.x, col.y, col.z, 1.0f};
            }
        }
        // the mirror rays: a sample's own fold records go out at once, its ray is compacted
        // into the next level's segment
        if constexpr (FUSE) continue;  // one level: no mirror rays
        const unsigned long long mask = __ballot(spawn);
        if (spawn) {
            B.rec0(level)[idx] = {rec_d.x, rec_d.y, rec_d.z, __int_as_float(rec_mat)};
            B.rec1(level)[idx] = {rec_la.x, rec_la.y, rec_la.z, 0};
        }
        compact_mirror_rays<SB>(B, level, gout, idx, spawn, mask, p, dr, cmp_count, cmp_base);
    }
    }
    if (FUSE) {
        // raytrace.cpp:232-249: s*s samples of a pixel summed in jj/ii order, then / s*s
        __syncthreads();
        const int ppb = SB / C.spp;
        // one lane per (pixel, colour component): each lane's sum is the reference's ordered
        // chain of adds (raytrace.cpp:232-249) for that component, so a pixel's three
        // dependent chains run side by side (A/B: c4 shade 2.00 -> 1.96 ms)
        sum_pixels<SB>(A, C, out, fused_rad, (int)(blockIdx.x * SB / C.spp), ppb, (int)threadIdx.x);
    }
    flush(counters, cnt_depth_truncated, truncated);
    if (COUNT) flush_work(counters, wc);
}

template <bool COUNT, bool FUSE, int SB = WF_BLOCK, bool OCC4 = false>
__global__ __launch_bounds__(SB, FUSE ? YRT_SHADE_WAVES : YRT_SHADE_LEVEL_WAVES) void k_shade(dev_scene_view S, dev_render_args A, int level, int nsamp_level0,
                                                    int max_depth, wf_buffers B, unsigned long long* counters,
                                                    chunk_args C, float4* __restrict__ out) {
    shade_samples<COUNT, FUSE, SB, OCC4, false>(S, A, level, nsamp_level0, max_depth, B, counters, C, out);
}

// every level of a ray batch (run_rays): the unfused k_shade; amb and max_depth are all it
// reads of the render arguments
template <bool OCC4>
__global__ __launch_bounds__(WF_BLOCK, YRT_SHADE_LEVEL_WAVES) void k_rays_shade(dev_scene_view S, float3 amb3, int level,
                                                                                int nsamp_level0, int max_depth,
                                                                                wf_buffers B,
                                                                                unsigned long long* counters) {
    dev_render_args A = {};
    A.amb[0] = amb3.x, A.amb[1] = amb3.y, A.amb[2] = amb3.z;
    const chunk_args C = {0, nsamp_level0, 1, 1};
    shade_samples<false, false, WF_BLOCK, OCC4, true>(S, A, level, nsamp_level0, max_depth, B, counters, C, nullptr);
}

// every level of a soft ray batch (run_rays with soft_shadow_args): k_rays_shade with the
// occlusion bytes read as k_soft_shadow's counts of unoccluded rays out of K
template <bool OCC4>
__global__ __launch_bounds__(WF_BLOCK, YRT_SHADE_LEVEL_WAVES) void k_soft_shade(dev_scene_view S, float3 amb3, int level,
                                                                                int nsamp_level0, int max_depth,
                                                                                wf_buffers B,
                                                                                unsigned long long* counters, int K) {
    dev_render_args A = {};
    A.amb[0] = amb3.x, A.amb[1] = amb3.y, A.amb[2] = amb3.z;
    const chunk_args C = {0, nsamp_level0, 1, 1};
    shade_samples<false, false, WF_BLOCK, OCC4, true, false, true>(S, A, level, nsamp_level0, max_depth, B, counters, C,
                                                                   nullptr, nullptr, K);
}

// the shading passes (yrt_render_passes). Unfused (mirror levels, or pixels that are not whole
// in a block): shade_samples. Fused: a body of its own, with the two more accumulators (d, s)
// beside c. Through shade_hit's TERMS the fused kernel was measurably slower, and
// so was this body with small changes of form: its own sRGB staging (not stage_srgb) and the
// loop over its one segment are what keeps the compiler's output. It shares light_reach and
// light_term with shade_hit and sum_plane_rows with k_shade_groups; the statements listed at
// shade_hit and the OCC4 gather (shade_samples') are written out here and change with theirs
// (tests/test_gpu_passes*.py compare its beauty with k_shade's bit for bit).
// Fused: 70-72 VGPRs and no scratch; at k_shade's 7 waves d and s put 32 bytes per lane into
// scratch
constexpr int shade_pass_waves = 6;
template <bool FUSE, int SB = WF_BLOCK, bool OCC4 = false>
__global__ __launch_bounds__(SB, FUSE ? shade_pass_waves : YRT_SHADE_LEVEL_WAVES) void k_shade_passes(
    dev_scene_view S, dev_render_args A, int level, int nsamp_level0, int max_depth, wf_buffers B, pass_buffers P,
    unsigned long long* counters, chunk_args C) {
    if constexpr (!FUSE) {
        shade_samples<false, false, SB, OCC4, false, true>(S, A, level, nsamp_level0, max_depth, B, counters, C, nullptr,
                                                           &P);
        return;
    }
    // the per-sample values of a block's whole pixels, one row of SB floats per (plane,
    // component): 12 bytes per sample and plane, 18 KiB for the six planes, so eight blocks
    // still fit a CU's 160 KiB and the LDS does not bound the kernel's 6 waves per SIMD. The
    // rows are one float apart in the banks, so the 18 chains of a pixel read 18 banks
    constexpr int ROW = SB + 1;
    __shared__ float fused[FUSE ? pass_planes * 3 * ROW : 1];
    __shared__ float srgb_lds[256];
    const float* lut = srgb_lds;
    if (S.ntextures > 0) {  // uniform over the grid
        for (int q = (int)threadIdx.x; q < 256; q += SB) srgb_lds[q] = S.srgb[q];
        __syncthreads();
    }
    work_counts wc;
    unsigned long long truncated = 0;
    const vec3f amb = {A.amb[0], A.amb[1], A.amb[2]};
    const vec3f cam_o = {A.cam.ox, A.cam.oy, A.cam.oz};
    const int stride = gridDim.x * SB;
    for (int g = 0; g < 1; g++) {  // (shade_samples' loop over segments: level 0 has one)
    const int n = nsamp_level0;
    const int nround = (n + stride - 1) / stride;
    for (int round = 0; round < nround; round++) {
        const int j = round * stride + blockIdx.x * SB + threadIdx.x;
        const int idx = j;
        vec3f p = {0, 0, 0};
        // this sample's pass values (level 0): a miss and a lane past the chunk keep +0
        vec3f R = {0, 0, 0}, pc = {0, 0, 0}, pd = {0, 0, 0}, ps = {0, 0, 0}, pr = {0, 0, 0}, pla = {0, 0, 0};
        if (j < n) {
            float4 s0 = ld4s(B.surf0 + idx);
            uint32_t occ_bits = 0;
            if constexpr (OCC4) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int lq = q < S.nlights ? q : 0;  // an unconditional load, masked after
                    const uint32_t ob = ldb(B.occl + (size_t)lq * B.capacity + idx);
                    occ_bits |= (q < S.nlights && ob != 0u) ? 1u << q : 0u;
                }
            }
            const int info = sample_state(s0);
            const float4 ro4 = make_float4(cam_o.x, cam_o.y, cam_o.z, 0.0f);
            if (info >= 0) {
                vec3f nrm;
                vec2f uv;
                int mat, kind;
                {
                    const float4 s1 = ld4s(B.surf1 + idx);
                    p = xyz(s0), nrm = xyz(s1), uv = {s1.w, B.need_v ? lds1(B.surfv + idx) : 0.0f};
                    mat = info_mat(info), kind = info & 3;
                }
                const vec3f ro = xyz(ro4);
                const float4 m0 = ld4(S.mats + 4 * mat), m1 = ld4(S.mats + 4 * mat + 1);
                const float4 m2 = ld4(S.mats + 4 * mat + 2), m3 = ld4(S.mats + 4 * mat + 3);
                const vec3f kd0 = xyz(m0), ks0 = xyz(m1), kr = xyz(m2);
                const float ns = m0.w;
                const int kd_txt = ibits(m1.w), ks_txt = ibits(m2.w);
                const bool reflective = ibits(m3.w) & mat_reflective;
                vec3f la = amb * kd0;
                vec3f tkd = {1, 1, 1}, tks = {1, 1, 1};
                if (kd_txt >= 0) {
                    tkd = eval_texture<false>(S, kd_txt, uv, wc, lut);
                    la = la * tkd;
                }
                if (ks_txt >= 0) tks = eval_texture<false>(S, ks_txt, uv, wc, lut);
                vec3f c = {0.0f, 0.0f, 0.0f}, cd = {0.0f, 0.0f, 0.0f}, cs = {0.0f, 0.0f, 0.0f};
                vec3f v;
                float vlen;
                normalize_len(ro - p, v, vlen);
                for (int li = 0; li < S.nlights; li++) {
                    if (OCC4 ? ((occ_bits >> li) & 1u) != 0u : ldb(B.occl + (size_t)li * B.capacity + idx) != 0) continue;
                    vec3f l, ke;
                    float r;
                    light_reach(S.lights + 6 * li, p, l, r, ke);
                    vec3f kd = kd0, ks = ks0;
                    if (kd_txt >= 0) kd = kd * tkd;
                    if (ks_txt >= 0) ks = ks * tks;
                    vec3f ld, ls;
                    light_term(kind, nrm, v, l, r, ke, kd, ks, ns, ld, ls);
                    c = c + (ld + ls);
                    cd = cd + ld;
                    cs = cs + ls;
                }
                pc = c, pd = cd, ps = cs, pla = la;
                if (!reflective) {
                    R = c + la;
                } else {
                    // depth cap: the reflected contribution counts as a miss (col = 0)
                    truncated++;
                    vec3f t = {0.0f * kr.x, 0.0f * kr.y, 0.0f * kr.z};
                    pr = t;
                    R = (c + t) + la;
                }
            }
        }
        if constexpr (FUSE) {
            // (one round per block: the rows are written once)
            auto put = [&](int k, const vec3f& val) {
                if (!(P.mask >> k & 1)) return;  // (uniform)
                fused[(k * 3 + 0) * ROW + threadIdx.x] = val.x;
                fused[(k * 3 + 1) * ROW + threadIdx.x] = val.y;
                fused[(k * 3 + 2) * ROW + threadIdx.x] = val.z;
            };
            put(pass_direct, pc), put(pass_diffuse, pd), put(pass_specular, ps);
            put(pass_reflection, pr), put(pass_ambient, pla), put(pass_count, R);
            continue;  // one level: no mirror rays
        }
    }
    }
    if (FUSE) {
        // raytrace.cpp:232-249 per plane: one lane per (pixel, plane, colour component), each
        // lane's sum the reference's ordered chain of adds for that component
        __syncthreads();
        sum_plane_rows<SB>(
            A, C, fused, std::integral_constant<int, pass_planes>{}, [&](int k) { return P.mask >> k & 1; },
            [&](int k) { return P.out[k]; });
    }
    flush(counters, cnt_depth_truncated, truncated);
}

// ---- light groups (yrt_render_light_groups): one walk, one beauty plane per set of lights ----
// A plane is the image of a scene variant: plane k's shade() runs the light loop over its own
// lights only, in scene order, from c = +0, and adds la = amb * kd only where the plane has the
// ambient term. A group plane has its group's lights and no ambient; the ambient plane no light
// and the caller's ambient; the beauty every light and the ambient. The closest hits, the shadow
// rays' answers and the mirror rays (the spawn depends on kr alone) are the same for every
// plane, so they are made once; what differs is the light loop, the fold and the per-pixel sum.
// The planes are shaded group-major with ONE accumulator: per sample the surface, the material,
// the textures and v once, then per plane c = +0, that plane's lights (the host sorts them by
// plane, stably, into `tab`; the indices do not depend on the lane and are scalar reads), and c
// -- or the value folded from it -- leaves for plane k before the next plane starts. Inside a
// plane the additions are shade_hit's in shade_hit's order, so a plane has the bits yrt_render
// writes for its variant. A plane without the ambient term skips the mirror fold's `+ la`: its
// la is (0 * kd) * texel, +0 or -0 for a finite kd, and the sum it would be added to is never
// -0 (it ends in an addition to c, which starts at +0), so the bits are the same; level 0's
// `+ la` and the `0 * kr` of a cut mirror ray are computed as written.
// k_shade_groups has a body of its own, like the fused k_shade_passes: shade_hit keeps one c
// per call. It shares light_reach, light_term and compact_mirror_rays with shade_hit and
// shade_samples, and sum_plane_rows with the fused k_shade_passes; the statements listed at
// shade_hit are written out here (kd and ks once per sample, the spawn ahead of the planes) and
// change with theirs, and the fold is shade_samples' per plane (tests/test_gpu_light_groups.py
// compares every plane with yrt_render of its variant bit for bit).
struct group_buffers {  // (group_planes planes: wf_workspace.h)
    int nplanes;              // planes in use, [0, nplanes)
    unsigned amb_mask;        // bit k: plane k adds la (the ambient plane and the beauty)
    // behind the workspace: tab[k], tab[k + 1] bound plane k's entries of tab + group_planes + 1,
    // each the index of a light
    const int* tab;
    float4* out[group_planes];  // the caller's planes (window layout, out_stride)
    f4* smp[group_planes];      // per-sample values (unfused and mirror shapes); plane 0's is B.rad
    // mirror levels: plane k's {c.xyz, material index} of level l at rec[k] + l * capacity (plane
    // 0's is B.rec0_); la, the same for every plane that adds it, is B.rec1
    f4* rec[group_planes];
};

// Fused (one level, whole pixels per block): the per-sample values go to LDS rows of SB + 1
// floats per (plane, component), 30.8 KB for the ten planes; with the sRGB table a block takes
// 31.9 KB, five blocks fit a CU's 160 KB: 5 waves per SIMD, the kernel's launch bound.
constexpr int shade_group_waves = 5;
template <bool FUSE, int SB = WF_BLOCK, bool OCC4 = false>
__global__ __launch_bounds__(SB, shade_group_waves) void k_shade_groups(dev_scene_view S, dev_render_args A, int level,
                                                                        int nsamp_level0, int max_depth, wf_buffers B,
                                                                        group_buffers G, unsigned long long* counters,
                                                                        chunk_args C) {
    constexpr int ROW = SB + 1;
    __shared__ float fused[FUSE ? group_planes * 3 * ROW : 1];
    __shared__ int cmp_count[SB / 64], cmp_base[SB / 64];
    __shared__ srgb_table srgb_lds;
    const float* lut = stage_srgb<SB, true>(S, srgb_lds);
    work_counts wc;
    unsigned long long truncated = 0;
    // (the ambient and the view point as scalars of their own, not as parts of the eight-dword
    // kernel-argument loads that bring them in: such a tuple, live across the kernel, left an
    // unused 32-byte spill slot, and with it a private segment, behind)
    float amb_x = A.amb[0], amb_y = A.amb[1], amb_z = A.amb[2];
    float cam_x = A.cam.ox, cam_y = A.cam.oy, cam_z = A.cam.oz;
    asm volatile("" : "+s"(amb_x), "+s"(amb_y), "+s"(amb_z), "+s"(cam_x), "+s"(cam_y), "+s"(cam_z));
    const vec3f amb = {amb_x, amb_y, amb_z};
    const vec3f cam_o = {cam_x, cam_y, cam_z};
    const int nplanes = G.nplanes;
    const int* order = G.tab + group_planes + 1;
    const int stride = gridDim.x * SB;
    const int gout = (int)(blockIdx.x % (unsigned)level_segments);
    const int nseg = FUSE ? 1 : level ? level_segments : 1;
    for (int g = 0; g < nseg; g++) {
    const int n = (!FUSE && level) ? *seg_counter(B.count, level, g) : nsamp_level0;
    const int nround = (n + stride - 1) / stride;
    for (int round = 0; round < nround; round++) {
        const int j = round * stride + blockIdx.x * SB + threadIdx.x;
        const int idx = FUSE ? j : g * B.seg + j;
        // what does not depend on the plane, once per sample
        bool hit = false, write_r = false, spawn = false, reflective = false;
        vec3f p = {0, 0, 0}, nrm = {0, 0, 0}, v = {0, 0, 0}, dr = {0, 0, 0};
        vec3f kd = {0, 0, 0}, ks = {0, 0, 0}, kr = {0, 0, 0}, la = {0, 0, 0}, la0 = {0, 0, 0}, t = {0, 0, 0};
        float ns = 0.0f;
        int mat = 0, kind = 0;
        uint32_t occ_bits = 0;
        if (j < n) {
            const float4 s0 = ld4s(B.surf0 + idx);
            if constexpr (OCC4) {
                // (four unconditional loads, a light past the scene's reading light 0's byte;
                // only the bits of the plane's own lights are looked at, so no `q < S.nlights`
                // mask as in shade_samples' gather: with it the kernel has other instructions)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int lq = q < S.nlights ? q : 0;
                    occ_bits |= (ldb(B.occl + (size_t)lq * B.capacity + idx) != 0u ? 1u : 0u) << q;
                }
            }
            const int info = sample_state(s0);
            write_r = info != -2;
            hit = info >= 0;
            if (hit) {
                // level >= 1: this sample's ray record {origin, parent index}
                const float4 ro4 =
                    (!FUSE && level) ? ld4(B.ray_o(level) + idx) : make_float4(cam_o.x, cam_o.y, cam_o.z, 0.0f);
                vec2f uv;
                {
                    const float4 s1 = ld4s(B.surf1 + idx);
                    p = xyz(s0), nrm = xyz(s1), uv = {s1.w, B.need_v ? lds1(B.surfv + idx) : 0.0f};
                    mat = info_mat(info), kind = info & 3;
                }
                const vec3f ro = xyz(ro4);
                const float4 m0 = ld4(S.mats + 4 * mat), m1 = ld4(S.mats + 4 * mat + 1);
                const float4 m2 = ld4(S.mats + 4 * mat + 2), m3 = ld4(S.mats + 4 * mat + 3);
                const vec3f kd0 = xyz(m0), ks0 = xyz(m1);
                kr = xyz(m2), ns = m0.w;
                const int kd_txt = ibits(m1.w), ks_txt = ibits(m2.w);
                reflective = ibits(m3.w) & mat_reflective;
                const vec3f zero = {0.0f, 0.0f, 0.0f};
                la = amb * kd0, la0 = zero * kd0;
                vec3f tkd = {1, 1, 1}, tks = {1, 1, 1};
                if (kd_txt >= 0) {
                    tkd = eval_texture<false>(S, kd_txt, uv, wc, lut);
                    la = la * tkd, la0 = la0 * tkd;
                }
                if (ks_txt >= 0) tks = eval_texture<false>(S, ks_txt, uv, wc, lut);
                // (shade_hit forms kd and ks per light, from the same operands each time)
                kd = kd0, ks = ks0;
                if (kd_txt >= 0) kd = kd * tkd;
                if (ks_txt >= 0) ks = ks * tks;
                float vlen;
                normalize_len(ro - p, v, vlen);
                if (reflective) {
                    if (FUSE || level + 1 >= max_depth || level + 1 >= B.nlevels) {
                        // depth cap: the reflected contribution counts as a miss (col = 0); counted once
                        truncated++;
                        t = {0.0f * kr.x, 0.0f * kr.y, 0.0f * kr.z};
                    } else {
                        spawn = true;
                        dr = (nrm * 2.0f * dot(nrm, v)) - v;
                        write_r = false;
                    }
                }
            }
        }
        // the planes, one after the other (uniform over the block: every lane walks the table)
        for (int k = 0; k < nplanes; k++) {
            const int q0 = __builtin_amdgcn_readfirstlane(G.tab[k]), q1 = __builtin_amdgcn_readfirstlane(G.tab[k + 1]);
            const bool ambk = G.amb_mask >> k & 1;
            vec3f R = {0, 0, 0};
            if (hit) {
                vec3f c = {0.0f, 0.0f, 0.0f};
                for (int q = q0; q < q1; q++) {
                    const int li = __builtin_amdgcn_readfirstlane(order[q]);
                    if (OCC4 ? ((occ_bits >> li) & 1u) != 0u : ldb(B.occl + (size_t)li * B.capacity + idx) != 0) continue;
                    vec3f l, ke, ld, ls;
                    float r;
                    light_reach(S.lights + 6 * li, p, l, r, ke);
                    light_term(kind, nrm, v, l, r, ke, kd, ks, ns, ld, ls);
                    c = c + (ld + ls);
                }
                const vec3f lak = ambk ? la : la0;
                if (!reflective)
                    R = c + lak;
                else if (!spawn)
                    R = (c + t) + lak;
                else
                    G.rec[k][(size_t)level * B.capacity + idx] = {c.x, c.y, c.z, __int_as_float(mat)};
            }
            if constexpr (FUSE) {
                // (one round per block: the rows are written once; a lane past the chunk writes +0)
                fused[(k * 3 + 0) * ROW + threadIdx.x] = R.x;
                fused[(k * 3 + 1) * ROW + threadIdx.x] = R.y;
                fused[(k * 3 + 2) * ROW + threadIdx.x] = R.z;
            } else if (write_r) {
                // a final value at level k >= 1 folds up its chain of parents (raytrace.cpp:201-206,
                // R_k-1 = (D + R_k * kr) + la) to the camera sample, plane by plane
                vec3f col = R;
                int lev = level, node = idx;
                while (lev > 0) {
                    const int parent = ibits(B.ray_o(lev)[node].w);
                    const float4 d = ld4(G.rec[k] + (size_t)(lev - 1) * B.capacity + parent);
                    const float4 pkr = ld4(S.mats + 4 * ibits(d.w) + 2);  // the parent's material kr
                    vec3f cc = {d.x, d.y, d.z};
                    const vec3f tt = {col.x * pkr.x, col.y * pkr.y, col.z * pkr.z};
                    cc = cc + tt;
                    if (ambk) cc = cc + xyz(ld4(B.rec1(lev - 1) + parent));
                    col = cc, node = parent, lev--;
                }
                G.smp[k][node] = {col.x, col.y, col.z, 1.0f};
            }
        }
        if constexpr (FUSE) continue;  // one level: no mirror rays
        // the mirror rays, spawned and compacted once for all planes
        const unsigned long long mask = __ballot(spawn);
        if (spawn) B.rec1(level)[idx] = {la.x, la.y, la.z, 0};
        compact_mirror_rays<SB>(B, level, gout, idx, spawn, mask, p, dr, cmp_count, cmp_base);
    }
    }
    if (FUSE) {
        // raytrace.cpp:232-249 per plane: one lane per (pixel, plane, colour component), each
        // lane's sum the reference's ordered chain of adds for that component
        __syncthreads();
        sum_plane_rows<SB>(A, C, fused, nplanes, [](int) { return true; }, [&](int k) { return G.out[k]; });
    }
    flush(counters, cnt_depth_truncated, truncated);
}

// ---- level 0's shadow rays and shading in one persistent grid ----
#if !defined(YRT_SHADOW_SHADE_FUSE)  // (its non-default build is the `unfused` library of tools/build_variants.py)
// one level, 1 / 4 / 16 / 64 spp, at most 32 lights: an item of the any-hit grid (a 64-sample
// block with all its lights, YRT_SHADOW_ITEM_LIGHTS) is whole pixels in one wave, which knows
// every light's answer when the item ends. The wave shades and sums its pixels at once
// (k_shadow_shade_persist) instead of writing occlusion bytes for a k_shade launch to read back
// (A/B, one process, shadow + shade: c4 9.29 -> 9.02 ms, instance1k 6.37 -> 6.11, instance100k
// 4.89 -> 4.60, rank 0 of 8 1.28 -> 1.23; with the 64-spp sum not unrolled c4 was 9.31)
#define YRT_SHADOW_SHADE_FUSE 1
#endif
// (built on the item-lights grid: the variant without it, YRT_SHADOW_ITEM_LIGHTS=0, keeps the
// two kernels)
#define YRT_SHADOW_SHADE_KERNEL (YRT_SHADOW_SHADE_FUSE && YRT_SHADOW_ITEM_LIGHTS)
#if !defined(YRT_LIGHT_CARRY)
// k_shadow_shade_persist: each of an item's first four lights leaves its {l, r} per lane in LDS for
// the item's shading, which then does not redo transform_point + normalize_len per unoccluded
// light; 0: shade_hit computes them again
#define YRT_LIGHT_CARRY 1
#endif
#if (YRT_SHADOW_SHADE_KERNEL)
// k_shadow_persist<0>'s item loop with the answers kept as one bit per light and lane, then
// per item k_shade<fused>'s body: shade_hit for the lane's sample, the 64 values through a
// per-wave LDS slab, sum_pixels over the item's 64 / spp pixels. A wave does its own items:
// no block barrier inside the loop.
__global__ __launch_bounds__(SP_BLOCK, YRT_SHADOW_WAVES) void k_shadow_shade_persist(dev_scene_view S,
                                                                                      dev_render_args A, int nsamp,
                                                                                      int nx, wf_buffers B,
                                                                                      unsigned long long* counters,
                                                                                      chunk_args C,
                                                                                      float4* __restrict__ out) {
    constexpr int WPB = SP_BLOCK / 64;  // waves per block
    constexpr unsigned RUN = YRT_SHADOW_ITEM_RUN;
    // per wave: the item's 64 radiance values for sum_pixels, and (YRT_LIGHT_CARRY) ahead of them,
    // in the same rows, each of the first CARRY lights' {l, r} per lane from its light step to the
    // item's shading: row 0 is written as radiance once the shading has read it
    constexpr int CARRY = YRT_LIGHT_CARRY ? 4 : 0;
    __shared__ float4 wave_slab[WPB][CARRY ? CARRY : 1][64];
    __shared__ unsigned wave_truncated[WPB];  // (in LDS: a register would be live across the walks)
    __shared__ srgb_table srgb_lds;
    // the epilogue reads the frame's and the chunk's arguments from an LDS copy, per item: as
    // scalars they and what the compiler derives from them ahead of the loop (the reciprocals
    // of the pixel enumeration's divisors, float(spp)) would be held across the walks
    __shared__ struct {
        dev_render_args A;
        chunk_args C;
    } args;
    const float* lut = stage_srgb<SP_BLOCK, false>(S, srgb_lds);  // (its barrier: the one below)
    if (threadIdx.x == 0) args.A = A, args.C = C;
    __syncthreads();
    // (the view point as three scalars of their own, not as part of the four-dword kernel-argument
    // load that brings it in: that tuple, live across the whole kernel, left an unused 16-byte
    // spill slot, and with it a private segment, behind)
    float cam_x = A.cam.ox, cam_y = A.cam.oy, cam_z = A.cam.oz;
    asm volatile("" : "+s"(cam_x), "+s"(cam_y), "+s"(cam_z));
    const vec3f cam_o = {cam_x, cam_y, cam_z};
    const int nl = S.nlights;
    __builtin_assume(nl > 0);  // (run() launches the any-hit grid for scenes with lights)
    const unsigned n_items = (unsigned)nx;
    // The lane index is taken again wherever it is needed, opaque to the compiler, and the
    // wave index is a scalar: nothing derived from threadIdx.x is live across the walks. (With
    // one `lane` for the kernel the compiler hoists what the epilogue derives from it -- the
    // pixel, the component, the LDS addresses -- out of the item loop and spills it, 9 VGPRs.)
    auto lane_now = []() {
        unsigned l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return l;
    };
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned xcd = blockIdx.x % 8u;
    // wave-uniform: this wave's shadow rays (the reference's count) and those answered without a walk
    unsigned rays = 0, culled = 0;
    if (lane_now() == 0) wave_truncated[w] = 0;
    constexpr unsigned CS = YRT_SHADOW_BLOCK_CHUNK;
    __shared__ chunk_ring ring;
    const unsigned head = head_items<RUN, CS>(n_items);
    chunk_ring_init<CS>(ring, B.queue + xcd, B.queue + 8, head / 8u);
    for (;;) {
        const unsigned q = chunk_ring_next<CS>(ring, B.queue + xcd, lane_now(), B.queue + 8, head / 8u);
        const unsigned it = split_item<RUN>(q, xcd, n_items, head);
        if (it >= n_items) break;
        const int bx = (int)it;
        uint32_t occ_bits = 0;  // bit li: light li is occluded for this lane's sample (or its term is zero)
        for (int li = 0; li < nl; li++) {
            bool valid;
            const bool occ = shadow_item_light<0, true, true>(S, B, nsamp, bx, li, nl, lane_now(), cam_o, nullptr, rays,
                                                              culled, valid, li < CARRY ? wave_slab[w][li] : nullptr);
            occ_bits |= (occ ? 1u : 0u) << li;
        }
        // the item's samples are shaded (k_shade<fused>'s body for one sample) ...
        const int idx = bx * 64 + (int)lane_now();
        vec3f R = {0, 0, 0};
        unsigned long long truncated = 0;
        if (idx < nsamp) {
            const float4 s0 = ld4(B.surf0 + idx);
            const int info = sample_state(s0);
            if (info >= 0) {
                const float4 ro4 = make_float4(cam_o.x, cam_o.y, cam_o.z, 0.0f);
                const float* amb = args.A.amb;
                work_counts wc;
                vec3f p = {0, 0, 0}, dr = {0, 0, 0}, rec_d = {0, 0, 0}, rec_la = {0, 0, 0};
                int rec_mat = 0;
                bool spawn = false, write_r = true;
                shade_hit<false, true, true, true>(S, B, idx, info, s0, ro4, occ_bits, 0, 1, amb, lut, wc, truncated, R, p,
                                             spawn, dr, rec_d, rec_la, rec_mat, write_r, (no_terms*)nullptr,
                                             CARRY ? &wave_slab[w][0][lane_now()] : nullptr, CARRY);
            }
        }
        const unsigned lane = lane_now();
        const unsigned ntrunc = (unsigned)__popcll(ballot(truncated != 0));
        if (ntrunc && lane == 0) wave_truncated[w] += ntrunc;
        // ... and its pixels summed from the wave's own slab: the wave's LDS operations complete
        // in order, the waits keep the compiler from moving them across each other
        wave_slab[w][0][lane] = make_float4(R.x, R.y, R.z, 1.0f);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every lane's value, before any lane sums
        // (one pixel per item, 64 spp, is the long chain: 64 dependent adds per item)
        const int spp = __builtin_amdgcn_readfirstlane(args.C.spp);
        if (spp == 64) {
            sum_pixels<64, 64>(args.A, args.C, out, wave_slab[w][0], bx, 1, (int)lane);
        } else {
            const int sl = __builtin_ctz((unsigned)spp);  // (spp divides 64: a power of two)
            sum_pixels<64>(args.A, args.C, out, wave_slab[w][0], bx << (6 - sl), 64 >> sl, (int)lane);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the sums' reads, before the next item's values
    }
    const unsigned lane = lane_now();
    const unsigned long long first = lane == 0 ? 1ull : 0ull;
    // (the counters' indices as selects: a table of three indexed by a register takes a stack slot)
    flush_block_at<3, SP_BLOCK>(
        counters, {first * rays, first * culled, first * (lane == 0 ? wave_truncated[w] : 0u)},
        (unsigned)w * 64u + lane,
        [](unsigned k) { return k == 0 ? cnt_shadow_rays : k == 1 ? cnt_shadow_culled : cnt_depth_truncated; });
}
#endif

// ---- ordered per-pixel sum (raytrace.cpp:232-249) ----
// A wave sums 64 pixels. Their samples are consecutive in memory (spp per pixel), so the
// wave stages them through LDS AQ samples of every pixel at a time with loads in which
// neighbouring lanes read neighbouring samples (a pixel's AQ samples are one contiguous
// run), then each lane adds its own pixel's samples in the reference's order.
// One plane: the chunk's per-sample values samples() summed into the window out() (the body of
// k_accumulate and, per plane, of k_accumulate_passes). The two pointers come as callables,
// read where they are used, and A and C by value as the kernels take them: so both kernels
// compile to the instructions they had with a body each.
constexpr int AQ = 8;
template <class SMP, class OUT>
__device__ __forceinline__ void accumulate_plane(dev_render_args A, chunk_args C, SMP&& samples, OUT&& out) {
    __shared__ float4 stage[WF_BLOCK / 64][64 * (AQ + 1)];  // rows padded against bank conflicts
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pl0 = blockIdx.x * WF_BLOCK + w * 64;
    const int np = max(0, min(64, C.npix - pl0));  // pixels of this wave
    float4* S = stage[w];
    const f4* base = samples() + (size_t)pl0 * C.spp;
    vec3f acc = {0, 0, 0};
    for (int q0 = 0; q0 < C.spp; q0 += AQ) {  // the same trip count in every wave of the block
        const int qn = min(AQ, C.spp - q0);
        for (int e = lane; e < np * qn; e += 64) {
            const int px = e / qn, q = e % qn;
            S[px * (AQ + 1) + q] = ld4(base + (size_t)px * C.spp + q0 + q);
        }
        __syncthreads();
        if (lane < np)
            for (int q = 0; q < qn; q++) {
                const float4 c = S[lane * (AQ + 1) + q];
                acc = {acc.x + c.x, acc.y + c.y, acc.z + c.z};
            }
        __syncthreads();
    }
    if (lane >= np) return;
    const int pl = pl0 + lane;
    int lx, ly, i, j;
    const bool valid = pixel_of(A, C, C.pix0 + pl, lx, ly, i, j);
    if (lx >= A.tile_w || ly >= A.tile_h) return;
    const float d = float(C.spp);
    out()[(size_t)ly * A.out_stride + lx] =
        valid ? make_float4(acc.x / d, acc.y / d, acc.z / d, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(WF_BLOCK) void k_accumulate(dev_render_args A, chunk_args C, wf_buffers B,
                                                         float4* __restrict__ out) {
    accumulate_plane(A, C, [&] { return B.rad; }, [&] { return out; });
}

// the shading passes' planes: blockIdx.y is the plane, its samples P.smp[k] (the beauty's B.rad)
__global__ __launch_bounds__(WF_BLOCK) void k_accumulate_passes(dev_render_args A, chunk_args C, wf_buffers B,
                                                                pass_buffers P) {
    const int k = (int)blockIdx.y;
    if (!(P.mask >> k & 1)) return;  // (uniform over the block)
    accumulate_plane(A, C, [&] { return k == pass_count ? B.rad : P.smp[k]; }, [&] { return P.out[k]; });
}

// the light groups' planes: blockIdx.y is the plane, its samples G.smp[k]
__global__ __launch_bounds__(WF_BLOCK) void k_accumulate_groups(dev_render_args A, chunk_args C, group_buffers G) {
    const int k = (int)blockIdx.y;
    accumulate_plane(A, C, [&] { return G.smp[k]; }, [&] { return G.out[k]; });
}

// The workspace at `base` as the kernels' buffers: every slab of the walk (wf_workspace.h) to the
// member it is. P, G: the planes of yrt_render_passes or yrt_render_light_groups, else null.
wf_buffers carve(void* base, const workspace_shape& s, pass_buffers* P, group_buffers* G) {
    wf_buffers B = {};
    workspace_carver w(base);
    int pass = -1;  // the wanted pass that took the last slab_pass_smp
    walk_workspace(s, [&](wf_slab slab, int k, size_t bytes) {
        void* const p = w.take(bytes);
        switch (slab) {
            case slab_count: B.count = (int*)p; break;
            case slab_queue: B.queue = (unsigned*)p; break;
            case slab_lstats: B.lstats = (unsigned long long*)p; break;
            case slab_surf0: B.surf0 = (f4*)p; break;
            case slab_surf1: B.surf1 = (f4*)p; break;
            case slab_surfv: B.surfv = (float*)p; break;
            case slab_occl: B.occl = (unsigned char*)p; break;
            case slab_rad: B.rad = (f4*)p; break;
            case slab_pbox: B.pbox = (f4*)p; break;
            case slab_lcount: B.lcount = (int*)p; break;
            case slab_lskip: B.lskip = (int*)p; break;
            case slab_lists: B.lists = (f4*)p; break;
            case slab_slists: B.slists = (f4*)p; break;
            case slab_ccount: B.ccount = (int*)p; break;
            case slab_cskip: B.cskip = (int*)p; break;
            case slab_clist: B.clist = (f4*)p; break;
            case slab_ray_o: B.ray_o_ = (f4*)p; break;
            case slab_ray_d: B.ray_d_ = (f4*)p; break;
            case slab_rec0: B.rec0_ = (f4*)p; break;
            case slab_rec1: B.rec1_ = (f4*)p; break;
            case slab_pass_smp:
                do pass++;
                while (!(P->mask >> pass & 1));
                P->smp[pass] = (f4*)p;
                break;
            case slab_group_tab: G->tab = (const int*)p; break;
            case slab_group_smp: G->smp[k] = (f4*)p; break;
            case slab_group_rec: G->rec[k] = (f4*)p; break;
        }
    });
    if (G) G->smp[0] = B.rad, G->rec[0] = B.rec0_;
    B.capacity = s.cap;
    B.nlevels = s.nlevels;
    return B;
}

// ---- the host code of run() and run_rays() ----

// a call without a chunk launches no k_chunk_setup: the counters still start at 0, or
// yrt_last_stats would report the call before this one
hipError_t clear_counters(unsigned long long* counters, hipStream_t stream) {
    return counters ? hipMemsetAsync(counters, 0, (size_t)cnt_slots * cnt_count * sizeof(unsigned long long), stream)
                    : hipSuccess;
}

// Samples per chunk, bytes_of(target) being the workspace of a chunk of `target` samples: a
// whole frame at c3/c4, 15 chunks at c5. A reflective scene keeps per-level records for
// every level (64 B per sample and level). The chunk is halved until the workspace takes at
// most half of the free HBM (deep mirror recursions run as more, smaller chunks); a depth
// whose smallest chunk (2^16 samples, or the knob's own target when that starts lower: the
// halving never raises it) still does not fit is refused.
template <class F>
long long chunk_target(const device_scene& ds, const dev_render_args& A, F&& bytes_of) {
    long long target = 1ll << (ds.reflective ? MIRROR_CHUNK_LOG2 : CHUNK_LOG2);
    // the free-memory query (a driver round trip) only when the workspace must grow: a
    // steady frame loop reuses the workspace it already has
    if (bytes_of(target) > ds.work_bytes) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        free_b += ds.work_bytes;  // the current workspace is given back if it is regrown
        while (target > (1ll << 16) && bytes_of(target) > free_b / 2) target /= 2;
        if (bytes_of(target) > free_b)
            throw unsupported_error("max_depth " + std::to_string(A.max_depth) + " needs " +
                                    std::to_string(bytes_of(target) >> 20) + " MiB of mirror-level records for its " +
                                    "smallest chunk; " + std::to_string(free_b >> 20) + " MiB of HBM are free");
    }
    return target;
}

// the handle's workspace holds at least `need` bytes
hipError_t grow_workspace(device_scene& ds, size_t need) {
    if (need <= ds.work_bytes) return hipSuccess;
    if (ds.work) (void)hipFree(ds.work);
    ds.work = nullptr;
    ds.work_bytes = 0;
    hipError_t e = hipMalloc(&ds.work, need);
    if (e == hipSuccess) ds.work_bytes = need;
    return e;
}

// The mirror levels' ray counts on the host. The host reads each level's count (written by the
// previous level's shading) without draining the stream: the copy is queued behind that
// shading (fetch_level_counts), the level's k_bounce, which takes its count on the device,
// behind the copy, and only then does the host wait for the copy (level_has_rays).
hipError_t make_level_counts(device_scene& ds) {
    if (!ds.level_count_host) {
        hipError_t e = hipHostMalloc((void**)&ds.level_count_host, sizeof(int) * level_segments * count_stride,
                                     hipHostMallocDefault);
        if (e != hipSuccess) return e;
    }
    if (!ds.level_count_ev) return hipEventCreateWithFlags(&ds.level_count_ev, hipEventDisableTiming);
    return hipSuccess;
}
// the list sums of the last render that built lists, on the host (behind list_stats_ev)
hipError_t make_list_stats(device_scene& ds) {
    if (!ds.list_stats_host) {
        hipError_t e =
            hipHostMalloc((void**)&ds.list_stats_host, list_sums * sizeof(unsigned long long), hipHostMallocDefault);
        if (e != hipSuccess) return e;
        memset(ds.list_stats_host, 0, list_sums * sizeof(unsigned long long));
    }
    if (!ds.list_stats_ev) return hipEventCreateWithFlags(&ds.list_stats_ev, hipEventDisableTiming);
    return hipSuccess;
}
hipError_t fetch_level_counts(device_scene& ds, const wf_buffers& B, int level, hipStream_t stream) {
    hipError_t e = hipMemcpyAsync(ds.level_count_host, B.count + (size_t)level * level_segments * count_stride,
                                  sizeof(int) * level_segments * count_stride, hipMemcpyDeviceToHost, stream);
    return e == hipSuccess ? hipEventRecord(ds.level_count_ev, stream) : e;
}
hipError_t level_has_rays(device_scene& ds, bool& any) {
    hipError_t e = hipEventSynchronize(ds.level_count_ev);
    any = false;
    for (int g = 0; e == hipSuccess && g < level_segments; g++) any |= ds.level_count_host[g * count_stride] != 0;
    return e;
}

// The chunk's setup (k_chunk_setup): the zeroed work queues and mirror-level counters; in a
// call's first chunk the zeroed work counters; the zeroed list sums where lstats is given; and
// the nrec camera-relative instance-level records of a render seen from cam4 (0: none).
void launch_chunk_setup(const device_scene& ds, const wf_buffers& B, int nrec, const float4& cam4,
                        unsigned long long* lstats, int nlevels, unsigned long long* counters, bool first_chunk,
                        hipStream_t stream) {
    const int count_ints = nlevels > 1 ? (int)(count_bytes(nlevels) / sizeof(int)) : 0;
    const int counter_words = first_chunk && counters ? cnt_slots * cnt_count : 0;
    const int work = std::max(std::max(nrec, count_ints), std::max(counter_words, 32));
    const int nb = std::min((work + WF_BLOCK - 1) / WF_BLOCK, 1024);
    hipLaunchKernelGGL(k_chunk_setup, dim3(nb), dim3(WF_BLOCK), 0, stream, nrec ? ds.view.tpair : nullptr, nrec,
                       cam4.x, cam4.y, cam4.z, ds.trel, B.queue, lstats, B.count, count_ints, counters,
                       counter_words);
}

// How a call is split into chunks, and the carved workspace of one chunk. A unit is a pixel
// (run(): whole tiles, so `granule` is TILE * TILE) or a ray (run_rays(): spp 1, granule 1).
struct chunk_plan {
    int nlevels;    // one level per trace_first call a sample may make
    bool fuse;      // one level and whole pixels per block: the shading kernels sum the pixels themselves
    int per_chunk;  // units of a chunk
    int seg, cap;   // slots per segment of a mirror level, and per sample record
    wf_buffers B;
};
// P, G: the call's copy of its passes' or groups' planes, which gets their slabs; else null
hipError_t plan_chunks(device_scene& ds, const dev_render_args& A, long long units, int granule, int spp,
                       pass_buffers* P, group_buffers* G, chunk_plan& plan) {
    // one level per trace_first call a camera sample may make (A.max_depth; the reference
    // recursion is unbounded, so the caller's depth is kept as given)
    const int nlevels = plan.nlevels = ds.reflective ? std::max(A.max_depth, 1) : 1;
    // (k_shade FUSE; one-wave fused blocks lose: +9 %)
    const bool fuse = plan.fuse = nlevels == 1 && WF_BLOCK % spp == 0;
    // the passes' per-sample planes (16 B per wanted pass and sample; the fused shape keeps
    // them in LDS)
    const int smp_planes = P && !fuse ? __builtin_popcount(P->mask & ((1u << pass_count) - 1)) : 0;
    auto units_for = [&](long long tgt) {
        const int u = (int)std::max<long long>(1, std::min<long long>(units, tgt / spp));
        return (u + granule - 1) / granule * granule;
    };
    // slots per sample record: a chunk's samples, and with mirror levels a slack so that
    // every segment of a level holds whatever k_shade's blocks of that segment spawn: at
    // level 0 one round of 256-sample blocks puts at most cap / 8 + 256 rays into a
    // segment, at later levels (a grid-stride grid of 2048 blocks over up to 8 input
    // segments) at most cap / 8 + 8 * 256
    auto seg_of = [&](int u) { return u * spp / level_segments + level_segments * WF_BLOCK; };
    auto cap_of = [&](int u) { return nlevels > 1 ? level_segments * seg_of(u) : u * spp; };
    auto shape_of = [&](int u) {
        const size_t samples = (size_t)u * spp;
        return workspace_shape{cap_of(u), spp, ds.nlights, nlevels, smp_planes, samples,
                               G ? G->nplanes : 0, fuse ? 0 : samples};
    };
    plan.per_chunk =
        units_for(chunk_target(ds, A, [&](long long tgt) { return workspace_bytes(shape_of(units_for(tgt))); }));
    plan.seg = seg_of(plan.per_chunk);
    plan.cap = cap_of(plan.per_chunk);
    const workspace_shape shape = shape_of(plan.per_chunk);
    if (hipError_t e = grow_workspace(ds, workspace_bytes(shape)); e != hipSuccess) return e;
    plan.B = carve(ds.work, shape, P, G);
    plan.B.seg = plan.seg;
    plan.B.need_v = ds.view.ntextures > 0;
    return nlevels > 1 ? make_level_counts(ds) : hipSuccess;
}

// f(std::bool_constant<b>()): a run-time bool as a template argument inside a generic lambda
template <class F>
decltype(auto) with_bool(bool b, F&& f) {
    return b ? f(std::true_type()) : f(std::false_type());
}

// f(std::bool_constant<PACKET>(), SE()): the walk of a call. The packet walk's per-wave stack
// holds 32-bit node indices (no narrow/wide split needed); the per-lane walks' stack entries SE
// are 16-bit where every node index fits them.
template <class F>
hipError_t with_walk(const device_scene& ds, bool packet, F&& f) {
    if (packet) return f(std::true_type(), uint32_t());
    if (ds.narrow_stack) return f(std::false_type(), uint16_t());
    return f(std::false_type(), uint32_t());
}

constexpr int stride_grid = 2048;  // grid-stride kernels: 8 blocks of 256 per CU

// The levels of one chunk of nsamp samples whose level-0 closest hits are in B. A level with no
// mirror rays ends the chunk's recursion. The level's k_bounce is queued before the host waits
// for the level's ray count, so the GPU works on it while the count comes back; only a level
// that turns out empty costs a launch (one k_bounce of no rays).
// shadow(level): launches the level's shadow rays where the caller has a kernel of its own for
// them; false: they run on the k_shadow grid.
// shade(level, grid): launches the kernel that shades a level.
// level0_shaded: the caller's shadow kernel has shaded level 0 too.
template <bool COUNT, bool PACKET, typename SE, class SHADOW, class SHADE>
hipError_t run_levels(device_scene& ds, const wf_buffers& B, int nlevels, int nsamp, const float4& cam4,
                      unsigned long long* counters, hipStream_t stream, SHADOW&& shadow, bool level0_shaded,
                      SHADE&& shade) {
    phase_timer& T = ds.timer;
    constexpr int TB = shadow_block<PACKET>();
    for (int level = 0; level < nlevels; level++) {
        if (level > 0) {
            int t = T.begin(phase_bounce, stream);
            hipLaunchKernelGGL((k_bounce<COUNT, PACKET, SE>), dim3(stride_grid), dim3(WF_BLOCK), 0, stream, ds.view,
                               level, B, counters);
            T.end(t, stream);
            bool any;
            if (hipError_t e = level_has_rays(ds, any); e != hipSuccess) return e;
            if (!any) break;
        }
        if (ds.nlights > 0) {
            int t = T.begin(phase_shadow, stream);
            if (!shadow(level)) {
                const dim3 sg(level ? stride_grid * WF_BLOCK / TB : (nsamp + TB - 1) / TB, ds.nlights);
                with_bool(!COUNT && PACKET && ds.wide_ok, [&](auto wide) {
                    hipLaunchKernelGGL((k_shadow<COUNT, PACKET, SE, decltype(wide)::value>), sg, dim3(TB), 0, stream,
                                       ds.view, level, nsamp, B, counters, cam4);
                });
            }
            T.end(t, stream);
        }
        if (level == 0 && level0_shaded) continue;
        int t = T.begin(phase_shade, stream);
        shade(level, dim3(level ? stride_grid : (nsamp + WF_BLOCK - 1) / WF_BLOCK));
        T.end(t, stream);
        if (level + 1 < nlevels) {
            if (hipError_t e = fetch_level_counts(ds, B, level + 1, stream); e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

// passes: yrt_render_passes' planes (P.mask, P.out; out is then P.out[pass_count], the beauty,
// or null), shaded by k_shade_passes and summed by k_accumulate_passes; null: yrt_render
// groups: yrt_render_light_groups' planes (nplanes, amb_mask, out; ds.group_tab their table),
// shaded by k_shade_groups and summed by k_accumulate_groups; not together with passes
template <bool COUNT, bool PACKET, typename SE>
hipError_t run(device_scene& ds, const dev_render_args& A, float4* out, unsigned long long* counters,
               hipStream_t stream, const pass_buffers* passes = nullptr, const group_buffers* groups = nullptr) {
    const int spp = A.samples * A.samples;
    const int tiles_x = (A.tile_w + TILE - 1) / TILE;
    const int tiles_y = (A.tile_h + TILE - 1) / TILE;
    const long long npix_total = (long long)tiles_x * tiles_y * TILE * TILE;
    pass_buffers P = passes ? *passes : pass_buffers{};
    group_buffers G = groups ? *groups : group_buffers{};
    chunk_plan plan;
    if (hipError_t e = plan_chunks(ds, A, npix_total, TILE * TILE, spp, passes ? &P : nullptr,
                                   groups ? &G : nullptr, plan);
        e != hipSuccess)
        return e;
    const int nlevels = plan.nlevels, pix_per_chunk = plan.per_chunk;
    const bool fuse = plan.fuse;
    wf_buffers& B = plan.B;
    B.trel = ds.trel;
    // the frame's division pairs and range decisions, the same for every chunk (item_magic.h)
    const item_magic M = make_item_magic(spp, A.samples, tiles_x, A.band, (uint64_t)npix_total,
                                         (uint64_t)pix_per_chunk * spp, (uint64_t)tiles_y * TILE, A.width, A.height,
                                         A.x0, A.y0);
    if (groups) {
        // (the table's source, ds.group_tab, outlives the call; a copy from pageable memory is
        // staged before hipMemcpyAsync returns)
        if (hipError_t e = hipMemcpyAsync((void*)G.tab, ds.group_tab.data(), sizeof(int) * ds.group_tab.size(),
                                          hipMemcpyHostToDevice, stream);
            e != hipSuccess)
            return e;
    }
    bool list_stats = false;
    ds.last_camera_lists = ds.last_bundles = false;
    if (hipError_t e = make_list_stats(ds); e != hipSuccess) return e;
    phase_timer& T = ds.timer;
    // LDS staging of the instance tree's top (yrt_scene_set_lds_staging): the persistent walks
    // read it from LDS; the tile lists, whose walks start below it, are not built
    const bool stage = ds.lds_staging != 0 && !COUNT && PACKET;
    ds.last_lds_staging = 0;
    const float4 cam4 = make_float4(A.cam.ox, A.cam.oy, A.cam.oz, 0.0f);
    if (npix_total == 0) {  // (no chunk)
        if (hipError_t e = clear_counters(counters, stream); e != hipSuccess) return e;
    }
    for (long long pix0 = 0; pix0 < npix_total; pix0 += pix_per_chunk) {
        chunk_args C = {pix0, (int)std::min<long long>(pix_per_chunk, npix_total - pix0), spp, tiles_x};
        if (YRT_ITEM_MAGIC) C.M = M;
        const int nsamp = C.npix * spp;
        constexpr int TB = shadow_block<PACKET>();
        const int tgrid = (nsamp + TB - 1) / TB;
        // level 0's shadow rays run on the persistent any-hit grid (k_shadow_persist) -- on
        // any frame size when the caller forces the lists on (the bundles live there)
        const bool shadow_persist = !COUNT && PACKET && ds.wide_ok && TB == 64 && ds.nlights > 0 &&
                                    ((long long)tgrid * ds.nlights >= YRT_SHADOW_PERSIST_MIN_ITEMS ||
                                     ds.lists_mode == 1 || stage);
        // ... which shades its items too (k_shadow_shade_persist: no occlusion bytes, no k_shade
        // launch) where an item is whole pixels and a lane's lights fit its mask
        const bool shadow_shade = YRT_SHADOW_SHADE_KERNEL && shadow_persist && !stage &&
                                  nlevels == 1 && !passes && !groups && 64 % spp == 0 && ds.nlights <= 32;
        // ... and walk the bundles' candidate lists (k_bundle_lists) instead of the tree
        const bool bundles_possible = !stage && shadow_persist && bundle_lights(ds.nlights) > 0 &&
                                      ds.view.nwtop >= YRT_BUNDLE_MIN_TOP;
        // the camera rays walk their tiles' leaf lists (k_camera_lists)
        const bool cam_lists_possible = !stage && !COUNT && PACKET && ds.wide_ok && ds.view.nwtop >= YRT_BUNDLE_MIN_TOP;
        // YRT_LISTS_ON: whenever the scene allows; YRT_LISTS_AUTO: the same from
        // YRT_LISTS_MIN_SPP samples per pixel; _OFF: never (yrt_scene_set_tile_lists)
        const bool lists = ds.lists_mode == 1 || (ds.lists_mode == 0 && spp >= YRT_LISTS_MIN_SPP);
        B.cam_lists = cam_lists_possible && lists;
        B.bundles = bundles_possible && lists;
        ds.last_camera_lists |= B.cam_lists != 0, ds.last_bundles |= B.bundles != 0;
        const bool zero_lstats = (B.cam_lists || B.bundles) && !list_stats;
        list_stats |= zero_lstats;
        int t = T.begin(phase_lists, stream);
        // the camera-relative instance-level records of this render: the first chunk of a packet
        // render; timed in the lists phase, YRT_PHASE_LISTS, with the camera lists built from them
        launch_chunk_setup(ds, B, (PACKET && pix0 == 0) ? (int)ds.ntnodes * 2 * spine_len : 0, cam4,
                           zero_lstats ? B.lstats : nullptr, nlevels, counters, pix0 == 0, stream);
        if (B.cam_lists) {
            const int nt = C.npix / (TILE * TILE);
            hipLaunchKernelGGL(k_camera_lists, dim3((nt + 3) / 4), dim3(256), 0, stream, ds.view, A, C, B);
        }
        T.end(t, stream);
        t = T.begin(phase_primary, stream);
        bool persist = false;
        if constexpr (!COUNT && PACKET) {
            persist = ((long long)nsamp + 63) / 64 >= (long long)YRT_PRIMARY_PERSIST_MIN_ITEMS;
            if (persist) {  // (its work counters B.queue[16, 25) were zeroed by k_chunk_setup)
                const int nb = ds.num_cus * (YRT_PRIMARY_WAVES * 4 * 64 / YRT_PRIMARY_SP_BLOCK);
                if (B.cam_lists)
                    hipLaunchKernelGGL((k_primary_persist<SE, 0, true>), dim3(nb), dim3(YRT_PRIMARY_SP_BLOCK), 0,
                                       stream, ds.view, A, C, B, counters);
                else if (stage) {
                    hipLaunchKernelGGL((k_primary_persist<SE, YRT_PRIMARY_LDS_RECORDS, false>), dim3(nb),
                                       dim3(YRT_PRIMARY_SP_BLOCK), 0, stream, ds.view, A, C, B, counters);
                    ds.last_lds_staging |= 1;
                } else
                    hipLaunchKernelGGL((k_primary_persist<SE, 0, false>), dim3(nb), dim3(YRT_PRIMARY_SP_BLOCK), 0,
                                       stream, ds.view, A, C, B, counters);
            }
        }
        if (!persist)
            with_bool(B.cam_lists != 0, [&](auto list) {
                hipLaunchKernelGGL((k_primary<COUNT, PACKET, SE, decltype(list)::value>),
                                   dim3((nsamp + YRT_PRIMARY_BLOCK - 1) / YRT_PRIMARY_BLOCK), dim3(YRT_PRIMARY_BLOCK),
                                   0, stream, ds.view, A, C, B, counters);
            });
        T.end(t, stream);
        if (B.bundles) {  // the candidate lists of level 0's shadow items (shadow_persist, lights)
            t = T.begin(phase_lists, stream);
            const long long ns = (long long)super_count(nsamp) * ds.nlights;
            if (YRT_BUNDLE_FUSED) {
                hipLaunchKernelGGL(k_bundle_lists<true>, dim3((unsigned)ns), dim3(256), 0, stream, ds.view, B, tgrid);
            } else {
                hipLaunchKernelGGL(k_bundle_super, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, stream, ds.view, B,
                                   tgrid);
                const long long nw = (long long)bundle_count(nsamp) * ds.nlights;
                hipLaunchKernelGGL(k_bundle_lists<false>, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, stream,
                                   ds.view, B, tgrid);
            }
            T.end(t, stream);
        }
        // level 0 only: at c3 the mirror levels' compacted samples trace faster with the
        // hardware's dealing (shadow 1.64 -> 1.72 ms with them persistent)
        auto shadow = [&](int level) {
            if (level > 0 || !shadow_persist) return false;
            // one resident grid: two 1024-thread blocks per CU (8 waves per SIMD)
            // (its work counters B.queue[0, 9) were zeroed by k_chunk_setup)
            const int nb = ds.num_cus * (YRT_SHADOW_WAVES * 4 * 64 / SP_BLOCK);
            constexpr int L = YRT_SHADOW_LDS_RECORDS;
            if (stage && L > 0 && ds.view.nwtop >= L) {  // (the copy reads L whole records)
                hipLaunchKernelGGL((k_shadow_persist<L>), dim3(nb), dim3(SP_BLOCK), 0, stream, ds.view, nsamp, tgrid,
                                   B, counters, cam4);
                ds.last_lds_staging |= 2;
            }
#if (YRT_SHADOW_SHADE_KERNEL)
            else if (shadow_shade)
                hipLaunchKernelGGL(k_shadow_shade_persist, dim3(nb), dim3(SP_BLOCK), 0, stream, ds.view, A, nsamp,
                                   tgrid, B, counters, C, out);
#endif
            else
                hipLaunchKernelGGL((k_shadow_persist<0>), dim3(nb), dim3(SP_BLOCK), 0, stream, ds.view, nsamp, tgrid,
                                   B, counters, cam4);
            return true;
        };
        // (a fused shape has one level: its grid is level 0's)
        auto shade = [&](int level, dim3 grid) {
            with_bool(fuse, [&](auto fu) {
                with_bool(ds.nlights <= 4, [&](auto occ4) {
                    constexpr bool FU = decltype(fu)::value, OCC4 = decltype(occ4)::value;
                    if (groups) {
                        if constexpr (!COUNT)  // (launch_render_wavefront_light_groups never counts work)
                            hipLaunchKernelGGL((k_shade_groups<FU, WF_BLOCK, OCC4>), grid, dim3(WF_BLOCK), 0, stream,
                                               ds.view, A, level, nsamp, A.max_depth, B, G, counters, C);
                    } else if (passes) {
                        if constexpr (!COUNT)  // (launch_render_wavefront_passes never counts work)
                            hipLaunchKernelGGL((k_shade_passes<FU, WF_BLOCK, OCC4>), grid, dim3(WF_BLOCK), 0, stream,
                                               ds.view, A, level, nsamp, A.max_depth, B, P, counters, C);
                    } else
                        hipLaunchKernelGGL((k_shade<COUNT, FU, WF_BLOCK, OCC4>), grid, dim3(WF_BLOCK), 0, stream,
                                           ds.view, A, level, nsamp, A.max_depth, B, counters, C, out);
                });
            });
        };
        // (shadow_shade: k_shadow_shade_persist has shaded the chunk and written its pixels)
        if (hipError_t e = run_levels<COUNT, PACKET, SE>(ds, B, nlevels, nsamp, cam4, counters, stream, shadow,
                                                         shadow_shade, shade);
            e != hipSuccess)
            return e;
        if (!fuse) {
            t = T.begin(phase_accumulate, stream);
            if (groups)
                hipLaunchKernelGGL(k_accumulate_groups, dim3((C.npix + WF_BLOCK - 1) / WF_BLOCK, G.nplanes),
                                   dim3(WF_BLOCK), 0, stream, A, C, G);
            else if (passes)
                hipLaunchKernelGGL(k_accumulate_passes, dim3((C.npix + WF_BLOCK - 1) / WF_BLOCK, pass_planes),
                                   dim3(WF_BLOCK), 0, stream, A, C, B, P);
            else
                hipLaunchKernelGGL(k_accumulate, dim3((C.npix + WF_BLOCK - 1) / WF_BLOCK), dim3(WF_BLOCK), 0, stream, A,
                                   C, B, out);
            T.end(t, stream);
        }
        if (B.cam_lists || B.bundles) {
            t = T.begin(phase_lists, stream);
            hipLaunchKernelGGL(k_list_stats, dim3(64), dim3(256), 0, stream, B, C.npix / (TILE * TILE),
                               (int)(bundle_count(nsamp) * (size_t)ds.nlights));
            T.end(t, stream);
        }
    }
    if (list_stats) {
        hipError_t e = hipMemcpyAsync(ds.list_stats_host, B.lstats, list_sums * sizeof(unsigned long long),
                                      hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipEventRecord(ds.list_stats_ev, stream);
        if (e != hipSuccess) return e;
        ds.list_stats_recorded = true;
    }
    return hipGetLastError();
}

// ---- a ray batch (yrt_shade_rays): run()'s chunks and levels with the caller's rays as level 0 ----
// A ray is a sample and spp is 1: chunk r0 holds rays [r0, r0 + nsamp), its sample idx is ray
// r0 + idx. k_rays_first replaces eval_camera and the camera-relative walk; level 0's shadow
// rays run on the plain k_rays_shadow grid (the persistent any-hit grid's item order and the
// bundles' boxes are laid out for pixel tiles, and no camera list exists without a common
// origin), so the tile-list mode and the LDS staging of the handle change nothing here and the
// handle reports neither as used. The mirror levels, the fold and the workspace are run()'s;
// the fold's last step writes the ray's colour straight into `out` (B.rad), in batch order.
// soft (yrt_shade_rays_soft): every level's shadow rays are k_soft_shadow's K rays per light and
// its shading k_soft_shade's; null: yrt_shade_rays. keep_counters: no chunk is the call's first,
// so the batch's counts add to what the counter lines hold (a pixel-batch render's later batches)
template <bool PACKET, typename SE>
hipError_t run_rays(device_scene& ds, const dev_render_args& A, const float* rays, int n, float4* out,
                    unsigned long long* counters, hipStream_t stream, const soft_shadow_args* soft = nullptr,
                    bool keep_counters = false) {
    chunk_plan plan;
    if (hipError_t e = plan_chunks(ds, A, n, 1, 1, nullptr, nullptr, plan); e != hipSuccess) return e;
    wf_buffers& B = plan.B;
    ds.last_camera_lists = ds.last_bundles = false;
    ds.last_lds_staging = 0;
    phase_timer& T = ds.timer;
    const float4 cam4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (no level takes its view point from a camera)
    constexpr int TB = shadow_block<PACKET>();
    const float3 amb3 = make_float3(A.amb[0], A.amb[1], A.amb[2]);
    for (long long r0 = 0; r0 < n; r0 += plan.per_chunk) {
        const int nsamp = (int)std::min<long long>(plan.per_chunk, n - r0);
        B.rays = rays + (size_t)r0 * 8;
        B.rad = reinterpret_cast<f4*>(out + r0);
        int t = T.begin(phase_lists, stream);
        // (no camera-relative records)
        launch_chunk_setup(ds, B, 0, cam4, nullptr, plan.nlevels, counters, r0 == 0 && !keep_counters, stream);
        T.end(t, stream);
        t = T.begin(phase_primary, stream);
        hipLaunchKernelGGL((k_rays_first<PACKET, SE>), dim3((nsamp + WF_BLOCK - 1) / WF_BLOCK), dim3(WF_BLOCK), 0,
                           stream, ds.view, nsamp, B, counters);
        T.end(t, stream);
        auto shadow = [&](int level) {
            if (level > 0 && !soft) return false;
            with_bool(PACKET && ds.wide_ok, [&](auto wide) {
                constexpr bool WIDE = PACKET && decltype(wide)::value;  // (no wide per-lane walk)
                if (soft) {
                    const dim3 sg(level ? stride_grid * WF_BLOCK / TB : (nsamp + TB - 1) / TB, ds.nlights);
                    hipLaunchKernelGGL((k_soft_shadow<PACKET, SE, WIDE>), sg, dim3(TB), 0, stream, ds.view, level, nsamp,
                                       B, counters, soft->rays, soft->radius);
                } else
                    hipLaunchKernelGGL((k_rays_shadow<PACKET, SE, WIDE>), dim3((nsamp + TB - 1) / TB, ds.nlights),
                                       dim3(TB), 0, stream, ds.view, nsamp, B, counters);
            });
            return true;
        };
        auto shade = [&](int level, dim3 grid) {
            with_bool(ds.nlights <= 4, [&](auto occ4) {
                if (soft)
                    hipLaunchKernelGGL(k_soft_shade<decltype(occ4)::value>, grid, dim3(WF_BLOCK), 0, stream, ds.view,
                                       amb3, level, nsamp, A.max_depth, B, counters, soft->rays);
                else
                    hipLaunchKernelGGL(k_rays_shade<decltype(occ4)::value>, grid, dim3(WF_BLOCK), 0, stream, ds.view,
                                       amb3, level, nsamp, A.max_depth, B, counters);
            });
        };
        if (hipError_t e = run_levels<false, PACKET, SE>(ds, B, plan.nlevels, nsamp, cam4, counters, stream, shadow,
                                                         false, shade);
            e != hipSuccess)
            return e;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_shade_rays_wavefront(device_scene& ds, const dev_render_args& args, const float* rays, int n,
                                       void* out_rgba, unsigned long long* counters, bool packet, hipStream_t stream,
                                       const soft_shadow_args* soft, bool keep_counters) {
    if (n <= 0) return keep_counters ? hipSuccess : clear_counters(counters, stream);  // (no chunk)
    if (soft && (soft->rays < 1 || soft->rays > soft_shadow_rays_max || (ds.nlights > 0 && !soft->radius)))
        return hipErrorInvalidValue;
    return with_walk(ds, packet, [&](auto pk, auto se) {
        return run_rays<decltype(pk)::value, decltype(se)>(ds, args, rays, n, (float4*)out_rgba, counters, stream,
                                                           soft, keep_counters);
    });
}

hipError_t upload_soft_shadow_radii(device_scene& ds, const float* radius, float all, hipStream_t stream) {
    ds.soft_radius_host.assign((size_t)ds.nlights, all);
    if (radius) std::copy(radius, radius + ds.nlights, ds.soft_radius_host.begin());
    if (ds.nlights == 0) return hipSuccess;
    if (!ds.soft_radius) {  // (a scene's light count is fixed)
        if (hipError_t e = hipMalloc((void**)&ds.soft_radius, sizeof(float) * (size_t)ds.nlights); e != hipSuccess) return e;
    }
    // One stream at a time per handle, as for the workspace (ds.work) and the groups' table
    // (ds.group_tab): the device array and its host source are the handle's, so two soft calls of
    // one handle on different streams would share them. Within a stream the order is safe: the
    // source is pageable memory, for which hipMemcpyAsync copies it into the runtime's staging
    // buffer before it returns (the documented behaviour of a pageable host-to-device copy), so
    // the next call may overwrite soft_radius_host; the device array is rewritten in stream order,
    // behind the kernels of the call before.
    return hipMemcpyAsync(ds.soft_radius, ds.soft_radius_host.data(), sizeof(float) * (size_t)ds.nlights,
                          hipMemcpyHostToDevice, stream);
}

hipError_t launch_render_wavefront(device_scene& ds, const dev_render_args& args, void* out_rgba,
                                   unsigned long long* counters, bool count_work, bool packet, hipStream_t stream) {
    // an empty window (a band offset without bands): no chunk
    if (args.tile_w <= 0 || args.tile_h <= 0) return clear_counters(counters, stream);
    return with_walk(ds, packet, [&](auto pk, auto se) {
        return with_bool(count_work, [&](auto count) {
            return run<decltype(count)::value, decltype(pk)::value, decltype(se)>(ds, args, (float4*)out_rgba, counters,
                                                                                  stream);
        });
    });
}

hipError_t launch_render_wavefront_passes(device_scene& ds, const dev_render_args& args, unsigned mask,
                                          const dev_pass_planes& out, void* beauty_rgba, unsigned long long* counters,
                                          bool packet, hipStream_t stream) {
    if (args.tile_w <= 0 || args.tile_h <= 0) return clear_counters(counters, stream);  // (an empty window)
    pass_buffers P = {};
    P.mask = (mask & ((1u << pass_count) - 1)) | (beauty_rgba ? 1u << pass_count : 0u);
    for (int k = 0; k < pass_count; k++) P.out[k] = (mask >> k & 1) ? (float4*)out.plane[k] : nullptr;
    P.out[pass_count] = (float4*)beauty_rgba;
    return with_walk(ds, packet, [&](auto pk, auto se) {
        return run<false, decltype(pk)::value, decltype(se)>(ds, args, (float4*)beauty_rgba, counters, stream, &P);
    });
}

// The planes in the kernels' order: the groups, then the ambient plane and the beauty where
// asked for. The table (group_buffers::tab): per plane the bounds of its lights, then the
// lights sorted by plane, scene order inside a plane (the beauty's are all of them).
hipError_t launch_render_wavefront_light_groups(device_scene& ds, const dev_render_args& args, const int* group_of,
                                                int ngroups, const dev_light_group_planes& out,
                                                unsigned long long* counters, bool packet, hipStream_t stream) {
    if (args.tile_w <= 0 || args.tile_h <= 0) return clear_counters(counters, stream);  // (an empty window)
    group_buffers G = {};
    std::vector<int>& tab = ds.group_tab;
    tab.assign(group_planes + 1, 0);
    for (int g = 0; g < ngroups; g++) {
        tab[G.nplanes] = (int)tab.size() - (group_planes + 1);
        for (int li = 0; li < ds.nlights; li++)
            if (group_of[li] == g) tab.push_back(li);
        G.out[G.nplanes++] = (float4*)out.group[g];
    }
    if (out.ambient) {
        tab[G.nplanes] = (int)tab.size() - (group_planes + 1);
        G.amb_mask |= 1u << G.nplanes;
        G.out[G.nplanes++] = (float4*)out.ambient;
    }
    if (out.beauty) {
        tab[G.nplanes] = (int)tab.size() - (group_planes + 1);
        for (int li = 0; li < ds.nlights; li++) tab.push_back(li);
        G.amb_mask |= 1u << G.nplanes;
        G.out[G.nplanes++] = (float4*)out.beauty;
    }
    for (int k = G.nplanes; k <= group_planes; k++) tab[k] = (int)tab.size() - (group_planes + 1);
    return with_walk(ds, packet, [&](auto pk, auto se) {
        return run<false, decltype(pk)::value, decltype(se)>(ds, args, nullptr, counters, stream, nullptr, &G);
    });
}

}  // namespace yrt

#ifdef YRT_WIDE_STATS
extern "C" int yrt_debug_wide_stats(unsigned long long* out16, int reset) {
    static unsigned long long h[1024 * 16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(yrt::g_wide_stats), sizeof h) != hipSuccess) return -1;
    for (int i = 0; i < 16; i++) {
        out16[i] = 0;
        for (int k = 0; k < 1024; k++) out16[i] += h[16 * k + i];
    }
    if (reset) {
        static const unsigned long long z[1024 * 16] = {};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(yrt::g_wide_stats), z, sizeof z);
    }
    return 0;
}
#endif

#ifdef YRT_WIDE_STATS
extern "C" int yrt_debug_first_stats(unsigned long long* out16, int reset) {
    static unsigned long long h[1024 * 16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(yrt::g_first_stats), sizeof h) != hipSuccess) return -1;
    for (int i = 0; i < 16; i++) {
        out16[i] = 0;
        for (int k = 0; k < 1024; k++) out16[i] += h[16 * k + i];
    }
    if (reset) {
        static const unsigned long long z[1024 * 16] = {};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(yrt::g_first_stats), z, sizeof z);
    }
    return 0;
}
#endif

#ifdef YRT_LIST_TIMING
// out: n x {phase times..., size} of list builder k (0 k_camera_lists, 1 k_bundle_super,
// 2 k_bundle_lists), n <= 65536; reset: zero them afterwards
extern "C" int yrt_debug_list_time(unsigned long long* out, int k, int n, int reset) {
    if (k < 0 || k > 2 || n < 0 || n > 65536) return -1;
    const size_t off = (size_t)k * sizeof(yrt::g_list_time[0]);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(yrt::g_list_time), (size_t)n * 32, off) != hipSuccess) return -1;
    if (reset) {
        static unsigned long long z[65536 * 4];
        (void)hipMemcpyToSymbol(HIP_SYMBOL(yrt::g_list_time), z, sizeof z, off);
    }
    return 0;
}
#endif

#ifdef YRT_TAIL_STATS
// out: 8192 x {start, end, items, xcd} for kernel k (0 k_primary_persist, 1 k_shadow_persist)
extern "C" int yrt_debug_tail(unsigned long long* out, int k) {
    if (k < 0 || k > 1) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(yrt::g_tail), sizeof(yrt::g_tail[0]), k * sizeof(yrt::g_tail[0])) ==
                   hipSuccess
               ? 0
               : -1;
}
#endif

#ifdef YRT_DEBUG_BOUNDS
extern "C" int yrt_debug_bounds(unsigned* out8, int reset) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(yrt::g_dbg_bounds), 8 * sizeof(unsigned)) != hipSuccess) return -1;
    if (reset) {
        unsigned z[8] = {};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(yrt::g_dbg_bounds), z, sizeof z);
    }
    return 0;
}
#endif

