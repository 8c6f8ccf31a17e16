// mattes.hip -- the ID-matte pass (yrt_render_mattes): per pixel and key (instance, material,
// shape) the few ids that cover the pixel, each with its share of the pixel's s*s camera
// samples, ranked by that share (the Cryptomatte form). A pass of its own beside yrt_render
// and yrt_render_aovs, on the beauty's sample grid (raytrace(), src/raytrace.cpp:228-250).
// render.hip includes this file after aov.hip: the pass is a part of that translation unit
// and of its gfx950 code object, and runs on aov.hip's tile frame (tile_pixel_of,
// tile_camera_sample, tile_count_camera_samples, hit_ids_of, tile_grid).
//
// The tile passes' geometry: one lane owns one pixel, a wave an 8 x 8 tile walked together by
// packet_first, the lane loops over the s*s sub-samples in the reference's order. Every
// requested key is served by the one walk: the keys differ only in which integer of the hit's
// instance record is counted.
//
// The contract: per pixel and key a table of R = 4 * layers entries, empty at
// first. A sample that hits with id v adds one to v's count if v is in the table, else appends
// (v, 1) if an entry is free, else is dropped (counted per key). After the last sample the
// entries are ordered by count descending, ties by id ascending; rank r is
// (id, float(count) / float(s*s)), an unused rank (-1, +0.0f). Integer work and one IEEE
// division per entry: the same bits on every run.
//
// The tables live in registers: R is a template parameter, find-or-insert is an unrolled scan
// with constant indices and predicated updates, the final order a fixed compare-exchange
// network. No table is ever indexed by a run-time value (that would put it into scratch, inside
// the sample loop).
#include <hip/hip_runtime.h>

#include "packet_trace.h"
#include "trace_common.h"
#include "yrt_render.h"

namespace yrt {
namespace {

// entries fill from index 0 on; a free entry has count 0 (and id -1)
template <int R>
struct matte_table {
    int id[R];
    int n[R];
};

template <int R>
__device__ __forceinline__ void matte_clear(matte_table<R>& t) {
#pragma unroll
    for (int r = 0; r < R; r++) t.id[r] = -1, t.n[r] = 0;
}

// find-or-insert of a hit's id v (>= 0); returns false when the sample is dropped (a miss,
// hit = false, changes nothing and is not dropped). The first entry that holds v or is free
// takes the sample: v is in the table at most once, and always before the free entries.
template <int R>
__device__ __forceinline__ bool matte_add(matte_table<R>& t, int v, bool hit) {
    bool open = hit;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const bool take = open && (t.id[r] == v || t.n[r] == 0);
        t.id[r] = take ? v : t.id[r];
        t.n[r] += take ? 1 : 0;
        open = open && !take;
    }
    return !open;
}

// entry A goes before entry B: more samples, or as many and the smaller id
template <int A, int B, int R>
__device__ __forceinline__ void matte_cswap(matte_table<R>& t) {
    static_assert(A < B && B < R, "a comparator of the network");
    const bool swap = t.n[B] > t.n[A] || (t.n[B] == t.n[A] && t.id[B] < t.id[A]);
    const int ia = t.id[A], na = t.n[A];
    t.id[A] = swap ? t.id[B] : ia;
    t.n[A] = swap ? t.n[B] : na;
    t.id[B] = swap ? ia : t.id[B];
    t.n[B] = swap ? na : t.n[B];
}

// the optimal 5-comparator network for 4 entries
__device__ __forceinline__ void matte_sort(matte_table<4>& t) {
    matte_cswap<0, 1>(t), matte_cswap<2, 3>(t);
    matte_cswap<0, 2>(t), matte_cswap<1, 3>(t);
    matte_cswap<1, 2>(t);
}

// Batcher's odd-even merge sort for 8 entries, 19 comparators
__device__ __forceinline__ void matte_sort(matte_table<8>& t) {
    matte_cswap<0, 1>(t), matte_cswap<2, 3>(t), matte_cswap<4, 5>(t), matte_cswap<6, 7>(t);
    matte_cswap<0, 2>(t), matte_cswap<1, 3>(t), matte_cswap<4, 6>(t), matte_cswap<5, 7>(t);
    matte_cswap<1, 2>(t), matte_cswap<5, 6>(t);
    matte_cswap<0, 4>(t), matte_cswap<1, 5>(t), matte_cswap<2, 6>(t), matte_cswap<3, 7>(t);
    matte_cswap<2, 4>(t), matte_cswap<3, 5>(t);
    matte_cswap<1, 2>(t), matte_cswap<3, 4>(t), matte_cswap<5, 6>(t);
}

// the planes of the requested keys, compacted in key order: entry k is the k-th requested key
template <int LAYERS, int NKEYS>
struct matte_out {
    int4* ids[NKEYS][LAYERS];
    float4* coverage[NKEYS][LAYERS];
};

// the dropped totals: matte_drop_slots lines of matte_key_count u64 (+1 of padding), a wave
// adding into the line its index picks, as the ray counters do (yrt_device.h cnt_slots)
__device__ __forceinline__ unsigned long long* matte_drop_line(unsigned long long* dropped) {
    const unsigned wave = (blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    return dropped + (size_t)(wave % matte_drop_slots) * matte_drop_stride;
}

// `keys` holds the requested keys, 2 bits each, the k-th requested in bits 2k..2k+1: a kernel
// argument, the same in every lane, so that picking a key's id is a scalar select.
template <int LAYERS, int NKEYS>
__global__ __launch_bounds__(AOV_BLOCK) void k_matte(dev_scene_view S, dev_render_args A, unsigned keys,
                                                     matte_out<LAYERS, NKEYS> O, unsigned long long* dropped,
                                                     unsigned long long* counters) {
    constexpr int R = 4 * LAYERS;
    // local rows past the image edge read as empty tables: id -1, coverage 0
    const tile_pixel P = tile_pixel_of(A);
    if (!__ballot(P.in_window)) return;  // a tile outside the window: nothing to trace or write

    const int ns = A.samples;
    matte_table<R> tab[NKEYS];
    int drops[NKEYS];
#pragma unroll
    for (int k = 0; k < NKEYS; k++) matte_clear(tab[k]), drops[k] = 0;
    if (__ballot(P.valid)) {
        for (int jj = 0; jj < ns; jj++) {
            for (int ii = 0; ii < ns; ii++) {
                work_counts wc;
                const tile_sample cs = tile_camera_sample(S, A, P, ii, jj, wc);
                const bool hit = P.valid && cs.hit;
                hit_ids ids = {-1, -1, -1};
                if (hit) ids = hit_ids_of(S, cs.hr);
#pragma unroll
                for (int k = 0; k < NKEYS; k++) {
                    const unsigned key = keys >> (2 * k) & 3u;
                    const int v = key == matte_instance ? ids.inst : key == matte_material ? ids.mat : ids.shape;
                    drops[k] += matte_add(tab[k], v, hit) ? 0 : 1;
                }
            }
        }
    }
    const float d = float(ns * ns);
#pragma unroll
    for (int k = 0; k < NKEYS; k++) {
        matte_sort(tab[k]);
        if (P.in_window) {
            const size_t at = P.at(A);
#pragma unroll
            for (int l = 0; l < LAYERS; l++) {
                O.ids[k][l][at] = make_int4(tab[k].id[4 * l], tab[k].id[4 * l + 1], tab[k].id[4 * l + 2], tab[k].id[4 * l + 3]);
                O.coverage[k][l][at] = make_float4(float(tab[k].n[4 * l]) / d, float(tab[k].n[4 * l + 1]) / d,
                                                   float(tab[k].n[4 * l + 2]) / d, float(tab[k].n[4 * l + 3]) / d);
            }
        }
        // the key's dropped samples: one wave sum, at most one atomic per wave and key
        const unsigned long long dk = wave_sum((unsigned long long)drops[k]);
        if (P.lane == 0 && dk) atomicAdd(matte_drop_line(dropped) + (keys >> (2 * k) & 3u), dk);
    }
    tile_count_camera_samples(counters, P, ns);
}

template <int LAYERS, int NKEYS>
hipError_t launch_mattes_as(const device_scene& ds, const dev_render_args& args, unsigned key_mask,
                            const dev_matte_planes& out, unsigned long long* dropped, unsigned long long* counters,
                            hipStream_t stream) {
    matte_out<LAYERS, NKEYS> o = {};
    unsigned keys = 0;
    int k = 0;
    for (int key = 0; key < matte_key_count; key++) {
        if (!(key_mask >> key & 1)) continue;
        keys |= (unsigned)key << (2 * k);
        for (int l = 0; l < LAYERS; l++) {
            o.ids[k][l] = reinterpret_cast<int4*>(out.ids[key][l]);
            o.coverage[k][l] = reinterpret_cast<float4*>(out.coverage[key][l]);
        }
        k++;
    }
    hipLaunchKernelGGL((k_matte<LAYERS, NKEYS>), tile_grid(args), dim3(AOV_BLOCK), 0, stream, ds.view, args, keys, o, dropped,
                       counters);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_mattes(const device_scene& ds, const dev_render_args& args, unsigned key_mask, int layers,
                         const dev_matte_planes& out, unsigned long long* dropped, unsigned long long* counters,
                         hipStream_t stream) {
    if (args.tile_w <= 0 || args.tile_h <= 0) return hipSuccess;
    const int nkeys = __builtin_popcount(key_mask & ((1u << matte_key_count) - 1));
    switch (layers * 4 + nkeys) {
        case 1 * 4 + 1: return launch_mattes_as<1, 1>(ds, args, key_mask, out, dropped, counters, stream);
        case 1 * 4 + 2: return launch_mattes_as<1, 2>(ds, args, key_mask, out, dropped, counters, stream);
        case 1 * 4 + 3: return launch_mattes_as<1, 3>(ds, args, key_mask, out, dropped, counters, stream);
        case 2 * 4 + 1: return launch_mattes_as<2, 1>(ds, args, key_mask, out, dropped, counters, stream);
        case 2 * 4 + 2: return launch_mattes_as<2, 2>(ds, args, key_mask, out, dropped, counters, stream);
        case 2 * 4 + 3: return launch_mattes_as<2, 3>(ds, args, key_mask, out, dropped, counters, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace yrt
