// adaptive.hip -- adaptive supersampling (yrt_render_adaptive): Whitted's own answer to the
// cost of s*s camera samples in every pixel. A base frame at b*b samples per pixel, a contrast
// test between neighbouring pixels of that frame, and the full s*s samples only in the pixels
// the test flags. render.hip includes this file after mattes.hip: the feature's kernels are a
// part of that translation unit and of its gfx950 code object.
//
// The contract (include/yrt.h): B is yrt_render's frame at `base` samples per
// axis, over the window grown by one pixel on every side and clipped to the image (the apron;
// it lives in scratch, never in `out`). A pixel P of the window is flagged iff a pixel Q of the
// image at Chebyshev distance 1 and a channel c of r, g, b exist with fabsf(B[P].c - B[Q].c) >
// threshold, in float32, an IEEE comparison (false on NaN). A flagged pixel receives exactly
// yrt_render's value at s samples per axis, every other pixel B.
//
// The refined pixels are shaded as a ray batch (wavefront.hip run_rays, through
// launch_shade_rays_wavefront): k_adaptive_rays writes a chunk's camera rays, a pixel's s*s
// samples consecutive with jj outer and ii inner, the batch shades them, k_adaptive_resolve
// sums each pixel's colours in that order. A pixel's value depends on its own rays alone, so
// neither the order of the flagged list (an atomic per block) nor the chunk size changes a bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "trace_common.h"
#include "yrt_render.h"

namespace yrt {
namespace {

constexpr int AD_BLOCK_X = 64, AD_BLOCK_Y = 4;  // k_adaptive_flag: a wave is 64 pixels of one row
constexpr int AD_BLOCK = 256;                   // the one-dimensional kernels

// the base frame B: the grown window's pixels, row-major, gw per row, from image pixel (gx0, gy0)
struct adaptive_base {
    const float4* px;
    int gx0, gy0, gw;
};

__device__ __forceinline__ float4 base_at(const adaptive_base& B, int i, int j) {
    return B.px[(size_t)(j - B.gy0) * B.gw + (i - B.gx0)];
}

// One lane per window pixel (A: the call's window; out and refined in its layout). The lane
// copies its base pixel to `out` (zeros in a local row past the image edge), tests it against
// its up to eight neighbours in the image, writes the byte mask where asked for, and appends a
// flagged pixel's window index ly * tile_w + lx to `list`: a ballot per wave, one atomic per
// block. Neighbouring lanes read neighbouring pixels of a row in each of the nine loads.
__global__ __launch_bounds__(AD_BLOCK_X * AD_BLOCK_Y) void k_adaptive_flag(dev_render_args A, adaptive_base B,
                                                                          float threshold, float4* __restrict__ out,
                                                                          unsigned char* __restrict__ refined,
                                                                          unsigned* __restrict__ list,
                                                                          unsigned long long* __restrict__ count) {
    __shared__ unsigned wave_first[AD_BLOCK_Y];
    __shared__ unsigned block_first;
    const int lane = threadIdx.x, wave = threadIdx.y;
    const int lx = blockIdx.x * AD_BLOCK_X + lane, ly = blockIdx.y * AD_BLOCK_Y + wave;
    const bool in_window = lx < A.tile_w && ly < A.tile_h;
    const int i = A.x0 + lx, j = A.y0 + ly;
    const bool valid = in_window && i < A.width && j < A.height;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool flag = false;
    if (valid) {
        p = base_at(B, i, j);
        for (int dj = -1; dj <= 1; dj++) {
            for (int di = -1; di <= 1; di++) {
                const int qi = i + di, qj = j + dj;
                if ((di == 0 && dj == 0) || qi < 0 || qj < 0 || qi >= A.width || qj >= A.height) continue;
                const float4 q = base_at(B, qi, qj);
                flag = flag || fabsf(p.x - q.x) > threshold || fabsf(p.y - q.y) > threshold ||
                       fabsf(p.z - q.z) > threshold;
            }
        }
    }
    if (in_window) {
        const size_t at = (size_t)ly * A.out_stride + lx;
        out[at] = p;
        if (refined) refined[at] = flag ? 1 : 0;
    }
    // the flagged pixels' places in the list: this wave's after the block's earlier waves'
    const unsigned long long mine = __ballot(flag);
    if (lane == 0) wave_first[wave] = (unsigned)__popcll(mine);
    __syncthreads();
    if (lane == 0 && wave == 0) {
        unsigned n = 0;
        for (int w = 0; w < AD_BLOCK_Y; w++) {
            const unsigned c = wave_first[w];
            wave_first[w] = n;
            n += c;
        }
        block_first = n ? (unsigned)atomicAdd(count, (unsigned long long)n) : 0u;
    }
    __syncthreads();
    if (flag) {
        const unsigned before = (unsigned)__popcll(mine & ((1ull << lane) - 1ull));
        list[block_first + wave_first[wave] + before] = (unsigned)(ly * A.tile_w + lx);
    }
}

// One lane per camera ray of a chunk of npix flagged pixels: ray r is sample r % spp (jj outer,
// ii inner) of pixel list[r / spp], camera_ray's bits with its tmin and tmax (k_primary's), as
// two 16-byte stores of the 32-byte record {o.xyz, d.xyz, tmin, tmax}.
__global__ __launch_bounds__(AD_BLOCK) void k_adaptive_rays(dev_render_args A, const unsigned* __restrict__ list,
                                                            int npix, float4* __restrict__ rays) {
    const int ns = A.samples, spp = ns * ns;
    const long long r = (long long)blockIdx.x * AD_BLOCK + threadIdx.x;
    if (r >= (long long)npix * spp) return;
    const int k = (int)(r / spp), q = (int)(r % spp);
    const unsigned p = list[k];
    const int i = A.x0 + (int)(p % (unsigned)A.tile_w), j = A.y0 + (int)(p / (unsigned)A.tile_w);
    const ray3 ray = camera_ray(A.cam, A.width, A.height, ns, i, j, q % ns, q / ns);
    rays[2 * r] = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.d.x);
    rays[2 * r + 1] = make_float4(ray.d.y, ray.d.z, ray.tmin, ray.tmax);
}

// One lane per flagged pixel of the chunk: the float32 sum of its spp colours in sample order
// from +0, divided by float(spp), .w = 1 (wavefront.hip accumulate_plane), into its place in out.
__global__ __launch_bounds__(AD_BLOCK) void k_adaptive_resolve(dev_render_args A, const unsigned* __restrict__ list,
                                                               int npix, const float4* __restrict__ colours,
                                                               float4* __restrict__ out) {
    const int k = blockIdx.x * AD_BLOCK + threadIdx.x;
    if (k >= npix) return;
    const int spp = A.samples * A.samples;
    const float4* c = colours + (size_t)k * spp;
    vec3f acc = {0, 0, 0};
    for (int q = 0; q < spp; q++) {
        const float4 v = c[q];
        acc = {acc.x + v.x, acc.y + v.y, acc.z + v.z};
    }
    const unsigned p = list[k];
    const size_t at = (size_t)(p / (unsigned)A.tile_w) * A.out_stride + p % (unsigned)A.tile_w;
    const float d = float(spp);
    out[at] = make_float4(acc.x / d, acc.y / d, acc.z / d, 1.0f);
}

// a batch zeroes the counter lines in its first kernel: the call's counts so far, saved before
// the batch, are added back after it
__global__ __launch_bounds__(AD_BLOCK) void k_adaptive_add_counters(unsigned long long* __restrict__ counters,
                                                                    const unsigned long long* __restrict__ saved) {
    const int k = blockIdx.x * AD_BLOCK + threadIdx.x;
    if (k < cnt_slots * cnt_count) counters[k] += saved[k];
}

size_t adaptive_align(size_t x) { return (x + 255) & ~size_t(255); }

hipError_t grow(void*& buf, size_t& have, size_t need) {
    if (need <= have) return hipSuccess;
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    have = 0;
    const hipError_t e = hipMalloc(&buf, need);
    if (e == hipSuccess) have = need;
    return e;
}

}  // namespace

hipError_t launch_render_adaptive(device_scene& ds, const dev_render_args& args, int base_samples, float threshold,
                                  int chunk_pixels, void* out_rgba, unsigned char* refined,
                                  unsigned long long* counters, bool packet, hipStream_t stream) {
    ds.adaptive_refined = 0;
    if (args.tile_w <= 0 || args.tile_h <= 0) {  // an empty window: nothing written, nothing counted
        return hipMemsetAsync(counters, 0, (size_t)cnt_slots * cnt_count * sizeof(unsigned long long), stream);
    }
    const int spp = args.samples * args.samples;
    if ((long long)args.tile_w * args.tile_h > (1ll << 31) - 1)
        throw unsupported_error("adaptive supersampling indexes a window's pixels in 31 bits");
    // the apron: the window's image rows and columns, grown by one pixel and clipped to the image
    const int rows = std::min(args.tile_h, args.height - args.y0);
    dev_render_args base = args;
    base.samples = base_samples;
    base.x0 = std::max(args.x0 - 1, 0);
    base.y0 = std::max(args.y0 - 1, 0);
    base.tile_w = std::min(args.x0 + args.tile_w + 1, args.width) - base.x0;
    base.tile_h = std::min(args.y0 + rows + 1, args.height) - base.y0;
    base.out_stride = base.tile_w;
    // the frame scratch: the flagged count, the saved counter lines, the base frame, the list
    const size_t counter_bytes = (size_t)cnt_slots * cnt_count * sizeof(unsigned long long);
    const size_t base_bytes = adaptive_align((size_t)base.tile_w * base.tile_h * sizeof(float4));
    const size_t list_bytes = adaptive_align((size_t)args.tile_w * rows * sizeof(unsigned));
    if (hipError_t e = grow(ds.adaptive_frame, ds.adaptive_frame_bytes, 256 + counter_bytes + base_bytes + list_bytes);
        e != hipSuccess)
        return e;
    char* at = (char*)ds.adaptive_frame;
    unsigned long long* count = (unsigned long long*)at;
    unsigned long long* saved = (unsigned long long*)(at + 256);
    float4* base_px = (float4*)(at + 256 + counter_bytes);
    unsigned* list = (unsigned*)(at + 256 + counter_bytes + base_bytes);
    if (!ds.adaptive_count_host) {
        if (hipError_t e = hipHostMalloc((void**)&ds.adaptive_count_host, sizeof(unsigned long long), hipHostMallocDefault);
            e != hipSuccess)
            return e;
    }
    if (!ds.adaptive_count_ev) {
        if (hipError_t e = hipEventCreateWithFlags(&ds.adaptive_count_ev, hipEventDisableTiming); e != hipSuccess) return e;
    }
    phase_timer& T = ds.timer;

    // base -> flag -> the count, on the host behind the flag kernel (wavefront.hip level_count_host)
    if (hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned long long), stream); e != hipSuccess) return e;
    if (hipError_t e = launch_render_wavefront(ds, base, base_px, counters, false, packet, stream); e != hipSuccess)
        return e;
    int t = T.begin(phase_lists, stream);
    hipLaunchKernelGGL(k_adaptive_flag,
                       dim3((args.tile_w + AD_BLOCK_X - 1) / AD_BLOCK_X, (args.tile_h + AD_BLOCK_Y - 1) / AD_BLOCK_Y),
                       dim3(AD_BLOCK_X, AD_BLOCK_Y), 0, stream, args, adaptive_base{base_px, base.x0, base.y0, base.tile_w},
                       threshold, (float4*)out_rgba, refined, list, count);
    T.end(t, stream);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (hipError_t e = hipMemcpyAsync(ds.adaptive_count_host, count, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream);
        e != hipSuccess)
        return e;
    if (hipError_t e = hipEventRecord(ds.adaptive_count_ev, stream); e != hipSuccess) return e;
    if (hipError_t e = hipEventSynchronize(ds.adaptive_count_ev); e != hipSuccess) return e;
    const long long flagged = (long long)*ds.adaptive_count_host;
    ds.adaptive_refined = (unsigned long long)flagged;
    if (flagged == 0) return hipSuccess;

    // whole pixels per chunk: the caller's, or what keeps rays + colours within the budget
    // (adaptive_chunk_rays; a batch's rays are counted in an int)
    const long long budget = chunk_pixels > 0 ? chunk_pixels : std::max<long long>(1, adaptive_chunk_rays / spp);
    const int per_chunk = (int)std::min({flagged, budget, std::max<long long>(1, (1ll << 30) / spp)});
    const size_t ray_bytes = adaptive_align((size_t)per_chunk * spp * 2 * sizeof(float4));
    if (hipError_t e = grow(ds.adaptive_rays, ds.adaptive_rays_bytes, ray_bytes + (size_t)per_chunk * spp * sizeof(float4));
        e != hipSuccess)
        return e;
    float4* rays = (float4*)ds.adaptive_rays;
    float4* colours = (float4*)((char*)ds.adaptive_rays + ray_bytes);
    // what the base render reported of its lists and staging stays the call's report
    const bool camera_lists = ds.last_camera_lists, bundles = ds.last_bundles;
    const int staged = ds.last_lds_staging;
    hipError_t e = hipSuccess;
    for (long long k0 = 0; k0 < flagged && e == hipSuccess; k0 += per_chunk) {
        const int npix = (int)std::min<long long>(per_chunk, flagged - k0);
        const int n = npix * spp;
        t = T.begin(phase_primary, stream);
        hipLaunchKernelGGL(k_adaptive_rays, dim3((n + AD_BLOCK - 1) / AD_BLOCK), dim3(AD_BLOCK), 0, stream, args, list + k0,
                           npix, rays);
        T.end(t, stream);
        e = hipMemcpyAsync(saved, counters, counter_bytes, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess)
            e = launch_shade_rays_wavefront(ds, args, (const float*)rays, n, colours, counters, packet, stream);
        if (e != hipSuccess) break;
        t = T.begin(phase_accumulate, stream);
        hipLaunchKernelGGL(k_adaptive_add_counters, dim3((cnt_slots * cnt_count + AD_BLOCK - 1) / AD_BLOCK), dim3(AD_BLOCK),
                           0, stream, counters, saved);
        hipLaunchKernelGGL(k_adaptive_resolve, dim3((npix + AD_BLOCK - 1) / AD_BLOCK), dim3(AD_BLOCK), 0, stream, args,
                           list + k0, npix, colours, (float4*)out_rgba);
        T.end(t, stream);
        e = hipGetLastError();
    }
    ds.last_camera_lists = camera_lists, ds.last_bundles = bundles;
    ds.last_lds_staging = staged;
    return e;
}

}  // namespace yrt
