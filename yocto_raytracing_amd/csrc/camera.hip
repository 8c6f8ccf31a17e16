// camera.hip -- camera models (yrt_render_camera, yrt_camera_rays): the thin-lens perspective
// camera, the orthographic camera and the equirectangular panorama, as camera rays generated on
// the device and shaded as ray batches. render.hip includes this file after ao.hip: the
// feature's kernels are a part of that translation unit and of its gfx950 code object, and the
// lens samples are ao.hip's tables (ao_dirs, ao_rots).
//
// This file also holds the pixel-batch pipeline (render_pixel_batches) that yrt_render_camera,
// yrt_render_soft_shadows and, through adaptive.hip, yrt_render_adaptive run on: the one chunk
// size, the one scratch buffer and the one loop of rays, batch and resolve.
//
// The contract (include/yrt.h): a ray is camera_models.h's expression of its
// model; a pixel is the float32 sum of its s*s rays' shade() colours in sample order (jj outer,
// ii inner) from +0, divided by float(s*s), .w = 1. k_camera_rays writes a chunk of whole
// pixels' rays, a pixel's samples consecutive (a wave is 64 samples of one pixel: with a lens
// too this is the tighter bundle), wavefront.hip's run_rays shades them
// (launch_shade_rays_wavefront), k_camera_resolve sums each pixel's colours. A pixel's value
// depends on its own rays alone, so neither the chunk size nor the order of a list changes a bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "camera_models.h"
#include "trace_common.h"
#include "yrt_render.h"

namespace yrt {
namespace {

constexpr int BATCH_BLOCK = 256;  // the one-dimensional kernels of the pixel batches

// Pixel k of a chunk, as an index into the window (row-major, tile_w per row): the k-th of a
// list (adaptive.hip's flagged pixels, in any order) or of the range from `first`. `list` is a
// kernel argument, the same in every lane: a scalar branch.
__device__ __forceinline__ unsigned chunk_pixel(const unsigned* __restrict__ list, unsigned first, int k) {
    return list ? list[k] : first + (unsigned)k;
}

// One lane per camera ray of a chunk of npix whole pixels: ray r is sample r % spp (jj outer, ii
// inner) of chunk pixel r / spp, as two 16-byte stores of the 32-byte record {o.xyz, d.xyz,
// tmin, tmax}. MODEL is a camera_model.
template <int MODEL>
__global__ __launch_bounds__(BATCH_BLOCK) void k_camera_rays(dev_render_args A, float aperture,
                                                             const unsigned* __restrict__ list, unsigned first,
                                                             int npix, float4* __restrict__ rays) {
    const int ns = A.samples, spp = ns * ns;
    const long long r = (long long)blockIdx.x * BATCH_BLOCK + threadIdx.x;
    if (r >= (long long)npix * spp) return;
    const int k = (int)(r / spp), q = (int)(r % spp);
    const unsigned p = chunk_pixel(list, first, k);
    const int i = A.x0 + (int)(p % (unsigned)A.tile_w), j = A.y0 + (int)(p / (unsigned)A.tile_w);
    const camera_model_ray ray = camera_model_eval<MODEL>(A.cam, aperture, ao_dirs, ao_rots, A.width, A.height, ns, i, j, q);
    rays[2 * r] = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.d.x);
    rays[2 * r + 1] = make_float4(ray.d.y, ray.d.z, ray.tmin, ray.tmax);
}

// One lane per pixel of a chunk of npix: the float32 sum of its spp colours in sample order
// from +0, divided by float(spp), .w = 1 (wavefront.hip accumulate_plane), into its place in
// out. Without colours (the local rows past the image edge) zeros.
__global__ __launch_bounds__(BATCH_BLOCK) void k_camera_resolve(dev_render_args A, const unsigned* __restrict__ list,
                                                                unsigned first, int npix,
                                                                const float4* __restrict__ colours,
                                                                float4* __restrict__ out) {
    const int k = blockIdx.x * BATCH_BLOCK + threadIdx.x;
    if (k >= npix) return;
    const unsigned p = chunk_pixel(list, first, k);
    const size_t at = (size_t)(p / (unsigned)A.tile_w) * A.out_stride + p % (unsigned)A.tile_w;
    if (!colours) {
        out[at] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const int spp = A.samples * A.samples;
    const float4* c = colours + (size_t)k * spp;
    vec3f acc = {0, 0, 0};
    for (int q = 0; q < spp; q++) {
        const float4 v = c[q];
        acc = {acc.x + v.x, acc.y + v.y, acc.z + v.z};
    }
    const float d = float(spp);
    out[at] = make_float4(acc.x / d, acc.y / d, acc.z / d, 1.0f);
}

dim3 batch_grid(long long lanes) { return dim3((unsigned)((lanes + BATCH_BLOCK - 1) / BATCH_BLOCK)); }

// the rays of a chunk's npix pixels (chunk_pixel) into `rays`
void launch_camera_rays_chunk(const dev_render_args& args, int model, float aperture, const unsigned* list,
                              unsigned first, int npix, float4* rays, hipStream_t stream) {
    const dim3 grid = batch_grid((long long)npix * args.samples * args.samples), block(BATCH_BLOCK);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, args, aperture, list, first, npix, rays);
    };
    if (model == camera_orthographic)
        launch(k_camera_rays<camera_orthographic>);
    else if (model == camera_equirect)
        launch(k_camera_rays<camera_equirect>);
    else
        launch(k_camera_rays<camera_perspective>);
}

// the most whole pixels whose rays one launch counts in an int
long long camera_pixels_cap(int spp) { return std::max<long long>(1, (1ll << 30) / spp); }

size_t scratch_align(size_t x) { return (x + 255) & ~size_t(255); }

// a scratch buffer of the handle, grown on demand and never shrunk
hipError_t grow_scratch(void*& buf, size_t& have, size_t need) {
    if (need <= have) return hipSuccess;
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    have = 0;
    const hipError_t e = hipMalloc(&buf, need);
    if (e == hipSuccess) have = need;
    return e;
}

// The pixel-batch pipeline: `pixels` (> 0) pixels of the window -- list[0 .. pixels) where a
// list is given (device memory), else the window's first `pixels` in row-major order -- in
// chunks of whole pixels: the chunk's camera rays, shaded as a ray batch (soft: as a soft one),
// summed per pixel into `out`. counters_started: something before this call (the adaptive base
// render) has started the call's counters, so the first batch adds to them as every later one
// does; otherwise the first batch zeroes them.
hipError_t render_pixel_batches(device_scene& ds, const dev_render_args& args, int model, float aperture,
                                const unsigned* list, long long pixels, int chunk_pixels, const soft_shadow_args* soft,
                                float4* out, unsigned long long* counters, bool counters_started, bool packet,
                                hipStream_t stream) {
    const int spp = args.samples * args.samples;
    // whole pixels per chunk: the caller's, or what keeps rays + colours within the budget
    // (pixel_batch_rays; a batch's rays are counted in an int)
    const long long budget = chunk_pixels > 0 ? chunk_pixels : std::max<long long>(1, pixel_batch_rays / spp);
    const int per_chunk = (int)std::min({pixels, budget, camera_pixels_cap(spp)});
    const size_t ray_bytes = scratch_align((size_t)per_chunk * spp * 2 * sizeof(float4));
    hipError_t e = grow_scratch(ds.batch_rays, ds.batch_rays_bytes, ray_bytes + (size_t)per_chunk * spp * sizeof(float4));
    float4* rays = (float4*)ds.batch_rays;
    float4* colours = (float4*)((char*)ds.batch_rays + ray_bytes);
    phase_timer& T = ds.timer;
    for (long long k0 = 0; k0 < pixels && e == hipSuccess; k0 += per_chunk) {
        const int npix = (int)std::min<long long>(per_chunk, pixels - k0);
        const unsigned* chunk_list = list ? list + k0 : nullptr;
        int t = T.begin(phase_primary, stream);
        launch_camera_rays_chunk(args, model, aperture, chunk_list, (unsigned)k0, npix, rays, stream);
        T.end(t, stream);
        e = launch_shade_rays_wavefront(ds, args, (const float*)rays, npix * spp, colours, counters, packet, stream, soft,
                                        counters_started || k0 > 0);
        if (e != hipSuccess) break;
        t = T.begin(phase_accumulate, stream);
        hipLaunchKernelGGL(k_camera_resolve, batch_grid(npix), dim3(BATCH_BLOCK), 0, stream, args, chunk_list,
                           (unsigned)k0, npix, (const float4*)colours, out);
        T.end(t, stream);
        e = hipGetLastError();
    }
    return e;
}

// launch_render_camera and launch_render_soft_shadows: the window's image rows as pixel batches
hipError_t render_camera_batches(device_scene& ds, const dev_render_args& args, int model, float aperture,
                                 int chunk_pixels, const soft_shadow_args* soft, void* out_rgba,
                                 unsigned long long* counters, bool packet, hipStream_t stream) {
    const size_t counter_bytes = (size_t)cnt_slots * cnt_count * sizeof(unsigned long long);
    if (args.tile_w <= 0 || args.tile_h <= 0)  // an empty window: nothing written, nothing counted
        return hipMemsetAsync(counters, 0, counter_bytes, stream);
    if ((long long)args.tile_w * args.tile_h > (1ll << 31) - 1)
        throw unsupported_error("a camera-model render indexes a window's pixels in 31 bits");
    // the window's image rows; the local rows below them are zeros
    const int rows = std::max(0, std::min(args.tile_h, args.height - args.y0));
    const long long pixels = (long long)args.tile_w * rows;
    if (rows < args.tile_h) {
        const int npix = args.tile_w * (args.tile_h - rows);
        const int t = ds.timer.begin(phase_accumulate, stream);
        hipLaunchKernelGGL(k_camera_resolve, batch_grid(npix), dim3(BATCH_BLOCK), 0, stream, args,
                           (const unsigned*)nullptr, (unsigned)pixels, npix, (const float4*)nullptr, (float4*)out_rgba);
        ds.timer.end(t, stream);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    ds.last_camera_lists = ds.last_bundles = false;
    ds.last_lds_staging = 0;
    if (pixels == 0) return hipMemsetAsync(counters, 0, counter_bytes, stream);
    return render_pixel_batches(ds, args, model, aperture, nullptr, pixels, chunk_pixels, soft, (float4*)out_rgba,
                                counters, false, packet, stream);
}

}  // namespace

hipError_t launch_render_camera(device_scene& ds, const dev_render_args& args, int model, float aperture,
                                int chunk_pixels, void* out_rgba, unsigned long long* counters, bool packet,
                                hipStream_t stream) {
    return render_camera_batches(ds, args, model, aperture, chunk_pixels, nullptr, out_rgba, counters, packet, stream);
}

hipError_t launch_render_soft_shadows(device_scene& ds, const dev_render_args& args, int model, float aperture,
                                      int chunk_pixels, const soft_shadow_args& soft, void* out_rgba,
                                      unsigned long long* counters, bool packet, hipStream_t stream) {
    return render_camera_batches(ds, args, model, aperture, chunk_pixels, &soft, out_rgba, counters, packet, stream);
}

hipError_t launch_camera_rays(device_scene& ds, const dev_render_args& args, int model, float aperture, void* rays,
                              hipStream_t stream) {
    if (args.tile_w <= 0 || args.tile_h <= 0) return hipSuccess;
    if ((long long)args.tile_w * args.tile_h > (1ll << 31) - 1)
        throw unsupported_error("a camera-model render indexes a window's pixels in 31 bits");
    const int spp = args.samples * args.samples;
    const long long pixels = (long long)args.tile_w * args.tile_h, per_launch = camera_pixels_cap(spp);
    for (long long k0 = 0; k0 < pixels; k0 += per_launch)
        launch_camera_rays_chunk(args, model, aperture, nullptr, (unsigned)k0, (int)std::min(per_launch, pixels - k0),
                                 (float4*)rays + (size_t)k0 * spp * 2, stream);
    return hipGetLastError();
}

}  // namespace yrt
