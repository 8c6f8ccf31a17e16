// camera.hip -- camera models (yrt_render_camera, yrt_camera_rays): the thin-lens perspective
// camera, the orthographic camera and the equirectangular panorama, as camera rays generated on
// the device and shaded as ray batches. render.hip includes this file after ao.hip: the
// feature's kernels are a part of that translation unit and of its gfx950 code object, and it
// shares adaptive.hip's batch plumbing (grow, adaptive_align, k_adaptive_add_counters) and
// ao.hip's tables (ao_dirs, ao_rots).
//
// The contract (include/yrt.h): a ray is camera_models.h's expression of its
// model; a pixel is the float32 sum of its s*s rays' shade() colours in sample order (jj outer,
// ii inner) from +0, divided by float(s*s), .w = 1. k_camera_rays writes a chunk of whole
// pixels' rays, a pixel's samples consecutive (a wave is 64 samples of one pixel: with a lens
// too this is the tighter bundle), wavefront.hip's run_rays shades them
// (launch_shade_rays_wavefront), k_camera_resolve sums each pixel's colours. A pixel's value
// depends on its own rays alone, so the chunk size changes no bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "camera_models.h"
#include "trace_common.h"
#include "yrt_render.h"

namespace yrt {
namespace {

// One lane per camera ray of a chunk of npix whole pixels: ray r is sample r % spp (jj outer, ii
// inner) of window pixel first + r / spp (row-major over the window, tile_w per row), as two
// 16-byte stores of the 32-byte record {o.xyz, d.xyz, tmin, tmax}. MODEL is a camera_model.
template <int MODEL>
__global__ __launch_bounds__(AD_BLOCK) void k_camera_rays(dev_render_args A, float aperture, unsigned first, int npix,
                                                          float4* __restrict__ rays) {
    const int ns = A.samples, spp = ns * ns;
    const long long r = (long long)blockIdx.x * AD_BLOCK + threadIdx.x;
    if (r >= (long long)npix * spp) return;
    const int k = (int)(r / spp), q = (int)(r % spp);
    const unsigned p = first + (unsigned)k;
    const int i = A.x0 + (int)(p % (unsigned)A.tile_w), j = A.y0 + (int)(p / (unsigned)A.tile_w);
    const camera_model_ray ray = camera_model_eval<MODEL>(A.cam, aperture, ao_dirs, ao_rots, A.width, A.height, ns, i, j, q);
    rays[2 * r] = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.d.x);
    rays[2 * r + 1] = make_float4(ray.d.y, ray.d.z, ray.tmin, ray.tmax);
}

// One lane per window pixel first + k of a chunk of npix: the float32 sum of its spp colours in
// sample order from +0, divided by float(spp), .w = 1 (k_adaptive_resolve without the list),
// into its place in out. Without colours (the local rows past the image edge) zeros.
__global__ __launch_bounds__(AD_BLOCK) void k_camera_resolve(dev_render_args A, unsigned first, int npix,
                                                             const float4* __restrict__ colours,
                                                             float4* __restrict__ out) {
    const int k = blockIdx.x * AD_BLOCK + threadIdx.x;
    if (k >= npix) return;
    const unsigned p = first + (unsigned)k;
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

// the rays of window pixels [first, first + npix) into `rays`
void launch_camera_rays_chunk(const dev_render_args& args, int model, float aperture, unsigned first, int npix,
                              float4* rays, hipStream_t stream) {
    const long long n = (long long)npix * args.samples * args.samples;
    const dim3 grid((unsigned)((n + AD_BLOCK - 1) / AD_BLOCK)), block(AD_BLOCK);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, args, aperture, first, npix, rays);
    };
    if (model == camera_orthographic)
        launch(k_camera_rays<camera_orthographic>);
    else if (model == camera_equirect)
        launch(k_camera_rays<camera_equirect>);
    else
        launch(k_camera_rays<camera_perspective>);
}

// the most whole pixels whose rays one launch counts in an int (adaptive.hip's cap)
long long camera_pixels_cap(int spp) { return std::max<long long>(1, (1ll << 30) / spp); }

// launch_render_camera and launch_render_soft_shadows: the window's image in chunks of whole
// pixels, each shaded as a ray batch (soft: as a soft one)
hipError_t render_camera_batches(device_scene& ds, const dev_render_args& args, int model, float aperture,
                                 int chunk_pixels, const soft_shadow_args* soft, void* out_rgba,
                                 unsigned long long* counters, bool packet, hipStream_t stream) {
    const size_t counter_bytes = (size_t)cnt_slots * cnt_count * sizeof(unsigned long long);
    if (args.tile_w <= 0 || args.tile_h <= 0)  // an empty window: nothing written, nothing counted
        return hipMemsetAsync(counters, 0, counter_bytes, stream);
    if ((long long)args.tile_w * args.tile_h > (1ll << 31) - 1)
        throw unsupported_error("a camera-model render indexes a window's pixels in 31 bits");
    const int spp = args.samples * args.samples;
    // the window's image rows; the local rows below them are zeros
    const int rows = std::max(0, std::min(args.tile_h, args.height - args.y0));
    const long long pixels = (long long)args.tile_w * rows;
    phase_timer& T = ds.timer;
    hipError_t e = hipSuccess;
    if (rows < args.tile_h) {
        const int npix = args.tile_w * (args.tile_h - rows);
        const int t = T.begin(phase_accumulate, stream);
        hipLaunchKernelGGL(k_camera_resolve, dim3((npix + AD_BLOCK - 1) / AD_BLOCK), dim3(AD_BLOCK), 0, stream, args,
                           (unsigned)pixels, npix, (const float4*)nullptr, (float4*)out_rgba);
        T.end(t, stream);
        if (e = hipGetLastError(); e != hipSuccess) return e;
    }
    ds.last_camera_lists = ds.last_bundles = false;
    ds.last_lds_staging = 0;
    if (pixels == 0) return hipMemsetAsync(counters, 0, counter_bytes, stream);
    // whole pixels per chunk: the caller's, or what keeps rays + colours within the budget
    // (adaptive_chunk_rays; a batch's rays are counted in an int)
    const long long budget = chunk_pixels > 0 ? chunk_pixels : std::max<long long>(1, adaptive_chunk_rays / spp);
    const int per_chunk = (int)std::min({pixels, budget, camera_pixels_cap(spp)});
    const size_t ray_bytes = adaptive_align((size_t)per_chunk * spp * 2 * sizeof(float4));
    if (e = grow(ds.adaptive_rays, ds.adaptive_rays_bytes, ray_bytes + (size_t)per_chunk * spp * sizeof(float4));
        e != hipSuccess)
        return e;
    // the saved counter lines, where launch_render_adaptive keeps its own
    if (e = grow(ds.adaptive_frame, ds.adaptive_frame_bytes, 256 + counter_bytes); e != hipSuccess) return e;
    unsigned long long* saved = (unsigned long long*)((char*)ds.adaptive_frame + 256);
    float4* rays = (float4*)ds.adaptive_rays;
    float4* colours = (float4*)((char*)ds.adaptive_rays + ray_bytes);
    for (long long k0 = 0; k0 < pixels && e == hipSuccess; k0 += per_chunk) {
        const int npix = (int)std::min<long long>(per_chunk, pixels - k0);
        int t = T.begin(phase_primary, stream);
        launch_camera_rays_chunk(args, model, aperture, (unsigned)k0, npix, rays, stream);
        T.end(t, stream);
        // a batch zeroes the counter lines in its first kernel: from the second batch on the
        // call's counts so far are saved before it and added back after it
        if (k0 > 0) e = hipMemcpyAsync(saved, counters, counter_bytes, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess)
            e = launch_shade_rays_wavefront(ds, args, (const float*)rays, npix * spp, colours, counters, packet, stream,
                                            soft);
        if (e != hipSuccess) break;
        t = T.begin(phase_accumulate, stream);
        if (k0 > 0)
            hipLaunchKernelGGL(k_adaptive_add_counters, dim3((cnt_slots * cnt_count + AD_BLOCK - 1) / AD_BLOCK),
                               dim3(AD_BLOCK), 0, stream, counters, saved);
        hipLaunchKernelGGL(k_camera_resolve, dim3((npix + AD_BLOCK - 1) / AD_BLOCK), dim3(AD_BLOCK), 0, stream, args,
                           (unsigned)k0, npix, (const float4*)colours, (float4*)out_rgba);
        T.end(t, stream);
        e = hipGetLastError();
    }
    return e;
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
        launch_camera_rays_chunk(args, model, aperture, (unsigned)k0, (int)std::min(per_launch, pixels - k0),
                                 (float4*)rays + (size_t)k0 * spp * 2, stream);
    return hipGetLastError();
}

}  // namespace yrt
