// adaptive.hip -- adaptive supersampling (yrt_render_adaptive): Whitted's own answer to the
// cost of s*s camera samples in every pixel. A base frame at b*b samples per pixel, a contrast
// test between neighbouring pixels of that frame, and the full s*s samples only in the pixels
// the test flags. render.hip includes this file after camera.hip: the feature's kernels are a
// part of that translation unit and of its gfx950 code object, and the refinement runs on
// camera.hip's pixel-batch pipeline (render_pixel_batches, with grow_scratch and scratch_align).
//
// The contract (include/yrt.h): B is yrt_render's frame at `base` samples per
// axis, over the window grown by one pixel on every side and clipped to the image (the apron;
// it lives in scratch, never in `out`). A pixel P of the window is flagged iff a pixel Q of the
// image at Chebyshev distance 1 and a channel c of r, g, b exist with fabsf(B[P].c - B[Q].c) >
// threshold, in float32, an IEEE comparison (false on NaN). A flagged pixel receives exactly
// yrt_render's value at s samples per axis, every other pixel B.
//
// The refined pixels are the flagged list through render_pixel_batches with the pinhole camera:
// camera_perspective at aperture 0 is camera_ray's expression term for term (camera_models.h),
// so a refined pixel is yrt_render's. A pixel's value depends on its own rays alone, so neither
// the order of the flagged list (an atomic per block) nor the chunk size changes a bit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "camera_models.h"
#include "trace_common.h"
#include "yrt_render.h"

namespace yrt {
namespace {

constexpr int AD_BLOCK_X = 64, AD_BLOCK_Y = 4;  // k_adaptive_flag: a wave is 64 pixels of one row

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

}  // namespace

hipError_t launch_render_adaptive(device_scene& ds, const dev_render_args& args, int base_samples, float threshold,
                                  int chunk_pixels, void* out_rgba, unsigned char* refined,
                                  unsigned long long* counters, bool packet, hipStream_t stream) {
    ds.adaptive_refined = 0;
    if (args.tile_w <= 0 || args.tile_h <= 0) {  // an empty window: nothing written, nothing counted
        return hipMemsetAsync(counters, 0, (size_t)cnt_slots * cnt_count * sizeof(unsigned long long), stream);
    }
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
    // the frame scratch: the flagged count, the base frame, the list
    const size_t base_bytes = scratch_align((size_t)base.tile_w * base.tile_h * sizeof(float4));
    const size_t list_bytes = scratch_align((size_t)args.tile_w * rows * sizeof(unsigned));
    if (hipError_t e = grow_scratch(ds.adaptive_frame, ds.adaptive_frame_bytes, 256 + base_bytes + list_bytes);
        e != hipSuccess)
        return e;
    char* at = (char*)ds.adaptive_frame;
    unsigned long long* count = (unsigned long long*)at;
    float4* base_px = (float4*)(at + 256);
    unsigned* list = (unsigned*)(at + 256 + base_bytes);
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
    const int t = T.begin(phase_lists, stream);
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

    // the listed pixels at the call's samples, added to the counters the base render started;
    // what the base render reported of its lists and staging stays the call's report
    const bool camera_lists = ds.last_camera_lists, bundles = ds.last_bundles;
    const int staged = ds.last_lds_staging;
    const hipError_t e = render_pixel_batches(ds, args, camera_perspective, 0.0f, list, flagged, chunk_pixels, nullptr,
                                              (float4*)out_rgba, counters, true, packet, stream);
    ds.last_camera_lists = camera_lists, ds.last_bundles = bundles;
    ds.last_lds_staging = staged;
    return e;
}

}  // namespace yrt
