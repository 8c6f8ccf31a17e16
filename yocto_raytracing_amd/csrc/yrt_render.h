// yrt_render.h -- internal host API between the C-ABI layer (capi.cpp), the device
// scene builder (device_scene.cpp) and the kernel launchers (render.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "yrt_device.h"
#include "yrt_scene.h"

namespace yrt {

// per-phase GPU time of the last render call: HIP events recorded on the launch
// stream around every kernel launch of a phase (enabled by yrt_render_params.timing)
enum render_phase {
    phase_primary = 0,   // camera rays + closest hit + surface (k_primary); a ray batch's level 0 (k_rays_first)
    phase_shadow = 1,    // shadow rays, any hit (k_shadow)
    phase_shade = 2,     // lighting + mirror-ray compaction (k_shade)
    phase_bounce = 3,    // closest hit of mirror rays (k_bounce)
    phase_fold = 4,      // reflection fold (k_fold_children)
    phase_accumulate = 5,
    phase_megakernel = 6,
    phase_lists = 7,     // per-render records and candidate lists (k_relative_records, k_camera_lists, k_bundle_lists, k_list_stats)
    phase_count = 8
};

struct phase_timer {
    bool on = false;
    std::vector<hipEvent_t> pool;  // start/stop pairs
    std::vector<int> phase_of;     // per pair
    size_t used = 0;
    int begin(int phase, hipStream_t s);  // -1 when off
    void end(int idx, hipStream_t s);
    void reset(bool enable) {
        on = enable;
        used = 0;
    }
    // sums elapsed ms per phase (synchronises the recorded events)
    void collect(float* ms, int* launches);
    void destroy();
};

// one scene resident in one GPU's HBM (a single hipMalloc arena)
struct device_scene {
    int device = 0;
    void* arena = nullptr;
    size_t arena_bytes = 0;
    dev_scene_view view = {};
    std::vector<camera> cameras;
    int top_depth = 0;    // instance-BVH depth (stack entries needed)
    int shape_depth = 0;  // deepest shape BVH
    size_t ntnodes = 0, nsnodes = 0, nsprims = 0, ninst = 0;
    size_t max_shape_nodes = 0;
    bool narrow_stack = true;  // all node indices fit 16-bit stack entries
    bool reflective = false;   // any material with kr > 0 (bounce levels needed)
    bool wide_ok = false;      // the 4-wide any-hit walk's stack fits (else the binary walk)
    // the instance-level spine records with the camera origin subtracted from every bound
    // (wavefront.hip k_relative_records, rewritten per render): the primary rays' box tests
    f4* trel = nullptr;
    int nlights = 0;
    int num_cus = 256;  // compute units of the device (persistent grids)
    // wavefront workspace (device), grown on demand
    void* work = nullptr;
    size_t work_bytes = 0;
    // mirror levels: the next level's ray count, copied back behind the level's kernels
    int* level_count_host = nullptr;  // pinned
    hipEvent_t level_count_ev = nullptr;
    // the candidate lists (wavefront.hip k_camera_lists / k_bundle_lists): each render that
    // builds them sums their lengths on the device and copies the sums back behind its kernels
    // (yrt_scene_tile_lists reads them). Lists on or off give the same image.
    // pinned: {camera entries, camera tiles, bundle entries, bundle lists, instances the camera
    // lists' masks exclude, instances the bundle lists' masks exclude} (wavefront.hip list_sums)
    unsigned long long* list_stats_host = nullptr;
    hipEvent_t list_stats_ev = nullptr;
    bool list_stats_recorded = false;  // list_stats_ev has been recorded (yrt_scene_tile_lists waits on it)
    // YRT_LISTS_AUTO / YRT_LISTS_ON: lists whenever the scene allows (ON also puts level 0's
    // shadow rays on the persistent grid at any frame size); YRT_LISTS_OFF: never
    int lists_mode = 0;
    bool last_camera_lists = false, last_bundles = false;  // what the last render used
    // yrt_scene_set_lds_staging: the persistent walks read the instance tree's top from LDS
    int lds_staging = 0;
    int last_lds_staging = 0;  // what the last render staged: bit 0 closest hit, bit 1 any hit
    // yrt_render_light_groups: the last call's table of lights sorted by plane, the source of
    // its copy to the device (wavefront.hip group_buffers::tab)
    std::vector<int> group_tab;
    // the pixel-batch renders (camera.hip render_pixel_batches: yrt_render_adaptive,
    // yrt_render_camera, yrt_render_soft_shadows), grown on demand like `work`: a chunk's rays
    // and colours
    void* batch_rays = nullptr;
    size_t batch_rays_bytes = 0;
    // yrt_render_adaptive (adaptive.hip), grown on demand too: the frame scratch (the flagged
    // count, the base frame with its apron, the flagged list); the flagged count on the host
    // (pinned), copied back behind the flag kernel, and the last call's value of it
    void* adaptive_frame = nullptr;
    size_t adaptive_frame_bytes = 0;
    unsigned long long* adaptive_count_host = nullptr;
    hipEvent_t adaptive_count_ev = nullptr;
    unsigned long long adaptive_refined = 0;
    // soft shadows (upload_soft_shadow_radii): the last call's radius per light, on the host (the
    // source of its copy) and on the device (nlights floats, allocated by the first soft call)
    std::vector<float> soft_radius_host;
    float* soft_radius = nullptr;
    phase_timer timer;
};

// Flatten a host scene (with BVH built) into the HBM layout and upload it.
// Throws std::runtime_error on unsupported input or HIP failure.
device_scene* device_scene_create(const scene& scn, int device);
void device_scene_destroy(device_scene* ds);

// camera constants (raytrace.cpp:16-24): h = 2*focus*tanf(fovy/2), w = h*aspect, y negated
dev_camera make_dev_camera(const camera& c);

// kernels (render.hip)
hipError_t launch_render(device_scene& ds, const dev_render_args& args, void* out_rgba,
                         unsigned long long* counters, bool count_work, hipStream_t stream);
hipError_t launch_trace(const device_scene& ds, const float* rays, int n, int any,
                        unsigned char* hit, int* inst, int* ei, float* ew, float* dist,
                        unsigned long long* counters, bool packet, hipStream_t stream);
// tonemap on the device against the host's thresholds (tonemap_thresholds): bit-exact
// with tonemap_rgba8, i.e. with the host libm's powf
struct tonemap_table {
    float thr[256];
    int neg_inf_level;  // pow(-inf, 1/2.2) = +inf: the one non-positive input that is not 0
};
hipError_t launch_tonemap(const float* rgba, int n, unsigned char* out, const tonemap_table& table,
                          hipStream_t stream);
// the .hdr writer's RGBE bytes on the device (rgbe.h; the layout of rgbe_encode)
hipError_t launch_rgbe(const float* rgba, int w, int h, unsigned char* out, hipStream_t stream);

// the AOV pass (aov.hip k_aov): the planes of yrt_render_aovs in the order of YRT_AOV_*,
// 16 bytes per pixel each (float4, ids int4), window layout and out_stride of launch_render;
// only the planes whose bit is set in `mask` are read or written. The caller zeroes the
// counter lines before the launch; an empty window launches nothing.
enum aov_index {
    aov_depth = 0,
    aov_position = 1,
    aov_normal = 2,
    aov_texcoord = 3,
    aov_albedo = 4,
    aov_ids = 5,
    aov_count = 6
};
struct dev_aov_planes {
    void* plane[aov_count];
};
hipError_t launch_aovs(const device_scene& ds, const dev_render_args& args, unsigned mask, const dev_aov_planes& out,
                       unsigned long long* counters, hipStream_t stream);

// the ID-matte pass (mattes.hip k_matte): the planes of yrt_render_mattes, per key (in the
// order of YRT_MATTE_*) and layer an int4 plane of ids and a float4 plane of coverages, ranks
// 4l..4l+3, window layout and out_stride of launch_render; only the planes of the keys in
// `key_mask` and of the first `layers` (1 or 2) layers are read or written. `dropped` is the
// pass's own device buffer of matte_drop_slots lines of matte_drop_stride u64, the first
// matte_key_count of a line the keys' dropped samples; the caller zeroes it and the counter
// lines before the launch, and adds the lines up afterwards. An empty window launches nothing.
enum matte_key { matte_instance = 0, matte_material = 1, matte_shape = 2, matte_key_count = 3 };
constexpr int matte_layers_max = 2;
constexpr int matte_drop_slots = 256;
constexpr int matte_drop_stride = 4;
struct dev_matte_planes {
    void* ids[matte_key_count][matte_layers_max];
    void* coverage[matte_key_count][matte_layers_max];
};
hipError_t launch_mattes(const device_scene& ds, const dev_render_args& args, unsigned key_mask, int layers,
                         const dev_matte_planes& out, unsigned long long* dropped, unsigned long long* counters,
                         hipStream_t stream);

// the ambient occlusion pass (ao.hip k_ao): yrt_render_ao's plane, float4 per pixel in
// launch_render's layout. rays (1..64), bias and distance are the resolved parameters
// (ao_args.h): K, and the tmin and tmax of every occlusion ray. The caller zeroes the counter
// lines before the launch; an empty window launches nothing.
hipError_t launch_ao(const device_scene& ds, const dev_render_args& args, int rays, float bias, float distance,
                     void* out_rgba, unsigned long long* counters, hipStream_t stream);

// mirror levels the megakernel records per lane (render.hip); the wavefront pipeline
// keeps per-level records in HBM and takes any max_depth
constexpr int megakernel_max_depth = 16;

// traversal stack entries per lane (LDS resident): instance level + shape level
constexpr int traversal_stack_cap = 40;

// wavefront pipeline (wavefront.hip): same contract as launch_render
hipError_t launch_render_wavefront(device_scene& ds, const dev_render_args& args, void* out_rgba,
                                   unsigned long long* counters, bool count_work, bool packet, hipStream_t stream);

// shade() (raytrace.cpp:88-211) for n caller rays (yrt_shade_rays): rays n x {o.xyz, d.xyz,
// tmin, tmax} and out n x RGBA f32, both device pointers; args carries amb and max_depth only.
// The wavefront pipeline in ray mode (wavefront.hip run_rays: k_rays_first as level 0, then the
// render's levels; counters zeroed in its first kernel, timings per phase) ...
// With keep_counters that kernel leaves the counter lines alone and the batch's counts add to
// what they hold: a render made of several batches (camera.hip) passes it from its second on.
// With `soft` (yrt_shade_rays_soft) every light is a disk: K = soft->rays any-hit rays per (hit
// sample, light) at every level (k_soft_shadow), the light's term scaled by the unoccluded share
// (k_soft_shade). soft->radius is device memory, a radius per light (upload_soft_shadow_radii).
constexpr int soft_shadow_rays_max = 64;  // a ray per entry of the table (ao_tables.h)
struct soft_shadow_args {
    int rays;             // K, 1..soft_shadow_rays_max
    const float* radius;  // device: nlights radii, each >= 0 and finite; 0 is the point light
};
hipError_t launch_shade_rays_wavefront(device_scene& ds, const dev_render_args& args, const float* rays, int n,
                                       void* out_rgba, unsigned long long* counters, bool packet, hipStream_t stream,
                                       const soft_shadow_args* soft = nullptr, bool keep_counters = false);
// the call's radii into ds.soft_radius, in stream order: radius[nlights] (host), or `all` for
// every light when radius is null
hipError_t upload_soft_shadow_radii(device_scene& ds, const float* radius, float all, hipStream_t stream);
// ... or one lane per ray through the megakernel's shade_path (render.hip; the caller zeroes
// the counters and caps max_depth at megakernel_max_depth)
hipError_t launch_shade_rays(device_scene& ds, const dev_render_args& args, const float* rays, int n, void* out_rgba,
                             unsigned long long* counters, hipStream_t stream);

// the shading passes (wavefront.hip k_shade_passes / k_accumulate_passes): the planes of
// yrt_render_passes in the order of YRT_PASS_*, float4 per pixel in launch_render's layout;
// only the planes whose bit is set in `mask` are written. beauty_rgba, when not null, receives
// launch_render_wavefront's image from the same walk. Counters and timings as there.
enum pass_index {
    pass_direct = 0,
    pass_diffuse = 1,
    pass_specular = 2,
    pass_reflection = 3,
    pass_ambient = 4,
    pass_count = 5
};
struct dev_pass_planes {
    float* plane[pass_count];
};
hipError_t launch_render_wavefront_passes(device_scene& ds, const dev_render_args& args, unsigned mask,
                                          const dev_pass_planes& out, void* beauty_rgba, unsigned long long* counters,
                                          bool packet, hipStream_t stream);

// light groups (wavefront.hip k_shade_groups / k_accumulate_groups): the planes of
// yrt_render_light_groups, float4 per pixel in launch_render's layout. group_of (host memory,
// copied during the call) gives each of the scene's lights its group in [-1, ngroups); the
// first ngroups of out.group are written, and ambient and beauty where not null. One walk:
// counters and timings as after launch_render_wavefront.
constexpr int light_groups_max = 8;
struct dev_light_group_planes {
    float* group[light_groups_max];
    float* ambient;
    float* beauty;
};
hipError_t launch_render_wavefront_light_groups(device_scene& ds, const dev_render_args& args, const int* group_of,
                                                int ngroups, const dev_light_group_planes& out,
                                                unsigned long long* counters, bool packet, hipStream_t stream);

// The pixel-batch renders (camera.hip render_pixel_batches) shade whole pixels as ray batches:
// k_camera_rays generates a chunk of pixels' rays, launch_shade_rays_wavefront shades them,
// k_camera_resolve sums each pixel's colours into the image, chunk_pixels pixels a batch (0: as
// many as keep a chunk within pixel_batch_rays rays). A chunk's rays and colours live in
// ds.batch_rays. The first batch of a call whose counters nothing has started zeroes them;
// every other batch adds to them (keep_counters).
constexpr long long pixel_batch_rays = 1ll << 23;  // 48 B a ray (32 B ray + 16 B colour): 384 MiB

// adaptive supersampling (adaptive.hip, yrt_render_adaptive): args is the call's frame at its
// full samples per axis (contiguous rows: band 1, stride 1, offset 0). The base frame at
// base_samples per axis comes from launch_render_wavefront over the window grown by one pixel
// (into scratch), k_adaptive_flag tests it against `threshold`, writes it to out_rgba, the byte
// mask to `refined` (may be null; out's layout, 1 B per pixel) and the flagged pixels to a list,
// and the listed pixels are refined as pixel batches of the pinhole (camera_perspective at
// aperture 0: camera_ray's bits). Waits once on the stream, for the flagged count (kept in
// ds.adaptive_refined). The base render starts the counters and every batch adds to them;
// timings are added per phase.
hipError_t launch_render_adaptive(device_scene& ds, const dev_render_args& args, int base_samples, float threshold,
                                  int chunk_pixels, void* out_rgba, unsigned char* refined,
                                  unsigned long long* counters, bool packet, hipStream_t stream);

// camera models (camera.hip, yrt_render_camera / yrt_camera_rays): `model` is a camera_model of
// camera_models.h and `aperture` the resolved lens diameter (camera_args.h); args is the call's
// frame with the call's focus in args.cam (contiguous rows: band 1, stride 1, offset 0).
// launch_render_camera writes the window's image as pixel batches over the window's pixels in
// row-major order. The counters are the batches' sums; timings are added per phase; the handle
// reports no lists and no staging afterwards.
hipError_t launch_render_camera(device_scene& ds, const dev_render_args& args, int model, float aperture,
                                int chunk_pixels, void* out_rgba, unsigned long long* counters, bool packet,
                                hipStream_t stream);
// yrt_render_soft_shadows: launch_render_camera with the soft batch shader
// (launch_shade_rays_wavefront with `soft`): the same chunks and resolve, any camera model
hipError_t launch_render_soft_shadows(device_scene& ds, const dev_render_args& args, int model, float aperture,
                                      int chunk_pixels, const soft_shadow_args& soft, void* out_rgba,
                                      unsigned long long* counters, bool packet, hipStream_t stream);
// k_camera_rays alone over the whole window (which lies inside the image), tile_w * tile_h *
// samples^2 records of 32 bytes into `rays` (device memory); touches no counter
hipError_t launch_camera_rays(device_scene& ds, const dev_render_args& args, int model, float aperture, void* rays,
                              hipStream_t stream);

}  // namespace yrt
