/* yrt.h -- C-ABI of the MI355X-native renderer for the yocto_raytracing hot path.
 *
 * Plain C: opaque handles, plain pointers and sizes, int status codes, no
 * exceptions and no torch types across the boundary. Every entry point names the
 * reference interface it replaces (reference = sebcossu/yocto_raytracing, src/).
 *
 * Typical use, mirroring main() in src/raytrace.cpp:256-287:
 *     yrt_host_scene* hs;  yrt_scene_load("scene.obj", &hs);       // load_scene
 *     yrt_host_scene_build_bvh(hs, 0);                             // build_bvh(scn, false)
 *     yrt_scene* ds;  yrt_scene_upload(hs, 0, &ds);                // (new) copy to HBM
 *     yrt_render_params p;  yrt_render_params_default(&p);  p.resolution = 720; p.samples = 3;
 *     int w, h;  yrt_image_size(ds, &p, &w, &h);
 *     yrt_render(ds, &p, host_rgba_w_h_4, YRT_MEM_HOST, NULL);     // raytrace()
 *     yrt_save_image("out.png", host_rgba_w_h_4, w, h);            // save_hdr_or_ldr
 */
#ifndef YRT_H
#define YRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YRT_ABI_VERSION 1

/* status codes (the reference has none: it exit(1)s in the loader, scene.cpp:119-122) */
enum {
    YRT_OK = 0,
    YRT_ERR_INVALID_ARG = 1,
    YRT_ERR_IO = 2,          /* file missing / unreadable / malformed */
    YRT_ERR_UNSUPPORTED = 3, /* input the kernels do not handle (mixed shapes, hdr textures, deep BVH) */
    YRT_ERR_HIP = 4,         /* HIP runtime error (message via yrt_last_error) */
    YRT_ERR_NO_DEVICE = 5,
    YRT_ERR_OOM = 6,
    YRT_ERR_INTERNAL = 7
};

typedef struct yrt_host_scene yrt_host_scene; /* host scene + BVH (scene*, scene.h:136-155) */
typedef struct yrt_scene yrt_scene;           /* scene resident in one GPU's HBM */

/* memory location of a caller buffer */
enum { YRT_MEM_HOST = 0, YRT_MEM_DEVICE = 1 };

typedef struct yrt_render_params {
    float ambient[3];  /* raytrace(..., amb, ...): main() passes {a,a,a}, a = -a (0.1) */
    int resolution;    /* vertical resolution -r (raytrace.cpp:216) */
    int width;         /* 0: round(camera.aspect * resolution) as the reference; >0: explicit */
    int samples;       /* -s: samples PER AXIS, s*s per pixel (raytrace.cpp:232-234) */
    int max_depth;     /* trace_first calls per camera sample; reference: unbounded. 0 -> 16.
                          Any depth with the wavefront algorithms (per-level records in HBM);
                          the megakernel keeps 16 per lane (deeper: YRT_ERR_UNSUPPORTED) */
    int camera;        /* camera index; reference: cameras.front() == 0 */
    int x0, y0;        /* window origin in image pixels */
    int tile_w, tile_h;/* window size; 0 -> to the image edge */
    int band;          /* row interleave for multi-GPU sharding: rows are taken in bands of */
    int band_stride;   /*   `band` rows; local band b is image band b*band_stride+band_offset */
    int band_offset;   /*   (band=1,stride=1,offset=0: contiguous rows) */
    int out_stride;    /* output row stride in pixels; 0 -> tile_w */
    int count_work;    /* 1: also count box/instance/primitive tests (slower; for roofline bytes) */
    int algorithm;     /* YRT_ALGO_*: identical results, different schedules */
    int timing;        /* 1: record HIP events per kernel phase (read with yrt_last_timings);
                          2: keep adding to the previous record (time a loop of renders) */
} yrt_render_params;

/* render algorithms: identical outputs, different schedules
 *   WAVEFRONT       kernel per stage, one lane per camera sample, wave-coherent (packet) BVH walk
 *   MEGAKERNEL      one kernel, one lane per pixel walking the reference's loops
 *   WAVEFRONT_LANE  kernel per stage, one independent BVH walk per lane */
enum { YRT_ALGO_WAVEFRONT = 0, YRT_ALGO_MEGAKERNEL = 1, YRT_ALGO_WAVEFRONT_LANE = 2 };
enum { YRT_LISTS_AUTO = 0, YRT_LISTS_ON = 1, YRT_LISTS_OFF = 2 };

/* counters accumulated by the last yrt_render / yrt_trace_* on a scene handle */
typedef struct yrt_stats {
    unsigned long long rays;            /* intersect_first + intersect_any calls */
    unsigned long long camera_samples;  /* eval_camera calls */
    unsigned long long depth_truncated; /* paths cut by max_depth (0 = parity-neutral) */
    unsigned long long stack_overflow;
    unsigned long long box_tests;       /* count_work only */
    unsigned long long instance_entries;
    unsigned long long prim_tests;
    unsigned long long shaded_hits;
    unsigned long long texture_lookups;
    unsigned long long shadow_rays;     /* the shadow-ray phase alone (intersect_any calls; the
                                         * reference's count: a shadow ray whose light term is
                                         * exactly zero is counted but not traced, DESIGN.md §5,
                                         * see shadow_rays_culled) */
    unsigned long long shadow_box_tests;        /* count_work only */
    unsigned long long shadow_instance_entries; /* count_work only */
    unsigned long long shadow_prim_tests;       /* count_work only */
    unsigned long long wave_node_visits;        /* count_work, packet walk: node steps per wave */
    unsigned long long wave_prim_visits;        /* count_work, packet walk: primitive steps per wave */
    unsigned long long shadow_wave_node_visits; /* the same, shadow-ray phase alone */
    unsigned long long shadow_rays_culled;      /* of shadow_rays: answered without a walk because
                                                 * the light term is exactly zero (recorded as
                                                 * occluded; 0 with count_work, which walks every
                                                 * ray). Rays walked = rays - shadow_rays_culled */
} yrt_stats;

/* GPU time per kernel phase of the last render (HIP events on the launch stream) */
enum {
    YRT_PHASE_PRIMARY = 0,    /* camera rays + closest hit + surface */
    YRT_PHASE_SHADOW = 1,     /* shadow rays (any hit) */
    YRT_PHASE_SHADE = 2,      /* lighting + mirror-ray compaction */
    YRT_PHASE_BOUNCE = 3,     /* closest hit of mirror rays */
    YRT_PHASE_FOLD = 4,       /* reflection fold */
    YRT_PHASE_ACCUMULATE = 5, /* ordered per-pixel sum */
    YRT_PHASE_MEGAKERNEL = 6, /* the one-kernel path */
    YRT_PHASE_LISTS = 7,      /* per-render camera-relative records and candidate-leaf lists */
    YRT_PHASE_COUNT = 8
};
typedef struct yrt_timings {
    float ms[YRT_PHASE_COUNT];
    int launches[YRT_PHASE_COUNT];
} yrt_timings;

/* ---- library ---- */
int yrt_abi_version(void);
const char* yrt_status_string(int status);
/* message of the last error on this thread (empty string if none) */
const char* yrt_last_error(void);
int yrt_device_count(int* count);

/* ---- host scene: loader, serialisation, BVH ---- */
/* load_scene (src/scene.cpp:113-225): Yocto OBJ (.obj) or the .yrtscene interchange file */
int yrt_scene_load(const char* path, yrt_host_scene** out);
/* serialise the shading-relevant arrays (.yrtscene, gzip) */
int yrt_scene_save(const yrt_host_scene* hs, const char* path);
/* build_bvh(scene*, bool equal_num) (src/scene.cpp:554-565, decl scene.h:238) */
int yrt_host_scene_build_bvh(yrt_host_scene* hs, int equal_num);
/* build_bvh with the tree construction (node boxes, splits, partitions) on GPU `device`:
 * the same nodes and leaf order as yrt_host_scene_build_bvh, byte for byte. equal_num != 0
 * is YRT_ERR_UNSUPPORTED. kernel_ms (may be NULL): GPU time of the build's level passes */
int yrt_host_scene_build_bvh_gpu(yrt_host_scene* hs, int equal_num, int device, float* kernel_ms);
/* dump the BVHs (.yrtbvh) byte-compatible with the reference's bvh_node (scene.h:9-15) */
int yrt_host_scene_save_bvh(const yrt_host_scene* hs, const char* path);
/* counts: [cameras, textures, materials, shapes, instances, lights, bvh nodes(instance
 * level), bvh depth(instance level), max shape bvh depth, triangles, lines, points] */
int yrt_host_scene_info(const yrt_host_scene* hs, long long* info12);
/* image size raytrace() would produce: W = round(aspect*res), H = res (raytrace.cpp:215-216) */
int yrt_host_image_size(const yrt_host_scene* hs, int camera, int resolution, int* w, int* h);
void yrt_host_scene_free(yrt_host_scene* hs);

/* ---- host scene from memory: the reference's scene* built field by field ----
 * For a host program that already holds a scene (scene.h:26-155) -- e.g. the
 * reference's own main() after load_scene -- instead of a file. Arrays are copied.
 * Frames are 12 floats {x.xyz, y.xyz, z.xyz, o.xyz} (frame3f, vmath.h). Indices
 * returned through `index` are what materials/instances refer to (-1 = none). */
typedef struct yrt_material_desc { /* material, scene.h:62-86 */
    float ke[3], kd[3], ks[3], kr[3];
    float rs;
    int kd_txt, ks_txt; /* texture index or -1 */
} yrt_material_desc;
typedef struct yrt_shape_desc { /* shape, scene.h:26-50; one primitive kind per shape */
    int npos;
    const float* pos;      /* npos x 3 */
    const float* norm;     /* npos x 3 or NULL */
    const float* texcoord; /* npos x 2 or NULL */
    const float* radius;   /* npos or NULL (required for points/lines) */
    int npoints;
    const int* points;     /* npoints */
    int nlines;
    const int* lines;      /* nlines x 2 */
    int ntriangles;
    const int* triangles;  /* ntriangles x 3 */
} yrt_shape_desc;
int yrt_host_scene_create(yrt_host_scene** out);
/* camera, scene.h:115-123 */
int yrt_host_scene_add_camera(yrt_host_scene* hs, const float frame[12], float fovy, float aspect, float aperture,
                              float focus, int* index);
/* texture, scene.h:54-58: 8-bit RGBA rows, pixels[j*w+i] */
int yrt_host_scene_add_texture(yrt_host_scene* hs, int w, int h, const unsigned char* rgba8, int* index);
int yrt_host_scene_add_material(yrt_host_scene* hs, const yrt_material_desc* m, int* index);
int yrt_host_scene_add_shape(yrt_host_scene* hs, const yrt_shape_desc* s, int* index);
/* instance, scene.h:99-111 */
int yrt_host_scene_add_instance(yrt_host_scene* hs, const float frame[12], int shape, int material, int* index);

/* ---- device scene ---- */
/* flatten to the HBM layout and upload to `device` (needs a built BVH) */
int yrt_scene_upload(const yrt_host_scene* hs, int device, yrt_scene** out);
size_t yrt_scene_device_bytes(const yrt_scene* ds);
void yrt_scene_free(yrt_scene* ds);

/* ---- the hot path ---- */
void yrt_render_params_default(yrt_render_params* p);
int yrt_image_size(const yrt_scene* ds, const yrt_render_params* p, int* w, int* h);
/* raytrace() (src/raytrace.cpp:213-254). out: RGBA f32, row-major pixels[j*W+i]
 * (image4f, image.h:8-17) restricted to the params window/bands; `mem` says whether
 * `out` is a host or device pointer; `stream` is a hipStream_t (NULL = default).
 * A host `out` makes the call synchronous; a device `out` is stream-ordered. */
int yrt_render(yrt_scene* ds, const yrt_render_params* p, float* out, int mem, void* stream);
/* batch intersect_first (src/scene.cpp:483-488). rays: n x {o.xyz, d.xyz, tmin, tmax}.
 * Outputs per ray: hit (0/1), instance index (-1 on miss), element index ei (-1 on miss),
 * ew[4] barycentrics, dist. All pointers in `mem` space. */
int yrt_trace_first(yrt_scene* ds, const float* rays, int n, unsigned char* hit, int* inst, int* ei,
                    float* ew, float* dist, int mem, void* stream);
/* batch intersect_any (src/scene.cpp:489-493) */
int yrt_trace_any(yrt_scene* ds, const float* rays, int n, unsigned char* hit, int mem, void* stream);
/* walks used by yrt_trace_first/any on this handle (identical results): YRT_ALGO_WAVEFRONT
 * (default) = the render path's wave-coherent closest-hit walk and 4-wide any-hit walk;
 * YRT_ALGO_MEGAKERNEL / YRT_ALGO_WAVEFRONT_LANE = one independent walk per lane */
int yrt_scene_set_trace_algorithm(yrt_scene* ds, int algorithm);
/* per-tile candidate lists of yrt_render (camera frontier lists and shadow
 * bundles; identical images either way): YRT_LISTS_ON builds them whenever the scene allows
 * (an instance tree of >= 8 wide records; shadow bundles for at most 8 lights, a rotated
 * light's rays walking the tree; ON also runs level 0's shadow rays on the persistent grid at
 * any frame size), YRT_LISTS_AUTO (default) does the same from 9 samples per pixel (their
 * cost is per pixel tile, their gain per sample), YRT_LISTS_OFF never builds them. No mode
 * reads anything back during a render. Set it between renders of the handle, not while one
 * is in flight. */
int yrt_scene_set_tile_lists(yrt_scene* ds, int mode);
/* the lists' state after the last yrt_render on this handle (synchronises with it):
 * whether each kind is in use, and sums[4] = {camera-list entries, camera lists, bundle-list
 * entries, bundle lists} of the last render that built lists (a list that fell back to the
 * tree counts as its capacity + 1) */
int yrt_scene_tile_lists(yrt_scene* ds, int* camera_on, int* bundles_on, unsigned long long* sums);
/* the instances the lists' masks excluded in the last render that built lists (synchronises
 * with it): excluded[0] = over every camera list's leaves, the instances whose world box the
 * tile's cone excludes; excluded[1] = the same over every shadow bundle's list and its hull
 * (instance masks; the walks pass over them, identical images) */
int yrt_scene_tile_list_masks(yrt_scene* ds, unsigned long long* excluded);
/* LDS staging of the instance tree's hot top (the north_star's "hot node tiles staged in LDS";
 * DESIGN.md §5). on = 1: yrt_render's persistent closest-hit grid copies the first 511
 * camera-relative spine records, and its persistent any-hit grid the first 85 4-wide records
 * (scenes with at least that many), into LDS once per block, and the walks read those records
 * from LDS instead of through the scalar cache. The tile lists are not built while it is on:
 * their walks start below the tree's top. Identical images either way. Off (0) by default:
 * measured slower, the top records being scalar-cache hits already. Set it between renders. */
int yrt_scene_set_lds_staging(yrt_scene* ds, int on);
/* what the last yrt_render on this handle staged: bit 0 the closest hit, bit 1 the any hit */
int yrt_scene_lds_staging(yrt_scene* ds, int* staged);
/* counters of the last render/trace call on this handle (synchronises the stream) */
int yrt_last_stats(yrt_scene* ds, yrt_stats* stats);
/* per-phase GPU times of the last yrt_render with p->timing = 1 (synchronises) */
int yrt_last_timings(yrt_scene* ds, yrt_timings* timings);

/* ---- image output ---- */
/* tonemap (src/image.cpp:55-77, exposure 0, srgb) of n RGBA f32 pixels into RGBA8 */
int yrt_tonemap(const float* rgba, int n, unsigned char* out, int mem, void* stream);
/* save_hdr_or_ldr (src/image.cpp:81-88): .hdr -> RGBE, else PNG of the tonemap */
int yrt_save_image(const char* path, const float* rgba, int w, int h);
/* the same for a frame in `mem` space: with YRT_MEM_DEVICE the PNG's tonemap runs on the
 * GPU (the stream's device) and only the RGBA8 image crosses PCIe; .hdr copies the floats */
int yrt_save_image_mem(const char* path, const float* rgba, int w, int h, int mem, void* stream);

/* ---- the GPUs of one node, one host process ----
 * Replaces main()'s single raytrace() call (src/raytrace.cpp:282) for N devices: the
 * scene is replicated on every device, device r renders the interleaved 8-row image
 * bands r, r+n, r+2n, ..., and the float framebuffer is gathered to devices[0] over
 * RCCL (grouped ncclSend/ncclRecv over xGMI) and reassembled in image order. A device
 * listed twice uses plain device copies instead (a rehearsal on fewer GPUs). */
typedef struct yrt_multi yrt_multi;
enum { YRT_TRANSPORT_COPY = 0, YRT_TRANSPORT_RCCL = 1 };
int yrt_multi_create(const yrt_host_scene* hs, const int* devices, int n, yrt_multi** out);
void yrt_multi_free(yrt_multi* m);
/* n devices and the gather transport (YRT_TRANSPORT_*) */
int yrt_multi_info(const yrt_multi* m, int* n, int* transport);
/* raytrace() of the whole frame (window/band fields of p must be defaults). out: W*H*4
 * floats, host memory or device memory on devices[0]. Synchronous. */
int yrt_multi_render(yrt_multi* m, const yrt_render_params* p, float* out, int mem);
/* counters of the last yrt_multi_render summed over the devices */
int yrt_multi_last_stats(yrt_multi* m, yrt_stats* stats);
/* ms of the last yrt_multi_render on the root's stream: until every shard is rendered,
 * then gather + reassembly */
int yrt_multi_last_timings(const yrt_multi* m, float* render_ms, float* gather_ms);
/* one-shot: create, render, free */
int yrt_render_multi(const yrt_host_scene* hs, const int* devices, int n, const yrt_render_params* p, float* out,
                     int mem);

/* ---- AOVs: the camera hit's geometry buffers ----
 * A pass of its own over the beauty's sample grid and box filter (raytrace.cpp:228-250): per
 * pixel the s*s camera samples, jj outer and ii inner, each answered by intersect_first. A
 * float AOV is the float32 sum, in that order, of the value below over the samples that hit,
 * divided by float(s*s); a miss adds nothing, so .xyz is premultiplied by .w, the coverage
 * (hits / (s*s)) -- divide by .w to un-premultiply.
 *   DEPTH     float4 {dist, 0, 0, w}  intersection3f::dist along the normalised camera ray
 *   POSITION  float4 {eval_pos, w}    world position (scene.h:159-172)
 *   NORMAL    float4 {eval_norm, w}   world shading normal, not renormalised after averaging
 *   TEXCOORD  float4 {u, v, 0, w}     eval_texcoord; points give {0, 0}
 *   ALBEDO    float4 {kd, w}          mat->kd, times its kd_txt lookup (raytrace.cpp:150-154)
 *   IDS       int4, not averaged: the pixel's first sample (jj = 0, ii = 0) as {instance index
 *             in scene order, ei, material index, shape index}; all -1 on a miss */
enum { YRT_AOV_DEPTH = 0, YRT_AOV_POSITION = 1, YRT_AOV_NORMAL = 2, YRT_AOV_TEXCOORD = 3,
       YRT_AOV_ALBEDO = 4, YRT_AOV_IDS = 5, YRT_AOV_COUNT = 6 };
typedef struct yrt_aov_planes { void* plane[YRT_AOV_COUNT]; } yrt_aov_planes; /* 16 B per pixel each */
/* mask: bit 1 << YRT_AOV_x per requested AOV; only their planes are read from `out` and
 * written. Planes have the layout of yrt_render's output (row-major window, out_stride), and
 * resolution, width, samples, camera, the window, the band interleave and out_stride of `p`
 * mean what they mean there (local rows past the image edge read as zeros, ids -1); ambient,
 * max_depth, algorithm, count_work and timing are ignored. `mem` and `stream` as in
 * yrt_render: host planes make the call synchronous, device planes are stream-ordered.
 * yrt_last_stats then reports rays == camera_samples == window pixels * s*s. */
int yrt_render_aovs(yrt_scene* ds, const yrt_render_params* p, unsigned mask, const yrt_aov_planes* out, int mem,
                    void* stream);

/* ---- shading passes: the beauty split into the terms shade() adds up ----
 * One render gives the beauty and, per pixel, the box filter (the float32 sum over the s*s
 * camera samples, jj outer and ii inner, from +0, divided by float(s*s)) of each term of the
 * level-0 shade() call (raytrace.cpp:88-211), in the reference's operations and order:
 *   DIRECT      c after the light loop: from +0, c = c + (ld + ls) per unoccluded light
 *   DIFFUSE     the same chain over the same lights with ld alone
 *   SPECULAR    the same chain with ls alone
 *   REFLECTION  the vector added at raytrace.cpp:203, col * kr, col the whole recursive shade()
 *               of the mirror ray; 0 * kr where max_depth cuts the ray; +0 without kr
 *   AMBIENT     la = amb * kd (* its kd_txt lookup)
 * A sample that misses adds +0 to every pass. With s = 1, beauty == (DIRECT + REFLECTION) +
 * AMBIENT in float32, bit for bit. .w is 1 for a pixel of the image; local rows past the image
 * edge read as zeros, as in yrt_render. */
enum { YRT_PASS_DIRECT = 0, YRT_PASS_DIFFUSE = 1, YRT_PASS_SPECULAR = 2,
       YRT_PASS_REFLECTION = 3, YRT_PASS_AMBIENT = 4, YRT_PASS_COUNT = 5 };
typedef struct yrt_pass_planes { float* plane[YRT_PASS_COUNT]; } yrt_pass_planes; /* RGBA f32, 16 B per pixel */
/* mask: bit 1 << YRT_PASS_x per requested pass, one to all five; only their planes are read
 * from `out` and written (anything else: YRT_ERR_INVALID_ARG). `beauty`, when not NULL, receives
 * exactly what yrt_render writes for the same `p`, from the same walk. Every field of `p` means
 * what it means in yrt_render, except that the algorithm is YRT_ALGO_WAVEFRONT or
 * YRT_ALGO_WAVEFRONT_LANE and count_work is 0 (otherwise YRT_ERR_UNSUPPORTED). Planes have the
 * layout of yrt_render's output (row-major window, out_stride; padding columns keep the
 * caller's bytes). Host planes make the call synchronous, device planes are stream-ordered. An
 * empty window leaves the planes untouched. yrt_last_stats and yrt_last_timings then report
 * what they report after yrt_render of the same `p`. */
int yrt_render_passes(yrt_scene* ds, const yrt_render_params* p, unsigned mask, const yrt_pass_planes* out,
                      float* beauty /* may be NULL */, int mem, void* stream);

/* ---- shade() for caller-supplied rays ----
 * shade() (src/raytrace.cpp:88-211) for n caller rays. rays: n x {o.xyz, d.xyz, tmin, tmax}
 * as yrt_trace_first; out: n x RGBA f32, out[k] = shade(rays[k]) = {c.xyz, 1}, {0,0,0,1} on a miss.
 * The level-0 ray is used as given: o, d (not renormalised), tmin and tmax all reach the
 * closest-hit query, and the view vector is normalize(ray.o - p) from that ray's own origin
 * (raytrace.cpp:147,196), so a batch may mix origins freely (orthographic, fisheye or panoramic
 * cameras, light probes). Mirror and shadow rays, the accumulation order and max_depth are
 * yrt_render's: a batch of one camera's eval_camera rays gives that render's samples bit for bit.
 * Of `p`, ambient, max_depth, algorithm and timing mean what they mean in yrt_render (the
 * megakernel takes max_depth <= 16 on a reflective scene, else YRT_ERR_UNSUPPORTED); count_work
 * = 1 is YRT_ERR_UNSUPPORTED; every other field is ignored. `mem` says where both `rays` and
 * `out` live: host buffers make the call synchronous, device buffers (out 16-byte aligned) are
 * stream-ordered; `out` may not overlap `rays`. A null handle, p, rays or out with n > 0, n < 0
 * or a bad `mem` return YRT_ERR_INVALID_ARG before any device call; n == 0 returns YRT_OK, writes
 * nothing and leaves the counters at zero. The tile-list mode and the LDS staging of the handle
 * do not change the result: a batch builds no lists and stages nothing, and yrt_scene_tile_lists
 * / yrt_scene_lds_staging report that. yrt_last_stats then gives rays = the reference's
 * intersect_first + intersect_any calls for these n shade() calls, camera_samples = n, and
 * shadow_rays, shadow_rays_culled and depth_truncated as after yrt_render; yrt_last_timings the
 * level-0 closest hit under YRT_PHASE_PRIMARY and the other phases as in a render. */
int yrt_shade_rays(yrt_scene* ds, const yrt_render_params* p, const float* rays, int n, float* out_rgba, int mem,
                   void* stream);

/* ---- light groups: one beauty plane per set of lights, from one render ----
 * Light k is the k-th instance in scene order whose material has ke > 0 in every component
 * (raytrace.cpp:126). group_of[nlights] (host memory, copied during the call) gives each light
 * its group in [0, ngroups), or -1 for a light that is in no plane; 1 <= ngroups <=
 * YRT_LIGHT_GROUPS_MAX. Per camera sample, plane g's value is shade() (raytrace.cpp:88-211)
 * with the light loop over the lights of group g only, in scene order, from c = +0, and with
 * la = {0,0,0} * kd; the mirror term is that same function of the mirror ray, times kr (0 * kr
 * where max_depth cuts it); a miss is {0,0,0,1}. The ambient plane is the same recursion with no
 * light and la = ambient * kd. Each plane is the beauty's box filter of its value. So group g's
 * plane has the bits yrt_render writes for the scene in which every light outside g has ke = 0,
 * rendered with ambient 0; the ambient plane those of the scene with every ke = 0 and the
 * caller's ambient; `beauty` those of yrt_render for the same `p`, from the same walk; and the
 * beauty is the sum of the planes up to float32 rounding (the image is linear in each ke and in
 * the ambient). A shadow ray answered without a walk (yrt_stats.shadow_rays_culled) counts as
 * occluded, as in yrt_render. (Materials with a non-finite kd are outside this contract.)
 * Every field of `p` means what it means in yrt_render, except that the algorithm is
 * YRT_ALGO_WAVEFRONT or YRT_ALGO_WAVEFRONT_LANE and count_work is 0 (otherwise
 * YRT_ERR_UNSUPPORTED). Planes have yrt_render's layout (row-major window, out_stride; padding
 * columns keep the caller's bytes); host planes make the call synchronous, device planes are
 * stream-ordered; an empty window leaves them untouched. A null handle, p, group_of or out,
 * nlights other than the scene's light count, ngroups outside 1..8, a group_of entry outside
 * [-1, ngroups), a null plane among the first ngroups or a bad `mem` return
 * YRT_ERR_INVALID_ARG before any device call. A scene without lights takes nlights = 0; its
 * group planes, like an empty group's, are black with .w = 1. yrt_last_stats and
 * yrt_last_timings report what they report after yrt_render of the same `p` (every shadow ray
 * walked once, depth_truncated counted once), the group shading under YRT_PHASE_SHADE and the
 * per-pixel sums under YRT_PHASE_ACCUMULATE. The tile-list mode and the LDS staging do not
 * change the planes. */
#define YRT_LIGHT_GROUPS_MAX 8
/* instance index (scene order) of each light, in light order; n = their count. inst may be NULL (count only) */
int yrt_host_scene_lights(const yrt_host_scene* hs, int* inst, int cap, int* n);
typedef struct yrt_light_group_planes {
    float* group[YRT_LIGHT_GROUPS_MAX]; /* the first ngroups must be non-null */
    float* ambient;                     /* may be NULL */
    float* beauty;                      /* may be NULL */
} yrt_light_group_planes;
int yrt_render_light_groups(yrt_scene* ds, const yrt_render_params* p, const int* group_of, int nlights,
                            int ngroups, const yrt_light_group_planes* out, int mem, void* stream);

/* ---- ID mattes: ranked id/coverage pairs per pixel, from one pass ----
 * YRT_AOV_IDS is the pixel's first sample, so a mask cut from it is aliased at every
 * silhouette. A matte stores, per pixel, the few ids that cover it, each with its share of the
 * pixel's s*s camera samples: the matte of any set of ids is then a sum of coverages, box
 * filtered exactly as the beauty is. A matte is computed per key; a key's value for a hit is
 * the .x (INSTANCE: the instance index in scene order), .z (MATERIAL) or .w (SHAPE) of
 * YRT_AOV_IDS. R = 4 * layers ranks are stored. Per pixel and key, over the beauty's sample
 * grid (raytrace.cpp:228-250, jj outer, ii inner, each sample answered by intersect_first):
 * start with an empty table of R entries; a sample that misses does nothing; a sample that hits
 * with id v adds one to v's count if v is in the table, else appends (v, 1) if an entry is
 * free, else is dropped and counted in the key's dropped total. After the last sample the
 * entries are ordered by count descending, ties by id ascending; rank r is
 * {id, float(count) / float(s*s)}, an unused rank {-1, +0.0f}. So per pixel of the image
 * sum(counts) + the pixel's dropped samples == its hits; the misses' share is implicit.
 * Local rows past the image edge read as id -1 and coverage 0. */
enum { YRT_MATTE_INSTANCE = 0, YRT_MATTE_MATERIAL = 1, YRT_MATTE_SHAPE = 2, YRT_MATTE_KEY_COUNT = 3 };
#define YRT_MATTE_LAYERS_MAX 2
typedef struct yrt_matte_planes {          /* each plane 16 B per pixel, yrt_render's layout */
    int*   ids[YRT_MATTE_KEY_COUNT][YRT_MATTE_LAYERS_MAX];       /* int4: ranks 4l .. 4l+3 */
    float* coverage[YRT_MATTE_KEY_COUNT][YRT_MATTE_LAYERS_MAX];  /* float4, same ranks */
} yrt_matte_planes;
/* key_mask: bit 1 << YRT_MATTE_x per requested key, one to all three; layers: 1 or 2. Only the
 * planes of the requested keys' first `layers` layers are read from `out` and written. Every
 * key comes from the same walk. The fields of `p` are used and ignored exactly as in
 * yrt_render_aovs (resolution, width, samples, camera, the window, the band interleave and
 * out_stride are used); padding columns keep the caller's bytes; an empty window or band writes
 * nothing and counts nothing. Host planes make the call synchronous, device planes are
 * stream-ordered. yrt_last_stats then reports rays == camera_samples == window pixels * s*s,
 * whatever the number of keys. A null handle, p or out, a key_mask that is 0 or has bits beyond
 * the three keys, layers outside 1..2, a null plane among those requested, a bad `mem` or a bad
 * camera index return YRT_ERR_INVALID_ARG before any device call. The pass shares no state with
 * yrt_render. */
int yrt_render_mattes(yrt_scene* ds, const yrt_render_params* p, unsigned key_mask, int layers,
                      const yrt_matte_planes* out, int mem, void* stream);
/* the dropped samples per key of the last yrt_render_mattes on the handle, summed over its
 * window (0 for a key that was not requested, and before any such call); synchronises the stream */
int yrt_scene_matte_dropped(yrt_scene* ds, unsigned long long dropped[YRT_MATTE_KEY_COUNT]);
/* each instance's shape and material index, in scene order: what turns a material or shape id
 * back into a set of instances. n is always set to their count; shape and material may each be
 * NULL (both NULL: the count only), else the first min(n, cap) entries are written */
int yrt_host_scene_instances(const yrt_host_scene* hs, int* shape, int* material, int cap, int* n);

/* ---- adaptive supersampling: refine only the pixels that show contrast ----
 * yrt_render spends s*s camera samples on every pixel. This call samples the frame at b*b per
 * pixel and supersamples only where neighbouring pixels differ (Whitted's adaptive
 * supersampling). With s = p->samples and b = base_samples, 1 <= b <= s, and every other field
 * of `p` meaning what it means in yrt_render:
 *   1. B is what yrt_render writes for `p` with samples = b, over the window grown by one pixel
 *      on every side and clipped to the image (the apron; it goes to scratch, never to `out`).
 *   2. An image pixel P of the window is flagged iff a pixel Q of the image with
 *      max(|Px-Qx|, |Py-Qy|) == 1 and a channel c of r, g, b exist with
 *      fabsf(B[P].c - B[Q].c) > threshold: float32 arithmetic, an IEEE comparison (false on NaN),
 *      "exists", not "max of". Neighbours are pixels of the image, not of the window: a window's
 *      result is the crop of the whole frame's, bit for bit.
 *   3. A flagged pixel receives exactly yrt_render's value for samples = s: its s*s camera rays
 *      (raytrace.cpp:228-250, jj outer and ii inner), each shaded by shade(), summed in float32
 *      in that order from +0 and divided by float(s*s), .w = 1.
 *   4. `out` has yrt_render's window layout (padding columns keep the caller's bytes): a flagged
 *      pixel its refined value, every other image pixel B, local rows past the image edge zeros.
 *      `refined`, when not NULL, is one byte per pixel in the same layout and stride: 1 flagged,
 *      0 not, padding untouched.
 * So threshold = +inf gives yrt_render(samples = b); on a frame of at least 2 x 2 finite pixels
 * threshold < 0 gives yrt_render(samples = s); and b == s gives that render at any threshold.
 * A null handle, p, a or out, a NaN threshold, b outside [1, s] after defaulting, chunk_pixels
 * < 0, a bad `mem` or a bad camera return YRT_ERR_INVALID_ARG before any device call.
 * YRT_ALGO_MEGAKERNEL, count_work = 1 and a band interleave other than band = 1, band_stride =
 * 1, band_offset = 0 (the apron needs contiguous rows) return YRT_ERR_UNSUPPORTED. The call
 * waits once on the stream, for the flagged count (as a reflective render does for its level
 * counts); after that a host `out` makes it synchronous and a device `out` (16-byte aligned) is
 * stream-ordered. The tile-list mode and the LDS staging of the handle apply to the base render
 * and cannot change a bit. yrt_last_stats reports the base render's counters plus the refined
 * pixels': camera_samples == grown-window image pixels * b*b + flagged * s*s, and likewise rays,
 * shadow_rays, shadow_rays_culled and depth_truncated. yrt_last_timings adds the refinement's
 * phases to the base's, the flag kernel under YRT_PHASE_LISTS and the refined pixels' sums
 * under YRT_PHASE_ACCUMULATE. */
typedef struct yrt_adaptive_params {
    int   base_samples;  /* samples per axis of the base frame; 0 -> 1 */
    float threshold;     /* contrast above which a pixel is refined */
    int   chunk_pixels;  /* refined pixels per shading batch; 0 -> sized to the workspace; never changes a bit of the result */
} yrt_adaptive_params;
int yrt_render_adaptive(yrt_scene* ds, const yrt_render_params* p, const yrt_adaptive_params* a,
                        float* out, unsigned char* refined /* may be NULL */, int mem, void* stream);
/* the pixels the last yrt_render_adaptive on the handle flagged (0 before any); synchronises */
int yrt_scene_adaptive_refined(yrt_scene* ds, unsigned long long* pixels);

/* ---- ambient occlusion: cosine-weighted any-hit rays per camera sample ----
 * Per pixel the share of the hemisphere above the camera hit that is open within `distance`.
 * Over the beauty's sample grid (raytrace.cpp:228-250, jj outer, ii inner) each camera sample
 * is answered by intersect_first, exactly as in yrt_render_aovs. A sample that misses
 * contributes nothing. A sample that hits a shape of lines or points casts no ray and counts
 * as K unoccluded rays (eval_pos of a point is the sphere's centre, eval_norm of a line its
 * tangent: there is no hemisphere). A sample that hits a triangle casts K rays, all float32,
 * evaluated left to right with no contraction:
 *   1. p = eval_pos, n = eval_norm, d the camera ray's direction; if dot(n, d) > 0.0f then
 *      n = -n (false on NaN); dot is a.x*b.x + a.y*b.y + a.z*b.z.
 *   2. the basis (Duff et al., the sign taken so that +0 and -0 agree):
 *      sg = (n.z >= 0.0f) ? 1.0f : -1.0f;  a = -1.0f / (sg + n.z);  b = n.x * n.y * a;
 *      b1 = { 1.0f + sg * n.x * n.x * a, sg * b, -sg * n.x };  b2 = { b, sg + n.y * n.y * a, -n.y }.
 *   3. r = ((i & 3) | (j & 3) << 2) ^ ((jj * s + ii) & 15) with i, j the pixel's image
 *      coordinates (not the window's); (c, sn) = rots[r].
 *   4. for k = 0 .. K-1 with (tx, ty, tz) = dirs[k]:  x = c*tx - sn*ty;  y = sn*tx + c*ty;
 *      dir = (b1*x + b2*y) + n*tz componentwise; the ray {p, dir, bias, distance}, not
 *      renormalised, is answered by intersect_any.
 *   5. the sample's count is the number of its K rays that are not occluded.
 * The tables are compile-time constants (yrt_ao_tables returns them): dirs[k] =
 * (rr cos phi, rr sin phi, sqrt(1 - u1)) with u1 = halton_2(k+1), u2 = halton_3(k+1),
 * rr = sqrt(u1), phi = 2 pi u2 -- cosine-weighted, so the plain count is the estimator, any
 * prefix K is a usable set, and the smallest tz is 0.125; rots[r] = (cos t, sin t) with
 * t = 2 pi bitrev4(r) / 16. Each value is computed in double and rounded once to float32.
 * `out` has yrt_render's window layout (RGBA f32, out_stride, padding columns keep the
 * caller's bytes, local rows past the image edge read as zeros). Per image pixel U is the sum
 * of the sample counts (K per line or point hit), a = float(U) / float(K*s*s),
 * w = float(hits) / float(s*s), and the pixel is {a, a, a, w}: .w is the depth AOV's .w bit
 * for bit, 0 <= a <= w, and a / w is the pixel's ambient occlusion in [0, 1]. The result is a
 * count: the same bits on every run. The fields of `p` are used and ignored exactly as in
 * yrt_render_aovs (resolution, width, samples, camera, the window, the band interleave and
 * out_stride are used); a window is the crop of the whole frame's result and band shards
 * reassemble to it; an empty window or band writes nothing and counts nothing. A host `out`
 * makes the call synchronous, a device `out` (16-byte aligned) is stream-ordered. The pass
 * shares no state with yrt_render; the tile-list mode and the LDS staging do not apply.
 * yrt_last_stats reports camera_samples == window image pixels * s*s, shadow_rays == K *
 * (samples that hit a triangle), rays == camera_samples + shadow_rays, every other counter 0.
 * A null handle, p, a or out, rays outside 1..64 after defaulting, a distance that is NaN or
 * <= 0, a bias that is NaN, negative, infinite or >= distance, a bad `mem` or a bad camera
 * index return YRT_ERR_INVALID_ARG before any device call. */
#define YRT_AO_RAYS_MAX 64
typedef struct yrt_ao_params {
    int   rays;      /* K, occlusion rays per camera sample that hits a triangle; 0 -> 16; 1..64 */
    float distance;  /* tmax of an occlusion ray; > 0; +inf is taken as FLT_MAX */
    float bias;      /* tmin of an occlusion ray; finite, >= 0, < distance */
} yrt_ao_params;
void yrt_ao_params_default(yrt_ao_params* a);            /* 16, FLT_MAX, 0.01f (the shadow rays' tmin) */
int  yrt_ao_tables(float dirs[64 * 3], float rots[16 * 2]); /* the two tables above, as the kernel reads them */
int  yrt_render_ao(yrt_scene* ds, const yrt_render_params* p, const yrt_ao_params* a,
                   float* out, int mem, void* stream);
/* per shape its primitive kind: 0 triangles, 1 lines, 2 points, 3 empty; n always set; kind may be NULL */
int  yrt_host_scene_shape_kinds(const yrt_host_scene* hs, int* kind, int cap, int* n);

/* ---- camera models: thin-lens depth of field, orthographic, panorama ----
 * yrt_render traces eval_camera's pinhole rays. These two calls generate the camera rays of
 * another model on the device, and the first also shades them as ray batches (yrt_shade_rays'
 * pipeline) and box-filters the colours, so no ray and no per-ray colour crosses the host.
 * Notation: W x H the image, (i, j) the image pixel (not the window's), ns = p->samples,
 * q = jj*ns + ii, u = (i + (ii + 0.5f)/ns)/W and v = (j + (jj + 0.5f)/ns)/H as in yrt_render.
 * cam is the scene camera p->camera with its focus replaced by `focus` when that is > 0:
 * o, x, y (the frame's y * -1), z, h = 2*focus*tanf(fovy/2), w = h*aspect, focus. All
 * arithmetic is float32, left to right as written, with no contraction; every ray has
 * tmin = 1e-4f (the camera rays') and tmax = FLT_MAX; `.c` is each of x, y, z; normalize(a) is
 * a * (1 / sqrtf(a.x*a.x + a.y*a.y + a.z*a.z)), a itself at length 0.
 *   YRT_CAMERA_PERSPECTIVE, a thin lens. Q.c = o.c + (u-0.5f)*w*x.c + (v-0.5f)*h*y.c - focus*z.c
 *     is the point of the focal plane the sample looks at (eval_camera's expression). A is the
 *     lens diameter, as in Yocto: `aperture` >= 0, or the scene camera's own when `aperture` < 0.
 *     With A == 0.0f the origin is e = o: eval_camera's ray bit for bit, and the call's image is
 *     yrt_render's bit for bit. Otherwise R = A*0.5f, k = q & 63, (tx, ty) = dirs[k].xy,
 *     t = (i & 3) | ((j & 3) << 2), r = (t ^ (q >> 6)) & 15, (c, sn) = rots[r],
 *     lx = R*(c*tx - sn*ty), ly = R*(sn*tx + c*ty), e.c = (o.c + lx*x.c) + ly*y.c.
 *     The ray is {e, normalize(Q - e)}. dirs and rots are yrt_ao_tables' tables: dirs[k].xy is
 *     the Halton (2, 3) point k + 1 mapped uniformly onto the unit disk, so a pixel with
 *     ns*ns <= 64 uses the first ns*ns points under one of 16 rotations, chosen per 4 x 4 pixel
 *     tile, and beyond 64 samples the set repeats under another rotation. What lies at the
 *     distance `focus` is sharp; a point at distance d blurs over A*|d - focus|/d there.
 *   YRT_CAMERA_ORTHOGRAPHIC. e.c = o.c + (u-0.5f)*w*x.c + (v-0.5f)*h*y.c and
 *     d = normalize({-z.x, -z.y, -z.z}): the film is the w x h rectangle at the focus distance,
 *     so something at that distance has the size it has in the perspective view. The aperture is
 *     ignored.
 *   YRT_CAMERA_EQUIRECT, the 360 x 180 degree panorama. phi = (u-0.5f)*6.2831855f,
 *     th = v*3.1415927f, st = sinf(th), ct = cosf(th), sp = sinf(phi), cp = cosf(phi), a = st*sp,
 *     g = st*cp, d = normalize({(a*x.c - ct*y.c) - g*z.c}), e = o: the image centre looks along
 *     -z, the top row up, the left and right edges along +z. sinf and cosf are the device's, so a
 *     direction is reproducible on one device and within 2^-18 of the exact one per component.
 *     Aperture and focus are ignored. Pass width = 2 * resolution for pixels square in angle.
 * yrt_render_camera: `out` has yrt_render's window layout and out_stride (padding columns keep the
 * caller's bytes, local rows past the image edge are zeros); a pixel is the float32 sum of its
 * ns*ns rays' shade() colours in the order of q from +0, divided by float(ns*ns), .w = 1: the box
 * filter of yrt_shade_rays over yrt_camera_rays' records, bit for bit. An empty window writes
 * nothing and counts nothing. A host `out` makes the call synchronous; a device `out` (16-byte
 * aligned) is stream-ordered, except for the waits a reflective batch makes on its level counts.
 * Every field of `p` means what it means in yrt_render, except that YRT_ALGO_MEGAKERNEL,
 * count_work = 1 and a band interleave other than band = 1, band_stride = 1, band_offset = 0
 * return YRT_ERR_UNSUPPORTED. The rays are shaded in batches of whole pixels, chunk_pixels each
 * (0: sized to the workspace), which never changes a bit. The tile-list mode and the LDS staging
 * of the handle do not apply: a batch builds no lists and stages nothing, and
 * yrt_scene_tile_lists / yrt_scene_lds_staging report that. yrt_last_stats reports the sums over
 * the batches: camera_samples == window image pixels * ns*ns, and rays, shadow_rays,
 * shadow_rays_culled and depth_truncated as yrt_shade_rays reports them for those rays;
 * yrt_last_timings the ray generation under YRT_PHASE_PRIMARY beside the batches' level 0 and
 * the pixels' sums under YRT_PHASE_ACCUMULATE.
 * yrt_camera_rays: the rays alone, n = tile_w * tile_h * ns*ns records {o.xyz, d.xyz, tmin, tmax}
 * (32 B each, yrt_shade_rays' input) in the order (window row, window column, jj, ii), into host
 * or device memory (16-byte aligned). The window must lie inside the image, else
 * YRT_ERR_INVALID_ARG; a band interleave is YRT_ERR_UNSUPPORTED as above; ambient, max_depth and
 * algorithm are ignored, and no counter is touched.
 * Both: a null handle, p, model, out or rays, a model outside 0..2, a NaN or infinite aperture
 * or focus, chunk_pixels < 0, a bad `mem` or a bad camera index return YRT_ERR_INVALID_ARG
 * before any device call. */
enum { YRT_CAMERA_PERSPECTIVE = 0, YRT_CAMERA_ORTHOGRAPHIC = 1, YRT_CAMERA_EQUIRECT = 2 };
typedef struct yrt_camera_model {
    int   model;         /* YRT_CAMERA_* */
    float aperture;      /* lens diameter; < 0: the scene camera's; 0: pinhole */
    float focus;         /* <= 0: the scene camera's */
    int   chunk_pixels;  /* pixels per shading batch; 0: sized to the workspace; never changes a bit */
} yrt_camera_model;
void yrt_camera_model_default(yrt_camera_model* m);      /* {YRT_CAMERA_PERSPECTIVE, -1, 0, 0} */
int  yrt_render_camera(yrt_scene* ds, const yrt_render_params* p, const yrt_camera_model* m, float* out, int mem,
                       void* stream);
int  yrt_camera_rays(yrt_scene* ds, const yrt_render_params* p, const yrt_camera_model* m, float* rays, int mem,
                     void* stream);
/* camera `index` of a host scene, as yrt_host_scene_add_camera takes it: the frame {x, y, z, o},
 * fovy, aspect, aperture, focus; each pointer may be NULL. What a caller needs to override the
 * focus sensibly. A bad index is YRT_ERR_INVALID_ARG. */
int  yrt_host_scene_camera(const yrt_host_scene* hs, int index, float frame[12], float* fovy, float* aspect,
                           float* aperture, float* focus);

/* ---- soft shadows: area lights as K any-hit rays per light ----
 * shade() casts one shadow ray per (hit, light): every light is a point and every shadow edge a
 * step. These two calls give light li -- the li-th light in scene order, as in
 * yrt_host_scene_lights -- a radius R_li >= 0: `radius` for all, or light_radius[li]. A light is
 * then a disk of that radius about its point, facing the shading point, and a hit casts K = rays
 * shadow rays at it (1..64; 0 means 16). All arithmetic is float32, left to right as written,
 * with no contraction; bits(x) is the float's 32-bit pattern; dirs and rots are yrt_ao_tables'
 * tables. For a sample that hit, at any level, with hit point p, and light li:
 *   1. tp, l, r are the hard shadow ray's: tp = transform_point(lf, lp0 - p), r = |tp|, l = tp / r.
 *   2. R_li == 0.0f: the one ray {p, l, 0.01f, r - 0.01f}, the hard shadow ray bit for bit;
 *      open = K if it is unoccluded, else 0. No basis, no offset (a -0 of tp stays what it is).
 *   3. Otherwise u = bits(p.x + 0.0f) ^ bits(p.y + 0.0f) ^ bits(p.z + 0.0f); u ^= u >> 16;
 *      u ^= u >> 8; u ^= u >> 4; rot = (u ^ li) & 15; (c, sn) = rots[rot]. The rotation depends on
 *      the hit point and the light alone -- not on a pixel, a batch index or a compaction slot --
 *      so the rays have the same bits under any schedule, chunk size and level.
 *   4. The basis about l (Duff et al.): sg = l.z >= 0 ? 1 : -1, a = -1/(sg + l.z), b = l.x*l.y*a,
 *      b1 = {1 + sg*l.x*l.x*a, sg*b, -sg*l.x}, b2 = {b, sg + l.y*l.y*a, -l.y}.
 *   5. For k = 0..K-1: (tx, ty) = dirs[k].xy, x = c*tx - sn*ty, y = sn*tx + c*ty,
 *      tq = tp + (b1*x + b2*y) * R_li, rq = |tq|, lq = tq / rq, the ray {p, lq, 0.01f, rq - 0.01f},
 *      answered by intersect_any. open is the number of unoccluded rays.
 *   6. open == 0: the light is skipped, as an occluded light is in shade(). Otherwise
 *      f = float(open) / float(K) and c = c + (ld + ls) * f, ld and ls being shade()'s terms of the
 *      centre l, r, unchanged: open == K gives f == 1.0f and shade()'s bits. A light whose term is
 *      proven +-0 (the zero-term cull of yrt_render) may be answered without a walk, as open = 0.
 *   7. Everything else is shade() as yrt_shade_rays states it: the view vector from the ray's own
 *      origin, the mirror recursion, max_depth, the fold.
 * So with every radius 0 the result is yrt_shade_rays' / yrt_render's bit for bit whatever K is, a
 * pixel's value depends on its own rays alone, and the result has the same bits on every run.
 * The approximation: the light's term is taken at its centre, the disk faces the
 * shading point, and no light is sampled by solid angle.
 * yrt_shade_rays_soft is yrt_shade_rays with these shadow rays: the same records, layout, memory
 * kinds, stream order and n == 0. yrt_render_soft_shadows is yrt_render_camera with them: `m` is
 * the camera model (NULL: the pinhole, {YRT_CAMERA_PERSPECTIVE, 0, 0, 0}), so soft shadows and a
 * thin lens combine; window, out_stride, host and device memory, stream order, empty windows,
 * chunk_pixels and the refused band interleave are yrt_render_camera's. Both run in the wavefront
 * algorithms only: YRT_ALGO_MEGAKERNEL and count_work = 1 return YRT_ERR_UNSUPPORTED. The
 * tile-list mode and the LDS staging of the handle do not apply and are reported unused.
 * yrt_last_stats: a (hit sample, light) pair counts K shadow rays when R_li > 0 and 1 when
 * R_li == 0, a pair answered by the zero-term cull the same number in shadow_rays_culled; rays is
 * the closest-hit rays plus shadow_rays; camera_samples as after yrt_render_camera.
 * A null handle, p, soft params, rays or out, K outside 0..64, a negative, NaN or infinite
 * radius, nlights other than the scene's light count when light_radius is given, a bad `mem`,
 * camera or model return YRT_ERR_INVALID_ARG before any device call. */
#define YRT_SOFT_SHADOW_RAYS_MAX 64
typedef struct yrt_soft_shadow_params {
    int rays;                   /* K: 0 -> 16; 1..64 */
    float radius;               /* every light's radius when light_radius is NULL; >= 0, finite */
    const float* light_radius;  /* host memory, nlights entries, or NULL */
    int nlights;                /* the scene's light count when light_radius is given */
} yrt_soft_shadow_params;
void yrt_soft_shadow_params_default(yrt_soft_shadow_params* sp);   /* {16, 0, NULL, 0} */
int  yrt_shade_rays_soft(yrt_scene* ds, const yrt_render_params* p, const yrt_soft_shadow_params* sp,
                         const float* rays, int n, float* out_rgba, int mem, void* stream);
int  yrt_render_soft_shadows(yrt_scene* ds, const yrt_render_params* p, const yrt_camera_model* m /* NULL: pinhole */,
                             const yrt_soft_shadow_params* sp, float* out, int mem, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YRT_H */
