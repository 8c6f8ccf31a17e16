// capi.cpp -- the C-ABI of include/yrt.h over the host scene code and the gfx950
// kernels. No exceptions cross this boundary: every entry point catches and maps
// to a status code, with the message kept per thread (yrt_last_error).
#include <hip/hip_runtime_api.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/yrt.h"
#include "ao_args.h"
#include "ao_tables.h"
#include "camera_args.h"
#include "camera_models.h"
#include "matte_args.h"
#include "plane_staging.h"
#include "soft_shadow_args.h"
#include "yrt_render.h"

struct yrt_host_scene {
    yrt::scene scn;
};

struct yrt_scene {
    yrt::device_scene* ds = nullptr;
    unsigned long long* counters = nullptr;  // device, yrt::cnt_count entries
    void* scratch = nullptr;                 // device staging for host-memory calls
    size_t scratch_bytes = 0;
    hipStream_t last_stream = nullptr;
    int trace_algorithm = YRT_ALGO_WAVEFRONT;  // walks used by yrt_trace_first/any
    // yrt_render_mattes' dropped totals (device, yrt::matte_drop_slots lines), made by its first call
    unsigned long long* matte_dropped = nullptr;
};

namespace {

thread_local std::string g_last_error;

void hip_check(hipError_t e, const char* what) {
    if (e == hipErrorOutOfMemory) throw yrt::device_oom(std::string(what) + ": " + hipGetErrorString(e));
    if (e != hipSuccess) throw yrt::device_error(std::string(what) + ": " + hipGetErrorString(e));
}

// exception type -> status code (yrt_scene.h lists the mapping); the message is kept
template <class F>
int guarded(F&& f) {
    try {
        g_last_error.clear();
        return f();
    } catch (const yrt::device_oom& e) {
        g_last_error = e.what();
        return YRT_ERR_OOM;
    } catch (const yrt::device_error& e) {
        g_last_error = e.what();
        return YRT_ERR_HIP;
    } catch (const yrt::unsupported_error& e) {
        g_last_error = e.what();
        return YRT_ERR_UNSUPPORTED;
    } catch (const std::bad_alloc&) {
        g_last_error = "out of memory";
        return YRT_ERR_OOM;
    } catch (const std::invalid_argument& e) {
        g_last_error = e.what();
        return YRT_ERR_INVALID_ARG;
    } catch (const std::runtime_error& e) {
        g_last_error = e.what();
        return YRT_ERR_IO;
    } catch (...) {
        g_last_error = "internal error";
        return YRT_ERR_INTERNAL;
    }
}

// the device tonemap's level thresholds, computed once with this host's powf
const yrt::tonemap_table& tonemap_table() {
    static yrt::tonemap_table t;
    static std::once_flag once;
    std::call_once(once, [] {
        yrt::tonemap_thresholds(t.thr);
        t.neg_inf_level = yrt::tonemap_neg_inf_level();
    });
    return t;
}

void* scratch(yrt_scene* s, size_t bytes) {
    if (bytes > s->scratch_bytes) {
        if (s->scratch) hip_check(hipFree(s->scratch), "hipFree");
        s->scratch = nullptr;
        s->scratch_bytes = 0;
        hip_check(hipMalloc(&s->scratch, bytes), "hipMalloc(scratch)");
        s->scratch_bytes = bytes;
    }
    return s->scratch;
}

struct resolved_window {
    int W, H, x0, y0, tw, th;
};

resolved_window resolve(const yrt::device_scene& ds, const yrt_render_params& p) {
    if (p.resolution <= 0 || p.samples <= 0) throw std::invalid_argument("resolution and samples must be > 0");
    if (p.camera < 0 || p.camera >= (int)ds.cameras.size()) throw std::invalid_argument("camera index out of range");
    if (p.band <= 0 || p.band_stride <= 0 || p.band_offset < 0 || p.band_offset >= p.band_stride)
        throw std::invalid_argument("bad band interleave");
    const auto& cam = ds.cameras[p.camera];
    resolved_window r;
    r.W = p.width > 0 ? p.width : (int)std::round(cam.aspect * p.resolution);  // raytrace.cpp:216
    r.H = p.resolution;
    r.x0 = p.x0;
    r.y0 = p.y0;
    if (r.x0 < 0 || r.y0 < 0 || r.x0 >= r.W || r.y0 >= r.H) throw std::invalid_argument("window origin outside image");
    int rows_avail = r.H - r.y0;
    // local rows available under the band interleave
    int bands_total = (rows_avail + p.band - 1) / p.band;
    int my_bands = bands_total > p.band_offset ? (bands_total - p.band_offset + p.band_stride - 1) / p.band_stride : 0;
    r.tw = p.tile_w > 0 ? p.tile_w : r.W - r.x0;
    r.th = p.tile_h > 0 ? p.tile_h : my_bands * p.band;
    if (r.x0 + r.tw > r.W) throw std::invalid_argument("window wider than image");
    return r;
}

// the kernels' frame arguments of p and its resolved window; refuses an out_stride below the
// window's width. With `shading` the ambient and the recursion depth too: the AOV and matte
// passes, which shade nothing, leave them zero. A ray batch (yrt_shade_rays) has no camera and
// no window, r == nullptr, and takes the shading part alone.
yrt::dev_render_args frame_args(const yrt_scene* s, const yrt_render_params& p, const resolved_window* r, bool shading) {
    yrt::dev_render_args a = {};
    if (shading) {
        for (int k = 0; k < 3; k++) a.amb[k] = p.ambient[k];
        a.max_depth = p.max_depth > 0 ? p.max_depth : 16;
    }
    if (!r) return a;
    a.cam = yrt::make_dev_camera(s->ds->cameras[p.camera]);
    a.width = r->W;
    a.height = r->H;
    a.samples = p.samples;
    a.x0 = r->x0;
    a.tile_w = r->tw;
    a.y0 = r->y0;
    a.tile_h = r->th;
    a.band = p.band;
    a.band_stride = p.band_stride;
    a.band_offset = p.band_offset;
    a.out_stride = p.out_stride > 0 ? p.out_stride : r->tw;
    if (a.out_stride < r->tw) throw std::invalid_argument("out_stride smaller than the window width");
    return a;
}

void zero_counters(yrt_scene* s, hipStream_t st) {
    hip_check(hipMemsetAsync(s->counters, 0, yrt::cnt_slots * yrt::cnt_count * sizeof(unsigned long long), st),
              "hipMemsetAsync");
}

// timing 1: start a new record; 2: keep accumulating across calls (bench loops)
void start_timer(yrt_scene* s, const yrt_render_params& p) {
    if (!(p.timing == 2 && s->ds->timer.on)) s->ds->timer.reset(p.timing != 0);
}

// Host planes: device staging of their own (the handle's scratch stays yrt_render's) -- one
// block for the planes of `list`, uploaded first where the rows are padded (padding columns
// keep the caller's bytes), handed to `launch`, copied back when it succeeded, and released.
// The block is released only after the stream has drained, on every way out; the launch's
// error is reported before the drain's.
template <class Launch>
void stage_host_planes(const yrt::plane_list& list, bool padded, hipStream_t st, const char* alloc_what,
                       const char* render_what, Launch&& launch) {
    void* stage = nullptr;
    hip_check(hipMalloc(&stage, list.bytes), alloc_what);
    hipError_t e = hipSuccess;
    try {
        for (int k = 0; k < list.count && padded; k++)
            hip_check(hipMemcpyAsync(list.plane(k, stage), list.items[k].host, list.items[k].bytes, hipMemcpyHostToDevice, st),
                      "hipMemcpyAsync");
        e = launch(stage);
        for (int k = 0; k < list.count && e == hipSuccess; k++)
            e = hipMemcpyAsync(list.items[k].host, list.plane(k, stage), list.items[k].bytes, hipMemcpyDeviceToHost, st);
    } catch (...) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(stage);
        throw;
    }
    const hipError_t e2 = hipStreamSynchronize(st);
    (void)hipFree(stage);
    hip_check(e, render_what);
    hip_check(e2, "hipStreamSynchronize");
}

}  // namespace

void yrt::set_last_error(const std::string& msg) { g_last_error = msg; }

namespace {
yrt::frame3f frame_of(const float* f) {
    return {{f[0], f[1], f[2]}, {f[3], f[4], f[5]}, {f[6], f[7], f[8]}, {f[9], f[10], f[11]}};
}
// a scene edited after build_bvh needs a new build before upload
template <typename T>
int append(yrt_host_scene* hs, std::vector<T>& v, T&& item, int* index) {
    v.push_back(std::move(item));
    hs->scn.has_bvh = false;
    if (index) *index = (int)v.size() - 1;
    return YRT_OK;
}
}  // namespace

extern "C" {

int yrt_abi_version(void) { return YRT_ABI_VERSION; }

const char* yrt_status_string(int s) {
    switch (s) {
        case YRT_OK: return "ok";
        case YRT_ERR_INVALID_ARG: return "invalid argument";
        case YRT_ERR_IO: return "i/o or format error";
        case YRT_ERR_UNSUPPORTED: return "unsupported input";
        case YRT_ERR_HIP: return "HIP runtime error";
        case YRT_ERR_NO_DEVICE: return "no GPU device";
        case YRT_ERR_OOM: return "out of memory";
        case YRT_ERR_INTERNAL: return "internal error";
        default: return "unknown status";
    }
}

const char* yrt_last_error(void) { return g_last_error.c_str(); }

int yrt_device_count(int* count) {
    if (!count) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        *count = n;
        return n > 0 ? YRT_OK : YRT_ERR_NO_DEVICE;
    });
}

int yrt_scene_load(const char* path, yrt_host_scene** out) {
    if (!path || !out) return YRT_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded([&] {
        auto hs = new yrt_host_scene();
        try {
            yrt::load_scene_any(path, hs->scn);
        } catch (...) {
            delete hs;
            throw;
        }
        *out = hs;
        return YRT_OK;
    });
}

int yrt_scene_save(const yrt_host_scene* hs, const char* path) {
    if (!hs || !path) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        yrt::save_yrtscene(path, hs->scn);
        return YRT_OK;
    });
}

int yrt_host_scene_build_bvh(yrt_host_scene* hs, int equal_num) {
    if (!hs) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        yrt::build_bvh(hs->scn, equal_num != 0);
        return YRT_OK;
    });
}

int yrt_host_scene_build_bvh_gpu(yrt_host_scene* hs, int equal_num, int device, float* kernel_ms) {
    if (!hs) return YRT_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_last_error = "no HIP device visible";
        return YRT_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        yrt::build_bvh_gpu(hs->scn, equal_num != 0, device, kernel_ms);
        return YRT_OK;
    });
}

int yrt_host_scene_save_bvh(const yrt_host_scene* hs, const char* path) {
    if (!hs || !path) return YRT_ERR_INVALID_ARG;
    if (!hs->scn.has_bvh) {
        g_last_error = "scene has no BVH";
        return YRT_ERR_INVALID_ARG;
    }
    return guarded([&] {
        yrt::save_yrtbvh(path, hs->scn);
        return YRT_OK;
    });
}

int yrt_host_scene_info(const yrt_host_scene* hs, long long* info) {
    if (!hs || !info) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        const auto& s = hs->scn;
        long long lights = 0, tris = 0, lines = 0, points = 0, sdepth = 0;
        for (auto& i : s.instances) {
            if (i.mat < 0) continue;
            auto ke = s.materials[i.mat].ke;
            if (ke.x > 0 && ke.y > 0 && ke.z > 0) lights++;
        }
        for (auto& sh : s.shapes) {
            tris += sh.triangles.size();
            lines += sh.lines.size();
            points += sh.points.size();
            if (s.has_bvh) sdepth = std::max<long long>(sdepth, yrt::bvh_max_depth(sh.bvh));
        }
        long long v[12] = {(long long)s.cameras.size(), (long long)s.textures.size(),
                           (long long)s.materials.size(), (long long)s.shapes.size(),
                           (long long)s.instances.size(), lights,
                           s.has_bvh ? (long long)s.bvh.nodes.size() : 0,
                           s.has_bvh ? (long long)yrt::bvh_max_depth(s.bvh) : 0, sdepth, tris, lines, points};
        memcpy(info, v, sizeof v);
        return YRT_OK;
    });
}

int yrt_host_scene_lights(const yrt_host_scene* hs, int* inst, int cap, int* n) {
    if (!hs || !n || (inst && cap < 0)) return YRT_ERR_INVALID_ARG;
    // (the lights of device_scene_create, in its order: raytrace.cpp:126)
    int count = 0;
    const auto& s = hs->scn;
    for (size_t k = 0; k < s.instances.size(); k++) {
        if (s.instances[k].mat < 0) continue;
        const auto ke = s.materials[s.instances[k].mat].ke;
        if (!(ke.x > 0.0f && ke.y > 0.0f && ke.z > 0.0f)) continue;
        if (inst && count < cap) inst[count] = (int)k;
        count++;
    }
    *n = count;
    return YRT_OK;
}

int yrt_host_scene_instances(const yrt_host_scene* hs, int* shape, int* material, int cap, int* n) {
    if (!hs || !n || ((shape || material) && cap < 0)) return YRT_ERR_INVALID_ARG;
    const auto& s = hs->scn;
    for (size_t k = 0; k < s.instances.size() && (int)k < cap; k++) {
        if (shape) shape[k] = s.instances[k].shp;
        if (material) material[k] = s.instances[k].mat;
    }
    *n = (int)s.instances.size();
    return YRT_OK;
}

int yrt_host_scene_shape_kinds(const yrt_host_scene* hs, int* kind, int cap, int* n) {
    if (!hs || !n || (kind && cap < 0)) return YRT_ERR_INVALID_ARG;
    // (the kinds of device_scene_create: the first primitive list of a shape that is not empty)
    const auto& s = hs->scn;
    for (size_t k = 0; kind && k < s.shapes.size() && (int)k < cap; k++) {
        const auto& sh = s.shapes[k];
        kind[k] = !sh.triangles.empty() ? yrt::kind_triangles
                  : !sh.lines.empty()   ? yrt::kind_lines
                  : !sh.points.empty()  ? yrt::kind_points
                                        : yrt::kind_empty;
    }
    *n = (int)s.shapes.size();
    return YRT_OK;
}

int yrt_host_image_size(const yrt_host_scene* hs, int camera, int resolution, int* w, int* h) {
    if (!hs || !w || !h || camera < 0 || camera >= (int)hs->scn.cameras.size() || resolution <= 0)
        return YRT_ERR_INVALID_ARG;
    *w = (int)std::round(hs->scn.cameras[camera].aspect * resolution);
    *h = resolution;
    return YRT_OK;
}

int yrt_host_scene_camera(const yrt_host_scene* hs, int index, float frame[12], float* fovy, float* aspect,
                          float* aperture, float* focus) {
    if (!hs || index < 0 || index >= (int)hs->scn.cameras.size()) return YRT_ERR_INVALID_ARG;
    const yrt::camera& c = hs->scn.cameras[index];
    if (frame) {
        const yrt::vec3f v[4] = {c.frame.x, c.frame.y, c.frame.z, c.frame.o};
        for (int k = 0; k < 4; k++) frame[3 * k] = v[k].x, frame[3 * k + 1] = v[k].y, frame[3 * k + 2] = v[k].z;
    }
    if (fovy) *fovy = c.fovy;
    if (aspect) *aspect = c.aspect;
    if (aperture) *aperture = c.aperture;
    if (focus) *focus = c.focus;
    return YRT_OK;
}

void yrt_host_scene_free(yrt_host_scene* hs) { delete hs; }

int yrt_host_scene_create(yrt_host_scene** out) {
    if (!out) return YRT_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded([&] {
        *out = new yrt_host_scene();
        return YRT_OK;
    });
}


int yrt_host_scene_add_camera(yrt_host_scene* hs, const float frame[12], float fovy, float aspect, float aperture,
                              float focus, int* index) {
    if (!hs || !frame) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        yrt::camera c;
        c.frame = frame_of(frame);
        c.fovy = fovy, c.aspect = aspect, c.aperture = aperture, c.focus = focus;
        return append(hs, hs->scn.cameras, std::move(c), index);
    });
}

int yrt_host_scene_add_texture(yrt_host_scene* hs, int w, int h, const unsigned char* rgba8, int* index) {
    if (!hs || !rgba8 || w <= 0 || h <= 0) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        yrt::texture t;
        t.width = w, t.height = h;
        t.pixels.resize((size_t)w * h);
        memcpy(t.pixels.data(), rgba8, (size_t)w * h * 4);
        return append(hs, hs->scn.textures, std::move(t), index);
    });
}

int yrt_host_scene_add_material(yrt_host_scene* hs, const yrt_material_desc* d, int* index) {
    if (!hs || !d) return YRT_ERR_INVALID_ARG;
    const int nt = (int)hs->scn.textures.size();
    if (d->kd_txt < -1 || d->kd_txt >= nt || d->ks_txt < -1 || d->ks_txt >= nt) {
        g_last_error = "material texture index out of range";
        return YRT_ERR_INVALID_ARG;
    }
    return guarded([&] {
        yrt::material m;
        m.ke = {d->ke[0], d->ke[1], d->ke[2]};
        m.kd = {d->kd[0], d->kd[1], d->kd[2]};
        m.ks = {d->ks[0], d->ks[1], d->ks[2]};
        m.kr = {d->kr[0], d->kr[1], d->kr[2]};
        m.rs = d->rs;
        m.kd_txt = d->kd_txt, m.ks_txt = d->ks_txt;
        return append(hs, hs->scn.materials, std::move(m), index);
    });
}

int yrt_host_scene_add_shape(yrt_host_scene* hs, const yrt_shape_desc* d, int* index) {
    if (!hs || !d || d->npos < 0 || d->npoints < 0 || d->nlines < 0 || d->ntriangles < 0 ||
        (d->npos && !d->pos) || (d->npoints && !d->points) || (d->nlines && !d->lines) ||
        (d->ntriangles && !d->triangles))
        return YRT_ERR_INVALID_ARG;
    const int kinds = (d->npoints > 0) + (d->nlines > 0) + (d->ntriangles > 0);
    if (kinds > 1) {
        g_last_error = "shape mixes primitive types (unsupported)";
        return YRT_ERR_UNSUPPORTED;
    }
    if ((d->npoints || d->nlines) && !d->radius) {
        g_last_error = "points/lines need a radius per vertex";
        return YRT_ERR_INVALID_ARG;
    }
    auto bad = [&](const int* e, long long n) {
        for (long long k = 0; k < n; k++)
            if (e[k] < 0 || e[k] >= d->npos) return true;
        return false;
    };
    if (bad(d->points, d->npoints) || bad(d->lines, 2ll * d->nlines) || bad(d->triangles, 3ll * d->ntriangles)) {
        g_last_error = "element index outside the vertex array";
        return YRT_ERR_INVALID_ARG;
    }
    return guarded([&] {
        yrt::shape s;
        const size_t n = (size_t)d->npos;
        s.pos.resize(n);
        memcpy(s.pos.data(), d->pos, n * 12);
        if (d->norm) {
            s.norm.resize(n);
            memcpy(s.norm.data(), d->norm, n * 12);
        }
        if (d->texcoord) {
            s.texcoord.resize(n);
            memcpy(s.texcoord.data(), d->texcoord, n * 8);
        }
        if (d->radius) s.radius.assign(d->radius, d->radius + n);
        s.points.assign(d->points, d->points + d->npoints);
        s.lines.resize(d->nlines);
        if (d->nlines) memcpy(s.lines.data(), d->lines, (size_t)d->nlines * 8);
        s.triangles.resize(d->ntriangles);
        if (d->ntriangles) memcpy(s.triangles.data(), d->triangles, (size_t)d->ntriangles * 12);
        return append(hs, hs->scn.shapes, std::move(s), index);
    });
}

int yrt_host_scene_add_instance(yrt_host_scene* hs, const float frame[12], int shape, int material, int* index) {
    if (!hs || !frame || shape < 0 || shape >= (int)hs->scn.shapes.size() || material < 0 ||
        material >= (int)hs->scn.materials.size())
        return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        yrt::instance i;
        i.frame = frame_of(frame);
        i.shp = shape;
        i.mat = material;
        return append(hs, hs->scn.instances, std::move(i), index);
    });
}

int yrt_scene_upload(const yrt_host_scene* hs, int device, yrt_scene** out) {
    if (!hs || !out) return YRT_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        g_last_error = "no HIP device visible";
        return YRT_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        auto s = new yrt_scene();
        try {
            s->ds = yrt::device_scene_create(hs->scn, device);
            hip_check(hipMalloc(&s->counters, yrt::cnt_slots * yrt::cnt_count * sizeof(unsigned long long)), "hipMalloc(counters)");
            hip_check(hipMemset(s->counters, 0, yrt::cnt_slots * yrt::cnt_count * sizeof(unsigned long long)), "hipMemset");
            // hipMemset of device memory may still be running when it returns, on the null
            // stream, which a caller's non-blocking stream does not wait for: a first render
            // on such a stream would race it (seen: a fresh handle's first frame lost part of
            // k_primary's counts)
            hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
        } catch (...) {
            yrt_scene_free(s);
            throw;
        }
        *out = s;
        return YRT_OK;
    });
}

int yrt_scene_set_trace_algorithm(yrt_scene* s, int algorithm) {
    if (!s || algorithm < YRT_ALGO_WAVEFRONT || algorithm > YRT_ALGO_WAVEFRONT_LANE) return YRT_ERR_INVALID_ARG;
    s->trace_algorithm = algorithm;
    return YRT_OK;
}

int yrt_scene_set_tile_lists(yrt_scene* s, int mode) {
    if (!s || mode < YRT_LISTS_AUTO || mode > YRT_LISTS_OFF) return YRT_ERR_INVALID_ARG;
    s->ds->lists_mode = mode;
    return YRT_OK;
}

int yrt_scene_tile_lists(yrt_scene* s, int* camera_on, int* bundles_on, unsigned long long* sums) {
    if (!s) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        yrt::device_scene& ds = *s->ds;
        hip_check(hipSetDevice(ds.device), "hipSetDevice");
        if (ds.list_stats_ev && ds.list_stats_recorded) hip_check(hipEventSynchronize(ds.list_stats_ev), "list sums");
        if (camera_on) *camera_on = ds.last_camera_lists;
        if (bundles_on) *bundles_on = ds.last_bundles;
        if (sums)
            for (int i = 0; i < 4; i++) sums[i] = ds.list_stats_host ? ds.list_stats_host[i] : 0;
        return YRT_OK;
    });
}

int yrt_scene_tile_list_masks(yrt_scene* s, unsigned long long* excluded) {
    if (!s || !excluded) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        yrt::device_scene& ds = *s->ds;
        hip_check(hipSetDevice(ds.device), "hipSetDevice");
        if (ds.list_stats_ev && ds.list_stats_recorded) hip_check(hipEventSynchronize(ds.list_stats_ev), "list sums");
        for (int i = 0; i < 2; i++) excluded[i] = ds.list_stats_host ? ds.list_stats_host[4 + i] : 0;
        return YRT_OK;
    });
}

int yrt_scene_set_lds_staging(yrt_scene* s, int on) {
    if (!s || (on != 0 && on != 1)) return YRT_ERR_INVALID_ARG;
    s->ds->lds_staging = on;
    return YRT_OK;
}

int yrt_scene_lds_staging(yrt_scene* s, int* staged) {
    if (!s || !staged) return YRT_ERR_INVALID_ARG;
    *staged = s->ds->last_lds_staging;
    return YRT_OK;
}

size_t yrt_scene_device_bytes(const yrt_scene* s) { return s && s->ds ? s->ds->arena_bytes : 0; }

void yrt_scene_free(yrt_scene* s) {
    if (!s) return;
    if (s->ds) (void)hipSetDevice(s->ds->device);
    if (s->counters) (void)hipFree(s->counters);
    if (s->scratch) (void)hipFree(s->scratch);
    if (s->matte_dropped) (void)hipFree(s->matte_dropped);
    yrt::device_scene_destroy(s->ds);
    delete s;
}

void yrt_render_params_default(yrt_render_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->ambient[0] = p->ambient[1] = p->ambient[2] = 0.1f;  // main(): -a default 0.1
    p->resolution = 720;                                    // -r default 720
    p->samples = 1;                                         // -s default 1
    p->max_depth = 16;
    p->band = 1;
    p->band_stride = 1;
}

int yrt_image_size(const yrt_scene* s, const yrt_render_params* p, int* w, int* h) {
    if (!s || !p || !w || !h) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        auto r = resolve(*s->ds, *p);
        *w = r.W;
        *h = r.H;
        return YRT_OK;
    });
}

int yrt_render(yrt_scene* s, const yrt_render_params* p, float* out, int mem, void* stream) {
    if (!s || !p || !out) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        auto r = resolve(*s->ds, *p);
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        const yrt::dev_render_args a = frame_args(s, *p, &r, true);
        size_t bytes = (size_t)a.out_stride * r.th * 4 * sizeof(float);
        void* dst = mem == YRT_MEM_DEVICE ? (void*)out : scratch(s, bytes);
        // (the wavefront algorithms zero the counter lines in their first kernel, k_chunk_setup)
        if (p->algorithm == YRT_ALGO_MEGAKERNEL) zero_counters(s, st);
        start_timer(s, *p);
        if (p->algorithm == YRT_ALGO_MEGAKERNEL && s->ds->reflective && a.max_depth > yrt::megakernel_max_depth)
            throw yrt::unsupported_error("the megakernel keeps " + std::to_string(yrt::megakernel_max_depth) +
                                         " mirror levels per lane; deeper recursions need the wavefront algorithm");
        if (p->algorithm == YRT_ALGO_MEGAKERNEL)
            hip_check(yrt::launch_render(*s->ds, a, dst, s->counters, p->count_work != 0, st), "render kernel launch");
        else if (p->algorithm == YRT_ALGO_WAVEFRONT || p->algorithm == YRT_ALGO_WAVEFRONT_LANE)
            hip_check(yrt::launch_render_wavefront(*s->ds, a, dst, s->counters, p->count_work != 0,
                                                   p->algorithm == YRT_ALGO_WAVEFRONT, st),
                      "wavefront render launch");
        else
            throw std::invalid_argument("unknown algorithm");
        s->last_stream = st;
        if (mem != YRT_MEM_DEVICE) {
            hip_check(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
            hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
        }
        return YRT_OK;
    });
}

static_assert(YRT_AOV_COUNT == yrt::aov_count && YRT_AOV_DEPTH == yrt::aov_depth &&
                  YRT_AOV_POSITION == yrt::aov_position && YRT_AOV_NORMAL == yrt::aov_normal &&
                  YRT_AOV_TEXCOORD == yrt::aov_texcoord && YRT_AOV_ALBEDO == yrt::aov_albedo &&
                  YRT_AOV_IDS == yrt::aov_ids,
              "the kernel's plane order is the header's");

int yrt_render_aovs(yrt_scene* s, const yrt_render_params* p, unsigned mask, const yrt_aov_planes* out, int mem,
                    void* stream) {
    if (!s || !p || !out) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        if (mask == 0 || mask >> YRT_AOV_COUNT) throw std::invalid_argument("aov mask must name one to all of YRT_AOV_*");
        for (int k = 0; k < YRT_AOV_COUNT; k++)
            if ((mask >> k & 1) && !out->plane[k]) throw std::invalid_argument("a requested aov's plane is null");
        auto r = resolve(*s->ds, *p);
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        const yrt::dev_render_args a = frame_args(s, *p, &r, false);
        // the counters are zeroed whatever the window: an empty one (a band offset without
        // bands) launches nothing, and yrt_last_stats must not then report the call before
        zero_counters(s, st);
        s->last_stream = st;
        if (r.tw <= 0 || r.th <= 0) return YRT_OK;
        const yrt::plane_list list = yrt::aov_plane_list(mask, *out, (size_t)a.out_stride * r.th * 16);
        auto launch = [&](void* staging) {
            yrt::dev_aov_planes dp = {};
            for (int k = 0; k < list.count; k++) dp.plane[list.items[k].slot] = list.plane(k, staging);
            return yrt::launch_aovs(*s->ds, a, mask, dp, s->counters, st);
        };
        if (mem == YRT_MEM_DEVICE)
            hip_check(launch(nullptr), "aov kernel launch");
        else
            stage_host_planes(list, a.out_stride > r.tw, st, "hipMalloc(aov staging)", "aov render", launch);
        return YRT_OK;
    });
}

static_assert(YRT_MATTE_KEY_COUNT == yrt::matte_key_count && YRT_MATTE_INSTANCE == yrt::matte_instance &&
                  YRT_MATTE_MATERIAL == yrt::matte_material && YRT_MATTE_SHAPE == yrt::matte_shape &&
                  YRT_MATTE_LAYERS_MAX == yrt::matte_layers_max,
              "the kernel's key order and layer count are the header's");

int yrt_render_mattes(yrt_scene* s, const yrt_render_params* p, unsigned key_mask, int layers,
                      const yrt_matte_planes* out, int mem, void* stream) {
    if (!s || !p || !out) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        if (const char* bad = yrt::matte_args_error(key_mask, layers, out, mem)) throw std::invalid_argument(bad);
        auto r = resolve(*s->ds, *p);
        const yrt::dev_render_args a = frame_args(s, *p, &r, false);  // (its refusal comes before any device call)
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        const size_t drop_bytes = (size_t)yrt::matte_drop_slots * yrt::matte_drop_stride * sizeof(unsigned long long);
        if (!s->matte_dropped) hip_check(hipMalloc(&s->matte_dropped, drop_bytes), "hipMalloc(matte dropped totals)");
        // the counters and the dropped totals are zeroed whatever the window: an empty one (a
        // band offset without bands) launches nothing, and must not report the call before
        zero_counters(s, st);
        hip_check(hipMemsetAsync(s->matte_dropped, 0, drop_bytes, st), "hipMemsetAsync");
        s->last_stream = st;
        if (r.tw <= 0 || r.th <= 0) return YRT_OK;
        const yrt::plane_list list = yrt::matte_plane_list(key_mask, layers, *out, (size_t)a.out_stride * r.th * 16);
        auto launch = [&](void* staging) {
            yrt::dev_matte_planes dp = {};
            for (int k = 0; k < list.count; k++) {
                const int slot = list.items[k].slot;  // 4 key + 2 layer + coverage
                (slot & 1 ? dp.coverage : dp.ids)[slot >> 2][slot >> 1 & 1] = list.plane(k, staging);
            }
            return yrt::launch_mattes(*s->ds, a, key_mask, layers, dp, s->matte_dropped, s->counters, st);
        };
        if (mem == YRT_MEM_DEVICE)
            hip_check(launch(nullptr), "matte kernel launch");
        else
            stage_host_planes(list, a.out_stride > r.tw, st, "hipMalloc(matte staging)", "matte render", launch);
        return YRT_OK;
    });
}

int yrt_scene_matte_dropped(yrt_scene* s, unsigned long long* dropped) {
    if (!s || !dropped) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++) dropped[k] = 0;
        if (!s->matte_dropped) return YRT_OK;  // no matte pass on this handle yet
        std::vector<unsigned long long> lines((size_t)yrt::matte_drop_slots * yrt::matte_drop_stride);
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        hip_check(hipStreamSynchronize(s->last_stream), "hipStreamSynchronize");
        hip_check(hipMemcpy(lines.data(), s->matte_dropped, lines.size() * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost),
                  "hipMemcpy(matte dropped totals)");
        for (int l = 0; l < yrt::matte_drop_slots; l++)
            for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++) dropped[k] += lines[(size_t)l * yrt::matte_drop_stride + k];
        return YRT_OK;
    });
}

static_assert(YRT_PASS_COUNT == yrt::pass_count && YRT_PASS_DIRECT == yrt::pass_direct &&
                  YRT_PASS_DIFFUSE == yrt::pass_diffuse && YRT_PASS_SPECULAR == yrt::pass_specular &&
                  YRT_PASS_REFLECTION == yrt::pass_reflection && YRT_PASS_AMBIENT == yrt::pass_ambient,
              "the kernel's plane order is the header's");

int yrt_render_passes(yrt_scene* s, const yrt_render_params* p, unsigned mask, const yrt_pass_planes* out, float* beauty,
                      int mem, void* stream) {
    if (!s || !p || !out) return YRT_ERR_INVALID_ARG;
    if (mask == 0 || mask >> YRT_PASS_COUNT) {
        g_last_error = "pass mask must name one to all of YRT_PASS_*";
        return YRT_ERR_INVALID_ARG;
    }
    for (int k = 0; k < YRT_PASS_COUNT; k++)
        if ((mask >> k & 1) && !out->plane[k]) {
            g_last_error = "a requested pass's plane is null";
            return YRT_ERR_INVALID_ARG;
        }
    return guarded([&] {
        if (p->algorithm == YRT_ALGO_MEGAKERNEL)
            throw yrt::unsupported_error("the shading passes run in the wavefront algorithms");
        if (p->algorithm != YRT_ALGO_WAVEFRONT && p->algorithm != YRT_ALGO_WAVEFRONT_LANE)
            throw std::invalid_argument("unknown algorithm");
        if (p->count_work != 0) throw yrt::unsupported_error("the shading passes do not count work");
        auto r = resolve(*s->ds, *p);
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        const yrt::dev_render_args a = frame_args(s, *p, &r, true);
        start_timer(s, *p);
        s->last_stream = st;
        const yrt::plane_list list = yrt::pass_plane_list(mask, *out, beauty, (size_t)a.out_stride * r.th * 16);
        auto launch = [&](void* staging) {
            yrt::dev_pass_planes dp = {};
            float* planes[YRT_PASS_COUNT + 1] = {};  // the passes, then the beauty
            for (int k = 0; k < list.count; k++) planes[list.items[k].slot] = (float*)list.plane(k, staging);
            for (int k = 0; k < YRT_PASS_COUNT; k++) dp.plane[k] = planes[k];
            return yrt::launch_render_wavefront_passes(*s->ds, a, mask, dp, planes[YRT_PASS_COUNT], s->counters,
                                                       p->algorithm == YRT_ALGO_WAVEFRONT, st);
        };
        // (an empty window launches nothing but the counters' memset: the planes are not touched)
        if (mem == YRT_MEM_DEVICE || r.tw <= 0 || r.th <= 0)
            hip_check(launch(nullptr), "passes render launch");
        else
            stage_host_planes(list, a.out_stride > r.tw, st, "hipMalloc(pass staging)", "passes render", launch);
        return YRT_OK;
    });
}

static_assert(YRT_LIGHT_GROUPS_MAX == yrt::light_groups_max, "the kernel's plane count is the header's");

int yrt_render_light_groups(yrt_scene* s, const yrt_render_params* p, const int* group_of, int nlights, int ngroups,
                            const yrt_light_group_planes* out, int mem, void* stream) {
    if (!s || !p || !group_of || !out) return YRT_ERR_INVALID_ARG;
    auto refuse = [](const char* why) {
        g_last_error = why;
        return YRT_ERR_INVALID_ARG;
    };
    if (ngroups < 1 || ngroups > YRT_LIGHT_GROUPS_MAX) return refuse("light groups: ngroups must be 1 to YRT_LIGHT_GROUPS_MAX");
    if (nlights < 0) return refuse("light groups: nlights is negative");
    for (int k = 0; k < nlights; k++)
        if (group_of[k] < -1 || group_of[k] >= ngroups) return refuse("light groups: a group_of entry is outside [-1, ngroups)");
    for (int g = 0; g < ngroups; g++)
        if (!out->group[g]) return refuse("light groups: a group's plane is null");
    if (mem != YRT_MEM_HOST && mem != YRT_MEM_DEVICE) return refuse("light groups: mem is YRT_MEM_HOST or YRT_MEM_DEVICE");
    if (!s->ds || nlights != s->ds->nlights) return refuse("light groups: nlights is not the scene's light count");
    return guarded([&] {
        if (p->algorithm == YRT_ALGO_MEGAKERNEL) throw yrt::unsupported_error("light groups run in the wavefront algorithms");
        if (p->algorithm != YRT_ALGO_WAVEFRONT && p->algorithm != YRT_ALGO_WAVEFRONT_LANE)
            throw std::invalid_argument("unknown algorithm");
        if (p->count_work != 0) throw yrt::unsupported_error("light groups do not count work");
        auto r = resolve(*s->ds, *p);
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        const yrt::dev_render_args a = frame_args(s, *p, &r, true);
        start_timer(s, *p);
        s->last_stream = st;
        const yrt::plane_list list = yrt::light_group_plane_list(ngroups, *out, (size_t)a.out_stride * r.th * 16);
        auto launch = [&](void* staging) {
            float* planes[YRT_LIGHT_GROUPS_MAX + 2] = {};  // the groups, the ambient, the beauty
            for (int k = 0; k < list.count; k++) planes[list.items[k].slot] = (float*)list.plane(k, staging);
            yrt::dev_light_group_planes dp = {};
            for (int g = 0; g < YRT_LIGHT_GROUPS_MAX; g++) dp.group[g] = planes[g];
            dp.ambient = planes[YRT_LIGHT_GROUPS_MAX], dp.beauty = planes[YRT_LIGHT_GROUPS_MAX + 1];
            return yrt::launch_render_wavefront_light_groups(*s->ds, a, group_of, ngroups, dp, s->counters,
                                                             p->algorithm == YRT_ALGO_WAVEFRONT, st);
        };
        // (an empty window launches nothing but the counters' memset: the planes are not touched)
        if (mem == YRT_MEM_DEVICE || r.tw <= 0 || r.th <= 0)
            hip_check(launch(nullptr), "light groups render launch");
        else
            stage_host_planes(list, a.out_stride > r.tw, st, "hipMalloc(light group staging)", "light groups render",
                              launch);
        return YRT_OK;
    });
}

static int trace_impl(yrt_scene* s, const float* rays, int n, int any, unsigned char* hit, int* inst, int* ei,
                      float* ew, float* dist, int mem, void* stream) {
    if (!s || n < 0 || (n && (!rays || !hit))) return YRT_ERR_INVALID_ARG;
    if (!any && n && (!inst || !ei || !ew || !dist)) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        zero_counters(s, st);
        s->last_stream = st;
        if (n == 0) return YRT_OK;
        if (mem == YRT_MEM_DEVICE) {
            hip_check(yrt::launch_trace(*s->ds, rays, n, any, hit, inst, ei, ew, dist, s->counters,
                                              s->trace_algorithm == YRT_ALGO_WAVEFRONT, st), "trace launch");
            return YRT_OK;
        }
        size_t rb = (size_t)n * 8 * 4, hb = ((size_t)n + 255) & ~(size_t)255, ib = (size_t)n * 4, eb = (size_t)n * 16;
        char* base = (char*)scratch(s, rb + hb + 3 * ib + eb + 1024);
        float* d_rays = (float*)base;
        unsigned char* d_hit = (unsigned char*)(base + rb);
        int* d_inst = (int*)(base + rb + hb);
        int* d_ei = (int*)(base + rb + hb + ib);
        float* d_dist = (float*)(base + rb + hb + 2 * ib);
        float* d_ew = (float*)(base + rb + hb + 3 * ib);
        hip_check(hipMemcpyAsync(d_rays, rays, rb, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
        hip_check(yrt::launch_trace(*s->ds, d_rays, n, any, d_hit, d_inst, d_ei, d_ew, d_dist, s->counters,
                                    s->trace_algorithm == YRT_ALGO_WAVEFRONT, st),
                  "trace launch");
        hip_check(hipMemcpyAsync(hit, d_hit, n, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
        if (!any) {
            hip_check(hipMemcpyAsync(inst, d_inst, ib, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
            hip_check(hipMemcpyAsync(ei, d_ei, ib, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
            hip_check(hipMemcpyAsync(dist, d_dist, ib, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
            hip_check(hipMemcpyAsync(ew, d_ew, eb, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
        }
        hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
        return YRT_OK;
    });
}

int yrt_trace_first(yrt_scene* s, const float* rays, int n, unsigned char* hit, int* inst, int* ei, float* ew,
                    float* dist, int mem, void* stream) {
    return trace_impl(s, rays, n, 0, hit, inst, ei, ew, dist, mem, stream);
}

int yrt_trace_any(yrt_scene* s, const float* rays, int n, unsigned char* hit, int mem, void* stream) {
    return trace_impl(s, rays, n, 1, hit, nullptr, nullptr, nullptr, nullptr, mem, stream);
}

// yrt_shade_rays and, with soft parameters, yrt_shade_rays_soft; a refusal's message starts with
// the name of the entry point that was called
static int shade_rays_impl(yrt_scene* s, const yrt_render_params* p, const yrt_soft_shadow_params* sp, const float* rays,
                           int n, float* out, int mem, void* stream) {
    const char* const entry = sp ? "yrt_shade_rays_soft" : "yrt_shade_rays";
    // (before any device call, and before the handle is looked at)
    const char* bad = n < 0                                      ? ": rays: n < 0"
                      : mem != YRT_MEM_HOST && mem != YRT_MEM_DEVICE ? ": rays: mem is not YRT_MEM_*"
                      : n > 0 && !s                              ? ": rays: null scene handle"
                      : n > 0 && !p                              ? ": rays: null params"
                      : n > 0 && !rays                           ? ": rays: null rays"
                      : n > 0 && !out                            ? ": rays: null out"
                                                                 : nullptr;
    if (!bad && n > 0) {
        const char *r0 = (const char*)rays, *o0 = (const char*)out;
        if (r0 < o0 + (size_t)n * 16 && o0 < r0 + (size_t)n * 32) bad = ": out overlaps rays";
        if (mem == YRT_MEM_DEVICE && ((uintptr_t)out & 15)) bad = ": rays: a device out is 16-byte aligned";
    }
    if (bad) {
        g_last_error = std::string(entry) + bad;
        return YRT_ERR_INVALID_ARG;
    }
    if (!s) return YRT_OK;  // (n == 0 without a handle: nothing to do)
    return guarded([&] {
        if (sp) {
            if (const char* lights = yrt::soft_shadow_lights_error(*sp, s->ds->nlights)) throw std::invalid_argument(lights);
        }
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        if (n == 0) {  // nothing is written; the counters read zero
            zero_counters(s, st);
            s->ds->timer.reset(false);
            s->last_stream = st;
            return YRT_OK;
        }
        if (p->algorithm != YRT_ALGO_MEGAKERNEL && p->algorithm != YRT_ALGO_WAVEFRONT &&
            p->algorithm != YRT_ALGO_WAVEFRONT_LANE)
            throw std::invalid_argument("unknown algorithm");
        if (p->count_work != 0) throw yrt::unsupported_error("ray batches do not count work");
        if (sp && p->algorithm == YRT_ALGO_MEGAKERNEL)
            throw yrt::unsupported_error("soft shadows run in the wavefront algorithms");
        yrt::dev_render_args a = frame_args(s, *p, nullptr, true);
        a.samples = 1;
        if (p->algorithm == YRT_ALGO_MEGAKERNEL && s->ds->reflective && a.max_depth > yrt::megakernel_max_depth)
            throw yrt::unsupported_error("the megakernel keeps " + std::to_string(yrt::megakernel_max_depth) +
                                         " mirror levels per lane; deeper recursions need the wavefront algorithm");
        const size_t rb = (size_t)n * 32, ob = (size_t)n * 16;
        const float* d_rays = rays;
        void* d_out = out;
        if (mem != YRT_MEM_DEVICE) {  // a host batch is staged once
            char* base = (char*)scratch(s, ((rb + 255) & ~(size_t)255) + ob);
            hip_check(hipMemcpyAsync(base, rays, rb, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
            d_rays = (const float*)base;
            d_out = base + ((rb + 255) & ~(size_t)255);
        }
        start_timer(s, *p);
        s->last_stream = st;
        if (p->algorithm == YRT_ALGO_MEGAKERNEL) {
            zero_counters(s, st);
            hip_check(yrt::launch_shade_rays(*s->ds, a, d_rays, n, d_out, s->counters, st), "shade_rays launch");
        } else {
            yrt::soft_shadow_args soft = {};
            if (sp) {
                hip_check(yrt::upload_soft_shadow_radii(*s->ds, sp->light_radius, sp->radius, st), "soft shadow radii");
                soft = {yrt::soft_shadow_rays_of(*sp), s->ds->soft_radius};
            }
            hip_check(yrt::launch_shade_rays_wavefront(*s->ds, a, d_rays, n, d_out, s->counters,
                                                       p->algorithm == YRT_ALGO_WAVEFRONT, st, sp ? &soft : nullptr),
                      "wavefront shade_rays launch");
        }
        if (mem != YRT_MEM_DEVICE) {
            hip_check(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
            hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
        }
        return YRT_OK;
    });
}

int yrt_shade_rays(yrt_scene* s, const yrt_render_params* p, const float* rays, int n, float* out, int mem,
                   void* stream) {
    return shade_rays_impl(s, p, nullptr, rays, n, out, mem, stream);
}

void yrt_soft_shadow_params_default(yrt_soft_shadow_params* sp) {
    if (!sp) return;
    sp->rays = yrt::soft_shadow_rays_default;
    sp->radius = 0.0f;
    sp->light_radius = nullptr;
    sp->nlights = 0;
}

static_assert(YRT_SOFT_SHADOW_RAYS_MAX == yrt::soft_shadow_rays_max && YRT_SOFT_SHADOW_RAYS_MAX == yrt::ao_dir_count,
              "a ray per entry of the table");

int yrt_shade_rays_soft(yrt_scene* s, const yrt_render_params* p, const yrt_soft_shadow_params* sp, const float* rays,
                        int n, float* out, int mem, void* stream) {
    // (before any device call, and before the handle is looked at; with n == 0 too)
    const char* bad = !s ? "soft shadows: null scene handle" : !p ? "soft shadows: null params" : yrt::soft_shadow_params_error(sp);
    if (bad) {
        g_last_error = std::string(bad) + " (yrt_shade_rays_soft)";
        return YRT_ERR_INVALID_ARG;
    }
    return shade_rays_impl(s, p, sp, rays, n, out, mem, stream);
}

int yrt_render_adaptive(yrt_scene* s, const yrt_render_params* p, const yrt_adaptive_params* ap, float* out,
                        unsigned char* refined, int mem, void* stream) {
    // (before any device call, and before the handle is looked at)
    const int b = ap && ap->base_samples == 0 ? 1 : ap ? ap->base_samples : 0;
    const char* bad = !s                                           ? "yrt_render_adaptive: null scene handle"
                      : !p                                         ? "yrt_render_adaptive: null params"
                      : !ap                                        ? "yrt_render_adaptive: null adaptive params"
                      : !out                                       ? "yrt_render_adaptive: null out"
                      : std::isnan(ap->threshold)                  ? "yrt_render_adaptive: the threshold is NaN"
                      : b < 1 || b > p->samples                    ? "yrt_render_adaptive: base_samples outside [1, samples]"
                      : ap->chunk_pixels < 0                       ? "yrt_render_adaptive: chunk_pixels < 0"
                      : mem != YRT_MEM_HOST && mem != YRT_MEM_DEVICE ? "yrt_render_adaptive: mem is not YRT_MEM_*"
                      : p->camera < 0                              ? "yrt_render_adaptive: camera index out of range"
                                                                   : nullptr;
    if (bad) {
        g_last_error = bad;
        return YRT_ERR_INVALID_ARG;
    }
    return guarded([&] {
        auto r = resolve(*s->ds, *p);
        const yrt::dev_render_args a = frame_args(s, *p, &r, true);  // (its refusal comes before any device call)
        if (p->algorithm == YRT_ALGO_MEGAKERNEL)
            throw yrt::unsupported_error("adaptive supersampling runs in the wavefront algorithms");
        if (p->algorithm != YRT_ALGO_WAVEFRONT && p->algorithm != YRT_ALGO_WAVEFRONT_LANE)
            throw std::invalid_argument("unknown algorithm");
        if (p->count_work != 0) throw yrt::unsupported_error("adaptive supersampling does not count work");
        if (p->band != 1 || p->band_stride != 1 || p->band_offset != 0)
            throw yrt::unsupported_error("adaptive supersampling takes contiguous rows: its apron has no band interleave");
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        start_timer(s, *p);
        s->last_stream = st;
        const yrt::plane_list list = yrt::adaptive_plane_list(out, refined, (size_t)a.out_stride * r.th);
        auto launch = [&](void* staging) {
            return yrt::launch_render_adaptive(*s->ds, a, b, ap->threshold, ap->chunk_pixels, list.plane(0, staging),
                                               refined ? (unsigned char*)list.plane(1, staging) : nullptr, s->counters,
                                               p->algorithm == YRT_ALGO_WAVEFRONT, st);
        };
        // (an empty window launches nothing but the counters' memset: the planes are not touched)
        if (mem == YRT_MEM_DEVICE || r.tw <= 0 || r.th <= 0)
            hip_check(launch(nullptr), "adaptive render launch");
        else
            stage_host_planes(list, a.out_stride > r.tw, st, "hipMalloc(adaptive staging)", "adaptive render", launch);
        return YRT_OK;
    });
}

void yrt_ao_params_default(yrt_ao_params* a) {
    if (!a) return;
    a->rays = yrt::ao_rays_default;
    a->distance = FLT_MAX;
    a->bias = 0.01f;
}

static_assert(YRT_AO_RAYS_MAX == yrt::ao_dir_count, "a ray per direction of the table");

int yrt_ao_tables(float dirs[64 * 3], float rots[16 * 2]) {
    if (!dirs || !rots) return YRT_ERR_INVALID_ARG;
    static const float d[yrt::ao_dir_count * 3] = {YRT_AO_DIRS};
    static const float r[yrt::ao_rot_count * 2] = {YRT_AO_ROTS};
    memcpy(dirs, d, sizeof d);
    memcpy(rots, r, sizeof r);
    return YRT_OK;
}

int yrt_render_ao(yrt_scene* s, const yrt_render_params* p, const yrt_ao_params* ap, float* out, int mem,
                  void* stream) {
    // (before any device call, and before the handle is looked at)
    const char* bad = !s                 ? "yrt_render_ao: null scene handle"
                      : !p               ? "yrt_render_ao: null params"
                      : p->camera < 0    ? "yrt_render_ao: camera index out of range"
                                         : yrt::ao_args_error(ap, out, mem);
    if (bad) {
        g_last_error = bad;
        return YRT_ERR_INVALID_ARG;
    }
    return guarded([&] {
        const yrt::ao_resolved ao = yrt::ao_resolve(*ap);
        auto r = resolve(*s->ds, *p);
        const yrt::dev_render_args a = frame_args(s, *p, &r, false);  // (its refusal comes before any device call)
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        // the counters are zeroed whatever the window: an empty one (a band offset without
        // bands) launches nothing, and yrt_last_stats must not then report the call before
        zero_counters(s, st);
        s->last_stream = st;
        if (r.tw <= 0 || r.th <= 0) return YRT_OK;
        const yrt::plane_list list = yrt::ao_plane_list(out, (size_t)a.out_stride * r.th * 16);
        auto launch = [&](void* staging) {
            return yrt::launch_ao(*s->ds, a, ao.rays, ao.bias, ao.distance, list.plane(0, staging), s->counters, st);
        };
        if (mem == YRT_MEM_DEVICE)
            hip_check(launch(nullptr), "ao kernel launch");
        else
            stage_host_planes(list, a.out_stride > r.tw, st, "hipMalloc(ao staging)", "ao render", launch);
        return YRT_OK;
    });
}

void yrt_camera_model_default(yrt_camera_model* m) {
    if (!m) return;
    m->model = YRT_CAMERA_PERSPECTIVE;
    m->aperture = -1.0f;
    m->focus = 0.0f;
    m->chunk_pixels = 0;
}

static_assert(YRT_CAMERA_PERSPECTIVE == yrt::camera_perspective && YRT_CAMERA_ORTHOGRAPHIC == yrt::camera_orthographic &&
                  YRT_CAMERA_EQUIRECT == yrt::camera_equirect,
              "the kernel's models are the header's");

namespace {
// what yrt_render_camera and yrt_camera_rays refuse before the handle is looked at
const char* camera_call_error(const yrt_scene* s, const yrt_render_params* p, const yrt_camera_model* m, const float* out,
                              int mem) {
    return !s              ? "camera: null scene handle"
           : !p            ? "camera: null params"
           : p->camera < 0 ? "camera: camera index out of range"
                           : yrt::camera_args_error(m, out, mem);
}

// the call's frame: frame_args with the scene camera's focus replaced by the model's, and the
// resolved model; refuses a band interleave
yrt::dev_render_args camera_frame_args(const yrt_scene* s, const yrt_render_params& p, const resolved_window& r,
                                       const yrt_camera_model& m, bool shading, yrt::camera_resolved& cm) {
    yrt::dev_render_args a = frame_args(s, p, &r, shading);
    yrt::camera c = s->ds->cameras[p.camera];
    cm = yrt::camera_resolve(m, c.aperture, c.focus);
    c.focus = cm.focus;
    a.cam = yrt::make_dev_camera(c);
    if (p.band != 1 || p.band_stride != 1 || p.band_offset != 0)
        throw yrt::unsupported_error("camera models take contiguous rows: no band interleave");
    return a;
}
}  // namespace

// yrt_render_camera and, with soft parameters, yrt_render_soft_shadows
static int render_camera_impl(yrt_scene* s, const yrt_render_params* p, const yrt_camera_model* m,
                              const yrt_soft_shadow_params* sp, float* out, int mem, void* stream) {
    // (before any device call, and before the handle is looked at)
    if (const char* bad = camera_call_error(s, p, m, out, mem)) {
        g_last_error = bad;
        return YRT_ERR_INVALID_ARG;
    }
    return guarded([&] {
        if (sp) {
            if (const char* lights = yrt::soft_shadow_lights_error(*sp, s->ds->nlights)) throw std::invalid_argument(lights);
        }
        auto r = resolve(*s->ds, *p);
        yrt::camera_resolved cm;
        const yrt::dev_render_args a = camera_frame_args(s, *p, r, *m, true, cm);  // (refusals before any device call)
        if (p->algorithm == YRT_ALGO_MEGAKERNEL) throw yrt::unsupported_error("camera models run in the wavefront algorithms");
        if (p->algorithm != YRT_ALGO_WAVEFRONT && p->algorithm != YRT_ALGO_WAVEFRONT_LANE)
            throw std::invalid_argument("unknown algorithm");
        if (p->count_work != 0) throw yrt::unsupported_error("camera models do not count work");
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        start_timer(s, *p);
        s->last_stream = st;
        const yrt::plane_list list = yrt::ao_plane_list(out, (size_t)a.out_stride * r.th * 16);
        auto launch = [&](void* staging) {
            if (!sp)
                return yrt::launch_render_camera(*s->ds, a, cm.model, cm.aperture, m->chunk_pixels,
                                                 list.plane(0, staging), s->counters, p->algorithm == YRT_ALGO_WAVEFRONT, st);
            if (hipError_t e = yrt::upload_soft_shadow_radii(*s->ds, sp->light_radius, sp->radius, st); e != hipSuccess)
                return e;
            const yrt::soft_shadow_args soft = {yrt::soft_shadow_rays_of(*sp), s->ds->soft_radius};
            return yrt::launch_render_soft_shadows(*s->ds, a, cm.model, cm.aperture, m->chunk_pixels, soft,
                                                   list.plane(0, staging), s->counters,
                                                   p->algorithm == YRT_ALGO_WAVEFRONT, st);
        };
        // (an empty window launches nothing but the counters' memset: the plane is not touched)
        if (mem == YRT_MEM_DEVICE || r.tw <= 0 || r.th <= 0)
            hip_check(launch(nullptr), "camera render launch");
        else
            stage_host_planes(list, a.out_stride > r.tw, st, "hipMalloc(camera staging)", "camera render", launch);
        return YRT_OK;
    });
}

int yrt_render_camera(yrt_scene* s, const yrt_render_params* p, const yrt_camera_model* m, float* out, int mem,
                      void* stream) {
    return render_camera_impl(s, p, m, nullptr, out, mem, stream);
}

int yrt_render_soft_shadows(yrt_scene* s, const yrt_render_params* p, const yrt_camera_model* m,
                            const yrt_soft_shadow_params* sp, float* out, int mem, void* stream) {
    // (before any device call, and before the handle is looked at)
    if (const char* bad = yrt::soft_shadow_params_error(sp)) {
        g_last_error = std::string(bad) + " (yrt_render_soft_shadows)";
        return YRT_ERR_INVALID_ARG;
    }
    const yrt_camera_model pinhole = {YRT_CAMERA_PERSPECTIVE, 0.0f, 0.0f, 0};
    return render_camera_impl(s, p, m ? m : &pinhole, sp, out, mem, stream);
}

int yrt_camera_rays(yrt_scene* s, const yrt_render_params* p, const yrt_camera_model* m, float* rays, int mem,
                    void* stream) {
    // (before any device call, and before the handle is looked at)
    if (const char* bad = camera_call_error(s, p, m, rays, mem)) {
        g_last_error = bad;
        return YRT_ERR_INVALID_ARG;
    }
    return guarded([&] {
        yrt_render_params q = *p;
        q.out_stride = 0;  // (the records have no rows)
        auto r = resolve(*s->ds, q);
        if (r.tw <= 0 || r.th <= 0) return (int)YRT_OK;
        if (r.y0 + r.th > r.H) throw std::invalid_argument("window taller than image");
        if (mem == YRT_MEM_DEVICE && ((uintptr_t)rays & 15)) throw std::invalid_argument("device rays are 16-byte aligned");
        yrt::camera_resolved cm;
        const yrt::dev_render_args a = camera_frame_args(s, q, r, *m, false, cm);
        hipStream_t st = (hipStream_t)stream;
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        const size_t bytes = (size_t)r.tw * r.th * q.samples * q.samples * 32;
        void* dst = mem == YRT_MEM_DEVICE ? (void*)rays : scratch(s, bytes);
        hip_check(yrt::launch_camera_rays(*s->ds, a, cm.model, cm.aperture, dst, st), "camera rays launch");
        if (mem != YRT_MEM_DEVICE) {
            hip_check(hipMemcpyAsync(rays, dst, bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
            hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
        }
        return (int)YRT_OK;
    });
}

int yrt_scene_adaptive_refined(yrt_scene* s, unsigned long long* pixels) {
    if (!s || !pixels) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        hip_check(hipStreamSynchronize(s->last_stream), "hipStreamSynchronize");
        *pixels = s->ds->adaptive_refined;
        return YRT_OK;
    });
}

int yrt_last_stats(yrt_scene* s, yrt_stats* out) {
    if (!s || !out) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        std::vector<unsigned long long> lines((size_t)yrt::cnt_slots * yrt::cnt_count);
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        hip_check(hipStreamSynchronize(s->last_stream), "hipStreamSynchronize");
        hip_check(hipMemcpy(lines.data(), s->counters, lines.size() * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost),
                  "hipMemcpy(counters)");
        unsigned long long c[yrt::cnt_count] = {};
        for (int l = 0; l < yrt::cnt_slots; l++)
            for (int k = 0; k < yrt::cnt_count; k++) c[k] += lines[(size_t)l * yrt::cnt_count + k];
        // the wavefront path counts its shadow rays only under cnt_shadow_rays
        out->rays = c[yrt::cnt_rays] + c[yrt::cnt_shadow_rays];
        out->camera_samples = c[yrt::cnt_samples];
        out->depth_truncated = c[yrt::cnt_depth_truncated];
        out->stack_overflow = c[yrt::cnt_stack_overflow];
        out->box_tests = c[yrt::cnt_box_tests];
        out->instance_entries = c[yrt::cnt_inst_entries];
        out->prim_tests = c[yrt::cnt_prim_tests];
        out->shaded_hits = c[yrt::cnt_shaded_hits];
        out->texture_lookups = c[yrt::cnt_tex_lookups];
        out->shadow_rays = c[yrt::cnt_shadow_rays];
        out->shadow_box_tests = c[yrt::cnt_shadow_box_tests];
        out->shadow_instance_entries = c[yrt::cnt_shadow_inst_entries];
        out->shadow_prim_tests = c[yrt::cnt_shadow_prim_tests];
        out->wave_node_visits = c[yrt::cnt_wave_node_visits];
        out->wave_prim_visits = c[yrt::cnt_wave_prim_visits];
        out->shadow_wave_node_visits = c[yrt::cnt_shadow_wave_node_visits];
        out->shadow_rays_culled = c[yrt::cnt_shadow_culled];
        return YRT_OK;
    });
}

int yrt_last_timings(yrt_scene* s, yrt_timings* out) {
    if (!s || !out) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        hip_check(hipSetDevice(s->ds->device), "hipSetDevice");
        s->ds->timer.collect(out->ms, out->launches);
        return YRT_OK;
    });
}

int yrt_tonemap(const float* rgba, int n, unsigned char* out, int mem, void* stream) {
    if (n < 0 || (n && (!rgba || !out))) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        if (mem == YRT_MEM_DEVICE) {
            hip_check(yrt::launch_tonemap(rgba, n, out, tonemap_table(), (hipStream_t)stream), "tonemap launch");
        } else {
            int h = 1;
            yrt::tonemap_rgba8(rgba, n, h, out);
        }
        return YRT_OK;
    });
}

int yrt_save_image(const char* path, const float* rgba, int w, int h) {
    if (!path || !rgba || w <= 0 || h <= 0) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        yrt::save_hdr_or_ldr(path, rgba, w, h);
        return YRT_OK;
    });
}

int yrt_save_image_mem(const char* path, const float* rgba, int w, int h, int mem, void* stream) {
    if (mem != YRT_MEM_DEVICE) return yrt_save_image(path, rgba, w, h);
    if (!path || !rgba || w <= 0 || h <= 0) return YRT_ERR_INVALID_ARG;
    return guarded([&] {
        const std::string p = path;
        const size_t n = (size_t)w * h;
        hipStream_t st = (hipStream_t)stream;
        if (p.size() >= 4 && p.substr(p.size() - 4) == ".hdr") {
            // RGBE on the GPU (4 B/pixel over PCIe), the run-length scanlines on the host
            unsigned char* d8 = nullptr;
            hip_check(hipMalloc(&d8, n * 4), "hipMalloc(rgbe)");
            std::vector<unsigned char> rgbe(n * 4);
            hipError_t e = yrt::launch_rgbe(rgba, w, h, d8, st);
            if (e == hipSuccess) e = hipMemcpyAsync(rgbe.data(), d8, n * 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            (void)hipFree(d8);
            hip_check(e, "device rgbe");
            yrt::save_hdr_rgbe(p, rgbe.data(), w, h);
            return YRT_OK;
        }
        // tonemap on the GPU, then only the 8-bit image crosses PCIe
        unsigned char* d8 = nullptr;
        hip_check(hipMalloc(&d8, n * 4), "hipMalloc(tonemap)");
        std::vector<unsigned char> ldr(n * 4);
        hipError_t e = yrt::launch_tonemap(rgba, (int)n, d8, tonemap_table(), st);
        if (e == hipSuccess) e = hipMemcpyAsync(ldr.data(), d8, n * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        (void)hipFree(d8);
        hip_check(e, "device tonemap");
        yrt::save_ldr_png(p, ldr.data(), w, h);
        return YRT_OK;
    });
}

}  // extern "C"
