// plane_staging.h -- the caller's planes of one call of yrt_render_aovs, yrt_render_mattes,
// yrt_render_passes, yrt_render_light_groups, yrt_render_adaptive or yrt_render_ao as one list, and where each lies in the device
// staging of a call with host planes (capi.cpp stage_host_planes). Plain C++ without the HIP
// runtime, so that it also builds into a stand-alone program under the host sanitizers
// (tools/check_plane_staging.cpp).
#pragma once

#include <stddef.h>

#include "../../include/yrt.h"

namespace yrt {

// the requested planes in one device allocation, plane after plane in the order they were added
struct plane_list {
    // the largest list: every matte key and layer, ids and coverage
    static constexpr int capacity = 2 * YRT_MATTE_KEY_COUNT * YRT_MATTE_LAYERS_MAX;
    struct item {
        void* host;     // the caller's plane
        size_t offset;  // its place in the staging, in bytes
        int slot;       // which plane of the entry point's struct it is (the *_plane_list below)
        size_t bytes;   // the plane's size: plane_bytes, or what add_sized gave it
    };
    item items[capacity];
    int count = 0;
    size_t plane_bytes;
    size_t bytes = 0;  // of the whole staging

    explicit plane_list(size_t plane_bytes) : plane_bytes(plane_bytes) {}
    void add(void* host, int slot) { add_sized(host, slot, plane_bytes); }
    // a plane of another pixel size (yrt_render_adaptive's byte mask); such planes come last, so
    // that the 16-byte pixels before them keep their alignment
    void add_sized(void* host, int slot, size_t item_bytes) {
        items[count++] = {host, bytes, slot, item_bytes};
        bytes += item_bytes;
    }
    // the memory the kernels write for item k: in the staging, or without one the caller's plane
    void* plane(int k, void* staging) const { return staging ? (char*)staging + items[k].offset : items[k].host; }
};
static_assert(YRT_AOV_COUNT <= plane_list::capacity && YRT_PASS_COUNT + 1 <= plane_list::capacity &&
                  YRT_LIGHT_GROUPS_MAX + 2 <= plane_list::capacity,
              "every entry point's planes fit the list");

// yrt_render_aovs: the AOVs of `mask`; slot YRT_AOV_x
inline plane_list aov_plane_list(unsigned mask, const yrt_aov_planes& out, size_t plane_bytes) {
    plane_list l(plane_bytes);
    for (int k = 0; k < YRT_AOV_COUNT; k++)
        if (mask >> k & 1) l.add(out.plane[k], k);
    return l;
}

// yrt_render_mattes: key-major, layer, then ids before coverage; slot 4 key + 2 layer + coverage
static_assert(YRT_MATTE_LAYERS_MAX == 2, "a matte plane's slot has one bit for the layer");
inline plane_list matte_plane_list(unsigned key_mask, int layers, const yrt_matte_planes& out, size_t plane_bytes) {
    plane_list l(plane_bytes);
    for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++) {
        if (!(key_mask >> k & 1)) continue;
        for (int layer = 0; layer < layers; layer++) {
            l.add(out.ids[k][layer], 4 * k + 2 * layer);
            l.add(out.coverage[k][layer], 4 * k + 2 * layer + 1);
        }
    }
    return l;
}

// yrt_render_passes: the passes of `mask`, slot YRT_PASS_x, then the beauty when given, slot YRT_PASS_COUNT
inline plane_list pass_plane_list(unsigned mask, const yrt_pass_planes& out, float* beauty, size_t plane_bytes) {
    plane_list l(plane_bytes);
    for (int k = 0; k < YRT_PASS_COUNT; k++)
        if (mask >> k & 1) l.add(out.plane[k], k);
    if (beauty) l.add(beauty, YRT_PASS_COUNT);
    return l;
}

// yrt_render_light_groups: the first ngroups groups, slot g, then the ambient and the beauty
// when given, slots YRT_LIGHT_GROUPS_MAX and YRT_LIGHT_GROUPS_MAX + 1
inline plane_list light_group_plane_list(int ngroups, const yrt_light_group_planes& out, size_t plane_bytes) {
    plane_list l(plane_bytes);
    for (int g = 0; g < ngroups; g++) l.add(out.group[g], g);
    if (out.ambient) l.add(out.ambient, YRT_LIGHT_GROUPS_MAX);
    if (out.beauty) l.add(out.beauty, YRT_LIGHT_GROUPS_MAX + 1);
    return l;
}

// yrt_render_adaptive: the image, slot 0, then the byte mask when given, slot 1, of
// pixels bytes (1 B per pixel of the same rows and stride)
inline plane_list adaptive_plane_list(float* out, unsigned char* refined, size_t pixels) {
    plane_list l(pixels * 16);
    l.add(out, 0);
    if (refined) l.add_sized(refined, 1, pixels);
    return l;
}

// yrt_render_ao: the one plane, slot 0
inline plane_list ao_plane_list(float* out, size_t plane_bytes) {
    plane_list l(plane_bytes);
    l.add(out, 0);
    return l;
}

}  // namespace yrt
