// wf_workspace.h -- the workspace of one chunk of the wavefront path (wavefront.hip run(),
// run_rays()): the constants and counts that size it, and its slabs as one ordered description
// (walk_workspace). Its total is that walk with a summing visitor (workspace_bytes), carving it
// the same walk with a visitor that hands out pointers (workspace_carver), so no size is written
// twice. Plain C++ without the HIP runtime, so that it also builds into a stand-alone program
// under the host sanitizers (tools/check_wf_workspace.cpp).
#pragma once

#include <stddef.h>

#include <initializer_list>

#include "yrt_render.h"

namespace yrt {

constexpr int TILE = 8;         // pixel tiles of TILE x TILE in the sample enumeration

// the render's list sums (k_list_stats, yrt_scene_tile_lists / yrt_scene_tile_list_masks):
// camera-list entries, camera lists, bundle-list entries, bundle lists, then the instances the
// camera lists' and the bundle lists' masks exclude
constexpr int list_sums = 6;

// Mirror levels are compacted into level_segments segments of B.seg slots: segment g of
// level k + 1 holds the mirror rays spawned by k_shade's blocks b with b % 8 == g, at
// [g * seg, g * seg + count), each segment behind its own counter on its own 128-byte
// line. (One counter for the whole level serialised k_shade's block atomics: about 7 ns
// each on one address, ~1 ms of c3's level-0 shading.) Consumers walk the segments in
// turn, so their waves stay full except for each segment's last one.
#ifndef YRT_LEVEL_SEGMENTS
#define YRT_LEVEL_SEGMENTS 8
#endif
constexpr int level_segments = YRT_LEVEL_SEGMENTS;  // divides the 2048-block grid of the mirror levels
static_assert(2048 % level_segments == 0, "segment bound (chunk_plan) assumes level_segments | 2048");
constexpr int count_stride = 32;  // ints: one 128-byte line per counter

// shadow bundles (wavefront.hip k_bundle_lists)
#ifndef YRT_BUNDLE_ITEMS
#define YRT_BUNDLE_ITEMS 64  // 64-sample items per bundle (at most 64: one per lane of the list builder)
#endif
constexpr int bundle_g = YRT_BUNDLE_ITEMS;
static_assert(bundle_g >= 1 && bundle_g <= 64, "one item per lane of k_bundle_lists");
constexpr int bundle_recs = 5;        // wide records per list: a chain (3 + 3 + 3 + 3 + 4 leaves)
constexpr int bundle_max_lights = 8;  // more lights: no bundles (the lists' memory grows with them)
// super-bundles: the common leaf list of super_bundles bundles (k_bundle_super)
constexpr int super_bundles = 4;
static_assert(bundle_g * super_bundles <= 4 * 64, "bundle_box: up to four items per lane");
constexpr int super_max = 32;
constexpr int super_list_f4 = 1 + 2 * super_max;  // {count} then {lo, word} {hi, 0} per leaf
// camera rays walk per-tile leaf lists (k_camera_lists, packet_first's list mode)
#ifndef YRT_CAMERA_LIST_MAX
#define YRT_CAMERA_LIST_MAX 32  // leaves per tile list (more: the tile's rays walk the tree)
#endif
constexpr int camera_list_max = YRT_CAMERA_LIST_MAX;

constexpr int group_planes = light_groups_max + 2;  // the groups, the ambient, the beauty

inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

// the per-level, per-segment mirror-ray counters (seg_counter)
inline size_t count_bytes(int nlevels) { return sizeof(int) * ((size_t)nlevels + 1) * level_segments * count_stride; }

// shadow bundles: items (64-sample blocks) and bundles of a chunk of cap samples
inline size_t bundle_items(int cap) { return ((size_t)cap + 63) / 64; }
inline size_t bundle_count(int cap) { return (bundle_items(cap) + bundle_g - 1) / bundle_g; }
inline int bundle_lights(int nlights) { return nlights <= bundle_max_lights ? nlights : 0; }
inline size_t super_count(int cap) { return (bundle_count(cap) + super_bundles - 1) / super_bundles; }

// camera lists: 8x8-pixel tiles of a chunk of cap samples at spp samples per pixel
inline size_t camera_tiles(int cap, int spp) { return ((size_t)cap / (size_t)spp + TILE * TILE - 1) / (TILE * TILE); }

// the light groups' table: per plane the bounds of its lights, then the lights sorted by plane
inline size_t group_table_ints(int nlights) { return group_planes + 1 + 2 * (size_t)nlights; }

// What sizes a chunk's workspace. yrt_render's slabs are the same with or without passes and
// groups, whose planes follow them.
struct workspace_shape {
    int cap;      // slots per sample record: the chunk's samples, with mirror levels their segments' slack too
    int spp;
    int nlights;
    int nlevels;
    // yrt_render_passes in the unfused and mirror shapes: per-sample values of npass_planes wanted
    // passes, pass_samples of each (the fused shape keeps them in LDS: 0 planes)
    int npass_planes = 0;
    size_t pass_samples = 0;
    // yrt_render_light_groups: ngroup_planes planes in use (0: no groups), group_samples per-sample
    // values of each (the chunk's samples; 0 in the fused shape)
    int ngroup_planes = 0;
    size_t group_samples = 0;
};

// the slabs in the workspace's order; the members of wf_buffers, pass_buffers and group_buffers
// they are (wavefront.hip carve)
enum wf_slab {
    slab_count, slab_queue, slab_lstats,
    slab_surf0, slab_surf1, slab_surfv, slab_occl, slab_rad,
    slab_pbox, slab_lcount, slab_lskip, slab_lists, slab_slists,
    slab_ccount, slab_cskip, slab_clist,
    slab_ray_o, slab_ray_d, slab_rec0, slab_rec1,  // the mirror levels' records
    slab_pass_smp,                                 // one per wanted pass: k its rank among them
    slab_group_tab, slab_group_smp, slab_group_rec  // per plane k >= 1 (plane 0's are rad and rec0)
};

// visit(slab, k, bytes) for every slab of shape s in its order in memory, each taking
// align_up(bytes). A slab the shape does not have comes with 0 bytes: the mirror slabs at one
// level, the bundles' lists past bundle_max_lights, the groups' samples in the fused shape.
template <class V>
void walk_workspace(const workspace_shape& s, V&& visit) {
    const size_t c = (size_t)s.cap;
    visit(slab_count, 0, count_bytes(s.nlevels));
    visit(slab_queue, 0, 32 * sizeof(unsigned));
    visit(slab_lstats, 0, list_sums * sizeof(unsigned long long));
    visit(slab_surf0, 0, 16 * c);
    visit(slab_surf1, 0, 16 * c);
    visit(slab_surfv, 0, 4 * c);
    visit(slab_occl, 0, c * (size_t)(s.nlights > 1 ? s.nlights : 1));
    visit(slab_rad, 0, 16 * c);
    const size_t gl = bundle_count(s.cap) * bundle_lights(s.nlights);
    visit(slab_pbox, 0, 32 * bundle_items(s.cap));
    visit(slab_lcount, 0, 4 * gl);
    visit(slab_lskip, 0, 4 * gl);
    visit(slab_lists, 0, (size_t)bundle_recs * wide_record_bytes * gl);
    visit(slab_slists, 0, super_count(s.cap) * bundle_lights(s.nlights) * super_list_f4 * 16);
    const size_t nt = camera_tiles(s.cap, s.spp);
    visit(slab_ccount, 0, 4 * nt);
    visit(slab_cskip, 0, 4 * nt);
    visit(slab_clist, 0, nt * camera_list_max * 32);
    // levels >= 1: ray_o, ray_d; levels < last: rec0, rec1 (one slab each, 16 B per level and slot)
    const size_t levels = (size_t)(s.nlevels - 1) * 16 * c;
    for (wf_slab m : {slab_ray_o, slab_ray_d, slab_rec0, slab_rec1}) visit(m, 0, levels);
    for (int k = 0; k < s.npass_planes; k++) visit(slab_pass_smp, k, 16 * s.pass_samples);
    if (s.ngroup_planes > 0) visit(slab_group_tab, 0, sizeof(int) * group_table_ints(s.nlights));
    for (int k = 1; k < s.ngroup_planes; k++) visit(slab_group_smp, k, 16 * s.group_samples);
    for (int k = 1; k < s.ngroup_planes; k++) visit(slab_group_rec, k, levels);
}

inline size_t workspace_bytes(const workspace_shape& s) {
    size_t total = 0;
    walk_workspace(s, [&](wf_slab, int, size_t bytes) { total += align_up(bytes); });
    return total;
}

// hands the slabs out of the memory at `base`, in the walk's order; a slab of 0 bytes is null
struct workspace_carver {
    char* p;
    explicit workspace_carver(void* base) : p((char*)base) {}
    void* take(size_t bytes) {
        char* q = bytes ? p : nullptr;
        p += align_up(bytes);
        return q;
    }
};

}  // namespace yrt
