// check_wf_workspace -- the layout of the wavefront path's workspace (csrc/wf_workspace.h) as a
// stand-alone program, for the host sanitizers:
//
//     CXXFLAGS="-std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all"
//     INC="-D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iyocto_raytracing_amd/csrc -Iinclude"
//     clang++ $CXXFLAGS $INC tools/check_wf_workspace.cpp -o check_wf_workspace && ./check_wf_workspace
//
// It sweeps spp {1, 4, 9, 64} x lights {0, 1, 4, 8, 9} (9 is past bundle_max_lights: no bundle
// slabs) x levels {1, 2, 16} x 0..5 pass planes x 0..10 group planes, these with and without
// per-sample planes, x the samples of a 37 x 24 frame at s = 2 and s = 3, of the c4 frame
// (1920 x 1080 x 64) and 2^29 samples; with mirror levels the slots are the samples and the
// segments' slack, as plan_chunks (wavefront.hip) makes them. For every shape: every offset is
// a multiple of 256, the slabs come in the order of wf_slab and do not overlap, the total is the
// end of the last slab, and a slab of 0 bytes is one the shape does not have.
// The shapes of the 37 x 24 frames are carved into a malloc of exactly the total and every slab
// is memset over its full size: a slab that overruns, or a total that is short, is a sanitizer
// report; the carver's pointers are base + offset, null for a slab of 0 bytes. That touches every
// byte, so it leaves out the shapes with passes and groups together (no call has both), and of
// the 16-level shapes, tens of MiB each of mirror records whose size is the same expression
// as at 2 levels, it takes a thinned set.
// `pinned`: the totals of fifteen shapes of the sweep and of a ray batch's as constants. They are NOT taken from
// wf_workspace.h: they were produced once by evaluating workspace_bytes() + group_bytes() of
// wavefront.hip as they stood in the commit before this header existed (b3209ac), on the CPU.
// The total decides how a frame is chunked (chunk_target), so it must stay what it was.
// Exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "wf_workspace.h"

namespace {

using namespace yrt;

int failures = 0;
void expect(bool ok, const char* what, const workspace_shape& s) {
    if (ok) return;
    if (failures++ < 20)
        fprintf(stderr, "FAILED: %s (cap %d spp %d lights %d levels %d passes %d x %zu groups %d x %zu)\n", what, s.cap,
                s.spp, s.nlights, s.nlevels, s.npass_planes, s.pass_samples, s.ngroup_planes, s.group_samples);
}

struct placed {
    wf_slab slab;
    int k;
    size_t bytes, offset;
};

// whether shape s has the slab at all
bool has_slab(const workspace_shape& s, wf_slab slab) {
    switch (slab) {
        case slab_lcount: case slab_lskip: case slab_lists: case slab_slists: return bundle_lights(s.nlights) > 0;
        case slab_ray_o: case slab_ray_d: case slab_rec0: case slab_rec1: case slab_group_rec: return s.nlevels > 1;
        case slab_pass_smp: return s.pass_samples > 0;
        case slab_group_smp: return s.group_samples > 0;
        default: return true;
    }
}

std::vector<placed> layout(const workspace_shape& s) {
    std::vector<placed> v;
    size_t at = 0;
    walk_workspace(s, [&](wf_slab slab, int k, size_t bytes) {
        v.push_back({slab, k, bytes, at});
        at += align_up(bytes);
    });
    return v;
}

void check_layout(const workspace_shape& s) {
    const std::vector<placed> v = layout(s);
    int npass = 0, ngsmp = 0, ngrec = 0, ntab = 0;
    for (size_t i = 0; i < v.size(); i++) {
        expect(v[i].offset % 256 == 0, "every offset is a multiple of 256", s);
        expect((v[i].bytes != 0) == has_slab(s, v[i].slab), "exactly the slabs the shape lacks take 0 bytes", s);
        if (i > 0) {
            expect(v[i].offset >= v[i - 1].offset + v[i - 1].bytes, "slabs do not overlap", s);
            expect(v[i].slab > v[i - 1].slab || (v[i].slab == v[i - 1].slab && v[i].k == v[i - 1].k + 1),
                   "slabs come in wf_slab's order, a slab's planes in theirs", s);
        }
        npass += v[i].slab == slab_pass_smp, ngsmp += v[i].slab == slab_group_smp;
        ngrec += v[i].slab == slab_group_rec, ntab += v[i].slab == slab_group_tab;
    }
    expect(v.size() >= 20 && v[0].slab == slab_count && v[19].slab == slab_rec1, "the render's twenty slabs come first", s);
    expect(npass == s.npass_planes, "one slab per pass plane", s);
    const int others = s.ngroup_planes > 0 ? s.ngroup_planes - 1 : 0;
    expect(ntab == (s.ngroup_planes > 0) && ngsmp == others && ngrec == others,
           "the groups' table, and samples and records of every plane but the first", s);
    expect(workspace_bytes(s) == v.back().offset + align_up(v.back().bytes), "the total is the end of the last slab", s);
}

// the shape carved into exactly its total, every slab written over its full size
void check_carve(const workspace_shape& s) {
    const std::vector<placed> v = layout(s);
    const size_t total = workspace_bytes(s);
    char* base = (char*)malloc(total);
    if (!base) {
        expect(false, "malloc", s);
        return;
    }
    workspace_carver w(base);
    size_t i = 0;
    walk_workspace(s, [&](wf_slab, int, size_t bytes) {
        char* p = (char*)w.take(bytes);
        expect(bytes ? p == base + v[i].offset : p == nullptr, "a slab is base + offset, null when it has no bytes", s);
        if (p) memset(p, 0x5a, bytes);
        i++;
    });
    expect(w.p == base + total, "the carver ends at the total", s);
    free(base);
}

// (wavefront.hip plan_chunks: with mirror levels, level_segments segments of
// samples / level_segments + level_segments * 256 slots)
int slots_of(int samples, int nlevels) {
    return nlevels > 1 ? level_segments * (samples / level_segments + level_segments * 256) : samples;
}

const int frame_s2 = 40 * 24 * 4, frame_s3 = 40 * 24 * 9;  // 37 x 24 pixels are 5 x 3 tiles of 8 x 8
const int frame_c4 = 1920 * 1080 * 64, frame_max = 1 << 29;

bool in(int x, std::initializer_list<int> set) {
    for (int y : set)
        if (x == y) return true;
    return false;
}

void sweep() {
    long long shapes = 0, carved = 0;
    for (int samples : {frame_s2, frame_s3, frame_c4, frame_max})
        for (int spp : {1, 4, 9, 64})
            for (int nlights : {0, 1, 4, 8, 9})
                for (int nlevels : {1, 2, 16})
                    for (int npass = 0; npass <= pass_count; npass++)
                        for (int ngroup = 0; ngroup <= group_planes; ngroup++)
                            for (int group_smp = 0; group_smp < 2; group_smp++) {
                                const workspace_shape s = {slots_of(samples, nlevels), spp,    nlights,
                                                           nlevels,                    npass,  (size_t)samples,
                                                           ngroup,                     group_smp ? (size_t)samples : 0};
                                check_layout(s), shapes++;
                                const bool small = samples == frame_s2 || samples == frame_s3;
                                const bool thinned = samples == frame_s2 && spp == 4 && in(nlights, {1, 9}) &&
                                                     in(npass, {0, 5}) && in(ngroup, {0, 2, 10});
                                if (small && !(npass && ngroup) && (nlevels < 16 || thinned)) check_carve(s), carved++;
                            }
    printf("%lld shapes, %lld of them carved and written\n", shapes, carved);
}

// produced by the code of the commit before wf_workspace.h (see the header comment)
struct {
    workspace_shape s;
    unsigned long long total;
} const pinned[] = {
    {{132710400, 64, 4, 1, 0, 0, 0, 0}, 7649254144ull},    // c4
    {{132710400, 64, 0, 1, 0, 0, 0, 0}, 7133446144ull},
    {{132710400, 64, 9, 1, 0, 0, 0, 0}, 8195129344ull},
    {{25024, 9, 4, 16, 0, 0, 0, 0}, 25527296ull},          // 16 mirror levels
    {{536887296, 64, 8, 16, 0, 0, 0, 0}, 548980910848ull},
    {{20224, 4, 1, 2, 5, 3840, 0, 0}, 2775296ull},         // passes
    {{8640, 9, 4, 1, 3, 8640, 0, 0}, 933888ull},
    {{3840, 4, 8, 1, 0, 0, 10, 0}, 265216ull},             // groups: fused, unfused, mirror
    {{8640, 9, 4, 1, 0, 0, 4, 8640}, 934144ull},
    {{25024, 9, 9, 2, 0, 0, 10, 8640}, 8037632ull},
    {{20224, 4, 2, 16, 0, 0, 3, 3840}, 30459136ull},
    {{536870912, 1, 1, 1, 0, 0, 0, 0}, 37498653184ull},
    {{3840, 4, 0, 1, 0, 0, 0, 0}, 224000ull},
    {{888, 1, 2, 1, 0, 0, 0, 0}, 70400ull},                // a ray batch
    {{132726784, 64, 4, 2, 5, 132710400, 0, 0}, 26761546240ull},
    {{3840, 4, 4, 1, 0, 0, 1, 3840}, 243200ull},
};

}  // namespace

int main() {
    sweep();
    for (const auto& p : pinned) {
        check_layout(p.s);
        expect(workspace_bytes(p.s) == p.total, "the total is what it was before wf_workspace.h", p.s);
    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
