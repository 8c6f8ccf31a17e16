// check_soft_shadow_rays -- the soft shadows' ray formula (csrc/soft_shadow_rays.h), the argument
// rules of yrt_shade_rays_soft and yrt_render_soft_shadows (csrc/soft_shadow_args.h) and the
// tables' header (csrc/ao_tables.h) as a stand-alone program, for the host compiler and the host
// sanitizers:
//
//     CXXFLAGS="-std=c++17 -g -ffp-contract=off -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all"
//     c++ $CXXFLAGS tools/check_soft_shadow_rays.cpp -o check_soft_shadow_rays && ./check_soft_shadow_rays
//
// Without arguments it checks which parameters are refused and properties of the rays that hold
// whatever the light: unit directions, every target on the disk of radius R about the light's
// point and across the centre direction, radius 0 the hard shadow ray, a rotation index that
// does not see the sign of a zero. Exit status 0 and "ok" on success.
//
// With arguments it writes the rays of a list of cases, for tests/test_soft_shadows_api.py to
// compare with the numpy model (tests/soft_shadow_model.py):
//
//     check_soft_shadow_rays rays IN OUT
//
// IN holds records of 21 32-bit words: p.xyz, the light's frame {x, y, z, o} (12 floats), the
// light shape's first vertex lp0.xyz, R (floats), then K and li (ints). OUT receives, per case in
// order, K records of 8 float32 {o.xyz, d.xyz, tmin, tmax} -- one record when R == 0, the hard
// shadow ray. The kernel (wavefront.hip k_soft_shadow) evaluates the same header; its
// normalize_len gives normalize's and length's bits (trace_common.h).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../yocto_raytracing_amd/csrc/ao_tables.h"
#include "../yocto_raytracing_amd/csrc/soft_shadow_args.h"
#include "../yocto_raytracing_amd/csrc/soft_shadow_rays.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what, int n = 0) {
    if (ok) return;
    fprintf(stderr, "FAILED: %s (%d)\n", what, n);
    failures++;
}

const float inf = std::numeric_limits<float>::infinity(), nan_ = std::numeric_limits<float>::quiet_NaN();
const float dirs[] = {YRT_AO_DIRS};
const float rots[] = {YRT_AO_ROTS};

struct light_case {
    yrt::vec3f p;
    yrt::frame3f lf;
    yrt::vec3f lp0;
    float R;
    int K, li;
};
static_assert(sizeof(light_case) == 21 * 4, "a record of 21 words");

// the rays of one case appended to out: the contract's steps 1 to 5
void rays_of(const light_case& c, std::vector<float>& out) {
    const yrt::vec3f tp = yrt::transform_point(c.lf, c.lp0 - c.p);
    const yrt::vec3f l = yrt::normalize(tp);
    const float r = yrt::length(tp);
    auto put = [&](yrt::vec3f d, float len) {
        const float rec[8] = {c.p.x, c.p.y, c.p.z, d.x, d.y, d.z, 0.01f, len - 0.01f};
        out.insert(out.end(), rec, rec + 8);
    };
    if (c.R == 0.0f) return put(l, r);
    const int rot = yrt::soft_shadow_rot(c.p, c.li);
    yrt::vec3f b1, b2;
    yrt::soft_shadow_basis(l, b1, b2);
    for (int k = 0; k < c.K; k++) {
        const yrt::vec3f tq = yrt::soft_shadow_target(tp, b1, b2, rots[2 * rot], rots[2 * rot + 1], dirs, k, c.R);
        put(yrt::normalize(tq), yrt::length(tq));
    }
}

int write_rays(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: check_soft_shadow_rays rays IN OUT\n");
        return 2;
    }
    FILE* in = fopen(argv[2], "rb");
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 1;
    }
    std::vector<float> out;
    light_case c;
    while (fread(&c, sizeof c, 1, in) == 1) {
        if (c.K < 1 || c.K > YRT_SOFT_SHADOW_RAYS_MAX || c.li < 0 || !yrt::soft_radius_ok(c.R)) {
            fclose(in);
            return 2;
        }
        rays_of(c, out);
    }
    fclose(in);
    FILE* fp = fopen(argv[3], "wb");
    const bool ok = fp && fwrite(out.data(), 4, out.size(), fp) == out.size();
    if ((fp && fclose(fp) != 0) || !ok) {
        fprintf(stderr, "cannot write %s\n", argv[3]);
        return 1;
    }
    return 0;
}

bool refused(int rays, float radius, const float* light_radius = nullptr, int nlights = 0) {
    const yrt_soft_shadow_params sp = {rays, radius, light_radius, nlights};
    return yrt::soft_shadow_params_error(&sp) != nullptr;
}

double len3(yrt::vec3f a) { return std::sqrt((double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z); }

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "rays") == 0) return write_rays(argc, argv);
    if (argc > 1) return 2;

    // ---- the argument rules ----
    expect(yrt::soft_shadow_params_error(nullptr) != nullptr, "null params are refused");
    for (int k = -2; k <= 66; k++) expect(refused(k, 0.5f) == !(k >= 0 && k <= 64), "K within 0..64", k);
    expect(refused(16, -1.0f) && refused(16, nan_) && refused(16, inf) && refused(16, -inf), "a negative, NaN or infinite radius");
    expect(!refused(16, 0.0f) && !refused(16, -0.0f) && !refused(0, 3.0f) && !refused(64, 1e30f), "radii >= 0 are taken");
    {
        const float good[3] = {0.0f, 0.5f, 2.0f}, neg[3] = {0.5f, -0.25f, 1.0f}, bad[3] = {0.5f, 1.0f, nan_};
        expect(!refused(16, 0.0f, good, 3) && refused(16, 0.0f, neg, 3) && refused(16, 0.0f, bad, 3) && !refused(16, 0.0f, bad, 2),
               "every entry of light_radius");
        expect(refused(16, 0.0f, good, -1), "a negative nlights");
        const yrt_soft_shadow_params sp = {16, 0.0f, good, 3}, all = {16, 1.0f, nullptr, 7};
        expect(yrt::soft_shadow_lights_error(sp, 3) == nullptr && yrt::soft_shadow_lights_error(sp, 4) != nullptr &&
                   yrt::soft_shadow_lights_error(all, 3) == nullptr,
               "nlights is the scene's light count when light_radius is given");
        const yrt_soft_shadow_params zero = {0, 0.0f, nullptr, 0};
        expect(yrt::soft_shadow_rays_of(zero) == 16 && yrt::soft_shadow_rays_of(sp) == 16 && yrt::soft_shadow_rays_of({7, 0, nullptr, 0}) == 7,
               "K = 0 is 16");
    }
    expect(sizeof dirs == sizeof(float) * 3 * yrt::ao_dir_count && sizeof rots == sizeof(float) * 2 * yrt::ao_rot_count,
           "the tables' sizes");

    // ---- the rays: a rotated light frame, hit points on every side of it ----
    const float sq = std::sqrt(0.5f);
    const yrt::frame3f lf = {{sq, 0.0f, -sq}, {0.0f, 1.0f, 0.0f}, {sq, 0.0f, sq}, {1.0f, 4.0f, -2.0f}};
    const yrt::vec3f lp0 = {0.25f, -0.5f, 0.125f};
    int at = 0;
    for (float x = -3.0f; x <= 3.0f; x += 1.5f)
        for (float y = -1.0f; y <= 9.0f; y += 2.5f)  // above the light too: l.z and l.y of both signs
            for (float z = -6.0f; z <= 3.0f; z += 2.25f, at++) {
                const light_case c = {{x, y, z}, lf, lp0, 0.75f, 64, at % 7};
                std::vector<float> rays, hard;
                rays_of(c, rays);
                light_case h = c;
                h.R = 0.0f;
                rays_of(h, hard);
                expect(rays.size() == 64 * 8 && hard.size() == 8, "K rays, or the one hard ray", at);
                const yrt::vec3f tp = yrt::transform_point(lf, lp0 - c.p), l = {hard[3], hard[4], hard[5]};
                expect(std::fabs(len3(l) - 1.0) < 1e-6 && std::fabs(hard[7] + 0.01f - len3(tp)) < 1e-5 * len3(tp), "the hard ray", at);
                for (int k = 0; k < 64; k++) {
                    const float* r = &rays[8 * k];
                    const yrt::vec3f d = {r[3], r[4], r[5]};
                    const double len = r[7] + 0.01;
                    expect(memcmp(r, &c.p, 12) == 0 && r[6] == 0.01f && std::fabs(len3(d) - 1.0) < 1e-6, "origin, tmin, unit direction", at);
                    // the target relative to the light's point: on the disk, across l
                    const yrt::vec3f off = {(float)(d.x * len - tp.x), (float)(d.y * len - tp.y), (float)(d.z * len - tp.z)};
                    expect(len3(off) <= 0.75 * (1 + 1e-4) && std::fabs(yrt::dot(off, l)) < 1e-4, "a point of the light's disk", at);
                }
            }
    // the rotation index: the sign of a zero is not seen, the light index is
    {
        const yrt::vec3f a = {0.0f, 1.5f, -2.0f}, b = {-0.0f, 1.5f, -2.0f}, c = {1.5f, -0.0f, 0.0f}, d = {1.5f, 0.0f, -0.0f};
        for (int li = 0; li < 20; li++) {
            expect(yrt::soft_shadow_rot(a, li) == yrt::soft_shadow_rot(b, li) && yrt::soft_shadow_rot(c, li) == yrt::soft_shadow_rot(d, li),
                   "-0 and +0 are one point", li);
            expect(yrt::soft_shadow_rot(a, li) >= 0 && yrt::soft_shadow_rot(a, li) < 16, "an index into rots", li);
        }
        expect(yrt::soft_shadow_rot(a, 0) != yrt::soft_shadow_rot(a, 1), "the light index moves the rotation");
    }
    if (failures) return 1;
    puts("ok");
    return 0;
}
