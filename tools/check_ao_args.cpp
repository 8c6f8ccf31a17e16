// check_ao_args -- the argument handling of yrt_render_ao (csrc/ao_args.h), its one-plane list
// (csrc/plane_staging.h) and the tables' header (csrc/ao_tables.h) as a stand-alone program, for
// the host sanitizers:
//
//     CXXFLAGS="-std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all"
//     clang++ $CXXFLAGS tools/check_ao_args.cpp -o check_ao_args && ./check_ao_args
//
// It walks every ray count from -2 to 66, distances and biases accepted and refused (NaN, the
// infinities, zero, negative, bias at and above the distance), both `mem` values and a bad one,
// checks what ao_resolve hands the kernel, and does with the plane list what the entry point does
// with a host plane: stages it, fills the window's pixels, copies back, and checks that the
// padding columns kept the caller's bytes and nothing was written past an end. No GPU and no HIP
// runtime: memcpy stands in for the copies. Exit status 0 and "ok" on success.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../yocto_raytracing_amd/csrc/ao_args.h"
#include "../yocto_raytracing_amd/csrc/ao_tables.h"
#include "../yocto_raytracing_amd/csrc/plane_staging.h"

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

bool refused(int rays, float distance, float bias, int mem = YRT_MEM_HOST) {
    float px[4];
    const yrt_ao_params a = {rays, distance, bias};
    return yrt::ao_args_error(&a, px, mem) != nullptr;
}

}  // namespace

int main() {
    // the ray count: 0 is the default, 1..64 as given, everything else refused
    for (int k = -2; k <= YRT_AO_RAYS_MAX + 2; k++) {
        const bool ok = k >= 0 && k <= YRT_AO_RAYS_MAX;
        expect(refused(k, FLT_MAX, 0.01f) == !ok, "rays within 0, 1..64", k);
        if (ok) expect(yrt::ao_resolve({k, 1.0f, 0.0f}).rays == (k ? k : 16), "0 rays are 16", k);
    }
    // the distance: > 0, +inf taken as FLT_MAX
    expect(refused(16, nan_, 0.0f) && refused(16, 0.0f, 0.0f) && refused(16, -0.0f, 0.0f) && refused(16, -1.0f, 0.0f) &&
               refused(16, -inf, 0.0f),
           "distance NaN or <= 0 is refused");
    expect(!refused(16, inf, 0.01f) && !refused(16, FLT_MAX, 0.01f) && !refused(16, FLT_MIN, 0.0f), "distance > 0 is taken");
    expect(yrt::ao_resolve({16, inf, 0.01f}).distance == FLT_MAX && yrt::ao_resolve({16, 1.5f, 0.25f}).distance == 1.5f &&
               yrt::ao_resolve({16, 1.5f, 0.25f}).bias == 0.25f,
           "the kernel's tmax and tmin");
    // the bias: finite, >= 0, below the distance the kernel receives
    expect(refused(16, 1.0f, nan_) && refused(16, 1.0f, -0.5f) && refused(16, inf, inf) && refused(16, 1.0f, -inf) &&
               refused(16, 1.0f, 1.0f) && refused(16, 1.0f, 2.0f) && refused(16, inf, FLT_MAX),
           "bias NaN, negative, infinite or >= distance is refused");
    expect(!refused(16, 1.0f, 0.0f) && !refused(16, 1.0f, -0.0f) && !refused(16, 1.0f, std::nextafter(1.0f, 0.0f)),
           "bias in [0, distance) is taken");
    // mem and the null pointers
    expect(!refused(16, 1.0f, 0.0f, YRT_MEM_DEVICE) && refused(16, 1.0f, 0.0f, 2) && refused(16, 1.0f, 0.0f, -1), "mem");
    {
        float px[4];
        const yrt_ao_params a = {16, 1.0f, 0.0f};
        expect(yrt::ao_args_error(nullptr, px, YRT_MEM_HOST) && yrt::ao_args_error(&a, nullptr, YRT_MEM_HOST) &&
                   !yrt::ao_args_error(&a, px, YRT_MEM_HOST),
               "null parameters or out are refused");
    }
    // the tables: their sizes, unit vectors, no direction below the smallest z
    expect(sizeof dirs == sizeof(float) * 3 * yrt::ao_dir_count && sizeof rots == sizeof(float) * 2 * yrt::ao_rot_count &&
               yrt::ao_dir_count == YRT_AO_RAYS_MAX,
           "the tables' sizes");
    for (int k = 0; k < yrt::ao_dir_count; k++) {
        const double x = dirs[3 * k], y = dirs[3 * k + 1], z = dirs[3 * k + 2];
        expect(std::fabs(std::sqrt(x * x + y * y + z * z) - 1.0) < 1e-7 && z >= 0.125, "a unit direction with z >= 0.125", k);
    }
    for (int r = 0; r < yrt::ao_rot_count; r++)
        expect(std::fabs(std::hypot((double)rots[2 * r], (double)rots[2 * r + 1]) - 1.0) < 1e-7, "a unit rotation", r);

    // the plane list: one plane at offset 0; a padded host plane through the staging
    const int w = 5, h = 3, stride = 7;
    const size_t plane_bytes = (size_t)stride * h * 16;
    std::vector<float> caller(plane_bytes / 4, 77.0f);  // exactly sized: the sanitizer sees any access past its end
    const yrt::plane_list list = yrt::ao_plane_list(caller.data(), plane_bytes);
    expect(list.count == 1 && list.bytes == plane_bytes && list.items[0].offset == 0 && list.items[0].slot == 0 &&
               list.items[0].bytes == plane_bytes,
           "one plane, the whole staging");
    expect(list.plane(0, nullptr) == caller.data(), "without a staging the plane is the caller's");
    std::vector<char> stage(list.bytes);
    expect(list.plane(0, stage.data()) == stage.data(), "the staged plane is the staging");
    memcpy(list.plane(0, stage.data()), list.items[0].host, list.items[0].bytes);  // the padding's bytes
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const float px[4] = {(float)y, (float)x, 1.0f, 0.5f};
            memcpy((char*)list.plane(0, stage.data()) + ((size_t)y * stride + x) * 16, px, 16);
        }
    memcpy(list.items[0].host, list.plane(0, stage.data()), list.items[0].bytes);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < stride; x++) {
            const float* px = &caller[((size_t)y * stride + x) * 4];
            if (x < w)
                expect(px[0] == (float)y && px[1] == (float)x && px[2] == 1.0f && px[3] == 0.5f, "a window pixel", y * stride + x);
            else
                expect(px[0] == 77.0f && px[1] == 77.0f && px[2] == 77.0f && px[3] == 77.0f, "a padding pixel", y * stride + x);
        }
    if (failures) return 1;
    puts("ok");
    return 0;
}
