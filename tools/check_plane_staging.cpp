// check_plane_staging -- the plane lists and the staging layout of the entry points that take
// host planes (csrc/plane_staging.h), and the argument handling of yrt_render_mattes
// (csrc/matte_args.h), as a stand-alone program, for the host sanitizers:
//
//     CXXFLAGS="-std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all"
//     clang++ $CXXFLAGS tools/check_plane_staging.cpp -o check_plane_staging && ./check_plane_staging
//
// It walks every matte key mask, layer count and mem, accepted and refused, every AOV mask,
// every pass mask with and without a beauty, 1 to 8 light groups with and without ambient
// and beauty, and yrt_render_adaptive's image with and without its byte mask. For each accepted set it does what the entry point does with host planes: lays
// the requested planes out in one staging buffer, copies the caller's bytes in, fills every
// staged plane, copies back, and checks that exactly the requested planes changed, each with its
// own plane's contents, and that nothing was written past an end. No GPU and no HIP runtime:
// memcpy stands in for the copies. Exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yocto_raytracing_amd/csrc/matte_args.h"
#include "../yocto_raytracing_amd/csrc/plane_staging.h"

namespace {

const int w = 5, h = 3, stride = 7, marker = 77;
const size_t plane_bytes = (size_t)stride * h * 16, plane_words = plane_bytes / 4;

int failures = 0;
void expect(bool ok, const char* what, unsigned mask, int n) {
    if (ok) return;
    fprintf(stderr, "FAILED: %s (mask %u, %d)\n", what, mask, n);
    failures++;
}

// the caller's planes of one call, one per slot of the entry point's struct: exactly sized heap
// blocks, so that the sanitizer sees any access past an end
struct caller_planes {
    std::vector<std::vector<int>> v;
    explicit caller_planes(int slots) : v(slots, std::vector<int>(plane_words, marker)) {}
    template <class T>
    T* at(int slot) {
        return (T*)v[slot].data();
    }
};

// the staging of a call with host planes, then whether each of the caller's planes is as it
// must be: `requested` has the bit of every slot the call names
void round_trip(const yrt::plane_list& lay, caller_planes& planes, unsigned requested, const char* who, unsigned mask,
                int n) {
    const int want = __builtin_popcount(requested);
    expect(lay.count == want && lay.bytes == plane_bytes * want, "one staged plane per requested plane", mask, n);
    std::vector<char> stage(lay.bytes);
    for (int k = 0; k < lay.count; k++) {
        expect(lay.items[k].offset == plane_bytes * k, "planes lie one after the other", mask, n);
        expect(k == 0 || lay.items[k].slot > lay.items[k - 1].slot, "planes lie in the order of their slots", mask, n);
        expect(lay.plane(k, stage.data()) == stage.data() + lay.items[k].offset, "a staged plane is its place in the staging",
               mask, n);
        expect(lay.plane(k, nullptr) == lay.items[k].host, "without a staging a plane is the caller's", mask, n);
        memcpy(lay.plane(k, stage.data()), lay.items[k].host, plane_bytes);  // the padding's bytes
    }
    // the kernel's part: the window's pixels of every staged plane, not the padding columns
    for (int k = 0; k < lay.count; k++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const int px[4] = {lay.items[k].slot, k, y, x};
                memcpy((char*)lay.plane(k, stage.data()) + ((size_t)y * stride + x) * 16, px, 16);
            }
    for (int k = 0; k < lay.count; k++) memcpy(lay.items[k].host, lay.plane(k, stage.data()), plane_bytes);
    for (int slot = 0; slot < (int)planes.v.size(); slot++) {
        const int* a = planes.v[slot].data();
        if (requested >> slot & 1) {
            bool own = true, padding = true;
            for (int y = 0; y < h; y++)
                for (int x = 0; x < stride; x++) {
                    const int* px = a + ((size_t)y * stride + x) * 4;
                    if (x < w) own = own && px[0] == slot && px[2] == y && px[3] == x;
                    else padding = padding && px[0] == marker && px[1] == marker && px[2] == marker && px[3] == marker;
                }
            expect(own, who, mask, n);
            expect(padding, "padding columns keep the caller's bytes", mask, n);
        } else {
            bool untouched = true;
            for (size_t i = 0; i < plane_words; i++) untouched = untouched && a[i] == marker;
            expect(untouched, "an unrequested plane is untouched", mask, n);
        }
    }
}

// yrt_render_mattes: its refusals, and its list (slot 4 key + 2 layer + coverage)
void check_mattes() {
    int accepted = 0, refused = 0;
    for (int mem = -1; mem <= 2; mem++)
        for (unsigned mask = 0; mask < 20; mask++)
            for (int layers = -1; layers <= 4; layers++) {
                caller_planes mem_planes(2 * YRT_MATTE_KEY_COUNT * YRT_MATTE_LAYERS_MAX);
                yrt_matte_planes planes = {};
                for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++)
                    for (int l = 0; l < YRT_MATTE_LAYERS_MAX; l++) {
                        planes.ids[k][l] = mem_planes.at<int>(4 * k + 2 * l);
                        planes.coverage[k][l] = mem_planes.at<float>(4 * k + 2 * l + 1);
                    }
                const bool good = mask >= 1 && mask < 8 && (layers == 1 || layers == 2) && (mem == 0 || mem == 1);
                const char* err = yrt::matte_args_error(mask, layers, &planes, mem);
                expect((err == nullptr) == good, "accepted and refused arguments", mask, layers);
                expect(yrt::matte_args_error(mask, layers, nullptr, mem) != nullptr, "null planes refused", mask, layers);
                if (!good) {
                    refused++;
                    continue;
                }
                accepted++;
                // a requested plane that is null is refused, an unrequested one may be null
                unsigned requested = 0;
                for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++)
                    for (int l = 0; l < YRT_MATTE_LAYERS_MAX; l++)
                        for (int c = 0; c < 2; c++) {
                            yrt_matte_planes holed = planes;
                            if (c) holed.coverage[k][l] = nullptr;
                            else holed.ids[k][l] = nullptr;
                            const bool req = (mask >> k & 1) && l < layers;
                            expect((yrt::matte_args_error(mask, layers, &holed, mem) != nullptr) == req,
                                   "a null plane is refused exactly when it is requested", mask, layers);
                            if (req) requested |= 1u << (4 * k + 2 * l + c);
                        }
                expect(__builtin_popcount(requested) == 2 * layers * __builtin_popcount(mask),
                       "ids and coverage per key and layer", mask, layers);
                round_trip(yrt::matte_plane_list(mask, layers, planes, plane_bytes), mem_planes, requested,
                           "the ids and coverage planes came back to their owners", mask, layers);
            }
    expect(accepted == 7 * 2 * 2 && refused > 0, "every matte combination was visited", 0, 0);
    printf("mattes: %d accepted and %d refused argument sets\n", accepted, refused);
}

// yrt_render_aovs: every non-zero mask (slot YRT_AOV_x)
void check_aovs() {
    for (unsigned mask = 1; mask < 1u << YRT_AOV_COUNT; mask++) {
        caller_planes mem_planes(YRT_AOV_COUNT);
        yrt_aov_planes planes = {};
        for (int k = 0; k < YRT_AOV_COUNT; k++) planes.plane[k] = mem_planes.at<void>(k);
        round_trip(yrt::aov_plane_list(mask, planes, plane_bytes), mem_planes, mask, "the AOV came back to its plane", mask,
                   0);
    }
}

// yrt_render_passes: every non-zero mask, with and without a beauty (slot YRT_PASS_x, the beauty YRT_PASS_COUNT)
void check_passes() {
    for (unsigned mask = 1; mask < 1u << YRT_PASS_COUNT; mask++)
        for (int beauty = 0; beauty < 2; beauty++) {
            caller_planes mem_planes(YRT_PASS_COUNT + 1);
            yrt_pass_planes planes = {};
            for (int k = 0; k < YRT_PASS_COUNT; k++) planes.plane[k] = mem_planes.at<float>(k);
            float* const b = beauty ? mem_planes.at<float>(YRT_PASS_COUNT) : nullptr;
            round_trip(yrt::pass_plane_list(mask, planes, b, plane_bytes), mem_planes,
                       mask | (beauty ? 1u << YRT_PASS_COUNT : 0), "the pass came back to its plane", mask, beauty);
        }
}

// yrt_render_light_groups: 1 to 8 groups, with and without the ambient and the beauty (slot g,
// then YRT_LIGHT_GROUPS_MAX and YRT_LIGHT_GROUPS_MAX + 1); the planes of groups past ngroups
// are the caller's own business even when they are not null
void check_light_groups() {
    for (int ngroups = 1; ngroups <= YRT_LIGHT_GROUPS_MAX; ngroups++)
        for (unsigned extra = 0; extra < 4; extra++) {
            caller_planes mem_planes(YRT_LIGHT_GROUPS_MAX + 2);
            yrt_light_group_planes planes = {};
            for (int g = 0; g < YRT_LIGHT_GROUPS_MAX; g++) planes.group[g] = mem_planes.at<float>(g);
            if (extra & 1) planes.ambient = mem_planes.at<float>(YRT_LIGHT_GROUPS_MAX);
            if (extra & 2) planes.beauty = mem_planes.at<float>(YRT_LIGHT_GROUPS_MAX + 1);
            const unsigned requested = ((1u << ngroups) - 1) | extra << YRT_LIGHT_GROUPS_MAX;
            round_trip(yrt::light_group_plane_list(ngroups, planes, plane_bytes), mem_planes, requested,
                       "the light group came back to its plane", extra, ngroups);
        }
}

// yrt_render_adaptive: the image (slot 0, 16 B per pixel), then the byte mask when given (slot 1,
// 1 B per pixel of the same rows and stride): two planes of different sizes in one staging
void check_adaptive() {
    const size_t pixels = (size_t)stride * h;
    for (int with_mask = 0; with_mask < 2; with_mask++) {
        std::vector<float> img(pixels * 4, (float)marker);
        std::vector<unsigned char> mask(pixels, (unsigned char)marker);
        const yrt::plane_list lay = yrt::adaptive_plane_list(img.data(), with_mask ? mask.data() : nullptr, pixels);
        expect(lay.count == 1 + with_mask && lay.bytes == pixels * 16 + (with_mask ? pixels : 0),
               "the image and the mask in one staging", 0, with_mask);
        expect(lay.items[0].slot == 0 && lay.items[0].offset == 0 && lay.items[0].bytes == pixels * 16,
               "the image leads", 0, with_mask);
        if (with_mask)
            expect(lay.items[1].slot == 1 && lay.items[1].offset == pixels * 16 && lay.items[1].bytes == pixels,
                   "the mask follows the image, one byte per pixel", 0, with_mask);
        std::vector<char> stage(lay.bytes);
        for (int k = 0; k < lay.count; k++) memcpy(lay.plane(k, stage.data()), lay.items[k].host, lay.items[k].bytes);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const float px[4] = {(float)y, (float)x, 0.0f, 1.0f};
                memcpy((char*)lay.plane(0, stage.data()) + ((size_t)y * stride + x) * 16, px, 16);
                if (with_mask) ((unsigned char*)lay.plane(1, stage.data()))[(size_t)y * stride + x] = (unsigned char)(y ^ x);
            }
        for (int k = 0; k < lay.count; k++) memcpy(lay.items[k].host, lay.plane(k, stage.data()), lay.items[k].bytes);
        bool own = true, padding = true;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < stride; x++) {
                const float* px = &img[((size_t)y * stride + x) * 4];
                const unsigned char m = mask[(size_t)y * stride + x];
                if (x < w) own = own && px[0] == (float)y && px[1] == (float)x && (m == (with_mask ? (y ^ x) : marker));
                else padding = padding && px[0] == (float)marker && px[3] == (float)marker && m == marker;
            }
        expect(own, "the image and the mask came back to their owners", 0, with_mask);
        expect(padding, "padding columns keep the caller's bytes", 0, with_mask);
    }
}

}  // namespace

int main() {
    check_mattes();
    check_aovs();
    check_passes();
    check_light_groups();
    check_adaptive();
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
