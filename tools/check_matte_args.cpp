// check_matte_args -- the host-side argument handling and plane staging of yrt_render_mattes
// (csrc/matte_args.h) as a stand-alone program, for the host sanitizers:
//
//     clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -Iinclude tools/check_matte_args.cpp -o check_matte_args && ./check_matte_args
//
// It walks every key mask and layer count, accepted and refused, and for each accepted one
// does what the entry point does with host planes: lays the requested planes out in one
// staging buffer, copies the caller's bytes in, fills every staged plane, copies back, and
// checks that exactly the requested planes changed and that nothing was written past an end.
// No GPU and no HIP runtime: memcpy stands in for the copies. Exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yocto_raytracing_amd/csrc/matte_args.h"

namespace {

int failures = 0;
void expect(bool ok, const char* what, unsigned mask, int layers) {
    if (ok) return;
    fprintf(stderr, "FAILED: %s (mask %u, layers %d)\n", what, mask, layers);
    failures++;
}

}  // namespace

int main() {
    const int w = 5, h = 3, stride = 7;
    const size_t plane_bytes = (size_t)stride * h * 16, plane_words = plane_bytes / 4;
    int accepted = 0, refused = 0;
    for (int mem = -1; mem <= 2; mem++)
        for (unsigned mask = 0; mask < 20; mask++)
            for (int layers = -1; layers <= 4; layers++) {
                // exactly sized heap planes, so that the sanitizer sees any access past an end
                std::vector<std::vector<int>> ids(YRT_MATTE_KEY_COUNT * YRT_MATTE_LAYERS_MAX);
                std::vector<std::vector<float>> cov(YRT_MATTE_KEY_COUNT * YRT_MATTE_LAYERS_MAX);
                yrt_matte_planes planes = {};
                for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++)
                    for (int l = 0; l < YRT_MATTE_LAYERS_MAX; l++) {
                        ids[k * 2 + l].assign(plane_words, 77);
                        cov[k * 2 + l].assign(plane_words, 77.0f);
                        planes.ids[k][l] = ids[k * 2 + l].data();
                        planes.coverage[k][l] = cov[k * 2 + l].data();
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
                for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++)
                    for (int l = 0; l < YRT_MATTE_LAYERS_MAX; l++)
                        for (int c = 0; c < 2; c++) {
                            yrt_matte_planes holed = planes;
                            if (c) holed.coverage[k][l] = nullptr;
                            else holed.ids[k][l] = nullptr;
                            const bool requested = (mask >> k & 1) && l < layers;
                            expect((yrt::matte_args_error(mask, layers, &holed, mem) != nullptr) == requested,
                                   "a null plane is refused exactly when it is requested", mask, layers);
                        }
                // the staging of a call with host planes
                const yrt::matte_staging lay = yrt::matte_stage_layout(mask, layers, planes, plane_bytes);
                const int want = 2 * layers * __builtin_popcount(mask);
                expect(lay.count == want && lay.bytes == plane_bytes * want, "one staged plane per requested plane", mask,
                       layers);
                std::vector<char> stage(lay.bytes);
                for (int k = 0; k < lay.count; k++) {
                    expect(lay.items[k].offset == plane_bytes * k, "planes lie one after the other", mask, layers);
                    memcpy(stage.data() + lay.items[k].offset, lay.items[k].host, plane_bytes);  // the padding's bytes
                }
                // the kernel's part: the window's pixels of every staged plane, not the padding columns
                for (int k = 0; k < lay.count; k++)
                    for (int y = 0; y < h; y++)
                        for (int x = 0; x < w; x++) {
                            const int v[4] = {lay.items[k].key, lay.items[k].layer, lay.items[k].coverage, k};
                            memcpy(stage.data() + lay.items[k].offset + ((size_t)y * stride + x) * 16, v, 16);
                        }
                for (int k = 0; k < lay.count; k++) memcpy(lay.items[k].host, stage.data() + lay.items[k].offset, plane_bytes);
                for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++)
                    for (int l = 0; l < YRT_MATTE_LAYERS_MAX; l++) {
                        const bool requested = (mask >> k & 1) && l < layers;
                        const int* a = ids[k * 2 + l].data();
                        int c0[4], c1[4];
                        memcpy(c0, cov[k * 2 + l].data(), 16);
                        memcpy(c1, (const char*)cov[k * 2 + l].data() + (size_t)w * 16, 16);  // a padding pixel
                        if (requested) {
                            expect(a[0] == k && a[1] == l && a[2] == 0, "the ids plane came back to its owner", mask, layers);
                            expect(c0[0] == k && c0[1] == l && c0[2] == 1, "the coverage plane came back to its owner", mask,
                                   layers);
                            expect(a[w * 4] == 77, "padding columns keep the caller's bytes", mask, layers);
                            float pad;
                            memcpy(&pad, c1, 4);
                            expect(pad == 77.0f, "padding columns keep the caller's bytes", mask, layers);
                        } else {
                            bool untouched = true;
                            for (size_t i = 0; i < plane_words; i++)
                                untouched = untouched && a[i] == 77 && cov[k * 2 + l][i] == 77.0f;
                            expect(untouched, "an unrequested plane is untouched", mask, layers);
                        }
                    }
            }
    expect(accepted == 7 * 2 * 2 && refused > 0, "every combination was visited", 0, 0);
    if (failures) return 1;
    printf("ok: %d accepted and %d refused argument sets\n", accepted, refused);
    return 0;
}
