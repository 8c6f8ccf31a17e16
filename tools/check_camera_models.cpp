// check_camera_models -- the camera models' ray formulas (csrc/camera_models.h), the argument
// handling of yrt_render_camera and yrt_camera_rays (csrc/camera_args.h) and the tables' header
// (csrc/ao_tables.h) as a stand-alone program, for the host compiler and the host sanitizers:
//
//     CXXFLAGS="-std=c++17 -g -ffp-contract=off -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all"
//     c++ $CXXFLAGS tools/check_camera_models.cpp -o check_camera_models && ./check_camera_models
//
// Without arguments it checks which arguments are refused, what camera_resolve hands the kernel,
// and properties of the rays that hold whatever the camera: unit directions, the pinhole at
// aperture 0, lens origins within the lens, all lens rays of a pixel's sample meeting at the
// focal plane, the panorama's landmarks. Exit status 0 and "ok" on success.
//
// With arguments it writes the rays of one camera for a small frame to a binary file, for
// tests/test_camera_api.py to compare with the numpy model (tests/camera_model.py):
//
//     check_camera_models rays OUT MODEL APERTURE W H NS  fx fy fz .. (12 floats: x, y, z, o)  FOVY ASPECT FOCUS
//
// OUT receives H * W * NS * NS records of 8 float32 {o.xyz, d.xyz, tmin, tmax} in the order
// (j, i, jj, ii). The floats are given as hexadecimal bit patterns (8 digits), so that no
// decimal conversion stands between the test's camera and this one. make_dev_camera's
// arithmetic (csrc/device_scene.cpp) is repeated here: h = 2 * focus * tanf(fovy / 2), w = h * aspect.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../yocto_raytracing_amd/csrc/ao_tables.h"
#include "../yocto_raytracing_amd/csrc/camera_args.h"
#include "../yocto_raytracing_amd/csrc/camera_models.h"

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

// make_dev_camera (device_scene.cpp) of a frame {x, y, z, o}, fovy, aspect and focus
yrt::dev_camera dev_camera_of(const float f[12], float fovy, float aspect, float focus) {
    yrt::dev_camera d;
    d.xx = f[0], d.xy = f[1], d.xz = f[2];
    d.yx = f[3] * -1, d.yy = f[4] * -1, d.yz = f[5] * -1;
    d.zx = f[6], d.zy = f[7], d.zz = f[8];
    d.ox = f[9], d.oy = f[10], d.oz = f[11];
    d.h = 2.0f * focus * std::tan(fovy / 2.0f);
    d.w = d.h * aspect;
    d.focus = focus;
    return d;
}

yrt::camera_model_ray eval(int model, const yrt::dev_camera& cam, float aperture, int W, int H, int ns, int i, int j, int q) {
    if (model == yrt::camera_orthographic)
        return yrt::camera_model_eval<yrt::camera_orthographic>(cam, aperture, dirs, rots, W, H, ns, i, j, q);
    if (model == yrt::camera_equirect)
        return yrt::camera_model_eval<yrt::camera_equirect>(cam, aperture, dirs, rots, W, H, ns, i, j, q);
    return yrt::camera_model_eval<yrt::camera_perspective>(cam, aperture, dirs, rots, W, H, ns, i, j, q);
}

bool refused(int model, float aperture, float focus, int chunk, int mem = YRT_MEM_HOST) {
    float px[8];
    const yrt_camera_model m = {model, aperture, focus, chunk};
    return yrt::camera_args_error(&m, px, mem) != nullptr;
}

float bits_float(const char* hex) {
    const uint32_t u = (uint32_t)strtoul(hex, nullptr, 16);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int write_rays(int argc, char** argv) {
    if (argc != 23) {
        fprintf(stderr, "usage: check_camera_models rays OUT MODEL APERTURE W H NS <12 frame floats> FOVY ASPECT FOCUS\n");
        return 2;
    }
    const int model = atoi(argv[3]), W = atoi(argv[5]), H = atoi(argv[6]), ns = atoi(argv[7]);
    const float aperture = bits_float(argv[4]);
    float f[12];
    for (int k = 0; k < 12; k++) f[k] = bits_float(argv[8 + k]);
    if (model < 0 || model >= yrt::camera_model_count || W < 1 || H < 1 || ns < 1 || W > 4096 || H > 4096 || ns > 64) return 2;
    const yrt::dev_camera cam = dev_camera_of(f, bits_float(argv[20]), bits_float(argv[21]), bits_float(argv[22]));
    std::vector<float> out;
    out.reserve((size_t)W * H * ns * ns * 8);
    for (int j = 0; j < H; j++)
        for (int i = 0; i < W; i++)
            for (int q = 0; q < ns * ns; q++) {
                const yrt::camera_model_ray r = eval(model, cam, aperture, W, H, ns, i, j, q);
                const float rec[8] = {r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z, r.tmin, r.tmax};
                out.insert(out.end(), rec, rec + 8);
            }
    FILE* fp = fopen(argv[2], "wb");
    const bool ok = fp && fwrite(out.data(), 4, out.size(), fp) == out.size();
    if ((fp && fclose(fp) != 0) || !ok) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    return 0;
}

double len3(yrt::vec3f a) { return std::sqrt((double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z); }

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "rays") == 0) return write_rays(argc, argv);
    if (argc > 1) return 2;

    // ---- the argument rules ----
    for (int model = -2; model <= 4; model++)
        expect(refused(model, 0.0f, 0.0f, 0) == !(model >= 0 && model <= 2), "a model within 0..2", model);
    expect(refused(0, nan_, 0.0f, 0) && refused(0, inf, 0.0f, 0) && refused(0, -inf, 0.0f, 0), "a NaN or infinite aperture is refused");
    expect(refused(1, 0.0f, nan_, 0) && refused(2, 0.0f, inf, 0) && refused(0, 0.0f, -inf, 0), "a NaN or infinite focus is refused");
    expect(!refused(0, -1.0f, 0.0f, 0) && !refused(0, 0.0f, -3.0f, 0) && !refused(0, FLT_MAX, FLT_MAX, 0) &&
               !refused(0, -0.0f, -0.0f, 0),
           "finite apertures and focuses are taken");
    expect(refused(0, 0.0f, 0.0f, -1) && !refused(0, 0.0f, 0.0f, 0) && !refused(0, 0.0f, 0.0f, 1 << 30), "chunk_pixels >= 0");
    expect(!refused(0, 0.0f, 0.0f, 0, YRT_MEM_DEVICE) && refused(0, 0.0f, 0.0f, 0, 2) && refused(0, 0.0f, 0.0f, 0, -1), "mem");
    {
        float px[8];
        const yrt_camera_model m = {0, 0.0f, 0.0f, 0};
        expect(yrt::camera_args_error(nullptr, px, YRT_MEM_HOST) && yrt::camera_args_error(&m, nullptr, YRT_MEM_HOST) &&
                   !yrt::camera_args_error(&m, px, YRT_MEM_HOST),
               "a null model or out is refused");
    }
    // the defaults: aperture < 0 and focus <= 0 are the scene camera's; only PERSPECTIVE has a lens
    {
        const yrt::camera_resolved a = yrt::camera_resolve({0, -1.0f, 0.0f, 0}, 0.25f, 3.0f);
        expect(a.model == 0 && a.aperture == 0.25f && a.focus == 3.0f, "the scene camera's aperture and focus");
        const yrt::camera_resolved b = yrt::camera_resolve({0, 0.5f, 2.0f, 0}, 0.25f, 3.0f);
        expect(b.aperture == 0.5f && b.focus == 2.0f, "the caller's aperture and focus");
        const yrt::camera_resolved c = yrt::camera_resolve({0, 0.0f, -2.0f, 0}, 0.25f, 3.0f);
        expect(c.aperture == 0.0f && c.focus == 3.0f, "aperture 0 is the pinhole, a negative focus the scene's");
        const yrt::camera_resolved d = yrt::camera_resolve({0, -0.0f, 1.5f, 0}, 0.25f, 3.0f);
        expect(d.aperture == 0.0f && d.focus == 1.5f, "aperture -0 is the pinhole");
        for (int model = 1; model <= 2; model++) {
            const yrt::camera_resolved e = yrt::camera_resolve({model, 0.5f, 2.0f, 0}, 0.25f, 3.0f);
            expect(e.model == model && e.aperture == 0.0f && e.focus == 2.0f, "no lens outside PERSPECTIVE", model);
        }
    }
    expect(sizeof dirs == sizeof(float) * 3 * yrt::ao_dir_count && sizeof rots == sizeof(float) * 2 * yrt::ao_rot_count,
           "the tables' sizes");

    // ---- the rays: a rotated camera off the origin ----
    const float sq = std::sqrt(0.5f);
    const float frame[12] = {sq, 0.0f, -sq, 0.0f, 1.0f, 0.0f, sq, 0.0f, sq, 1.0f, 2.0f, 3.0f};
    const float focus = 3.0f, A = 0.3f;
    const yrt::dev_camera cam = dev_camera_of(frame, 0.9f, 1.5f, focus);
    const int W = 9, H = 6, ns = 9;  // q >= 64: the rotation changes within a pixel
    const yrt::vec3f o = {cam.ox, cam.oy, cam.oz}, z = {cam.zx, cam.zy, cam.zz};
    for (int j = 0; j < H; j++)
        for (int i = 0; i < W; i++)
            for (int q = 0; q < ns * ns; q++) {
                const int at = (j * W + i) * ns * ns + q;
                const yrt::camera_model_ray pin = eval(0, cam, 0.0f, W, H, ns, i, j, q);
                const yrt::camera_model_ray neg = eval(0, cam, -0.0f, W, H, ns, i, j, q);
                const yrt::camera_model_ray lens = eval(0, cam, A, W, H, ns, i, j, q);
                const yrt::camera_model_ray orth = eval(1, cam, A, W, H, ns, i, j, q);
                const yrt::camera_model_ray pano = eval(2, cam, A, W, H, ns, i, j, q);
                expect(memcmp(&pin.o, &o, 12) == 0 && memcmp(&pin, &neg, sizeof pin) == 0, "the pinhole starts at o", at);
                expect(memcmp(&pano.o, &o, 12) == 0, "the panorama starts at o", at);
                for (const yrt::camera_model_ray* r : {&pin, &lens, &orth, &pano})
                    expect(std::fabs(len3(r->d) - 1.0) < 1e-6 && r->tmin == yrt::ray_eps && r->tmax == yrt::flt_max,
                           "a unit direction, tmin and tmax", at);
                // the lens: within its radius, in the plane through o across z, aimed at the
                // pinhole ray's point of the focal plane
                const yrt::vec3f le = lens.o - o;
                expect(len3(le) <= 0.5 * A * (1 + 1e-6) && std::fabs(yrt::dot(le, z)) < 1e-6, "a point of the lens", at);
                const double tp = focus / -(double)yrt::dot(pin.d, z), tl = focus / -(double)yrt::dot(lens.d, z);
                const yrt::vec3f P = {(float)(pin.o.x + tp * pin.d.x), (float)(pin.o.y + tp * pin.d.y), (float)(pin.o.z + tp * pin.d.z)};
                const yrt::vec3f L = {(float)(lens.o.x + tl * lens.d.x), (float)(lens.o.y + tl * lens.d.y),
                                      (float)(lens.o.z + tl * lens.d.z)};
                expect(len3(P - L) < 1e-5, "the lens ray meets the pinhole ray at the focal plane", at);
                // the orthographic ray: along -z from the pinhole ray's point of the focal plane moved back by focus
                expect(len3(orth.d - z * -1.0f) < 1e-6 && len3((orth.o - z * focus) - P) < 1e-5, "the orthographic film", at);
            }
    // the lens points of a pixel's first 64 samples are distinct, and samples q and q + 64 differ by a rotation
    {
        const yrt::camera_model_ray a = eval(0, cam, A, W, H, ns, 2, 3, 5), b = eval(0, cam, A, W, H, ns, 2, 3, 69);
        expect(len3(a.o - b.o) > 1e-4 && std::fabs(len3(a.o - o) - len3(b.o - o)) < 1e-5, "q + 64 rotates the lens point");
    }
    // the panorama's landmarks at one sample per pixel: the pixels nearest the top, the centre
    // and the left and right edges of a 64 x 64 or 64 x 65 frame (v = 0.5 needs an odd height)
    {
        const yrt::vec3f y = {cam.yx, cam.yy, cam.yz};
        const yrt::camera_model_ray top = eval(2, cam, 0.0f, 64, 64, 1, 32, 0, 0), mid = eval(2, cam, 0.0f, 64, 65, 1, 32, 32, 0);
        const yrt::camera_model_ray left = eval(2, cam, 0.0f, 64, 65, 1, 0, 32, 0), right = eval(2, cam, 0.0f, 64, 65, 1, 63, 32, 0);
        expect(yrt::dot(top.d, y) < -0.99f, "the top row looks up (along the frame's +y)");
        expect(yrt::dot(mid.d, z) < -0.99f, "the image centre looks along -z");
        expect(yrt::dot(left.d, z) > 0.99f && yrt::dot(right.d, z) > 0.99f, "the left and right edges look along +z");
        expect(yrt::dot(left.d, {cam.xx, cam.xy, cam.xz}) < 0.0f && yrt::dot(right.d, {cam.xx, cam.xy, cam.xz}) > 0.0f,
               "the left edge turns to -x, the right edge to +x");
    }
    if (failures) return 1;
    puts("ok");
    return 0;
}
