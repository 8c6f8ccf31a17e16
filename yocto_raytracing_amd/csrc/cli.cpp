// yrt_raytrace -- drop-in for the reference's bin/raytrace (main, src/raytrace.cpp:256-287):
//
//     yrt_raytrace [-r RES] [-s SAMPLES] [-a AMBIENT] [-o OUT.png|OUT.hdr] scene.obj
//
// same options, defaults (720, 1, 0.1, out.png), messages and output file as the
// reference, over the C++ mirror in include/yrt_raytrace.hpp. Extra options (not in
// the reference): --device N, --width W, --max-depth D, --algorithm
// wavefront|megakernel|wavefront_lane, --time (print GPU time and Mrays/s), --aov LIST
// (the camera hit's geometry buffers as .npy files beside the image), --passes LIST (the
// image's lighting split, from the same render, as .npy files beside it), --light-groups LIST
// (one plane per group of lights and the ambient plane, from the same render, as .npy files),
// --mattes LIST with --matte-ranks 4|8 (ID mattes: per key the ranked ids covering each pixel and
// their coverages, from one pass, as .npy files), --adaptive THRESHOLD with --base-samples N (the
// image with adaptive supersampling, and the refined pixels' mask as a .npy file),
// --ao K[,DISTANCE[,BIAS]] (the ambient occlusion plane as a .npy file), --camera-model
// perspective|orthographic|equirect with --aperture A and --focus F (the image under another
// camera model: a thin lens, an orthographic film, a panorama), --soft-shadows R[,K] (the image
// with every light a disk of radius R, K shadow rays per light).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "yrt_raytrace.hpp"

namespace {

[[noreturn]] void usage(const char* msg) {
    if (msg) fprintf(stderr, "error: %s\n", msg);
    fprintf(stderr,
            "usage: yrt_raytrace [options] scenein\n"
            "  -r, --resolution N   vertical resolution [720]\n"
            "  -s, --samples N      per-pixel samples per axis (N*N rays per pixel) [1]\n"
            "  -a, --ambient F      ambient color [0.1]\n"
            "  -o, --output FILE    output image (.png tonemapped, .hdr float) [out.png]\n"
            "  --device N           GPU index [0]\n"
            "  --gpus N             split the frame over N GPUs from --device on [1]\n"
            "  --width N            explicit width (default round(aspect * resolution))\n"
            "  --max-depth N        cap on reflection depth [16]\n"
            "  --algorithm NAME     wavefront | megakernel | wavefront_lane [wavefront]\n"
            "  --time               print render time and Mrays/s\n"
            "  --aov LIST           also write OUT.<name>.npy, (H, W, 4) float32 (ids: int32), for each of\n"
            "                       depth,position,normal,texcoord,albedo,ids (one GPU)\n"
            "  --passes LIST        also write OUT.<name>.npy, (H, W, 4) float32, for each of\n"
            "                       direct,diffuse,specular,reflection,ambient, from the image's own render\n"
            "                       (one GPU, a wavefront algorithm)\n"
            "  --light-groups LIST  one entry per light of the scene, in scene order: its group, 0 to 7, or -1\n"
            "                       for none, e.g. 0,1,0,-1,2; also write OUT.group<g>.npy per group (the image\n"
            "                       its lights alone produce) and OUT.ambient.npy, (H, W, 4) float32, from the\n"
            "                       image's own render (one GPU, a wavefront algorithm)\n"
            "  --mattes LIST        also write OUT.matte_<key>.ids.npy, (H, W, ranks) int32, and\n"
            "                       OUT.matte_<key>.coverage.npy, (H, W, ranks) float32, for each key of\n"
            "                       instance,material,shape: per pixel the ids covering it, ranked by their\n"
            "                       share of the pixel's samples (-1 and 0 in unused ranks), from one pass\n"
            "                       (one GPU)\n"
            "  --matte-ranks N      ranks per pixel and key of --mattes, 4 or 8 [4]\n"
            "  --adaptive F         adaptive supersampling: --base-samples per axis in every pixel, -s per axis\n"
            "                       only where a pixel differs from a neighbour by more than F in a channel;\n"
            "                       prints the refined pixels and also writes OUT.refined.npy, (H, W) uint8\n"
            "                       (one GPU, a wavefront algorithm)\n"
            "  --base-samples N     samples per axis of --adaptive's base frame [1]\n"
            "  --ao K[,DIST[,BIAS]] also write OUT.ao.npy, (H, W, 4) float32 {a, a, a, coverage}: a the share of K\n"
            "                       (1 to 64) cosine-weighted rays per camera sample, from BIAS [0.01] to DIST\n"
            "                       [unbounded], that nothing occludes, times the coverage (one GPU)\n"
            "  --camera-model NAME  perspective | orthographic | equirect: render the image under this camera\n"
            "                       model, its rays generated on the GPU (one GPU, a wavefront algorithm);\n"
            "                       perspective is a thin lens with the scene camera's aperture and focus,\n"
            "                       equirect the 360 x 180 degree panorama (give --width 2 * -r)\n"
            "  --aperture A         lens diameter of the perspective model, 0 for the pinhole [the camera's]\n"
            "  --focus F            focus distance of the perspective and orthographic models [the camera's]\n"
            "  --soft-shadows R[,K] render the image with soft shadows: every light a disk of radius R that faces\n"
            "                       the shaded point, K (1 to 64) [16] shadow rays per light; R = 0 is the image\n"
            "                       itself; combines with --camera-model, --aperture and --focus (one GPU, a\n"
            "                       wavefront algorithm)\n");
    exit(msg ? 1 : 0);
}

int parse_int(const char* s, const char* opt) {
    char* end = nullptr;
    long v = strtol(s, &end, 10);
    if (!*s || *end) usage((std::string("bad value for ") + opt).c_str());
    return (int)v;
}

// the names of --aov, --mattes and --passes, in the order of YRT_AOV_*, YRT_MATTE_* and YRT_PASS_*
const char* const aov_names[YRT_AOV_COUNT] = {"depth", "position", "normal", "texcoord", "albedo", "ids"};
const char* const matte_names[YRT_MATTE_KEY_COUNT] = {"instance", "material", "shape"};
const char* const pass_names[YRT_PASS_COUNT] = {"direct", "diffuse", "specular", "reflection", "ambient"};

// option `opt`'s comma-separated names as the bit mask of their places in `names`
unsigned parse_names(const std::string& list, const char* const* names, int count, const char* opt) {
    unsigned mask = 0;
    for (size_t at = 0; at <= list.size();) {
        size_t end = list.find(',', at);
        if (end == std::string::npos) end = list.size();
        const std::string name = list.substr(at, end - at);
        int k = 0;
        while (k < count && name != names[k]) k++;
        if (k == count) usage((std::string("unknown ") + opt + " " + name).c_str());
        mask |= 1u << k;
        at = end + 1;
    }
    return mask;
}

// --ao's K[,distance[,bias]] over the defaults of yrt_ao_params_default
yrt_ao_params parse_ao(const std::string& list) {
    yrt_ao_params ao;
    yrt_ao_params_default(&ao);
    int field = 0;
    for (size_t at = 0; at <= list.size(); field++) {
        size_t end = list.find(',', at);
        if (end == std::string::npos) end = list.size();
        const std::string item = list.substr(at, end - at);
        char* stop = nullptr;
        if (field == 0) ao.rays = (int)strtol(item.c_str(), &stop, 10);
        else if (field == 1) ao.distance = strtof(item.c_str(), &stop);
        else if (field == 2) ao.bias = strtof(item.c_str(), &stop);
        if (field > 2 || item.empty() || *stop) usage("--ao takes K[,DISTANCE[,BIAS]]");
        at = end + 1;
    }
    if (ao.rays < 1 || ao.rays > YRT_AO_RAYS_MAX) usage("--ao: K must be from 1 to 64");
    return ao;
}

// --soft-shadows' R[,K] over the defaults of yrt_soft_shadow_params_default
yrt_soft_shadow_params parse_soft(const std::string& list) {
    yrt_soft_shadow_params sp;
    yrt_soft_shadow_params_default(&sp);
    int field = 0;
    for (size_t at = 0; at <= list.size(); field++) {
        size_t end = list.find(',', at);
        if (end == std::string::npos) end = list.size();
        const std::string item = list.substr(at, end - at);
        char* stop = nullptr;
        if (field == 0) sp.radius = strtof(item.c_str(), &stop);
        else if (field == 1) sp.rays = (int)strtol(item.c_str(), &stop, 10);
        if (field > 1 || item.empty() || *stop) usage("--soft-shadows takes R[,K]");
        at = end + 1;
    }
    if (!(sp.radius >= 0.0f) || sp.radius > 3.402823466e+38f) usage("--soft-shadows: R must be a finite number >= 0");
    if (sp.rays < 1 || sp.rays > YRT_SOFT_SHADOW_RAYS_MAX) usage("--soft-shadows: K must be from 1 to 64");
    return sp;
}

// --aperture's and --focus' value: a finite number >= 0, > 0 when `open`
float parse_lens(const char* v, const char* opt, bool open) {
    char* end = nullptr;
    const float x = strtof(v, &end);
    if (!*v || *end || !(x >= 0.0f) || x > 3.402823466e+38f || (open && x == 0.0f))
        usage((std::string(opt) + (open ? " takes a finite number > 0" : " takes a finite number >= 0")).c_str());
    return x;
}

// --light-groups' comma-separated group of each light
std::vector<int> parse_light_groups(const std::string& list) {
    std::vector<int> groups;
    for (size_t at = 0; at <= list.size();) {
        size_t end = list.find(',', at);
        if (end == std::string::npos) end = list.size();
        const std::string item = list.substr(at, end - at);
        char* stop = nullptr;
        const long g = strtol(item.c_str(), &stop, 10);
        if (item.empty() || *stop) usage(("bad --light-groups entry '" + item + "'").c_str());
        if (g < -1 || g >= YRT_LIGHT_GROUPS_MAX)
            usage(("--light-groups entry " + item + " is out of range: -1 (no plane) or a group from 0 to 7").c_str());
        groups.push_back((int)g);
        at = end + 1;
    }
    return groups;
}

// a (h, w, channels) array of 4-byte elements -- or, with channels = 0, a (h, w) array of bytes --
// as a NumPy format 1.0 file, C order: the magic, the version, the header dict's length, the
// dict padded with spaces so that the data starts on a multiple of 64 bytes, a newline, the data
void save_npy(const std::string& path, const void* data, int w, int h, const char* descr, int channels = 4) {
    std::string dict = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (" +
                       std::to_string(h) + ", " + std::to_string(w) +
                       (channels ? ", " + std::to_string(channels) : std::string()) + "), }";
    while ((10 + dict.size() + 1) % 64) dict += ' ';
    dict += '\n';
    const unsigned char head[10] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (unsigned char)(dict.size() & 0xff),
                                    (unsigned char)(dict.size() >> 8)};
    FILE* f = fopen(path.c_str(), "wb");
    const size_t bytes = channels ? (size_t)w * h * 4 * channels : (size_t)w * h;
    const bool ok = f && fwrite(head, 1, sizeof head, f) == sizeof head &&
                    fwrite(dict.data(), 1, dict.size(), f) == dict.size() && fwrite(data, 1, bytes, f) == bytes;
    if ((f && fclose(f) != 0) || !ok) throw yrt_cpp::error(YRT_ERR_IO, "cannot write " + path);
}

}  // namespace

int main(int argc, char** argv) {
    int resolution = 720, samples = 1, device = 0, gpus = 1, width = 0, max_depth = 16, algorithm = YRT_ALGO_WAVEFRONT;
    float amb = 0.1f;
    bool timing = false;
    unsigned aovs = 0, passes = 0, mattes = 0;
    int matte_ranks = 4;
    std::vector<int> light_groups;
    bool groups = false, adaptive = false, ao = false;
    yrt_ao_params ao_params = {};
    float threshold = 0.0f;
    int base_samples = 1;
    bool camera = false, aperture_given = false;  // --camera-model, --aperture or --focus: yrt_render_camera
    yrt_camera_model camera_model;
    yrt_camera_model_default(&camera_model);
    bool soft = false;  // --soft-shadows: yrt_render_soft_shadows
    yrt_soft_shadow_params soft_params = {};
    std::string out = "out.png", scenein;
    for (int k = 1; k < argc; k++) {
        std::string a = argv[k];
        auto val = [&]() -> const char* {
            if (k + 1 >= argc) usage(("missing value for " + a).c_str());
            return argv[++k];
        };
        if (a == "-r" || a == "--resolution") resolution = parse_int(val(), "-r");
        else if (a == "-s" || a == "--samples") samples = parse_int(val(), "-s");
        else if (a == "-a" || a == "--ambient") amb = strtof(val(), nullptr);
        else if (a == "-o" || a == "--output") out = val();
        else if (a == "--device") device = parse_int(val(), "--device");
        else if (a == "--gpus") gpus = parse_int(val(), "--gpus");
        else if (a == "--width") width = parse_int(val(), "--width");
        else if (a == "--max-depth") max_depth = parse_int(val(), "--max-depth");
        else if (a == "--algorithm") {
            std::string n = val();
            if (n == "wavefront") algorithm = YRT_ALGO_WAVEFRONT;
            else if (n == "megakernel") algorithm = YRT_ALGO_MEGAKERNEL;
            else if (n == "wavefront_lane") algorithm = YRT_ALGO_WAVEFRONT_LANE;
            else usage("unknown --algorithm");
        } else if (a == "--time") timing = true;
        else if (a == "--aov") aovs = parse_names(val(), aov_names, YRT_AOV_COUNT, "--aov");
        else if (a == "--passes") passes = parse_names(val(), pass_names, YRT_PASS_COUNT, "--passes");
        else if (a == "--mattes") mattes = parse_names(val(), matte_names, YRT_MATTE_KEY_COUNT, "--mattes");
        else if (a == "--matte-ranks") matte_ranks = parse_int(val(), "--matte-ranks");
        else if (a == "--light-groups") light_groups = parse_light_groups(val()), groups = true;
        else if (a == "--adaptive") {
            const char* v = val();
            char* end = nullptr;
            threshold = strtof(v, &end);
            if (!*v || *end || threshold != threshold) usage("bad value for --adaptive");
            adaptive = true;
        } else if (a == "--base-samples") base_samples = parse_int(val(), "--base-samples");
        else if (a == "--ao") ao_params = parse_ao(val()), ao = true;
        else if (a == "--camera-model") {
            std::string n = val();
            if (n == "perspective") camera_model.model = YRT_CAMERA_PERSPECTIVE;
            else if (n == "orthographic") camera_model.model = YRT_CAMERA_ORTHOGRAPHIC;
            else if (n == "equirect") camera_model.model = YRT_CAMERA_EQUIRECT;
            else usage(("unknown --camera-model " + n + ": perspective, orthographic or equirect").c_str());
            camera = true;
        } else if (a == "--aperture") camera_model.aperture = parse_lens(val(), "--aperture", false), camera = aperture_given = true;
        else if (a == "--focus") camera_model.focus = parse_lens(val(), "--focus", true), camera = true;
        else if (a == "--soft-shadows") soft_params = parse_soft(val()), soft = true;
        else if (a == "-h" || a == "--help") usage(nullptr);
        else if (!a.empty() && a[0] == '-') usage(("unknown option " + a).c_str());
        else if (scenein.empty()) scenein = a;
        else usage("too many arguments");
    }
    if (scenein.empty()) scenein = "scene.obj";  // the reference's default positional value
    if (gpus < 1) usage("--gpus must be >= 1");
    if (aovs && gpus > 1) usage("--aov renders on one GPU (--gpus 1)");
    if (mattes && gpus > 1) usage("--mattes renders on one GPU (--gpus 1)");
    if (matte_ranks != 4 && matte_ranks != 8) usage("--matte-ranks must be 4 or 8");
    if (ao && gpus > 1) usage("--ao renders on one GPU (--gpus 1)");
    if (passes && gpus > 1) usage("--passes renders on one GPU (--gpus 1)");
    if (passes && algorithm == YRT_ALGO_MEGAKERNEL) usage("--passes needs a wavefront algorithm, not --algorithm megakernel");
    if (groups && gpus > 1) usage("--light-groups renders on one GPU (--gpus 1)");
    if (groups && algorithm == YRT_ALGO_MEGAKERNEL)
        usage("--light-groups needs a wavefront algorithm, not --algorithm megakernel");
    if (groups && passes) usage("--light-groups and --passes are renders of their own: give one of them");
    if (adaptive && gpus > 1) usage("--adaptive renders on one GPU (--gpus 1)");
    if (adaptive && algorithm == YRT_ALGO_MEGAKERNEL)
        usage("--adaptive needs a wavefront algorithm, not --algorithm megakernel");
    if (adaptive && (passes || groups)) usage("--adaptive renders the image alone: not with --passes or --light-groups");
    if (adaptive && (base_samples < 1 || base_samples > samples)) usage("--base-samples must be from 1 to -s");
    if (camera && gpus > 1) usage("--camera-model, --aperture and --focus render on one GPU (--gpus 1)");
    if (camera && algorithm == YRT_ALGO_MEGAKERNEL)
        usage("--camera-model, --aperture and --focus need a wavefront algorithm, not --algorithm megakernel");
    if (camera && (passes || groups || adaptive))
        usage("--camera-model, --aperture and --focus render the image alone: not with --passes, --light-groups or --adaptive");
    if (aperture_given && camera_model.model != YRT_CAMERA_PERSPECTIVE) usage("--aperture is the perspective model's lens");
    if (soft && gpus > 1) usage("--soft-shadows renders on one GPU (--gpus 1)");
    if (soft && algorithm == YRT_ALGO_MEGAKERNEL)
        usage("--soft-shadows needs a wavefront algorithm, not --algorithm megakernel");
    if (soft && (passes || groups || adaptive))
        usage("--soft-shadows renders the image alone: not with --passes, --light-groups or --adaptive");
    try {
        printf("loading scene %s\n", scenein.c_str());
        auto scn = yrt_cpp::load_scene(scenein);
        if (groups) {
            int nlights = 0;
            yrt_cpp::check(yrt_host_scene_lights(scn->host, nullptr, 0, &nlights), "lights");
            if ((int)light_groups.size() != nlights)
                usage(("--light-groups names " + std::to_string(light_groups.size()) + " lights, the scene has " +
                       std::to_string(nlights)).c_str());
        }
        printf("creating bvh\n");
        yrt_cpp::build_bvh(scn, false);
        scn->device = device;
        scn->gpus = gpus;
        scn->params.width = width;
        scn->params.max_depth = max_depth;
        scn->params.algorithm = algorithm;
        printf("tracing scene\n");
        if (timing) yrt_cpp::raytrace(scn, {amb, amb, amb}, resolution, samples);  // upload + warm up
        const size_t slash = out.find_last_of('/'), dot = out.find_last_of('.');
        const std::string stem =
            dot != std::string::npos && (slash == std::string::npos || dot > slash) ? out.substr(0, dot) : out;
        std::vector<std::vector<float>> pass_data(YRT_PASS_COUNT);
        int ngroups = 1;
        for (int g : light_groups) ngroups = std::max(ngroups, g + 1);
        std::vector<std::vector<float>> group_data(groups ? ngroups + 1 : 0);  // the groups, then the ambient
        auto t0 = std::chrono::steady_clock::now();
        yrt_cpp::image4f hdr;
        std::vector<unsigned char> refined;  // --adaptive's mask
        if (passes) {
            // one render: the image and its passes in host memory
            yrt_render_params p = scn->params;
            p.ambient[0] = p.ambient[1] = p.ambient[2] = amb;
            p.resolution = resolution;
            p.samples = samples;
            int w = 0, h = 0;
            yrt_cpp::check(yrt_image_size(scn->on_device(), &p, &w, &h), "raytrace");
            hdr = yrt_cpp::image4f(w, h);
            yrt_pass_planes pp = {};
            for (int k = 0; k < YRT_PASS_COUNT; k++)
                if (passes >> k & 1) {
                    pass_data[k].resize((size_t)w * h * 4);
                    pp.plane[k] = pass_data[k].data();
                }
            yrt_cpp::check(yrt_render_passes(scn->on_device(), &p, passes, &pp, &hdr.pixels[0].x, YRT_MEM_HOST, nullptr),
                           "render_passes");
        } else if (groups) {
            // one render: the image, its light groups and the ambient plane in host memory
            yrt_render_params p = scn->params;
            p.ambient[0] = p.ambient[1] = p.ambient[2] = amb;
            p.resolution = resolution;
            p.samples = samples;
            int w = 0, h = 0;
            yrt_cpp::check(yrt_image_size(scn->on_device(), &p, &w, &h), "raytrace");
            hdr = yrt_cpp::image4f(w, h);
            yrt_light_group_planes lp = {};
            for (auto& d : group_data) d.resize((size_t)w * h * 4);
            for (int g = 0; g < ngroups; g++) lp.group[g] = group_data[g].data();
            lp.ambient = group_data[ngroups].data();
            lp.beauty = &hdr.pixels[0].x;
            const int none = -1;  // (a scene without lights: the list is empty, the pointer still given)
            yrt_cpp::check(yrt_render_light_groups(scn->on_device(), &p, light_groups.empty() ? &none : light_groups.data(),
                                                   (int)light_groups.size(), ngroups, &lp, YRT_MEM_HOST, nullptr),
                           "render_light_groups");
        } else if (adaptive) {
            hdr = yrt_cpp::raytrace_adaptive(scn, {amb, amb, amb}, resolution, samples, threshold, base_samples, &refined);
            const unsigned long long n = yrt_cpp::adaptive_refined(scn);
            printf("adaptive: refined %llu of %llu pixels (%.1f %%)\n", n, (unsigned long long)refined.size(),
                   refined.empty() ? 0.0 : 100.0 * (double)n / (double)refined.size());
        } else if (soft) {
            // the image with soft shadows, under the camera model where one is given (else the
            // pinhole), in host memory
            yrt_render_params p = scn->params;
            p.ambient[0] = p.ambient[1] = p.ambient[2] = amb;
            p.resolution = resolution;
            p.samples = samples;
            int w = 0, h = 0;
            yrt_cpp::check(yrt_image_size(scn->on_device(), &p, &w, &h), "raytrace");
            hdr = yrt_cpp::image4f(w, h);
            yrt_cpp::check(yrt_render_soft_shadows(scn->on_device(), &p, camera ? &camera_model : nullptr, &soft_params,
                                                   &hdr.pixels[0].x, YRT_MEM_HOST, nullptr),
                           "render_soft_shadows");
        } else if (camera) {
            // the image under the camera model, in host memory
            yrt_render_params p = scn->params;
            p.ambient[0] = p.ambient[1] = p.ambient[2] = amb;
            p.resolution = resolution;
            p.samples = samples;
            int w = 0, h = 0;
            yrt_cpp::check(yrt_image_size(scn->on_device(), &p, &w, &h), "raytrace");
            hdr = yrt_cpp::image4f(w, h);
            yrt_cpp::check(yrt_render_camera(scn->on_device(), &p, &camera_model, &hdr.pixels[0].x, YRT_MEM_HOST, nullptr),
                           "render_camera");
        } else
            hdr = yrt_cpp::raytrace(scn, {amb, amb, amb}, resolution, samples);
        auto t1 = std::chrono::steady_clock::now();
        if (timing) {
            const yrt_stats st = yrt_cpp::last_stats(scn);
            double s = std::chrono::duration<double>(t1 - t0).count();
            printf("render %dx%d x %d spp on %d GPU(s): %.3f ms (incl. copy to host), %llu rays, %.1f Mrays/s "
                   "(%llu shadow rays with a zero light term answered without a walk)\n",
                   hdr.width, hdr.height, samples * samples, gpus, s * 1e3, st.rays, st.rays / s / 1e6,
                   st.shadow_rays_culled);
        }
        printf("saving image %s\n", out.c_str());
        yrt_cpp::save_hdr_or_ldr(out, hdr);
        for (int k = 0; k < YRT_PASS_COUNT; k++)
            if (passes >> k & 1)
                save_npy(stem + "." + pass_names[k] + ".npy", pass_data[k].data(), hdr.width, hdr.height, "<f4");
        for (size_t g = 0; g < group_data.size(); g++)
            save_npy(stem + (g + 1 < group_data.size() ? ".group" + std::to_string(g) : std::string(".ambient")) + ".npy",
                     group_data[g].data(), hdr.width, hdr.height, "<f4");
        if (adaptive) save_npy(stem + ".refined.npy", refined.data(), hdr.width, hdr.height, "|u1", 0);
        if (aovs) {
            // the requested planes in host memory, each saved as <output without extension>.<name>.npy
            yrt_render_params p = scn->params;
            p.resolution = resolution;
            p.samples = samples;
            std::vector<std::vector<char>> planes(YRT_AOV_COUNT);
            yrt_aov_planes ap = {};
            for (int k = 0; k < YRT_AOV_COUNT; k++)
                if (aovs >> k & 1) {
                    planes[k].resize((size_t)hdr.width * hdr.height * 16);
                    ap.plane[k] = planes[k].data();
                }
            yrt_cpp::check(yrt_render_aovs(scn->on_device(), &p, aovs, &ap, YRT_MEM_HOST, nullptr), "render_aovs");
            for (int k = 0; k < YRT_AOV_COUNT; k++)
                if (aovs >> k & 1)
                    save_npy(stem + "." + aov_names[k] + ".npy", planes[k].data(), hdr.width, hdr.height,
                             k == YRT_AOV_IDS ? "<i4" : "<f4");
        }
        if (mattes) {
            // one pass for every requested key; a key's layers side by side in its two files
            yrt_render_params p = scn->params;
            p.resolution = resolution;
            p.samples = samples;
            const int layers = matte_ranks / 4;
            const size_t npix = (size_t)hdr.width * hdr.height;
            std::vector<std::vector<int>> ids(YRT_MATTE_KEY_COUNT * YRT_MATTE_LAYERS_MAX);
            std::vector<std::vector<float>> cov(YRT_MATTE_KEY_COUNT * YRT_MATTE_LAYERS_MAX);
            yrt_matte_planes mp = {};
            for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++)
                for (int l = 0; l < layers; l++)
                    if (mattes >> k & 1) {
                        ids[k * YRT_MATTE_LAYERS_MAX + l].resize(npix * 4);
                        cov[k * YRT_MATTE_LAYERS_MAX + l].resize(npix * 4);
                        mp.ids[k][l] = ids[k * YRT_MATTE_LAYERS_MAX + l].data();
                        mp.coverage[k][l] = cov[k * YRT_MATTE_LAYERS_MAX + l].data();
                    }
            yrt_cpp::check(yrt_render_mattes(scn->on_device(), &p, mattes, layers, &mp, YRT_MEM_HOST, nullptr),
                           "render_mattes");
            unsigned long long dropped[YRT_MATTE_KEY_COUNT] = {};
            yrt_cpp::check(yrt_scene_matte_dropped(scn->on_device(), dropped), "matte_dropped");
            std::vector<int> all_ids(npix * matte_ranks);
            std::vector<float> all_cov(npix * matte_ranks);
            for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++) {
                if (!(mattes >> k & 1)) continue;
                for (size_t at = 0; at < npix; at++)
                    for (int l = 0; l < layers; l++) {
                        memcpy(&all_ids[at * matte_ranks + 4 * l], &ids[k * YRT_MATTE_LAYERS_MAX + l][at * 4], 16);
                        memcpy(&all_cov[at * matte_ranks + 4 * l], &cov[k * YRT_MATTE_LAYERS_MAX + l][at * 4], 16);
                    }
                const std::string base = stem + ".matte_" + matte_names[k];
                save_npy(base + ".ids.npy", all_ids.data(), hdr.width, hdr.height, "<i4", matte_ranks);
                save_npy(base + ".coverage.npy", all_cov.data(), hdr.width, hdr.height, "<f4", matte_ranks);
                if (dropped[k])
                    fprintf(stderr, "matte %s: %llu samples dropped (more than %d ids in a pixel)\n", matte_names[k],
                            dropped[k], matte_ranks);
            }
        }
        if (ao) {
            yrt_render_params p = scn->params;
            p.resolution = resolution;
            p.samples = samples;
            std::vector<float> plane((size_t)hdr.width * hdr.height * 4);
            yrt_cpp::check(yrt_render_ao(scn->on_device(), &p, &ao_params, plane.data(), YRT_MEM_HOST, nullptr), "render_ao");
            save_npy(stem + ".ao.npy", plane.data(), hdr.width, hdr.height, "<f4");
        }
    } catch (const yrt_cpp::error& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
