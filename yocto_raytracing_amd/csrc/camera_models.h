// camera_models.h -- the camera models of yrt_render_camera and yrt_camera_rays (include/yrt.h
// has the contract): the thin-lens perspective camera, the orthographic camera and the
// equirectangular panorama, each as the one expression of a sample's ray. Plain C++ that compiles
// for the host and for the device: the kernel (camera.hip k_camera_rays) and the stand-alone host
// check (tools/check_camera_models.cpp) evaluate the same text, and tests/camera_model.py restates
// it in numpy. All arithmetic is float32, left to right as written, with no contraction.
//
// The lens samples are the ambient occlusion pass's tables (ao_tables.h): dirs[k].xy is the
// Halton (2, 3) point k + 1 mapped uniformly onto the unit disk, of which any prefix is a usable
// set, and rots[r] one of 16 rotations. A pixel's sample q takes point q & 63 under the rotation
// ((i & 3) | (j & 3) << 2) ^ (q >> 6): one rotation per 4 x 4 pixel tile for the first 64
// samples, another for each further 64.
#pragma once

#include <math.h>

#include "ao_tables.h"
#include "yrt_device.h"
#include "yrt_math.h"

namespace yrt {

enum camera_model : int { camera_perspective = 0, camera_orthographic = 1, camera_equirect = 2, camera_model_count = 3 };

// {o.xyz, d.xyz, tmin, tmax}: the 32-byte record of yrt_trace_first and yrt_shade_rays
struct camera_model_ray {
    vec3f o, d;
    float tmin, tmax;
};

// Sample q = jj * ns + ii of image pixel (i, j) of a W x H frame at ns samples per axis. `cam` is
// make_dev_camera of the scene camera (with the call's focus), `aperture` the resolved lens
// diameter (PERSPECTIVE alone reads it; 0 is the pinhole, camera_ray's bits), dirs and rots the
// two tables as 3 and 2 floats per entry.
template <int MODEL>
YRT_HD camera_model_ray camera_model_eval(const dev_camera& cam, float aperture, const float* dirs, const float* rots,
                                          int W, int H, int ns, int i, int j, int q) {
    const int ii = q % ns, jj = q / ns;
    const float u = (i + (ii + 0.5f) / ns) / W;
    const float v = (j + (jj + 0.5f) / ns) / H;
    const vec3f o = {cam.ox, cam.oy, cam.oz};
    if (MODEL == camera_orthographic) {
        vec3f e;
        e.x = cam.ox + (u - 0.5f) * cam.w * cam.xx + (v - 0.5f) * cam.h * cam.yx;
        e.y = cam.oy + (u - 0.5f) * cam.w * cam.xy + (v - 0.5f) * cam.h * cam.yy;
        e.z = cam.oz + (u - 0.5f) * cam.w * cam.xz + (v - 0.5f) * cam.h * cam.yz;
        return {e, normalize(vec3f{-cam.zx, -cam.zy, -cam.zz}), ray_eps, flt_max};
    }
    if (MODEL == camera_equirect) {
        const float phi = (u - 0.5f) * 6.2831855f, th = v * 3.1415927f;
        const float st = sinf(th), ct = cosf(th), sp = sinf(phi), cp = cosf(phi);
        const float a = st * sp, g = st * cp;
        vec3f d;
        d.x = (a * cam.xx - ct * cam.yx) - g * cam.zx;
        d.y = (a * cam.xy - ct * cam.yy) - g * cam.zy;
        d.z = (a * cam.xz - ct * cam.yz) - g * cam.zz;
        return {o, normalize(d), ray_eps, flt_max};
    }
    // the point of the focal plane the sample looks at: camera_ray's expression (trace_common.h)
    vec3f Q;
    Q.x = cam.ox + (u - 0.5f) * cam.w * cam.xx + (v - 0.5f) * cam.h * cam.yx - cam.focus * cam.zx;
    Q.y = cam.oy + (u - 0.5f) * cam.w * cam.xy + (v - 0.5f) * cam.h * cam.yy - cam.focus * cam.zy;
    Q.z = cam.oz + (u - 0.5f) * cam.w * cam.xz + (v - 0.5f) * cam.h * cam.yz - cam.focus * cam.zz;
    vec3f e = o;
    if (!(aperture == 0.0f)) {  // the point of the lens the ray leaves from
        const float R = aperture * 0.5f;
        const int k = q & (ao_dir_count - 1);
        const float tx = dirs[3 * k], ty = dirs[3 * k + 1];
        const int t = (i & 3) | ((j & 3) << 2);
        const int r = (t ^ (q >> 6)) & (ao_rot_count - 1);
        const float c = rots[2 * r], sn = rots[2 * r + 1];
        const float lx = R * (c * tx - sn * ty), ly = R * (sn * tx + c * ty);
        e.x = (cam.ox + lx * cam.xx) + ly * cam.yx;
        e.y = (cam.oy + lx * cam.xy) + ly * cam.yy;
        e.z = (cam.oz + lx * cam.xz) + ly * cam.yz;
    }
    return {e, normalize(Q - e), ray_eps, flt_max};
}
static_assert(ao_dir_count == 64 && ao_rot_count == 16, "q & 63 and (t ^ q >> 6) & 15 index the tables");

}  // namespace yrt
