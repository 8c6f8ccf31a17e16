// soft_shadow_rays.h -- the K shadow rays of an area light (yrt_render_soft_shadows,
// yrt_shade_rays_soft; include/yrt.h has the contract): a light of radius R is a disk about its
// point that faces the shading point, and ray k of a hit point p aims at the disk's point
// dirs[k].xy, rotated by one of 16 rotations that p and the light index choose. Plain C++ that
// compiles for the host and for the device: the kernel (wavefront.hip k_soft_shadow) and the
// stand-alone host program (tools/check_soft_shadow_rays.cpp) evaluate the same text, and
// tests/soft_shadow_model.py restates it in numpy. All arithmetic is float32, left to right as
// written, with no contraction.
//
// The rotation comes from the hit point's bits and the light index alone -- not from a pixel, a
// batch index or a compaction slot -- so a ray has the same bits under any schedule, chunk size
// and mirror level. p.x + 0.0f turns a -0 into +0: the two are one point.
#pragma once

#include <stdint.h>
#include <string.h>

#include "ao_tables.h"
#include "yrt_math.h"

namespace yrt {

YRT_HD uint32_t soft_float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
#endif
}

// the index into rots of hit point p under light li
YRT_HD int soft_shadow_rot(vec3f p, int li) {
    uint32_t u = soft_float_bits(p.x + 0.0f) ^ soft_float_bits(p.y + 0.0f) ^ soft_float_bits(p.z + 0.0f);
    u ^= u >> 16;
    u ^= u >> 8;
    u ^= u >> 4;
    return (int)((u ^ (uint32_t)li) & (uint32_t)(ao_rot_count - 1));
}

// the basis about the unit vector l (Duff et al., ao.hip k_ao's text): the sign of l.z taken so
// that +0 and -0 agree
YRT_HD void soft_shadow_basis(vec3f l, vec3f& b1, vec3f& b2) {
    const float sg = l.z >= 0.0f ? 1.0f : -1.0f;
    const float a = -1.0f / (sg + l.z);
    const float b = l.x * l.y * a;
    b1 = {1.0f + sg * l.x * l.x * a, sg * b, -sg * l.x};
    b2 = {b, sg + l.y * l.y * a, -l.y};
}

// the point ray k aims at, relative to p: tp is the light's point relative to p (the hard shadow
// ray's transform_point(lf, lp0 - p)), {c, sn} the rotation, dirs the table as 3 floats per
// entry, R the light's radius. The ray is {p, tq / |tq|, 0.01f, |tq| - 0.01f}.
YRT_HD vec3f soft_shadow_target(vec3f tp, vec3f b1, vec3f b2, float c, float sn, const float* dirs, int k, float R) {
    const float tx = dirs[3 * k], ty = dirs[3 * k + 1];
    const float x = c * tx - sn * ty;
    const float y = sn * tx + c * ty;
    return tp + (b1 * x + b2 * y) * R;
}

static_assert(ao_rot_count == 16, "(u ^ li) & 15 indexes the rotations");

}  // namespace yrt
