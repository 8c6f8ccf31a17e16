// ao_args.h -- the host-side argument handling of yrt_render_ao (capi.cpp): which arguments
// are refused, and the values the kernel receives (where the plane lies in the staging of a call
// with a host plane: plane_staging.h). Plain C++ without the HIP runtime, so that it also builds
// into a stand-alone program under the host sanitizers (tools/check_ao_args.cpp).
#pragma once

#include <float.h>
#include <math.h>
#include <stddef.h>

#include "../../include/yrt.h"

namespace yrt {

constexpr int ao_rays_default = 16;

// the kernel's K, tmin and tmax of valid parameters: rays 0 is the default count, an infinite
// distance the largest finite one (the walks' tmax of an unbounded ray)
struct ao_resolved {
    int rays;
    float bias, distance;
};

inline ao_resolved ao_resolve(const yrt_ao_params& a) {
    return {a.rays == 0 ? ao_rays_default : a.rays, a.bias, a.distance > FLT_MAX ? FLT_MAX : a.distance};
}

// the message of the first argument yrt_render_ao refuses, or nullptr (the handle and the
// frame's own fields, the camera index among them, are the caller's to check)
inline const char* ao_args_error(const yrt_ao_params* a, const float* out, int mem) {
    if (!a) return "ao: the parameters are null";
    if (!out) return "ao: out is null";
    const int k = a->rays == 0 ? ao_rays_default : a->rays;
    if (k < 1 || k > YRT_AO_RAYS_MAX) return "ao: rays must be 0 (16) or 1..64";
    if (isnan(a->distance) || !(a->distance > 0.0f)) return "ao: distance must be > 0";
    if (isnan(a->bias) || isinf(a->bias) || a->bias < 0.0f) return "ao: bias must be finite and >= 0";
    if (!(a->bias < ao_resolve(*a).distance)) return "ao: bias must be below distance";
    if (mem != YRT_MEM_HOST && mem != YRT_MEM_DEVICE) return "ao: mem is YRT_MEM_HOST or YRT_MEM_DEVICE";
    return nullptr;
}

}  // namespace yrt
