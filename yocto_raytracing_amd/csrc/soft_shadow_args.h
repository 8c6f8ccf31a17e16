// soft_shadow_args.h -- the host-side argument handling of yrt_shade_rays_soft and
// yrt_render_soft_shadows (capi.cpp): which soft-shadow parameters are refused before any device
// call, and the K the kernels receive. Plain C++ without the HIP runtime, so that it also builds
// into a stand-alone program under the host sanitizers (tools/check_soft_shadow_rays.cpp).
#pragma once

#include <math.h>
#include <stddef.h>

#include "../../include/yrt.h"

namespace yrt {

inline bool soft_radius_ok(float r) { return !isnan(r) && !isinf(r) && r >= 0.0f; }

// the message of the first parameter the two entry points refuse, or nullptr. With light_radius
// its nlights entries are read; that nlights is the scene's light count is the caller's to check,
// with the handle (soft_shadow_lights_error).
inline const char* soft_shadow_params_error(const yrt_soft_shadow_params* sp) {
    if (!sp) return "soft shadows: the soft shadow params are null";
    if (sp->rays < 0 || sp->rays > YRT_SOFT_SHADOW_RAYS_MAX) return "soft shadows: rays outside 0..64";
    if (!soft_radius_ok(sp->radius)) return "soft shadows: radius must be finite and >= 0";
    if (sp->light_radius) {
        if (sp->nlights < 0) return "soft shadows: nlights is not the scene's light count";
        for (int k = 0; k < sp->nlights; k++)
            if (!soft_radius_ok(sp->light_radius[k])) return "soft shadows: every light_radius must be finite and >= 0";
    }
    return nullptr;
}

inline const char* soft_shadow_lights_error(const yrt_soft_shadow_params& sp, int scene_lights) {
    return sp.light_radius && sp.nlights != scene_lights ? "soft shadows: nlights is not the scene's light count" : nullptr;
}

// K: 0 is the default
constexpr int soft_shadow_rays_default = 16;
inline int soft_shadow_rays_of(const yrt_soft_shadow_params& sp) { return sp.rays == 0 ? soft_shadow_rays_default : sp.rays; }

}  // namespace yrt
