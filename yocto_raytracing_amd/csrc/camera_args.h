// camera_args.h -- the host-side argument handling of yrt_render_camera and yrt_camera_rays
// (capi.cpp): which arguments are refused before any device call, and the aperture and focus
// the kernel receives. Plain C++ without the HIP runtime, so that it also builds into a
// stand-alone program under the host sanitizers (tools/check_camera_models.cpp).
#pragma once

#include <math.h>
#include <stddef.h>

#include "../../include/yrt.h"

namespace yrt {

// the message of the first argument the two entry points refuse, or nullptr (the handle and the
// frame's own fields, the camera index among them, are the caller's to check); `out` is
// yrt_render_camera's image or yrt_camera_rays' records
inline const char* camera_args_error(const yrt_camera_model* m, const float* out, int mem) {
    if (!m) return "camera: the camera model is null";
    if (!out) return "camera: out is null";
    if (m->model != YRT_CAMERA_PERSPECTIVE && m->model != YRT_CAMERA_ORTHOGRAPHIC && m->model != YRT_CAMERA_EQUIRECT)
        return "camera: model is one of YRT_CAMERA_*";
    if (isnan(m->aperture) || isinf(m->aperture)) return "camera: aperture must be finite";
    if (isnan(m->focus) || isinf(m->focus)) return "camera: focus must be finite";
    if (m->chunk_pixels < 0) return "camera: chunk_pixels < 0";
    if (mem != YRT_MEM_HOST && mem != YRT_MEM_DEVICE) return "camera: mem is YRT_MEM_HOST or YRT_MEM_DEVICE";
    return nullptr;
}

// what the kernel receives of valid parameters: an aperture < 0 is the scene camera's, a focus
// <= 0 the scene camera's; the orthographic camera and the panorama have no lens (aperture 0)
struct camera_resolved {
    int model;
    float aperture, focus;
};

inline camera_resolved camera_resolve(const yrt_camera_model& m, float scene_aperture, float scene_focus) {
    const float aperture = m.aperture < 0.0f ? scene_aperture : m.aperture;
    return {m.model, m.model == YRT_CAMERA_PERSPECTIVE ? aperture : 0.0f, m.focus <= 0.0f ? scene_focus : m.focus};
}

}  // namespace yrt
