// matte_args.h -- the host-side argument handling of yrt_render_mattes (capi.cpp): which
// arguments are refused (where each requested plane lies in the staging of a call with host
// planes: plane_staging.h). Plain C++ without the HIP runtime, so that it also builds into a
// stand-alone program under the host sanitizers (tools/check_plane_staging.cpp).
#pragma once

#include <stddef.h>

#include "../../include/yrt.h"

namespace yrt {

// the message of the first argument yrt_render_mattes refuses, or nullptr
inline const char* matte_args_error(unsigned key_mask, int layers, const yrt_matte_planes* out, int mem) {
    if (!out) return "mattes: the planes are null";
    if (key_mask == 0 || key_mask >> YRT_MATTE_KEY_COUNT) return "matte key mask must name one to all of YRT_MATTE_*";
    if (layers < 1 || layers > YRT_MATTE_LAYERS_MAX) return "matte layers must be 1 or 2";
    if (mem != YRT_MEM_HOST && mem != YRT_MEM_DEVICE) return "mattes: mem is YRT_MEM_HOST or YRT_MEM_DEVICE";
    for (int k = 0; k < YRT_MATTE_KEY_COUNT; k++)
        for (int l = 0; l < layers; l++)
            if ((key_mask >> k & 1) && (!out->ids[k][l] || !out->coverage[k][l])) return "a requested matte plane is null";
    return nullptr;
}

}  // namespace yrt
