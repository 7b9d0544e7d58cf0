// The handle's state behind aos_gvd_width and the calls that read its field (width.hip). HIP types appear here, so only
// .hip files include it; width.h stays readable by a plain C++ compiler.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "aos_internal.h"
#include "width.h"

namespace aos {

struct WidthState {
    ClrFieldBufs f;   // the distance field behind cap, this state's own
    DevBuf d_grid, cap, width, flags, ran, stats, nodes, src, pts;
    PinnedBuf h_peek, h_out, h_pts;
    std::vector<float> node_r;
    hipEvent_t ev[4] = {};
    bool have = false;
    clr::Grid g{};
    aos_grid_info info{};
    ~WidthState() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace aos
