// The handle's state behind aos_gvd_soft and the calls that read its field and weights (soft.hip). HIP types appear
// here, so only .hip files include it; soft.h stays readable by a plain C++ compiler.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "aos_internal.h"
#include "soft.h"

namespace aos {

struct SoftState {
    ClrFieldBufs f;   // the distance field behind the mask and the weights, this state's own
    DevBuf d_grid, wt, cost, flags, ran, stats, nodes, src, pts, path;
    PinnedBuf h_peek, h_out, h_pts, h_path;
    std::vector<uint32_t> cells;   // a descent's cells on the host; with plain_cost all of them, for the sum
    hipEvent_t ev[4] = {};
    bool have = false;
    clr::Grid g{};
    aos_grid_info info{};
    ~SoftState() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace aos
