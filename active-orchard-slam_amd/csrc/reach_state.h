// The handle's state behind aos_gvd_reach and the calls that read its field and mask (reach.hip, sight.hip). HIP types
// appear here, so only .hip files include it; reach.h and sight.h stay readable by a plain C++ compiler.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "aos_internal.h"
#include "reach.h"

namespace aos {

// aos_reach_sight's and aos_reach_pull's buffers (sight.hip): theirs alone, so the outputs of the other reach calls
// stay what they were
struct SightBufs {
    DevBuf from, to, path, wp;          // the segments' ends; the descent's cells; the waypoint steps
    PinnedBuf h_sight, h_len, h_peek, h_pull;   // n_touched and n_blocked; the descent's length; "done"; cells and steps
    std::vector<uint32_t> steps, cells;         // aos_reach_pull_out's arrays
    std::vector<double> xy;
    hipEvent_t ev[3] = {};
    ~SightBufs() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

struct ReachState {
    ClrFieldBufs f;   // the distance field behind the mask (min_d2 >= 2), this state's own
    DevBuf d_grid, pass, cost, flags, ran, stats, nodes, src, pts, path;
    PinnedBuf h_peek, h_out, h_pts, h_path;
    std::vector<float> node_m;
    hipEvent_t ev[4] = {};
    bool have = false;
    clr::Grid g{};
    aos_grid_info info{};
    SightBufs sight;
    ~ReachState() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

// k_rc_descend (reach.hip) on stream s: the descent from cell (x, y), whose cost is finite, into cells (device, room
// for cap words); *n_out (pinned) = the full length, at most max_len.
void rc_launch_descend(const ReachState &S, int x, int y, uint32_t *cells, unsigned long long cap,
                       unsigned long long max_len, unsigned long long *n_out, hipStream_t s);

}  // namespace aos
