// aos_gvd_soft: what the kernels (soft.hip), the host code (soft_host.cpp) and the stand-alone program
// (tests/soft_host/soft_host_main.cpp) share. No HIP type appears here, so a plain C++ compiler reads it too.
//
// Every quantity is an integer (include/aos_gpu.h states the definitions): passable is reach's rule; r = the integer
// square root of the clearance d2; wt = 1 + gain * max(0, soft_cells - r) on passable cells (1 where d2 is none), kept
// as one byte image with 0 for impassable; a move is reach's, and costs 5 or 7 times the greatest wt over the cells it
// touches (its two cells, and for a diagonal the two cells beside it); cost[c] = the least sum of move costs from a
// kept source cell. The tile, workgroup and batch sizes are reach's (reach.h): one value each for the wavefronts.
#pragma once
#include <cstdint>
#include <string>

#include "reach.h"

#if defined(__HIPCC__)
#define AOS_SOFT_HD __host__ __device__ __forceinline__
#else
#define AOS_SOFT_HD inline
#endif

namespace aos {
namespace sft {

constexpr uint32_t kNone = AOS_COST_NONE;
constexpr int32_t kMaxSources = rch::kMaxSources;
constexpr int32_t kMaxSoftCells = 255, kMaxGain = 254;
constexpr uint32_t kMaxWeight = 255;              // wt fits a byte
constexpr uint64_t kCostLimit = 1ull << 31;       // 7 * max_weight * n_passable stays below it

// floor(sqrt(d2)) for d2 < 2^31: the float root is only a first guess, the integer steps decide
AOS_SOFT_HD uint32_t isqrt(uint32_t d2) {
    uint32_t r = (uint32_t)sqrtf((float)d2);
    while (r * r > d2) --r;
    while ((r + 1) * (r + 1) <= d2) ++r;
    return r;
}

// the weight of a passable cell with clearance d2 (clr::kNone: no occupied cell anywhere)
AOS_SOFT_HD uint32_t weight(uint32_t d2, uint32_t soft_cells, uint32_t gain) {
    if (d2 == clr::kNone) return 1u;
    const uint32_t r = isqrt(d2);
    return r < soft_cells ? 1u + gain * (soft_cells - r) : 1u;
}

// the greatest weight the options can give a passable cell (a free cell has r >= 1)
inline uint32_t weight_bound(int32_t soft_cells, int32_t gain) {
    return 1u + (uint32_t)gain * (uint32_t)(soft_cells > 1 ? soft_cells - 1 : 0);
}
// the weights are not all 1: the distance field is needed for them
inline bool weighted(int32_t soft_cells, int32_t gain) { return gain > 0 && soft_cells > 1; }

struct Counts {
    uint64_t n_passable = 0, n_reached = 0, n_soft = 0;
    int32_t n_sources_used = 0;
    uint32_t max_cost = kNone, max_weight = 0;
};

// ---- soft_host.cpp
// The argument checks of aos_gvd_soft beyond clr::check_info / check_graph; nullptr: fine, else the message
const char *check_soft(const double *sources_xy, int32_t n_sources, int32_t soft_cells, int32_t gain);
// 7 * max_weight * n_passable >= 2^31: the message that names both factors; else empty
std::string check_bound(uint32_t max_weight, uint64_t n_passable);
// The exact statement on the host: the weights from clear_host_field, then a binary-heap Dijkstra over the move rule;
// for the stand-alone program and the benchmark's host column only. wt: W * H bytes, cost: W * H words. false: the
// bound is crossed (n holds n_passable, n_soft and max_weight; cost is not written).
bool soft_host(const int8_t *grid, const clr::Grid &g, const double *sources_xy, int32_t n_sources, uint32_t min_d2,
               int32_t soft_cells, int32_t gain, uint8_t *wt, uint32_t *cost, Counts &n);
// the costs at n points by the cell rule
void soft_host_points(const clr::Grid &g, const uint32_t *cost, const double *xy, int32_t n, uint32_t *out);
// The descent from (sx, sy) on a host field and its weights. Writes at most capacity cells; returns the full length.
uint64_t soft_host_descend(const clr::Grid &g, const uint8_t *wt, const uint32_t *cost, double sx, double sy,
                           uint32_t *cells, uint64_t capacity);
// the sum of 5 (axis) and 7 (diagonal) over the moves between n consecutive cells of a descent
uint32_t plain_cost(const uint32_t *cells, uint64_t n, int W);

}  // namespace sft
}  // namespace aos
