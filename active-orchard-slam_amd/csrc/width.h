// aos_gvd_width: what the kernels (width.hip), the host code (width_host.cpp) and the stand-alone program
// (tests/width_host/width_host_main.cpp) share. No HIP type appears here, so a plain C++ compiler reads it too.
//
// Every quantity is an integer (include/aos_gpu.h states the definitions): cap[c] = 0 where the cell's byte is 100,
// else the clearance d2 of the cell; a move goes to an 8-neighbour; its bottleneck is the least cap of its two cells
// and, for a diagonal, of the two cells beside it; width[c] = the greatest, over the move paths from a kept source cell
// to c, of the least bottleneck along the path (a path of one cell: cap[c]); 0 where no path has a bottleneck above 0.
// The tile, workgroup and batch sizes are reach's (reach.h): one value each for both wavefronts.
#pragma once
#include <cmath>
#include <cstdint>

#include "reach.h"

namespace aos {
namespace wd {

constexpr uint32_t kNone = AOS_WIDTH_NONE;
constexpr int32_t kMaxSources = rch::kMaxSources;

// width -> the radius in metres between cell centres; computed on the host from the integer
inline float radius(uint32_t width, double res) {
    if (width == clr::kNone) return INFINITY;
    if (width == kNone) return 0.0f;
    return (float)(std::sqrt((double)width) * res);
}

struct Counts {
    uint64_t n_free = 0, n_reached = 0;
    int32_t n_sources_used = 0;
    uint32_t min_width = 0, max_width = 0;
};

// ---- width_host.cpp
// The argument checks of aos_gvd_width beyond clr::check_info / check_graph; nullptr: fine, else the message
const char *check_width(const double *sources_xy, int32_t n_sources);
void to_radius(const uint32_t *width, size_t n, double res, float *out);
// The exact statement on the host: cap from clear_host_field, then a max-heap bottleneck Dijkstra over the move rule;
// for the stand-alone program and the benchmark's host column only. width: W * H words.
void width_host(const int8_t *grid, const clr::Grid &g, const double *sources_xy, int32_t n_sources, uint32_t *width,
                Counts &n);
// the widths at n points by the cell rule
void width_host_points(const clr::Grid &g, const uint32_t *width, const double *xy, int32_t n, uint32_t *out);

}  // namespace wd
}  // namespace aos
