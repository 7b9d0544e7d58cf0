// aos_gvd_reach: what the kernels (reach.hip), the host code (reach_host.cpp) and the stand-alone program
// (tests/reach_host/reach_host_main.cpp) share. No HIP type appears here, so a plain C++ compiler reads it too.
//
// Every quantity is an integer (include/aos_gpu.h states the definitions): a cell is passable iff its byte is not 100
// and its clearance d2 >= min_d2; a move goes to a passable 8-neighbour, 5 along an axis and 7 diagonally, the
// diagonal only between two passable cells; cost[c] = the least sum of move costs from a source cell. The cell rule is
// clearance.h's.
#pragma once
#include <cmath>
#include <cstdint>

#include "clearance.h"

namespace aos {
namespace rch {

constexpr uint32_t kNone = AOS_COST_NONE;
constexpr uint32_t kAxis = 5, kDiag = 7;   // the move costs
constexpr int32_t kMaxSources = 1 << 20;

// (tests/reach_scenes.py names these sizes: its sweeps run +-1 around the tile and past one batch of rounds)
constexpr int kTile = 32;       // a tile is kTile x kTile cells; its workgroup holds it with a one-cell halo in LDS
constexpr int kTileTB = 256;    // threads per tile workgroup: kTile * kTile / kTileTB cells each
constexpr int kBatch = 16;      // rounds issued between two reads of the "did a tile run" word

// the eight moves in the descent's order
constexpr int kDx[8] = {1, -1, 0, 0, 1, -1, 1, -1};
constexpr int kDy[8] = {0, 0, 1, -1, 1, 1, -1, -1};

// cost -> metres along the moves; computed on the host from the integer
inline float metres(uint32_t cost, double res) {
    if (cost == kNone) return INFINITY;
    return (float)((double)cost * res / 5.0);
}

// the centre of the cell with linear index c: origin + (column or row + 0.5) * res
inline void cell_centre(const clr::Grid &g, uint32_t c, double &x, double &y) {
    const uint32_t cy = c / (uint32_t)g.W, cx = c - cy * (uint32_t)g.W;
    x = g.ox + ((double)cx + 0.5) * g.res;
    y = g.oy + ((double)cy + 0.5) * g.res;
}

struct Counts {
    uint64_t n_passable = 0, n_reached = 0;
    int32_t n_sources_used = 0;
    uint32_t max_cost = kNone;
};

// ---- reach_host.cpp
// The argument checks of aos_gvd_reach beyond clr::check_info / check_graph; nullptr: fine, else the message
const char *check_reach(const double *sources_xy, int32_t n_sources);
void to_metres(const uint32_t *cost, size_t n, double res, float *out);
// The exact statement on the host: the mask from clear_host_field, then a binary-heap Dijkstra over the move rule; for
// the stand-alone program and the benchmark's host column only. cost: W * H words.
void reach_host(const int8_t *grid, const clr::Grid &g, const double *sources_xy, int32_t n_sources, uint32_t min_d2,
                uint32_t *cost, Counts &n);
// the costs at n points by the cell rule
void reach_host_points(const clr::Grid &g, const uint32_t *cost, const double *xy, int32_t n, uint32_t *out);
// The descent from (sx, sy) on a host field. The field alone decides it: an axis neighbour of a reached cell is
// passable iff it is reached too, so the corner rule reads "both cells beside the diagonal have a finite cost".
// Writes at most capacity cells; returns the full length.
uint64_t reach_host_descend(const clr::Grid &g, const uint32_t *cost, double sx, double sy, uint32_t *cells,
                            uint64_t capacity);

}  // namespace rch
}  // namespace aos
