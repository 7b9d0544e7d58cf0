// aos_reach_sight / aos_reach_pull: what the kernels (sight.hip), the host code (sight_host.cpp) and the stand-alone
// program (tests/sight_host/sight_host_main.cpp) share. No HIP type appears here, so a plain C++ compiler reads it too.
//
// The cells a segment touches (include/aos_gpu.h states the definition): for cells a and b with dx = bx - ax and
// dy = by - ay, the cells (x, y) of their bounding box with 2 |dx (y - ay) - dy (x - ax)| <= |dx| + |dy|. Walked along
// the major axis the set is an interval of the minor axis per column, at most three cells long. With A >= B the
// steps along the major and the minor axis, column t (0 .. A) holds the minor offsets w with |2 A w - 2 B t| <= A + B,
// cut to 0 .. B: every orientation and sign is this one form with its two unit steps. 2 B t < 2^30 (A, B < 16384).
#pragma once
#include <cmath>
#include <cstdint>

#include "reach.h"

namespace aos {
namespace sgt {

constexpr uint32_t kNone = AOS_COST_NONE;
constexpr uint64_t kMaxDescent = 65536;   // the longest descent aos_reach_pull pulls (aos_path_linearize's pose limit)

// (tests/sight_scenes.py names these sizes: its sweeps run +-1 around them)
constexpr int kSightTB = 256;     // threads per workgroup of both kernels: one wave per segment or candidate
constexpr int kSegsPerWG = kSightTB / 64;    // segments per workgroup of the sight kernel
constexpr int kCandsPerWG = kSightTB / 64;   // candidates per workgroup of an anchor step
constexpr int kPullBatch = 16;    // anchor steps issued between two reads of the "done" word

struct Walk {
    int ax, ay;            // the first cell
    int A, B;              // steps along the major and the minor axis, A >= B >= 0
    int mx, my, nx, ny;    // the unit step of the major axis and of the minor axis
};

AOS_CLR_HD Walk make_walk(int ax, int ay, int bx, int by) {
    const int dx = bx - ax, dy = by - ay;
    const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const int sx = (dx > 0) - (dx < 0), sy = (dy > 0) - (dy < 0);
    Walk w;
    w.ax = ax; w.ay = ay;
    if (adx >= ady) { w.A = adx; w.B = ady; w.mx = sx; w.my = 0; w.nx = 0; w.ny = sy; }
    else            { w.A = ady; w.B = adx; w.mx = 0; w.my = sy; w.nx = sx; w.ny = 0; }
    return w;
}

// the touched minor offsets lo .. hi of column t (0 <= t <= A); never empty: the offset nearest to B t / A is inside
AOS_CLR_HD void walk_column(const Walk &w, int t, int &lo, int &hi) {
    if (w.A == 0) { lo = hi = 0; return; }
    const int n = 2 * w.B * t, s = w.A + w.B, d = 2 * w.A;
    lo = n > s ? (n - s + d - 1) / d : 0;
    hi = (n + s) / d;
    if (hi > w.B) hi = w.B;
}

// the cell at column t, minor offset o
AOS_CLR_HD void walk_cell(const Walk &w, int t, int o, int &x, int &y) {
    x = w.ax + t * w.mx + o * w.nx;
    y = w.ay + t * w.my + o * w.ny;
}

struct PullCounts {
    uint64_t n_cells = 0;
    uint32_t start_cost = kNone;
    double length_m = 0.0, descent_m = INFINITY;
    uint64_t n_sight_tests = 0;
};

// ---- sight_host.cpp
// The argument checks; nullptr: fine, else the message (AOS_E_INVALID)
const char *check_sight(const double *from_xy, const double *to_xy, int32_t n);
const char *check_pull(uint64_t n_cells);   // the descent's length
// pass: W * H bytes, the passable mask of a field (cost != none is not it: a passable cell may be unreached)
void sight_host_mask(const int8_t *grid, const clr::Grid &g, uint32_t min_d2, uint8_t *pass);
// n_touched and n_blocked of one segment between two cells
void sight_host_cells(const uint8_t *pass, int W, int ax, int ay, int bx, int by, uint32_t &n_touched, uint32_t &n_blocked);
// aos_reach_sight on the host; either output may be null
void sight_host(const clr::Grid &g, const uint8_t *pass, const double *from_xy, const double *to_xy, int32_t n,
                uint32_t *n_touched, uint32_t *n_blocked);
// The waypoint steps of a descent of m cells by the farthest-visible rule; steps: room for m words. Returns their count.
uint32_t pull_host(const uint8_t *pass, int W, const uint32_t *cells, uint64_t m, int32_t max_span, uint32_t *steps);
// length_m, descent_m and n_sight_tests from the steps: host arithmetic on the integers, shared with the library
void pull_finish(const clr::Grid &g, const uint32_t *cells, uint64_t m, uint32_t start_cost, const uint32_t *steps,
                 uint32_t n_steps, int32_t max_span, PullCounts &out);

}  // namespace sgt
}  // namespace aos
