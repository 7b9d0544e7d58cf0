// aos_gvd_clearance: the arithmetic shared by the kernels (clearance.hip), the host code (clearance_host.cpp) and
// the stand-alone program (tests/clearance_host/clear_host_main.cpp). No HIP type appears here, so a plain C++
// compiler reads it too.
//
// The field is integer: d2 = the squared distance, in cells, between a cell's centre and the nearest occupied
// cell's centre (occupied: the byte is 100, the test of edgePassesThroughOccupiedPixels gvd:320-359 and
// trimPathNearOccupiedRegions). The clearances are therefore quantised to the grid on purpose: a point takes the
// value of the cell it falls in. The cell rule, the sample count and the sample point are copies of k_occupancy's
// and occ_trunc's expressions (gvd.hip), which stay where they are; doubles, no FMA contraction.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/aos_gpu.h"

#if defined(__HIPCC__)
#define AOS_CLR_HD __host__ __device__ __forceinline__
#else
#define AOS_CLR_HD inline
#endif

namespace aos {
namespace clr {

constexpr uint32_t kNone = AOS_D2_NONE;
constexpr uint32_t kMaxDim = 16384;      // width and height limit: d2 < 2^29 and a column distance fits uint16
constexpr uint16_t kColNone = 0xFFFF;    // column pass: no occupied cell in the column
constexpr double kMinLen = 1e-6;         // a shorter edge has the single sample s
constexpr int kClipFrom = 64;            // an edge with more samples is clipped to the grid's neighbourhood first

struct Grid {
    double ox, oy, res;   // info.origin, (double)info.resolution
    int W, H;
};

// occ_trunc's rule: the cell of a world point; false: the point has no cell
AOS_CLR_HD bool cell_of(const Grid &g, double px, double py, int &mx, int &my) {
    const double fx = (px - g.ox) / g.res, fy = (py - g.oy) / g.res;
    if (!(fx > -1.0 && fx < (double)g.W) || !(fy > -1.0 && fy < (double)g.H)) return false;
    mx = (int)fx;
    my = (int)fy;
    return mx >= 0 && mx < g.W && my >= 0 && my < g.H;
}

// num of edgePassesThroughOccupiedPixels for an edge of length len >= kMinLen: the samples are i = 0 .. num. The
// reference casts len / step to int; out of range x86 gives INT_MIN, so num = INT_MIN + 1 and the loop never runs.
AOS_CLR_HD int num_samples(double len, double res) {
    const double step = res * 0.5;
    const double q = len / step;
    return (q > -2147483649.0 && q < 2147483647.0) ? (int)q + 1 : INT_MIN + 1;
}

struct Edge {
    double sx, sy, ux, uy, len;
    int num;       // < 0: no samples
    int i0, i1;    // the samples that can have a cell: i0 .. i1 (i1 < i0: none)
};

// sample i of an edge (0 <= i <= num)
AOS_CLR_HD void sample_point(const Edge &e, int i, double &px, double &py) {
    const double t = (i == e.num) ? 1.0 : ((double)i / (double)e.num);
    px = e.sx + (t * e.ux) * e.len;
    py = e.sy + (t * e.uy) * e.len;
}

// The edge from (sx, sy) to (tx, ty) with len >= kMinLen. Samples whose t cannot touch the grid are left out of
// [i0, i1] with k_occupancy's slack (two cells around the grid, two samples around the range): they have no cell.
AOS_CLR_HD Edge make_edge(const Grid &g, double sx, double sy, double tx, double ty, double len) {
    Edge e;
    const double ex = tx - sx, ey = ty - sy;
    e.sx = sx; e.sy = sy; e.ux = ex / len; e.uy = ey / len; e.len = len;
    e.num = num_samples(len, g.res);
    e.i0 = 0; e.i1 = e.num;
    if (e.num > kClipFrom) {
        double lo_t = 0.0, hi_t = 1.0;
        const double gx0 = g.ox - 2 * g.res, gx1 = g.ox + (g.W + 2) * g.res;
        const double gy0 = g.oy - 2 * g.res, gy1 = g.oy + (g.H + 2) * g.res;
        for (int axis = 0; axis < 2; ++axis) {
            const double p0 = axis ? sy : sx, dp = axis ? ey : ex, a = axis ? gy0 : gx0, b = axis ? gy1 : gx1;
            if (dp == 0.0) {
                if (p0 < a || p0 > b) { lo_t = 1.0; hi_t = 0.0; }
                continue;
            }
            double t0 = (a - p0) / dp, t1 = (b - p0) / dp;
            if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
            lo_t = fmax(lo_t, t0);
            hi_t = fmin(hi_t, t1);
        }
        if (lo_t > hi_t) { e.i0 = 1; e.i1 = 0; }
        else {
            const int a = (int)floor(lo_t * e.num) - 2, b = (int)ceil(hi_t * e.num) + 2;
            e.i0 = a > 0 ? a : 0;
            e.i1 = b < e.num ? b : e.num;
        }
    }
    if (e.num < 0) { e.i0 = 1; e.i1 = 0; }
    return e;
}

// d2 -> metres between cell centres; computed on the host from the integer, so no device sqrt decides a bit
inline float metres(uint32_t d2, double res) {
    if (d2 == kNone) return INFINITY;
    return (float)(std::sqrt((double)d2) * res);
}

// ---- clearance_host.cpp
// The argument checks of aos_gvd_clearance that need no handle; nullptr: fine, else the message (AOS_E_INVALID)
const char *check_info(const aos_grid_info &info);
const char *check_graph(const double *nodes_xy, int32_t num_nodes, const int32_t *edges, int32_t num_edges);
void to_metres(const uint32_t *d2, size_t n, double res, float *out);
// The exact field on the host (an integer two-pass: column distances, then each row's lower envelope of parabolas);
// for the stand-alone program and the benchmark's host column only. d2: W * H words. Returns n_occupied.
uint64_t clear_host_field(const int8_t *grid, int W, int H, uint32_t *d2, uint32_t *max_d2);
// node_d2 / edge_d2 by the definitions above, from a host field (d2 may be null when W * H = 0)
void clear_host_graph(const Grid &g, const uint32_t *d2, const double *nodes_xy, int32_t num_nodes, const int32_t *edges,
                      int32_t num_edges, uint32_t *node_d2, uint32_t *edge_d2);

}  // namespace clr
}  // namespace aos
