// Host half of aos_gvd_clearance (clearance.h): the argument checks, the d2 -> metres conversion, and the exact field
// and graph clearances on the host. The host field serves the stand-alone program (tests/clearance_host) and the
// benchmark's host column only; the library never falls back to it.
#include "clearance.h"

#include <algorithm>

namespace aos {
namespace clr {

const char *check_info(const aos_grid_info &info) {
    if (info.width > kMaxDim || info.height > kMaxDim) return "grid width or height above 16384";
    if (!std::isfinite(info.resolution) || !(info.resolution > 0.0f)) return "grid resolution not finite or <= 0";
    return nullptr;
}

const char *check_graph(const double *nodes_xy, int32_t num_nodes, const int32_t *edges, int32_t num_edges) {
    if (num_nodes < 0 || num_edges < 0) return "negative count";
    if ((num_nodes > 0 && !nodes_xy) || (num_edges > 0 && !edges)) return "null array behind a count above 0";
    for (int64_t i = 0; i < 2 * (int64_t)num_nodes; ++i)
        if (!std::isfinite(nodes_xy[i])) return "non-finite node coordinate";
    for (int64_t i = 0; i < 2 * (int64_t)num_edges; ++i)
        if (edges[i] < 0 || edges[i] >= num_nodes) return "edge index outside [0, num_nodes)";
    return nullptr;
}

void to_metres(const uint32_t *d2, size_t n, double res, float *out) {
    for (size_t i = 0; i < n; ++i) out[i] = metres(d2[i], res);
}

namespace {

constexpr int64_t kInf = 1 << 20;   // a column distance no grid reaches; its square plus a row distance's fits int64

inline int64_t floor_div(int64_t a, int64_t b) {   // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

}  // namespace

// Meijster, Roerdink, Hesselink (2000): column distances, then per row the lower envelope of the parabolas
// (x - i)^2 + g(i)^2 by integer separators. Every step is integer, so the words are the definition's.
uint64_t clear_host_field(const int8_t *grid, int W, int H, uint32_t *d2, uint32_t *max_d2) {
    uint64_t n_occ = 0;
    uint32_t mx = 0;
    if (W <= 0 || H <= 0) { *max_d2 = kNone; return 0; }
    std::vector<int32_t> g((size_t)W * H), run(W, (int32_t)kInf);   // (rows outermost: every pass reads along x)
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) {
            const bool occ = grid[(size_t)y * W + x] == 100;
            n_occ += occ;
            run[x] = occ ? 0 : (run[x] >= kInf ? (int32_t)kInf : run[x] + 1);
            g[(size_t)y * W + x] = run[x];
        }
    }
    std::fill(run.begin(), run.end(), (int32_t)kInf);
    for (int y = H - 1; y >= 0; --y) {
        for (int x = 0; x < W; ++x) {
            int32_t &v = g[(size_t)y * W + x];
            run[x] = v == 0 ? 0 : (run[x] >= kInf ? (int32_t)kInf : run[x] + 1);
            v = std::min(v, run[x]);
        }
    }
    std::vector<int> s(W), t(W);
    for (int y = 0; y < H; ++y) {
        const int32_t *gr = &g[(size_t)y * W];
        auto f = [gr](int64_t x, int64_t i) { return (x - i) * (x - i) + (int64_t)gr[i] * gr[i]; };
        int q = 0;
        s[0] = 0; t[0] = 0;
        for (int u = 1; u < W; ++u) {
            while (q >= 0 && f(t[q], s[q]) > f(t[q], u)) --q;
            if (q < 0) { q = 0; s[0] = u; }
            else {
                const int64_t i = s[q], gu = gr[u], gi = gr[i];
                const int64_t w = 1 + floor_div((int64_t)u * u - i * i + gu * gu - gi * gi, 2 * (u - i));
                if (w < W) { ++q; s[q] = u; t[q] = (int)std::max<int64_t>(w, 0); }
            }
        }
        for (int u = W - 1; u >= 0; --u) {
            const int64_t v = f(u, s[q]);
            const uint32_t w = v >= kInf * kInf ? kNone : (uint32_t)v;
            d2[(size_t)y * W + u] = w;
            mx = std::max(mx, w);
            if (u == t[q]) --q;
        }
    }
    *max_d2 = n_occ ? mx : kNone;
    return n_occ;
}

void clear_host_graph(const Grid &g, const uint32_t *d2, const double *nodes_xy, int32_t num_nodes, const int32_t *edges,
                      int32_t num_edges, uint32_t *node_d2, uint32_t *edge_d2) {
    auto at = [&](double px, double py) {
        int mx, my;
        return cell_of(g, px, py, mx, my) ? d2[(size_t)my * g.W + mx] : kNone;
    };
    for (int32_t i = 0; i < num_nodes; ++i) node_d2[i] = at(nodes_xy[2 * i], nodes_xy[2 * i + 1]);
    for (int32_t k = 0; k < num_edges; ++k) {
        const int a = edges[2 * k], b = edges[2 * k + 1];
        const double sx = nodes_xy[2 * a], sy = nodes_xy[2 * a + 1], tx = nodes_xy[2 * b], ty = nodes_xy[2 * b + 1];
        const double ex = tx - sx, ey = ty - sy;
        const double len = std::sqrt(ex * ex + ey * ey);
        uint32_t best = kNone;
        if (len < kMinLen) best = at(sx, sy);
        else {
            const Edge e = make_edge(g, sx, sy, tx, ty, len);
            for (int i = e.i0; i <= e.i1; ++i) {
                double px, py;
                sample_point(e, i, px, py);
                best = std::min(best, at(px, py));
            }
        }
        edge_d2[k] = best;
    }
}

}  // namespace clr
}  // namespace aos
