// Host half of aos_gvd_reach (reach.h): the argument checks and an exact host statement of the whole call. The host
// statement serves the stand-alone program (tests/reach_host) and the benchmark's host column only; the library never
// falls back to it.
#include "reach.h"

#include <algorithm>
#include <queue>
#include <utility>
#include <vector>

namespace aos {
namespace rch {

const char *check_reach(const double *sources_xy, int32_t n_sources) {
    if (n_sources < 0) return "negative source count";
    if (n_sources > kMaxSources) return "more than 2^20 sources";
    if (n_sources > 0 && !sources_xy) return "null sources behind a count above 0";
    return nullptr;
}

void to_metres(const uint32_t *cost, size_t n, double res, float *out) {
    for (size_t i = 0; i < n; ++i) out[i] = metres(cost[i], res);
}

void reach_host(const int8_t *grid, const clr::Grid &g, const double *sources_xy, int32_t n_sources, uint32_t min_d2,
                uint32_t *cost, Counts &n) {
    n = Counts();
    const int W = g.W, H = g.H;
    if (W <= 0 || H <= 0) return;
    const size_t C = (size_t)W * H;
    std::vector<uint8_t> pass(C);
    {
        std::vector<uint32_t> d2;
        if (min_d2 >= 2) {
            d2.resize(C);
            uint32_t unused;
            clr::clear_host_field(grid, W, H, d2.data(), &unused);
        }
        for (size_t c = 0; c < C; ++c) {
            pass[c] = grid[c] != 100 && (min_d2 < 2 || d2[c] >= min_d2);
            n.n_passable += pass[c];
        }
    }
    std::fill(cost, cost + C, kNone);
    typedef std::pair<uint32_t, uint32_t> Item;   // (cost, cell)
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (int32_t i = 0; i < n_sources; ++i) {
        int mx, my;
        if (!clr::cell_of(g, sources_xy[2 * i], sources_xy[2 * i + 1], mx, my)) continue;
        const size_t c = (size_t)my * W + mx;
        if (!pass[c]) continue;
        ++n.n_sources_used;
        if (cost[c] != 0) { cost[c] = 0; heap.push(Item(0u, (uint32_t)c)); }
    }
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        const uint32_t c = it.second;
        if (it.first != cost[c]) continue;
        const int y = (int)(c / (uint32_t)W), x = (int)(c - (uint32_t)y * (uint32_t)W);
        for (int k = 0; k < 8; ++k) {
            const int nx = x + kDx[k], ny = y + kDy[k];
            if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
            const size_t m = (size_t)ny * W + nx;
            if (!pass[m]) continue;
            if (k >= 4 && !(pass[(size_t)y * W + nx] && pass[(size_t)ny * W + x])) continue;
            const uint32_t v = it.first + (k < 4 ? kAxis : kDiag);
            if (v < cost[m]) { cost[m] = v; heap.push(Item(v, (uint32_t)m)); }
        }
    }
    uint32_t mx = 0;
    for (size_t c = 0; c < C; ++c)
        if (cost[c] != kNone) { ++n.n_reached; mx = std::max(mx, cost[c]); }
    n.max_cost = n.n_reached ? mx : kNone;
}

void reach_host_points(const clr::Grid &g, const uint32_t *cost, const double *xy, int32_t n, uint32_t *out) {
    for (int32_t i = 0; i < n; ++i) {
        int mx, my;
        out[i] = clr::cell_of(g, xy[2 * i], xy[2 * i + 1], mx, my) ? cost[(size_t)my * g.W + mx] : kNone;
    }
}

uint64_t reach_host_descend(const clr::Grid &g, const uint32_t *cost, double sx, double sy, uint32_t *cells,
                            uint64_t capacity) {
    int x, y;
    if (g.W <= 0 || g.H <= 0 || !clr::cell_of(g, sx, sy, x, y)) return 0;
    const int W = g.W, H = g.H;
    auto at = [&](int ax, int ay) { return ax < 0 || ax >= W || ay < 0 || ay >= H ? kNone : cost[(size_t)ay * W + ax]; };
    uint32_t cur = at(x, y);
    if (cur == kNone) return 0;
    uint64_t len = 0;
    for (;;) {
        if (len < capacity) cells[len] = (uint32_t)y * (uint32_t)W + (uint32_t)x;
        ++len;
        if (cur == 0) break;
        int k = 0;
        for (; k < 8; ++k) {
            const uint32_t v = at(x + kDx[k], y + kDy[k]);
            if (v == kNone || v + (k < 4 ? kAxis : kDiag) != cur) continue;
            if (k >= 4 && (at(x + kDx[k], y) == kNone || at(x, y + kDy[k]) == kNone)) continue;
            break;
        }
        if (k == 8) break;   // (no fixed point has such a cell)
        x += kDx[k];
        y += kDy[k];
        cur = at(x, y);
    }
    return len;
}

}  // namespace rch
}  // namespace aos
