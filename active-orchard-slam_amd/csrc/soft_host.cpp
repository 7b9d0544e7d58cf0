// Host half of aos_gvd_soft (soft.h): the argument checks and an exact host statement of the whole call. The host
// statement serves the stand-alone program (tests/soft_host) and the benchmark's host column only; the library never
// falls back to it.
#include "soft.h"

#include <algorithm>
#include <queue>
#include <utility>
#include <vector>

namespace aos {
namespace sft {

const char *check_soft(const double *sources_xy, int32_t n_sources, int32_t soft_cells, int32_t gain) {
    if (n_sources < 0) return "negative source count";
    if (n_sources > kMaxSources) return "more than 2^20 sources";
    if (n_sources > 0 && !sources_xy) return "null sources behind a count above 0";
    if (soft_cells < 0 || soft_cells > kMaxSoftCells) return "soft_cells outside 0..255";
    if (gain < 0 || gain > kMaxGain) return "gain outside 0..254";
    if (weight_bound(soft_cells, gain) > kMaxWeight) return "1 + gain * (soft_cells - 1) above 255: the weight does not fit a byte";
    return nullptr;
}

std::string check_bound(uint32_t max_weight, uint64_t n_passable) {
    if ((uint64_t)rch::kDiag * max_weight * n_passable < kCostLimit) return std::string();
    return "7 * max_weight * n_passable reaches 2^31 (max_weight " + std::to_string(max_weight) + ", n_passable " +
           std::to_string(n_passable) + "): a cost may not fit";
}

namespace {

// base * the greatest weight over the cells the move k from (x, y) touches; 0: the move is not allowed
inline uint32_t move_cost(const uint8_t *wt, int W, int H, int x, int y, int k) {
    const int nx = x + rch::kDx[k], ny = y + rch::kDy[k];
    if (nx < 0 || nx >= W || ny < 0 || ny >= H) return 0;
    const uint32_t a = wt[(size_t)y * W + x], b = wt[(size_t)ny * W + nx];
    if (!a || !b) return 0;
    if (k < 4) return rch::kAxis * std::max(a, b);
    const uint32_t s = wt[(size_t)y * W + nx], t = wt[(size_t)ny * W + x];
    if (!s || !t) return 0;
    return rch::kDiag * std::max(std::max(a, b), std::max(s, t));
}

}  // namespace

bool soft_host(const int8_t *grid, const clr::Grid &g, const double *sources_xy, int32_t n_sources, uint32_t min_d2,
               int32_t soft_cells, int32_t gain, uint8_t *wt, uint32_t *cost, Counts &n) {
    n = Counts();
    const int W = g.W, H = g.H;
    if (W <= 0 || H <= 0) return true;
    const size_t C = (size_t)W * H;
    {
        std::vector<uint32_t> d2;
        const bool field = min_d2 >= 2 || weighted(soft_cells, gain);
        if (field) {
            d2.resize(C);
            uint32_t unused;
            clr::clear_host_field(grid, W, H, d2.data(), &unused);
        }
        for (size_t c = 0; c < C; ++c) {
            const bool pass = grid[c] != 100 && (!field || d2[c] >= min_d2);
            const uint32_t w = !pass ? 0u : field ? weight(d2[c], (uint32_t)soft_cells, (uint32_t)gain) : 1u;
            wt[c] = (uint8_t)w;
            n.n_passable += pass;
            n.n_soft += w > 1;
            n.max_weight = std::max(n.max_weight, w);
        }
    }
    if (!check_bound(n.max_weight, n.n_passable).empty()) return false;
    std::fill(cost, cost + C, kNone);
    typedef std::pair<uint32_t, uint32_t> Item;   // (cost, cell)
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    for (int32_t i = 0; i < n_sources; ++i) {
        int mx, my;
        if (!clr::cell_of(g, sources_xy[2 * i], sources_xy[2 * i + 1], mx, my)) continue;
        const size_t c = (size_t)my * W + mx;
        if (!wt[c]) continue;
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
            const uint32_t w = move_cost(wt, W, H, x, y, k);
            if (!w) continue;
            const size_t m = (size_t)(y + rch::kDy[k]) * W + (x + rch::kDx[k]);
            const uint32_t v = it.first + w;
            if (v < cost[m]) { cost[m] = v; heap.push(Item(v, (uint32_t)m)); }
        }
    }
    uint32_t mx = 0;
    for (size_t c = 0; c < C; ++c)
        if (cost[c] != kNone) { ++n.n_reached; mx = std::max(mx, cost[c]); }
    n.max_cost = n.n_reached ? mx : kNone;
    return true;
}

void soft_host_points(const clr::Grid &g, const uint32_t *cost, const double *xy, int32_t n, uint32_t *out) {
    for (int32_t i = 0; i < n; ++i) {
        int mx, my;
        out[i] = clr::cell_of(g, xy[2 * i], xy[2 * i + 1], mx, my) ? cost[(size_t)my * g.W + mx] : kNone;
    }
}

uint64_t soft_host_descend(const clr::Grid &g, const uint8_t *wt, const uint32_t *cost, double sx, double sy,
                           uint32_t *cells, uint64_t capacity) {
    int x, y;
    if (g.W <= 0 || g.H <= 0 || !clr::cell_of(g, sx, sy, x, y)) return 0;
    const int W = g.W, H = g.H;
    uint32_t cur = cost[(size_t)y * W + x];
    if (cur == kNone) return 0;
    uint64_t len = 0;
    for (;;) {
        if (len < capacity) cells[len] = (uint32_t)y * (uint32_t)W + (uint32_t)x;
        ++len;
        if (cur == 0) break;
        int k = 0;
        for (; k < 8; ++k) {
            const uint32_t w = move_cost(wt, W, H, x, y, k);
            if (!w) continue;
            const uint32_t v = cost[(size_t)(y + rch::kDy[k]) * W + (x + rch::kDx[k])];
            if (v != kNone && v + w == cur) break;
        }
        if (k == 8) break;   // (no fixed point has such a cell)
        x += rch::kDx[k];
        y += rch::kDy[k];
        cur = cost[(size_t)y * W + x];
    }
    return len;
}

uint32_t plain_cost(const uint32_t *cells, uint64_t n, int W) {
    uint32_t sum = 0;
    for (uint64_t k = 1; k < n; ++k) {
        const uint32_t a = cells[k - 1], b = cells[k];
        sum += a % (uint32_t)W != b % (uint32_t)W && a / (uint32_t)W != b / (uint32_t)W ? rch::kDiag : rch::kAxis;
    }
    return sum;
}

}  // namespace sft
}  // namespace aos
