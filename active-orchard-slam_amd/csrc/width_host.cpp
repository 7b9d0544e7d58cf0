// Host half of aos_gvd_width (width.h): the argument checks and an exact host statement of the whole call. The host
// statement serves the stand-alone program (tests/width_host) and the benchmark's host column only; the library never
// falls back to it.
#include "width.h"

#include <algorithm>
#include <queue>
#include <utility>
#include <vector>

namespace aos {
namespace wd {

const char *check_width(const double *sources_xy, int32_t n_sources) {
    if (n_sources < 0) return "negative source count";
    if (n_sources > kMaxSources) return "more than 2^20 sources";
    if (n_sources > 0 && !sources_xy) return "null sources behind a count above 0";
    return nullptr;
}

void to_radius(const uint32_t *width, size_t n, double res, float *out) {
    for (size_t i = 0; i < n; ++i) out[i] = radius(width[i], res);
}

void width_host(const int8_t *grid, const clr::Grid &g, const double *sources_xy, int32_t n_sources, uint32_t *width,
                Counts &n) {
    n = Counts();
    const int W = g.W, H = g.H;
    if (W <= 0 || H <= 0) return;
    const size_t C = (size_t)W * H;
    std::vector<uint32_t> cap(C);
    {
        uint32_t unused;
        clr::clear_host_field(grid, W, H, cap.data(), &unused);
        for (size_t c = 0; c < C; ++c) {
            if (grid[c] == 100) cap[c] = 0;
            n.n_free += cap[c] != 0;
        }
    }
    std::fill(width, width + C, kNone);
    typedef std::pair<uint32_t, uint32_t> Item;   // (width, cell); the widest first
    std::priority_queue<Item> heap;
    for (int32_t i = 0; i < n_sources; ++i) {
        int mx, my;
        if (!clr::cell_of(g, sources_xy[2 * i], sources_xy[2 * i + 1], mx, my)) continue;
        const size_t c = (size_t)my * W + mx;
        if (!cap[c]) continue;
        ++n.n_sources_used;
        if (width[c] != cap[c]) { width[c] = cap[c]; heap.push(Item(cap[c], (uint32_t)c)); }
    }
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        const uint32_t c = it.second;
        if (it.first != width[c]) continue;
        const int y = (int)(c / (uint32_t)W), x = (int)(c - (uint32_t)y * (uint32_t)W);
        for (int k = 0; k < 8; ++k) {
            const int nx = x + rch::kDx[k], ny = y + rch::kDy[k];
            if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
            const size_t m = (size_t)ny * W + nx;
            uint32_t v = std::min(it.first, cap[m]);   // (cap[c] is inside width[c])
            if (k >= 4) v = std::min(v, std::min(cap[(size_t)y * W + nx], cap[(size_t)ny * W + x]));
            if (v > width[m]) { width[m] = v; heap.push(Item(v, (uint32_t)m)); }
        }
    }
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (size_t c = 0; c < C; ++c)
        if (width[c] != kNone) { ++n.n_reached; lo = std::min(lo, width[c]); hi = std::max(hi, width[c]); }
    n.min_width = n.n_reached ? lo : 0;
    n.max_width = hi;
}

void width_host_points(const clr::Grid &g, const uint32_t *width, const double *xy, int32_t n, uint32_t *out) {
    for (int32_t i = 0; i < n; ++i) {
        int mx, my;
        out[i] = clr::cell_of(g, xy[2 * i], xy[2 * i + 1], mx, my) ? width[(size_t)my * g.W + mx] : kNone;
    }
}

}  // namespace wd
}  // namespace aos
