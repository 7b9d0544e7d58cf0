// Host half of aos_reach_sight and aos_reach_pull (sight.h): the argument checks, the host arithmetic of the pull's
// lengths, and an exact host statement of both calls. The host statement serves the stand-alone program
// (tests/sight_host) and the benchmark's host column only; the library never falls back to it.
#include "sight.h"

#include <algorithm>
#include <vector>

namespace aos {
namespace sgt {

const char *check_sight(const double *from_xy, const double *to_xy, int32_t n) {
    if (n < 0) return "negative segment count";
    if (n > 0 && (!from_xy || !to_xy)) return "null ends behind a count above 0";
    return nullptr;
}

const char *check_pull(uint64_t n_cells) {
    if (n_cells > kMaxDescent) return "descent longer than 65536 cells";
    return nullptr;
}

void sight_host_mask(const int8_t *grid, const clr::Grid &g, uint32_t min_d2, uint8_t *pass) {
    if (g.W <= 0 || g.H <= 0) return;
    const size_t C = (size_t)g.W * g.H;
    std::vector<uint32_t> d2;
    if (min_d2 >= 2) {
        d2.resize(C);
        uint32_t unused;
        clr::clear_host_field(grid, g.W, g.H, d2.data(), &unused);
    }
    for (size_t c = 0; c < C; ++c) pass[c] = grid[c] != 100 && (min_d2 < 2 || d2[c] >= min_d2);
}

void sight_host_cells(const uint8_t *pass, int W, int ax, int ay, int bx, int by, uint32_t &n_touched, uint32_t &n_blocked) {
    const Walk w = make_walk(ax, ay, bx, by);
    uint32_t nt = 0, nb = 0;
    for (int t = 0; t <= w.A; ++t) {
        int lo, hi;
        walk_column(w, t, lo, hi);
        for (int o = lo; o <= hi; ++o) {
            int x, y;
            walk_cell(w, t, o, x, y);
            ++nt;
            nb += !pass[(size_t)y * W + x];
        }
    }
    n_touched = nt;
    n_blocked = nb;
}

void sight_host(const clr::Grid &g, const uint8_t *pass, const double *from_xy, const double *to_xy, int32_t n,
                uint32_t *n_touched, uint32_t *n_blocked) {
    for (int32_t k = 0; k < n; ++k) {
        int ax, ay, bx, by;
        uint32_t nt = 0, nb = kNone;
        if (g.W > 0 && g.H > 0 && clr::cell_of(g, from_xy[2 * k], from_xy[2 * k + 1], ax, ay) &&
            clr::cell_of(g, to_xy[2 * k], to_xy[2 * k + 1], bx, by))
            sight_host_cells(pass, g.W, ax, ay, bx, by, nt, nb);
        if (n_touched) n_touched[k] = nt;
        if (n_blocked) n_blocked[k] = nb;
    }
}

// is the segment free? (stops at the first impassable cell)
static bool free_between(const uint8_t *pass, int W, int ax, int ay, int bx, int by) {
    const Walk w = make_walk(ax, ay, bx, by);
    for (int t = 0; t <= w.A; ++t) {
        int lo, hi;
        walk_column(w, t, lo, hi);
        for (int o = lo; o <= hi; ++o) {
            int x, y;
            walk_cell(w, t, o, x, y);
            if (!pass[(size_t)y * W + x]) return false;
        }
    }
    return true;
}

uint32_t pull_host(const uint8_t *pass, int W, const uint32_t *cells, uint64_t m, int32_t max_span, uint32_t *steps) {
    if (m == 0) return 0;
    uint32_t n = 0;
    uint64_t k = 0;
    steps[n++] = 0;
    while (k < m - 1) {
        const uint64_t hi = max_span > 0 ? std::min<uint64_t>(m - 1, k + (uint64_t)max_span) : m - 1;
        const int ax = (int)(cells[k] % (uint32_t)W), ay = (int)(cells[k] / (uint32_t)W);
        uint64_t j = hi;
        for (; j > k + 1; --j)   // the farthest free candidate; k + 1 is an allowed move and needs no test
            if (free_between(pass, W, ax, ay, (int)(cells[j] % (uint32_t)W), (int)(cells[j] / (uint32_t)W))) break;
        k = j;
        steps[n++] = (uint32_t)k;
    }
    return n;
}

void pull_finish(const clr::Grid &g, const uint32_t *cells, uint64_t m, uint32_t start_cost, const uint32_t *steps,
                 uint32_t n_steps, int32_t max_span, PullCounts &out) {
    out = PullCounts();
    out.n_cells = m;
    if (m == 0) return;
    out.start_cost = start_cost;
    out.descent_m = (double)start_cost * g.res / 5.0;
    double sum = 0.0;
    for (uint32_t i = 0; i + 1 < n_steps; ++i) {
        const uint32_t a = cells[steps[i]], b = cells[steps[i + 1]];
        const int64_t dx = (int64_t)(b % (uint32_t)g.W) - (int64_t)(a % (uint32_t)g.W);
        const int64_t dy = (int64_t)(b / (uint32_t)g.W) - (int64_t)(a / (uint32_t)g.W);
        sum += std::sqrt((double)(dx * dx + dy * dy));
        const uint64_t hi = max_span > 0 ? std::min<uint64_t>(m - 1, (uint64_t)steps[i] + (uint64_t)max_span) : m - 1;
        out.n_sight_tests += hi - steps[i];
    }
    out.length_m = sum * g.res;
}

}  // namespace sgt
}  // namespace aos
