// Host half of aos_gvd_regions (regions.h): the argument checks and an exact host statement of the whole call. The
// host statement serves the stand-alone program (tests/regions_host) and the benchmark's host column only; the
// library never falls back to it.
#include "regions.h"

#include <algorithm>

namespace aos {
namespace rgn {

const char *check_regions(bool have_grid, bool have_labels, const aos_regions_opts *opts) {
    if (have_labels && !have_grid) return "labels without a grid";
    if (have_labels && opts && opts->min_component_cells > 1) return "min_component_cells above 1 together with labels";
    return nullptr;
}

namespace {

constexpr int64_t kInf = 1 << 20;   // a column distance no grid reaches; its square plus a row distance's fits int64
constexpr int64_t kNoIndex = INT64_MAX;

inline int64_t floor_div(int64_t a, int64_t b) {   // b > 0
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

int32_t uf_root(std::vector<int32_t> &p, int32_t x) {
    while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; }
    return x;
}

// is_site[c] and label[c] (at site cells) without caller labels: 8-connected components by union-find whose roots are
// the components' least cells
void sites_from_components(const int8_t *grid, int W, int H, int min_cells, std::vector<uint8_t> &is_site,
                           std::vector<int32_t> &label, Counts &n) {
    const size_t C = (size_t)W * H;
    std::vector<int32_t> parent(C, -1), size(C, 0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int32_t c = y * W + x;
            if (grid[c] != 100) continue;
            parent[c] = c;
            ++n.n_occupied;
            const int nx[4] = {x - 1, x - 1, x, x + 1}, ny[4] = {y, y - 1, y - 1, y - 1};
            for (int k = 0; k < 4; ++k) {
                if (nx[k] < 0 || nx[k] >= W || ny[k] < 0) continue;
                const int32_t m = ny[k] * W + nx[k];
                if (parent[m] < 0) continue;
                const int32_t a = uf_root(parent, c), b = uf_root(parent, m);
                if (a != b) parent[std::max(a, b)] = std::min(a, b);
            }
        }
    for (size_t c = 0; c < C; ++c)
        if (parent[c] >= 0) ++size[uf_root(parent, (int32_t)c)];
    for (size_t c = 0; c < C; ++c) {
        if (parent[c] < 0) continue;
        const int32_t r = parent[c];   // (flattened by the loop above)
        const bool keep = size[r] >= min_cells;
        if ((int32_t)c == r) { ++n.n_components; n.n_regions += keep; }
        if (keep) { is_site[c] = 1; label[c] = r; ++n.n_sites; }
    }
}

}  // namespace

void regions_host(const int8_t *grid, const int32_t *labels, int W, int H, int min_component_cells, uint32_t *site,
                  int32_t *region, int8_t *ridge, uint32_t *ridge_d2, Counts &n) {
    n = Counts();
    if (labels) n.n_components = n.n_regions = -1;
    if (W <= 0 || H <= 0) return;
    const size_t C = (size_t)W * H;
    std::vector<uint8_t> is_site(C, 0);
    std::vector<int32_t> label(C, kRegionNone);
    if (labels) {
        for (size_t c = 0; c < C; ++c) {
            if (grid[c] != 100) continue;
            ++n.n_occupied;
            if (labels[c] >= 0) { is_site[c] = 1; label[c] = labels[c]; ++n.n_sites; }
        }
    } else sites_from_components(grid, W, H, min_component_cells, is_site, label, n);

    // column pass: near[c] = the row of the column's nearest site (the smaller row at equal distance), -1: none
    std::vector<int32_t> near(C), run(W, -1);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            if (is_site[(size_t)y * W + x]) run[x] = y;
            near[(size_t)y * W + x] = run[x];
        }
    std::fill(run.begin(), run.end(), -1);
    for (int y = H - 1; y >= 0; --y)
        for (int x = 0; x < W; ++x) {
            if (is_site[(size_t)y * W + x]) run[x] = y;
            int32_t &v = near[(size_t)y * W + x];
            if (run[x] >= 0 && (v < 0 || run[x] - y < y - v)) v = run[x];
        }
    // row pass: the lower envelope of the parabolas (x - i)^2 + g(i)^2 under the key (value, index of i's site); two
    // parabolas' difference is monotone in x, so one beats the other on a prefix or a suffix of the row also with
    // the ties decided by the index, and the separators stay integers
    std::vector<int> s(W), t(W);
    std::vector<int64_t> g(W), idx(W);
    uint32_t mx = 0;
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) {
            const int32_t r = near[(size_t)y * W + x];
            g[x] = r < 0 ? kInf : std::abs(y - r);
            idx[x] = r < 0 ? kNoIndex : (int64_t)r * W + x;
        }
        auto f = [&g](int64_t x, int64_t i) { return (x - i) * (x - i) + g[i] * g[i]; };
        auto beats = [&](int u, int i, int64_t x) {
            const int64_t a = f(x, u), b = f(x, i);
            return a < b || (a == b && idx[u] < idx[i]);
        };
        int q = 0;
        s[0] = 0; t[0] = 0;
        for (int u = 1; u < W; ++u) {
            while (q >= 0 && beats(u, s[q], t[q])) --q;
            if (q < 0) { q = 0; s[0] = u; }
            else {
                const int64_t i = s[q];
                const int64_t num = (int64_t)u * u - i * i + g[u] * g[u] - g[i] * g[i], den = 2 * (u - i);
                int64_t w = 1 + floor_div(num, den);          // the first x with f(x, u) < f(x, i)
                if (num % den == 0 && idx[u] < idx[i]) --w;   // equal there, and u's site has the smaller index
                if (w < W) { ++q; s[q] = u; t[q] = (int)std::max<int64_t>(w, 0); }
            }
        }
        for (int u = W - 1; u >= 0; --u) {
            const int64_t v = f(u, s[q]);
            const bool none = v >= kInf * kInf;
            site[(size_t)y * W + u] = none ? kSiteNone : (uint32_t)idx[s[q]];
            if (!none) mx = std::max(mx, (uint32_t)v);
            if (u == t[q]) --q;
        }
    }
    n.max_d2 = n.n_sites ? mx : clr::kNone;
    for (size_t c = 0; c < C; ++c) region[c] = site[c] == kSiteNone ? kRegionNone : label[site[c]];
    // the pair rule
    std::fill(ridge, ridge + C, (int8_t)0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t c = (size_t)y * W + x;
            for (int k = 0; k < 2; ++k) {
                if (k == 0 ? x + 1 >= W : y + 1 >= H) continue;
                const size_t m = k == 0 ? c + 1 : c + W;
                if (region[c] == kRegionNone || region[m] == kRegionNone || region[c] == region[m]) continue;
                if (!is_site[c]) ridge[c] = 100;
                else if (!is_site[m]) ridge[m] = 100;
            }
        }
    for (size_t c = 0; c < C; ++c) n.n_ridge += ridge[c] == 100;
    if (ridge_d2) {
        uint32_t unused;
        clr::clear_host_field(ridge, W, H, ridge_d2, &unused);
    }
}

void regions_host_points(const clr::Grid &g, const uint32_t *site, const int32_t *region, const uint32_t *ridge_d2,
                         const double *xy, int32_t n, uint32_t *site_out, int32_t *region_out, uint32_t *d2_out,
                         uint32_t *ridge_d2_out) {
    for (int32_t i = 0; i < n; ++i) {
        int mx, my;
        const bool ok = clr::cell_of(g, xy[2 * i], xy[2 * i + 1], mx, my);
        const size_t c = ok ? (size_t)my * g.W + mx : 0;
        site_out[i] = ok ? site[c] : kSiteNone;
        region_out[i] = ok ? region[c] : kRegionNone;
        d2_out[i] = ok ? d2_of(site[c], mx, my, g.W) : clr::kNone;
        ridge_d2_out[i] = ok && ridge_d2 ? ridge_d2[c] : clr::kNone;
    }
}

}  // namespace rgn
}  // namespace aos
