// aos_gvd_regions: what the kernels (regions.hip), the host code (regions_host.cpp) and the stand-alone program
// (tests/regions_host/regions_host_main.cpp) share. No HIP type appears here, so a plain C++ compiler reads it too.
//
// Every quantity is an integer (include/aos_gpu.h states the definitions): site[c] = the linear index of the site
// cell with the least (squared centre distance, linear index); region[c] = that site's label; the ridge by the pair
// rule; ridge_d2 = clearance.h's field over the ridge cells. The cell rule and the metres are clearance.h's.
#pragma once
#include <cstdint>
#include <cstring>

#include "clearance.h"

namespace aos {
namespace rgn {

constexpr uint32_t kSiteNone = AOS_SITE_NONE;
constexpr int32_t kRegionNone = AOS_REGION_NONE;
constexpr int16_t kOffNone = INT16_MIN;   // column pass: no site in the column (a row offset is within +-16383)

// the squared centre distance between cell (x, y) and the cell with linear index s
AOS_CLR_HD uint32_t d2_of(uint32_t s, int x, int y, int W) {
    if (s == kSiteNone) return clr::kNone;
    const int sy = (int)(s / (uint32_t)W), sx = (int)(s - (uint32_t)sy * (uint32_t)W);
    return (uint32_t)((x - sx) * (x - sx) + (y - sy) * (y - sy));
}

// the fields aos_regions_field_copy serves, in its order; -1: unknown name
enum Field { kSite = 0, kRegion = 1, kRidge = 2, kRidgeD2 = 3 };
inline int field_of(const char *which) {
    static const char *const names[4] = {"site", "region", "ridge", "ridge_d2"};
    for (int k = 0; which && k < 4; ++k)
        if (!std::strcmp(which, names[k])) return k;
    return -1;
}
inline size_t field_bytes(int f) { return f == kRidge ? 1 : 4; }

struct Counts {
    uint64_t n_occupied = 0, n_sites = 0, n_ridge = 0;
    int64_t n_components = 0, n_regions = 0;   // -1 with caller labels
    uint32_t max_d2 = clr::kNone;
};

// ---- regions_host.cpp
// The argument checks of aos_gvd_regions beyond clr::check_info / check_graph; nullptr: fine, else the message
const char *check_regions(bool have_grid, bool have_labels, const aos_regions_opts *opts);
// The exact statement on the host: union-find components, a two-pass field carrying (d2, index), the pair rule, and
// the ridge's distance field; for the stand-alone program and the benchmark's host column only. Every array holds
// W * H cells; ridge_d2 may be null (not wanted).
void regions_host(const int8_t *grid, const int32_t *labels, int W, int H, int min_component_cells, uint32_t *site,
                  int32_t *region, int8_t *ridge, uint32_t *ridge_d2, Counts &n);
// the values at n points by the cell rule (ridge_d2 null: every ridge_d2_out is kNone)
void regions_host_points(const clr::Grid &g, const uint32_t *site, const int32_t *region, const uint32_t *ridge_d2,
                         const double *xy, int32_t n, uint32_t *site_out, int32_t *region_out, uint32_t *d2_out,
                         uint32_t *ridge_d2_out);

}  // namespace rgn
}  // namespace aos
