// aos_gvd_regions: for every cell of a grid the nearest site (an occupied cell of a kept component, or of a caller
// label), the site's region, the ridge between the regions (the grid GVD) and, on request, the distance field to that
// ridge; the values at a GvdGraph's nodes and at arbitrary points (regions.h and include/aos_gpu.h have the
// definitions). Everything is integer, so the result is fixed word for word.
//
// What runs where:
//   sites, labels GPU  k_rg_pack: the occupied bytes as row-wise 64-bit words (one ballot per wave) with their
//                      popcounts; scan_1p and ccl_label (cluster_seed.hip, unchanged) label the 8-connected components
//                      with their raster-first cell as root, so list[parent[i]] is a component's least index;
//                      k_rg_size: one atomic per cell on its root; k_rg_sites: the site bytes (100 / 0) and the dense
//                      label image, and the kept components' count. With caller labels k_rg_label_sites alone.
//   column pass   GPU  clearance.hip's band words and carries on the site bytes (clr_launch_bands, shared unchanged),
//                      then k_rg_cols: per cell the signed row offset to its column's nearest site (int16, kOffNone:
//                      none); at equal distance the smaller row
//   row pass      GPU  k_rg_rows: one workgroup per row with the row's offsets in LDS (2 W bytes); a cell scans its
//                      own 64-column block, then the blocks left and right outwards as k_clr_rows does. Every prune is
//                      strict (a block or the walk is left out only when its bound is greater than the best d2 so
//                      far), so every candidate of equal d2 is met and the least linear index among them wins
//   region, ridge GPU  k_rg_region: region = label[site]; k_rg_ridge: a cell's two forward pairs and the two backward
//                      pairs that can mark it, no atomics on the image; the count costs one atomic per wave
//   ridge d2      GPU  clearance.hip's field passes on the ridge bytes into this state's own buffers (clr_launch_field)
//   sampling      GPU  k_rg_sample: one thread per node or point, stored into pinned host memory by the kernel
//   metres, checks     host (regions_host.cpp, clearance_host.cpp)
// Host waits: ccl_label's one (the occupied count sizes its buffers) and the call's final stream synchronise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "aos_ctx.h"
#include "cluster_geom.h"
#include "cluster_seed.h"
#include "dev_prims.h"
#include "field_passes.h"
#include "regions.h"

namespace aos {

// (the band, workgroup and block sizes: field_passes.h, one set with clearance.hip, whose band words this file reads)

// the words of the device statistics block (RegionsState::stats)
enum { kStSites = 0 /* 64 bits */, kStMaxD2 = 2, kStRegions = 3, kStRidge = 4 /* 64 bits */, kStOccupied = 6 /* 64 bits */,
       kStWords = 8 };

// fg[y * WW + w]: bit b = cell (64 w + b, y) is occupied; cnt: its popcount. grid (cdiv(W, 256), H)
__global__ void __launch_bounds__(kFieldTB) k_rg_pack(const int8_t *grid, int W, int WW, uint64_t *fg, int *cnt) {
    const int x = blockIdx.x * kFieldTB + threadIdx.x, y = blockIdx.y;
    const bool occ = x < W && grid[(size_t)y * W + x] == 100;
    const unsigned long long m = __ballot(occ);
    if ((threadIdx.x & 63) == 0 && x < W) {
        fg[(size_t)y * WW + (x >> 6)] = m;
        cnt[(size_t)y * WW + (x >> 6)] = __popcll(m);
    }
}

// size[root] = the component's cells (size zeroed before)
__global__ void __launch_bounds__(kFieldTB) k_rg_size(const int *parent, int nf, int *size) {
    const int i = blockIdx.x * kFieldTB + threadIdx.x;
    if (i < nf) atomicAdd(&size[parent[i]], 1);
}

// The kept components' cells become sites: sb[cell] = 100 (sb zeroed before), lab[cell] = the root's cell.
// st[kStRegions] += the kept components.
__global__ void __launch_bounds__(kFieldTB) k_rg_sites(const int *list, const int *parent, const int *size, int nf, int min_cells,
                                                       int8_t *sb, int32_t *lab, unsigned *st) {
    const int i = blockIdx.x * kFieldTB + threadIdx.x;
    bool kept_root = false;
    if (i < nf) {
        const int r = parent[i];
        if (size[r] >= min_cells) {
            const int cell = list[i];
            sb[cell] = 100;
            lab[cell] = list[r];
            kept_root = r == i;
        }
    }
    const unsigned long long m = __ballot(kept_root);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st[kStRegions], (unsigned)__popcll(m));
}

// Caller labels: sb[c] = 100 iff the cell is occupied and its label >= 0. st[kStOccupied] += the occupied cells.
__global__ void __launch_bounds__(kFieldTB) k_rg_label_sites(const int8_t *grid, const int32_t *labels, size_t C, int8_t *sb,
                                                             unsigned *st) {
    const size_t c = (size_t)blockIdx.x * kFieldTB + threadIdx.x;
    bool occ = false;
    if (c < C) {
        occ = grid[c] == 100;
        sb[c] = occ && labels[c] >= 0 ? 100 : 0;
    }
    const unsigned long long m = __ballot(occ);
    if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(reinterpret_cast<unsigned long long *>(st + kStOccupied), (unsigned long long)__popcll(m));
}

// off[y * W + x] = (the row of the column's nearest site) - y, the smaller row at equal distance; kOffNone without
// one. masks / up / down: k_clr_bands' and k_clr_carry's. grid (cdiv(W, 256), bands)
__global__ void __launch_bounds__(kFieldTB) k_rg_cols(const unsigned long long *masks, const int *up, const int *down, int W,
                                                      int H, int16_t *off) {
    const int x = blockIdx.x * kFieldTB + threadIdx.x, b = blockIdx.y;
    if (x >= W) return;
    const unsigned long long m = masks[(size_t)b * W + x];
    const int cu = up[(size_t)b * W + x], cd = down[(size_t)b * W + x];
    const int y0 = b * kFieldBand, rows = min(kFieldBand, H - y0);
    for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        const NearestRows n = band_nearest_rows(m, cu, cd, y0, r);
        int o = rgn::kOffNone;
        if (n.above >= 0) o = n.above - y;
        if (n.below >= 0 && (n.above < 0 || n.below - y < y - n.above)) o = n.below - y;
        off[(size_t)y * W + x] = (int16_t)o;
    }
}

// field_row_pass on the row offsets: a candidate is (d2, the site's linear index) and the least pair wins, so the
// prunes admit ties (an equal d2 may still win by its index)
struct RgRowPass {
    typedef int16_t Stored;
    static constexpr Stored kNone = rgn::kOffNone;
    static constexpr bool kTies = true;
    struct Cand { unsigned d2 = clr::kNone, idx = rgn::kSiteNone; };
    static __device__ __forceinline__ unsigned mag(int o) { return o == rgn::kOffNone ? kFieldMagNone : (unsigned)abs(o); }
    static __device__ __forceinline__ void update(Cand &c, int o, int x, int xp, int y, int W) {
        if (o == rgn::kOffNone) return;
        const int dx = x - xp;
        const unsigned v = (unsigned)(dx * dx + o * o);
        if (v > c.d2) return;
        const unsigned idx = (unsigned)(y + o) * (unsigned)W + (unsigned)xp;
        if (v < c.d2 || idx < c.idx) { c.d2 = v; c.idx = idx; }
    }
};

// One workgroup per row. site[y * W + x] = the linear index of the site with the least (d2, index); *max_d2: the
// maximum d2 (atomicMax per wave; kNone where no cell has a site).
__global__ void __launch_bounds__(kFieldTB) k_rg_rows(const int16_t *off, int W, uint32_t *site, unsigned *max_d2) {
    const int y = blockIdx.x;
    unsigned row_max = field_row_pass<RgRowPass>(off + (size_t)y * W, y, W, [&](int x, const RgRowPass::Cand &c) {
        site[(size_t)y * W + x] = c.idx;
    });
    row_max = wave_max_u32(row_max);
    if ((threadIdx.x & 63) == 0) atomicMax(max_d2, row_max);
}

__global__ void __launch_bounds__(kFieldTB) k_rg_region(const uint32_t *site, const int32_t *lab, size_t C, int32_t *region) {
    const size_t c = (size_t)blockIdx.x * kFieldTB + threadIdx.x;
    if (c >= C) return;
    const uint32_t s = site[c];
    region[c] = s == rgn::kSiteNone ? rgn::kRegionNone : lab[s];
}

// The pair rule seen from the cell that is marked: a cell that is no site cell is marked by its forward pairs (right,
// down) whose regions differ, and by its backward pairs (left, up) whose regions differ and whose first cell is a
// site cell. *n_ridge += the marked cells.
__global__ void __launch_bounds__(kFieldTB) k_rg_ridge(const uint32_t *site, const int32_t *region, int W, int H, int8_t *ridge,
                                                       unsigned long long *n_ridge) {
    const size_t C = (size_t)W * H, c = (size_t)blockIdx.x * kFieldTB + threadIdx.x;
    bool mark = false;
    if (c < C) {
        const int y = (int)(c / W), x = (int)(c - (size_t)y * W);
        const int32_t rc = region[c];
        if (rc != rgn::kRegionNone && site[c] != (uint32_t)c) {
            auto differs = [&](size_t n) { const int32_t r = region[n]; return r != rgn::kRegionNone && r != rc; };
            if (x + 1 < W) mark |= differs(c + 1);
            if (y + 1 < H) mark |= differs(c + W);
            if (x > 0) mark |= differs(c - 1) && site[c - 1] == (uint32_t)(c - 1);
            if (y > 0) mark |= differs(c - W) && site[c - W] == (uint32_t)(c - W);
        }
        ridge[c] = mark ? 100 : 0;
    }
    const unsigned long long m = __ballot(mark);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_ridge, (unsigned long long)__popcll(m));
}

// One thread per point; the outputs are pinned host memory, n words each. ridge_d2 nullable (every word kNone).
// st (nullable): the statistics block, copied to h_stats by the first thread with *n_comp (nullable) behind it.
__global__ void __launch_bounds__(kFieldTB) k_rg_sample(clr::Grid g, const uint32_t *site, const int32_t *region,
                                                        const uint32_t *ridge_d2, const double2 *pts, int n, uint32_t *o_site,
                                                        int32_t *o_region, uint32_t *o_d2, uint32_t *o_rd2, const unsigned *st,
                                                        const int *n_comp, uint32_t *h_stats) {
    const int i = blockIdx.x * kFieldTB + threadIdx.x;
    if (i == 0 && st) {
        for (int k = 0; k < kStWords; ++k) h_stats[k] = st[k];
        h_stats[kStWords] = n_comp ? (uint32_t)*n_comp : 0u;
    }
    if (i >= n) return;
    const double2 p = pts[i];
    int mx, my;
    uint32_t s = rgn::kSiteNone, d2 = clr::kNone, rd2 = clr::kNone;
    int32_t r = rgn::kRegionNone;
    if (clr::cell_of(g, p.x, p.y, mx, my)) {
        const size_t c = (size_t)my * g.W + mx;
        s = site[c];
        r = region[c];
        d2 = rgn::d2_of(s, mx, my, g.W);
        if (ridge_d2) rd2 = ridge_d2[c];
    }
    o_site[i] = s;
    o_region[i] = r;
    o_d2[i] = d2;
    o_rd2[i] = rd2;
}

struct RegionsState {
    CclScratch ccl;           // ccl_label's buffers; ccl.off: the words' offsets
    ClrFieldBufs sf, rf;      // the site bytes' band words and carries; the ridge's distance field (rf.d2)
    DevBuf d_grid, d_labels, fg, cnt, size, sb, lab, off, site, region, ridge, stats, nodes, pts;
    PinnedBuf h_peek, h_out, h_pts;
    std::vector<float> node_m;
    hipEvent_t ev[5] = {};
    bool have = false, have_rd = false;
    clr::Grid g{};
    aos_grid_info info{};
    ~RegionsState() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

namespace {

RegionsState &regions_state(aos_ctx *c) {
    RegionsState &S = c->regions_state.get<RegionsState>();
    for (hipEvent_t &e : S.ev) if (!e) AOS_HIP(hipEventCreate(&e));
    return S;
}

// Sites and labels from the components: S.sb, S.lab, st[kStRegions]; returns the occupied count, *n_comp_dev = where
// the component count lies on the device
int launch_components(RegionsState &S, const int8_t *d_grid, int W, int H, int min_cells, unsigned *st, const int **n_comp_dev,
                      hipStream_t s) {
    const size_t C = (size_t)W * H;
    GridC gc{};
    gc.W = W; gc.H = H; gc.WW = cdiv(W, 64);
    const size_t Cw = (size_t)gc.WW * H;
    uint64_t *fg = S.fg.ensure_n<uint64_t>(Cw);
    int *cnt = S.cnt.ensure_n<int>(Cw), *off = S.ccl.off.ensure_n<int>(Cw + 1);
    int8_t *sb = S.sb.ensure_n<int8_t>(C);
    int32_t *lab = S.lab.ensure_n<int32_t>(C);
    k_rg_pack<<<dim3(cdiv(W, kFieldTB), H), kFieldTB, 0, s>>>(d_grid, W, gc.WW, fg, cnt);
    AOS_HIP(hipGetLastError());
    scan_1p(S.ccl.lb, cnt, off, (int)Cw, false, s);
    AOS_HIP(hipMemsetAsync(sb, 0, C, s));
    int err = 0;
    const int nf = ccl_label(S.ccl, fg, off, gc, s, static_cast<int *>(S.h_peek.ensure(sizeof(int) * 2)), &err);
    if (err) throw std::runtime_error("a single-pass scan failed on the device");
    *n_comp_dev = S.ccl.rank_p + nf;
    if (nf > 0) {
        int *size = S.size.ensure_n<int>(nf);
        AOS_HIP(hipMemsetAsync(size, 0, sizeof(int) * (size_t)nf, s));
        k_rg_size<<<cdiv(nf, kFieldTB), kFieldTB, 0, s>>>(S.ccl.parent_p, nf, size);
        k_rg_sites<<<cdiv(nf, kFieldTB), kFieldTB, 0, s>>>(S.ccl.list_p, S.ccl.parent_p, size, nf, min_cells, sb, lab, st);
        AOS_HIP(hipGetLastError());
    }
    return nf;
}

}  // namespace

}  // namespace aos

using namespace aos;

extern "C" int aos_gvd_regions(aos_ctx *c, const aos_path_graph *graph, const int8_t *grid, int grid_on_device,
                               const aos_grid_info *info, const int32_t *labels, const aos_regions_opts *opts,
                               aos_regions_out *out) {
    if (!c || !out) return fail(AOS_E_INVALID, "aos_gvd_regions: null argument");
    if (grid && !info) return fail(AOS_E_INVALID, "aos_gvd_regions: grid without grid info");
    if (grid)
        if (const char *m = clr::check_info(*info)) return fail(AOS_E_INVALID, std::string("aos_gvd_regions: ") + m);
    if (graph)
        if (const char *m = clr::check_graph(graph->nodes_xy, graph->num_nodes, graph->edges, graph->num_edges))
            return fail(AOS_E_INVALID, std::string("aos_gvd_regions: ") + m);
    if (const char *m = rgn::check_regions(grid != nullptr, labels != nullptr, opts))
        return fail(AOS_E_INVALID, std::string("aos_gvd_regions: ") + m);
    const int min_cells = opts ? opts->min_component_cells : 0;
    const bool want_rd = opts && opts->want_ridge_distance != 0;
    return guarded("regions", "aos_gvd_regions", [&]() -> int {
        DeviceScope dev_scope(c->device);
        if (!graph || !grid) c->gvd_view_settle();
        // the graph (only its nodes are read) and the grid; the handle's own are checked like a caller's
        const aos_path_graph g = c->plan_graph(graph).g;
        const double *nodes_xy = g.nodes_xy;
        const int32_t nn = g.num_nodes;
        if (!graph)
            if (const char *m = clr::check_graph(nodes_xy, nn, nullptr, 0)) throw std::invalid_argument(m);
        RegionsState &S = regions_state(c);
        hipStream_t s = c->stream;
        const aos_ctx::PlanGrid pg = c->plan_grid(grid, grid_on_device, info, S.d_grid);
        const int8_t *d_grid = pg.d_grid;
        const aos_grid_info gi = pg.info;
        if (!grid)
            if (const char *m = clr::check_info(gi)) throw std::invalid_argument(m);
        const int32_t *d_labels = labels;   // (labels come with a grid, and lie where it lies: check_regions)
        if (labels && !grid_on_device) {
            const size_t C = (size_t)gi.width * gi.height;
            int32_t *dl = S.d_labels.ensure_n<int32_t>(C);
            if (C) AOS_HIP(hipMemcpyAsync(dl, labels, sizeof(int32_t) * C, hipMemcpyHostToDevice, s));
            d_labels = dl;
        }
        S.have = false;
        S.have_rd = false;
        S.info = gi;
        S.g = clr::Grid{gi.origin_x, gi.origin_y, (double)gi.resolution, (int)gi.width, (int)gi.height};
        const int W = S.g.W, H = S.g.H;
        const size_t C = (size_t)W * H;
        // pinned outputs: node site, region, d2, ridge d2, then the statistics words and the component count
        uint32_t *h = static_cast<uint32_t *>(S.h_out.ensure(sizeof(uint32_t) * (4 * (size_t)nn + kStWords + 1)));
        uint32_t *h_site = h, *h_d2 = h + 2 * (size_t)nn, *h_rd2 = h + 3 * (size_t)nn, *h_stats = h + 4 * (size_t)nn;
        int32_t *h_region = reinterpret_cast<int32_t *>(h + nn);
        float ms[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int nf = 0;
        if (C == 0) {   // no launch on an empty grid
            std::fill(h_site, h_site + nn, rgn::kSiteNone);
            std::fill(h_region, h_region + nn, rgn::kRegionNone);
            std::fill(h_d2, h_d2 + 2 * (size_t)nn, clr::kNone);
            std::fill(h_stats, h_stats + kStWords + 1, 0u);
            h_stats[kStMaxD2] = clr::kNone;
        } else {
            double2 *d_nodes = S.nodes.ensure_n<double2>(nn);
            if (nn) AOS_HIP(hipMemcpyAsync(d_nodes, nodes_xy, sizeof(double2) * (size_t)nn, hipMemcpyHostToDevice, s));
            unsigned *st = S.stats.ensure_n<unsigned>(kStWords);
            AOS_HIP(hipMemsetAsync(st, 0, sizeof(unsigned) * kStWords, s));
            AOS_HIP(hipEventRecord(S.ev[0], s));
            // 1. sites and labels
            const int32_t *lab;
            const int *n_comp_dev = nullptr;
            if (d_labels) {
                k_rg_label_sites<<<cdiv(C, kFieldTB), kFieldTB, 0, s>>>(d_grid, d_labels, C, S.sb.ensure_n<int8_t>(C), st);
                lab = d_labels;
            } else {
                nf = launch_components(S, d_grid, W, H, min_cells, st, &n_comp_dev, s);
                lab = S.lab.as<int32_t>();
            }
            const int8_t *sb = S.sb.as<int8_t>();
            AOS_HIP(hipEventRecord(S.ev[1], s));
            // 2, 3. the column pass with direction, the row pass with the site
            const int nb = cdiv(H, kFieldBand);
            int16_t *off = S.off.ensure_n<int16_t>(C);
            uint32_t *site = S.site.ensure_n<uint32_t>(C);
            clr_launch_bands(S.sf, sb, W, H, reinterpret_cast<unsigned long long *>(st + kStSites), s);
            k_rg_cols<<<dim3(cdiv(W, kFieldTB), nb), kFieldTB, 0, s>>>(S.sf.masks.as<unsigned long long>(), S.sf.up.as<int>(),
                                                                   S.sf.down.as<int>(), W, H, off);
            k_rg_rows<<<H, kFieldTB, 0, s>>>(off, W, site, st + kStMaxD2);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipEventRecord(S.ev[2], s));
            // 4, 5. region, ridge, the ridge's distance field
            int32_t *region = S.region.ensure_n<int32_t>(C);
            int8_t *ridge = S.ridge.ensure_n<int8_t>(C);
            k_rg_region<<<cdiv(C, kFieldTB), kFieldTB, 0, s>>>(site, lab, C, region);
            k_rg_ridge<<<cdiv(C, kFieldTB), kFieldTB, 0, s>>>(site, region, W, H, ridge,
                                                          reinterpret_cast<unsigned long long *>(st + kStRidge));
            AOS_HIP(hipGetLastError());
            if (want_rd) clr_launch_field(S.rf, ridge, W, H, s);
            AOS_HIP(hipEventRecord(S.ev[3], s));
            // 6. sampling and the statistics
            k_rg_sample<<<std::max(1, cdiv(nn, kFieldTB)), kFieldTB, 0, s>>>(
                S.g, site, region, want_rd ? S.rf.d2.as<uint32_t>() : nullptr, d_nodes, nn, h_site, h_region, h_d2, h_rd2, st,
                n_comp_dev, h_stats);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipEventRecord(S.ev[4], s));
            AOS_HIP(hipStreamSynchronize(s));
            for (int k = 0; k < 4; ++k) (void)hipEventElapsedTime(&ms[k], S.ev[k], S.ev[k + 1]);
        }
        S.node_m.resize(nn);
        clr::to_metres(h_rd2, nn, S.g.res, S.node_m.data());
        S.have = true;
        S.have_rd = want_rd && C;
        auto u64 = [&](int k) { return (uint64_t)h_stats[k] | ((uint64_t)h_stats[k + 1] << 32); };
        std::memset(out, 0, sizeof(*out));
        out->info = gi;
        out->n_sites = u64(kStSites);
        out->n_ridge = u64(kStRidge);
        out->n_occupied = labels ? u64(kStOccupied) : (uint64_t)nf;
        out->n_components = labels ? -1 : (int64_t)h_stats[kStWords];
        out->n_regions = labels ? -1 : (int64_t)h_stats[kStRegions];
        out->max_d2 = out->n_sites ? h_stats[kStMaxD2] : clr::kNone;
        if (C) {
            out->site_device = S.site.as<uint32_t>();
            out->region_device = S.region.as<int32_t>();
            out->ridge_device = S.ridge.as<int8_t>();
            out->ridge_d2_device = want_rd ? S.rf.d2.as<uint32_t>() : nullptr;
        }
        out->num_nodes = nn;
        out->node_site = h_site; out->node_region = h_region; out->node_d2 = h_d2; out->node_ridge_d2 = h_rd2;
        out->node_ridge_offset = S.node_m.data();
        out->ms_label = ms[0]; out->ms_field = ms[1]; out->ms_ridge = ms[2]; out->ms_graph = ms[3];
        return AOS_OK;
    });
}

extern "C" int aos_regions_field_copy(aos_ctx *c, const char *which, void *dst, uint64_t capacity_cells) {
    if (!c) return fail(AOS_E_INVALID, "aos_regions_field_copy: null handle");
    const int f = rgn::field_of(which);
    if (f < 0) return fail(AOS_E_INVALID, "aos_regions_field_copy: which is none of site, region, ridge, ridge_d2");
    const RegionsState *S = c->regions_state.peek<RegionsState>();
    if (!S || !S->have) return fail(AOS_E_STATE, "aos_regions_field_copy: no aos_gvd_regions on this handle yet");
    const uint64_t C = (uint64_t)S->g.W * (uint64_t)S->g.H;
    if (f == rgn::kRidgeD2 && C && !S->have_rd)
        return fail(AOS_E_INVALID, "aos_regions_field_copy: the last aos_gvd_regions did not compute ridge_d2");
    if (capacity_cells < C) return fail(AOS_E_INVALID, "aos_regions_field_copy: capacity below width x height");
    if (C && !dst) return fail(AOS_E_INVALID, "aos_regions_field_copy: null destination");
    return guarded("regions", "aos_regions_field_copy", [&]() -> int {
        DeviceScope dev_scope(c->device);
        if (C) {
            const void *src[4] = {S->site.p, S->region.p, S->ridge.p, S->rf.d2.p};
            AOS_HIP(hipMemcpyAsync(dst, src[f], rgn::field_bytes(f) * C, hipMemcpyDeviceToHost, c->stream));
            AOS_HIP(hipStreamSynchronize(c->stream));
        }
        return AOS_OK;
    });
}

extern "C" int aos_regions_points(aos_ctx *c, const double *xy, int32_t n, uint32_t *site, int32_t *region, uint32_t *d2,
                                  uint32_t *ridge_d2, float *ridge_offset_m) {
    if (!c) return fail(AOS_E_INVALID, "aos_regions_points: null handle");
    if (n < 0) return fail(AOS_E_INVALID, "aos_regions_points: negative count");
    if (n > 0 && !xy) return fail(AOS_E_INVALID, "aos_regions_points: null points behind a count above 0");
    RegionsState *S = c->regions_state.peek<RegionsState>();
    if (!S || !S->have) return fail(AOS_E_STATE, "aos_regions_points: no aos_gvd_regions on this handle yet");
    if (n == 0) return AOS_OK;
    return guarded("regions", "aos_regions_points", [&]() -> int {
        DeviceScope dev_scope(c->device);
        const size_t N = (size_t)n;
        uint32_t *h = static_cast<uint32_t *>(S->h_pts.ensure(sizeof(uint32_t) * 4 * N));
        if ((size_t)S->g.W * S->g.H == 0) {
            std::fill(h, h + N, rgn::kSiteNone);
            std::fill(h + N, h + 2 * N, (uint32_t)rgn::kRegionNone);
            std::fill(h + 2 * N, h + 4 * N, clr::kNone);
        } else {
            double2 *d_pts = S->pts.ensure_n<double2>(N);
            AOS_HIP(hipMemcpyAsync(d_pts, xy, sizeof(double2) * N, hipMemcpyHostToDevice, c->stream));
            k_rg_sample<<<cdiv(n, kFieldTB), kFieldTB, 0, c->stream>>>(
                S->g, S->site.as<uint32_t>(), S->region.as<int32_t>(), S->have_rd ? S->rf.d2.as<uint32_t>() : nullptr, d_pts, n,
                h, reinterpret_cast<int32_t *>(h + N), h + 2 * N, h + 3 * N, nullptr, nullptr, nullptr);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipStreamSynchronize(c->stream));
        }
        if (site) std::memcpy(site, h, sizeof(uint32_t) * N);
        if (region) std::memcpy(region, h + N, sizeof(uint32_t) * N);
        if (d2) std::memcpy(d2, h + 2 * N, sizeof(uint32_t) * N);
        if (ridge_d2) std::memcpy(ridge_d2, h + 3 * N, sizeof(uint32_t) * N);
        if (ridge_offset_m) clr::to_metres(h + 3 * N, N, S->g.res, ridge_offset_m);
        return AOS_OK;
    });
}
