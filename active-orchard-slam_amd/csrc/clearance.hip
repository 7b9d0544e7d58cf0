// aos_gvd_clearance: the exact squared Euclidean distance field over a grid's occupied cells (byte == 100) and the
// clearances of a GvdGraph's nodes and edges and of arbitrary points (clearance.h has the definitions). The
// reference declares GvdGraph.edge_clearances and never computes it (EdgeRecord::min_clearance_m stays 0,
// gvd:466, :1000-1006, :1637); aos_gvd_out.edge_clearances keeps that zero, this call is the real value.
//
// What runs where:
//   column pass   GPU  k_clr_bands: a (64-row band, column)'s occupancy as one 64-bit word, bytes read coalesced
//                      along x, and the occupied count; k_clr_carry: per column, the nearest occupied row above
//                      and below each band (one thread per column over H / 64 words); k_clr_cols: g[y][x] = the
//                      vertical distance to the column's nearest occupied cell (uint16, 0xFFFF: none), each
//                      (band, column) thread from its word and its two carries: W x H / 64 threads in all
//   row pass      GPU  k_clr_rows: one workgroup per row with the row's g in LDS, d2[x] = min over x' of
//                      (x - x')^2 + g[x']^2. A cell scans its own 64-column block, then the blocks left and right
//                      of it outwards; a block whose (distance to the block)^2 + (the block's smallest g)^2 cannot
//                      win is skipped, and the walk ends once (distance to the block)^2 alone cannot win on either
//                      side. Only candidates that cannot lower the minimum are left out, so the words are exact.
//                      A wave's 64 cells share their block, so every LDS read of the walk is a broadcast.
//   sampling      GPU  k_clr_sample: one thread per node (or point); a workgroup's 256 edges flattened into
//                      their samples as k_occupancy does, atomicMin into an LDS word per edge; the results are
//                      stored into pinned host memory by the kernel
//   metres, checks     host (clearance_host.cpp)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "aos_ctx.h"
#include "clearance.h"
#include "dev_prims_device.h"
#include "field_passes.h"

namespace aos {

// (the band, workgroup and block sizes: field_passes.h)
constexpr int kClrPer = 8;         // consecutive samples a thread takes per round (k_occupancy's kOccPer)

// masks[b * W + x]: bit r = cell (x, b * 64 + r) is occupied. grid (cdiv(W, 256), bands)
__global__ void __launch_bounds__(kFieldTB) k_clr_bands(const int8_t *grid, int W, int H, unsigned long long *masks,
                                                        unsigned long long *n_occ) {
    const int x = blockIdx.x * kFieldTB + threadIdx.x, b = blockIdx.y;
    unsigned long long m = 0;
    if (x < W) {
        const int y0 = b * kFieldBand, rows = min(kFieldBand, H - y0);
        const int8_t *p = grid + (size_t)y0 * W + x;
        for (int r = 0; r < rows; ++r)
            if (p[(size_t)r * W] == 100) m |= 1ull << r;
        masks[(size_t)b * W + x] = m;
    }
    int cnt = __popcll(m);
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_occ, (unsigned long long)cnt);
}

// up[b * W + x] / down[b * W + x]: the column's nearest occupied row above / below band b (-1: none)
__global__ void __launch_bounds__(kFieldTB) k_clr_carry(const unsigned long long *masks, int W, int nb, int *up, int *down) {
    const int x = blockIdx.x * kFieldTB + threadIdx.x;
    if (x >= W) return;
    int last = -1;
    for (int b = 0; b < nb; ++b) {
        up[(size_t)b * W + x] = last;
        const unsigned long long m = masks[(size_t)b * W + x];
        if (m) last = b * kFieldBand + 63 - __clzll((long long)m);
    }
    last = -1;
    for (int b = nb - 1; b >= 0; --b) {
        down[(size_t)b * W + x] = last;
        const unsigned long long m = masks[(size_t)b * W + x];
        if (m) last = b * kFieldBand + __ffsll((long long)m) - 1;
    }
}

// g[y * W + x] = min over the column's occupied rows y' of |y - y'|, kColNone without one. grid as k_clr_bands
__global__ void __launch_bounds__(kFieldTB) k_clr_cols(const unsigned long long *masks, const int *up, const int *down, int W,
                                                       int H, uint16_t *g) {
    const int x = blockIdx.x * kFieldTB + threadIdx.x, b = blockIdx.y;
    if (x >= W) return;
    const unsigned long long m = masks[(size_t)b * W + x];
    const int cu = up[(size_t)b * W + x], cd = down[(size_t)b * W + x];
    const int y0 = b * kFieldBand, rows = min(kFieldBand, H - y0);
    for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        const NearestRows n = band_nearest_rows(m, cu, cd, y0, r);
        int d = clr::kColNone;
        if (n.above >= 0) d = y - n.above;
        if (n.below >= 0) d = min(d, n.below - y);
        g[(size_t)y * W + x] = (uint16_t)d;
    }
}

// field_row_pass on the column distances: a candidate is its d2 alone, so a bound equal to the best cannot win
struct ClrRowPass {
    typedef uint16_t Stored;
    static constexpr Stored kNone = clr::kColNone;
    static constexpr bool kTies = false;
    struct Cand { unsigned d2 = clr::kNone; };
    static __device__ __forceinline__ unsigned mag(int v) { return (unsigned)v; }
    static __device__ __forceinline__ void update(Cand &c, unsigned gv, int x, int xp, int, int) {
        const unsigned dx = (unsigned)abs(x - xp);
        const unsigned v = gv == clr::kColNone ? clr::kNone : dx * dx + gv * gv;
        c.d2 = min(c.d2, v);
    }
};

// One workgroup per row. max_d2: the field's maximum (atomicMax per wave).
__global__ void __launch_bounds__(kFieldTB) k_clr_rows(const uint16_t *g, int W, uint32_t *d2, unsigned *max_d2) {
    const int y = blockIdx.x;
    unsigned row_max = field_row_pass<ClrRowPass>(g + (size_t)y * W, y, W, [&](int x, const ClrRowPass::Cand &c) {
        d2[(size_t)y * W + x] = c.d2;
    });
    row_max = wave_max_u32(row_max);
    if ((threadIdx.x & 63) == 0) atomicMax(max_d2, row_max);
}

__device__ __forceinline__ uint32_t clr_at(const uint32_t *d2, const clr::Grid &g, double px, double py) {
    int mx, my;
    return clr::cell_of(g, px, py, mx, my) ? d2[(size_t)my * g.W + mx] : clr::kNone;
}

// Workgroups [0, nbn) take 256 nodes each, one per thread; the others 256 edges each. node_out / edge_out: pinned
// host memory. stats (nullable): the field's occupied count and maximum, copied to h_stats[0 .. 2] (count low,
// count high, maximum) by the first thread.
__global__ void __launch_bounds__(kFieldTB) k_clr_sample(clr::Grid g, const uint32_t *d2, const double2 *nodes, int n_nodes,
                                                         const int2 *edges, int n_edges, int nbn, uint32_t *node_out,
                                                         uint32_t *edge_out, const unsigned long long *n_occ,
                                                         const unsigned *max_d2, uint32_t *h_stats) {
    __shared__ int pre[kFieldTB + 1], wsum[kFieldTB / 64], tot_s;
    __shared__ unsigned best_s[kFieldTB];
    __shared__ clr::Edge e_s[kFieldTB];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0 && h_stats) {
        const unsigned long long n = *n_occ;
        h_stats[0] = (uint32_t)n;
        h_stats[1] = (uint32_t)(n >> 32);
        h_stats[2] = *max_d2;
    }
    if ((int)blockIdx.x < nbn) {
        const int i = blockIdx.x * kFieldTB + tid;
        if (i < n_nodes) {
            const double2 p = nodes[i];
            node_out[i] = clr_at(d2, g, p.x, p.y);
        }
        return;
    }
    const int c = ((int)blockIdx.x - nbn) * kFieldTB + tid;
    int nsamp = 0;
    unsigned first = clr::kNone;
    if (c < n_edges) {
        const int2 e2 = edges[c];
        const double2 s = nodes[e2.x], t = nodes[e2.y];
        const double ex = t.x - s.x, ey = t.y - s.y;
        const double len = sqrt(ex * ex + ey * ey);
        if (len < clr::kMinLen) first = clr_at(d2, g, s.x, s.y);
        else {
            const clr::Edge e = clr::make_edge(g, s.x, s.y, t.x, t.y, len);
            e_s[tid] = e;
            if (e.i1 >= e.i0) nsamp = e.i1 - e.i0 + 1;
        }
    }
    best_s[tid] = first;
    const int before = block_excl_scan<kFieldTB>(nsamp, wsum, &tot_s);   // (synchronises)
    pre[tid] = before;
    if (tid == 0) pre[kFieldTB] = tot_s;
    __syncthreads();
    const int T = pre[kFieldTB];
    for (int q0 = 0; q0 < T; q0 += kFieldTB * kClrPer) {
        // the thread's kClrPer consecutive samples: one search for the first one's edge, then forward
        const int qb = q0 + tid * kClrPer;
        if (qb >= T) continue;
        int lo = 0, hi = kFieldTB - 1;   // the edge o with pre[o] <= qb < pre[o + 1]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pre[mid] <= qb) lo = mid; else hi = mid - 1;
        }
        int o = lo;
        unsigned v[kClrPer];
        int oo[kClrPer];
#pragma unroll
        for (int u = 0; u < kClrPer; ++u) {
            const int q = qb + u;
            v[u] = clr::kNone;
            oo[u] = -1;
            if (q >= T) continue;
            while (pre[o + 1] <= q) ++o;   // (q < T = pre[kFieldTB]: o stays below kFieldTB)
            oo[u] = o;
            double px, py;
            clr::sample_point(e_s[o], e_s[o].i0 + (q - pre[o]), px, py);
            v[u] = clr_at(d2, g, px, py);
        }
#pragma unroll
        for (int u = 0; u < kClrPer; ++u)
            if (oo[u] >= 0 && v[u] != clr::kNone) atomicMin(&best_s[oo[u]], v[u]);
    }
    __syncthreads();
    if (c < n_edges) edge_out[c] = best_s[tid];
}

struct ClearState {
    ClrFieldBufs f;   // the field's scratch, the field (f.d2) and its statistics (f.stats)
    DevBuf d_grid, d_nodes, d_edges, d_pts;
    PinnedBuf h_out, h_pts;
    std::vector<float> node_m, edge_m;
    hipEvent_t ev[3] = {};
    bool have_field = false;
    clr::Grid g{};
    aos_grid_info info{};
    ~ClearState() {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

// the band words and the carries of d_grid (W, H >= 1); *n_occ += the occupied count (regions.hip shares these two)
void clr_launch_bands(ClrFieldBufs &B, const int8_t *d_grid, int W, int H, unsigned long long *n_occ, hipStream_t s) {
    const int nb = cdiv(H, kFieldBand);
    auto *masks = B.masks.ensure_n<unsigned long long>((size_t)nb * W);
    int *up = B.up.ensure_n<int>((size_t)nb * W), *down = B.down.ensure_n<int>((size_t)nb * W);
    k_clr_bands<<<dim3(cdiv(W, kFieldTB), nb), kFieldTB, 0, s>>>(d_grid, W, H, masks, n_occ);
    k_clr_carry<<<cdiv(W, kFieldTB), kFieldTB, 0, s>>>(masks, W, nb, up, down);
}

// the three field passes on d_grid (W, H >= 1) into B.d2; B.stats: the occupied count (8 bytes), the maximum
void clr_launch_field(ClrFieldBufs &B, const int8_t *d_grid, int W, int H, hipStream_t s) {
    const size_t C = (size_t)W * H;
    const int nb = cdiv(H, kFieldBand);
    uint16_t *g = B.g.ensure_n<uint16_t>(C);
    uint32_t *d2 = B.d2.ensure_n<uint32_t>(C);
    char *st = B.stats.ensure_n<char>(16);
    AOS_HIP(hipMemsetAsync(st, 0, 16, s));
    clr_launch_bands(B, d_grid, W, H, reinterpret_cast<unsigned long long *>(st), s);
    k_clr_cols<<<dim3(cdiv(W, kFieldTB), nb), kFieldTB, 0, s>>>(B.masks.as<unsigned long long>(), B.up.as<int>(),
                                                                 B.down.as<int>(), W, H, g);
    k_clr_rows<<<H, kFieldTB, 0, s>>>(g, W, d2, reinterpret_cast<unsigned *>(st + 8));
    AOS_HIP(hipGetLastError());
}

namespace {

ClearState &clear_state(aos_ctx *c) {
    ClearState &S = c->clear_state.get<ClearState>();
    for (hipEvent_t &e : S.ev) if (!e) AOS_HIP(hipEventCreate(&e));
    return S;
}

}  // namespace

}  // namespace aos

using namespace aos;

extern "C" int aos_gvd_clearance(aos_ctx *c, const aos_path_graph *graph, const int8_t *grid, int grid_on_device,
                                 const aos_grid_info *info, aos_clearance_out *out) {
    if (!c || !out) return fail(AOS_E_INVALID, "aos_gvd_clearance: null argument");
    if (grid && !info) return fail(AOS_E_INVALID, "aos_gvd_clearance: grid without grid info");
    if (grid)
        if (const char *m = clr::check_info(*info)) return fail(AOS_E_INVALID, std::string("aos_gvd_clearance: ") + m);
    if (graph)
        if (const char *m = clr::check_graph(graph->nodes_xy, graph->num_nodes, graph->edges, graph->num_edges))
            return fail(AOS_E_INVALID, std::string("aos_gvd_clearance: ") + m);
    return guarded("clearance", "aos_gvd_clearance", [&]() -> int {
        DeviceScope dev_scope(c->device);
        if (!graph || !grid) c->gvd_view_settle();
        // the graph (only its nodes and edges are read) and the grid; the handle's own are checked like a caller's
        const aos_path_graph g = c->plan_graph(graph).g;
        const double *nodes_xy = g.nodes_xy;
        const int32_t *edges = g.edges;
        const int32_t nn = g.num_nodes, ne = g.num_edges;
        if (!graph)
            if (const char *m = clr::check_graph(nodes_xy, nn, edges, ne)) throw std::invalid_argument(m);
        ClearState &S = clear_state(c);
        const aos_ctx::PlanGrid pg = c->plan_grid(grid, grid_on_device, info, S.d_grid);
        const int8_t *d_grid = pg.d_grid;
        const aos_grid_info gi = pg.info;
        if (!grid)
            if (const char *m = clr::check_info(gi)) throw std::invalid_argument(m);
        S.have_field = false;
        S.info = gi;
        S.g = clr::Grid{gi.origin_x, gi.origin_y, (double)gi.resolution, (int)gi.width, (int)gi.height};
        const size_t C = (size_t)gi.width * gi.height;
        // pinned outputs: node d2, edge d2, then the three stats words
        const size_t n_words = (size_t)nn + (size_t)ne + 4;
        uint32_t *h = static_cast<uint32_t *>(S.h_out.ensure(sizeof(uint32_t) * n_words));
        uint32_t *h_node = h, *h_edge = h + nn, *h_stats = h + nn + ne;
        float ms_field = 0.0f, ms_graph = 0.0f;
        if (C == 0) {   // no launch on an empty field
            std::fill(h, h + nn + ne, clr::kNone);
            h_stats[0] = h_stats[1] = 0;
            h_stats[2] = clr::kNone;
        } else {
            double2 *d_nodes = S.d_nodes.ensure_n<double2>(nn);
            int2 *d_edges = S.d_edges.ensure_n<int2>(ne);
            if (nn) AOS_HIP(hipMemcpyAsync(d_nodes, nodes_xy, sizeof(double2) * (size_t)nn, hipMemcpyHostToDevice, c->stream));
            if (ne) AOS_HIP(hipMemcpyAsync(d_edges, edges, sizeof(int2) * (size_t)ne, hipMemcpyHostToDevice, c->stream));
            AOS_HIP(hipEventRecord(S.ev[0], c->stream));
            clr_launch_field(S.f, d_grid, S.g.W, S.g.H, c->stream);
            AOS_HIP(hipEventRecord(S.ev[1], c->stream));
            const int nbn = cdiv(nn, kFieldTB), nbe = cdiv(ne, kFieldTB);
            const char *st = S.f.stats.as<char>();
            k_clr_sample<<<std::max(1, nbn + nbe), kFieldTB, 0, c->stream>>>(
                S.g, S.f.d2.as<uint32_t>(), d_nodes, nn, d_edges, ne, nbn, h_node, h_edge,
                reinterpret_cast<const unsigned long long *>(st), reinterpret_cast<const unsigned *>(st + 8), h_stats);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipEventRecord(S.ev[2], c->stream));
            AOS_HIP(hipStreamSynchronize(c->stream));
            (void)hipEventElapsedTime(&ms_field, S.ev[0], S.ev[1]);
            (void)hipEventElapsedTime(&ms_graph, S.ev[1], S.ev[2]);
        }
        S.node_m.resize(nn);
        S.edge_m.resize(ne);
        clr::to_metres(h_node, nn, S.g.res, S.node_m.data());
        clr::to_metres(h_edge, ne, S.g.res, S.edge_m.data());
        S.have_field = true;
        std::memset(out, 0, sizeof(*out));
        out->info = gi;
        out->n_occupied = (uint64_t)h_stats[0] | ((uint64_t)h_stats[1] << 32);
        out->max_d2 = out->n_occupied ? h_stats[2] : clr::kNone;
        out->d2_device = C ? S.f.d2.as<uint32_t>() : nullptr;
        out->num_nodes = nn; out->num_edges = ne;
        out->node_d2 = h_node; out->edge_d2 = h_edge;
        out->node_clearances = S.node_m.data(); out->edge_clearances = S.edge_m.data();
        out->ms_field = ms_field; out->ms_graph = ms_graph;
        return AOS_OK;
    });
}

extern "C" int aos_clearance_field_copy(aos_ctx *c, uint32_t *dst, uint64_t capacity_cells) {
    if (!c) return fail(AOS_E_INVALID, "aos_clearance_field_copy: null handle");
    const ClearState *S = c->clear_state.peek<ClearState>();
    if (!S || !S->have_field) return fail(AOS_E_STATE, "aos_clearance_field_copy: no aos_gvd_clearance on this handle yet");
    const uint64_t C = (uint64_t)S->g.W * (uint64_t)S->g.H;
    if (capacity_cells < C) return fail(AOS_E_INVALID, "aos_clearance_field_copy: capacity below width x height");
    if (C && !dst) return fail(AOS_E_INVALID, "aos_clearance_field_copy: null destination");
    return guarded("clearance", "aos_clearance_field_copy", [&]() -> int {
        DeviceScope dev_scope(c->device);
        if (C) {
            AOS_HIP(hipMemcpyAsync(dst, S->f.d2.p, sizeof(uint32_t) * C, hipMemcpyDeviceToHost, c->stream));
            AOS_HIP(hipStreamSynchronize(c->stream));
        }
        return AOS_OK;
    });
}

extern "C" int aos_clearance_points(aos_ctx *c, const double *xy, int32_t n, uint32_t *d2_out, float *metres_out) {
    if (!c) return fail(AOS_E_INVALID, "aos_clearance_points: null handle");
    if (n < 0) return fail(AOS_E_INVALID, "aos_clearance_points: negative count");
    if (n > 0 && !xy) return fail(AOS_E_INVALID, "aos_clearance_points: null points behind a count above 0");
    ClearState *S = c->clear_state.peek<ClearState>();
    if (!S || !S->have_field) return fail(AOS_E_STATE, "aos_clearance_points: no aos_gvd_clearance on this handle yet");
    if (n == 0) return AOS_OK;
    return guarded("clearance", "aos_clearance_points", [&]() -> int {
        DeviceScope dev_scope(c->device);
        uint32_t *h = static_cast<uint32_t *>(S->h_pts.ensure(sizeof(uint32_t) * (size_t)n));
        if ((size_t)S->g.W * S->g.H == 0) std::fill(h, h + n, clr::kNone);
        else {
            double2 *d_pts = S->d_pts.ensure_n<double2>(n);
            AOS_HIP(hipMemcpyAsync(d_pts, xy, sizeof(double2) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            const int nbn = cdiv(n, kFieldTB);
            k_clr_sample<<<nbn, kFieldTB, 0, c->stream>>>(S->g, S->f.d2.as<uint32_t>(), d_pts, n, nullptr, 0, nbn, h, nullptr,
                                                        nullptr, nullptr, nullptr);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipStreamSynchronize(c->stream));
        }
        if (d2_out) std::memcpy(d2_out, h, sizeof(uint32_t) * (size_t)n);
        if (metres_out) clr::to_metres(h, n, S->g.res, metres_out);
        return AOS_OK;
    });
}
