// aos_gvd_reach: the clearance-limited cost-to-go field over a grid (5 per axis move, 7 per diagonal move between
// passable cells, no corner cutting), its values at a GvdGraph's nodes and at arbitrary points, and descent paths on it
// (reach.h and include/aos_gpu.h have the definitions). Everything is integer, and the field is the unique fixed point
// of cost[c] = min(cost[c], cost[n] + w) over the allowed moves: any relaxation order ends at the same words.
//
// What runs where:
//   mask          GPU  clearance.hip's field passes on this state's own buffers when min_d2 >= 2 (clr_launch_field);
//                      k_rc_mask: the passable bytes, every cost word set to none, the passable count (one atomic per
//                      wave); k_rc_seed: one thread per source, zeroes its cell and flags the 3 x 3 tiles around it
//   rounds        GPU  k_rc_round, one plain launch per round, one workgroup per kTile x kTile tile: a tile that is not
//                      flagged leaves at once; a flagged one loads its costs with a one-cell halo and its passable bytes
//                      into LDS, relaxes there until nothing changes, writes back the words that fell and flags the
//                      neighbours (8, corners included) behind every border cell that fell. The flags are double
//                      buffered: a round reads one image (each tile clears its own word) and writes the other.
//                      Rounds go out kBatch at a time; k_rc_peek then stores "did a tile run in the batch's last
//                      round" into pinned memory, and the host stops at zero. No workgroup waits for another.
//   statistics    GPU  k_rc_stats: one pass over the field, the reached count and the maximum per wave
//   sampling      GPU  k_rc_sample: one thread per node or point, stored into pinned host memory by the kernel
//   descent       GPU  k_rc_descend: one wave; lanes 0..7 read the eight neighbours, a ballot picks the first admissible
//   metres, centres, checks    host (reach_host.cpp)
// Host waits: one per batch of rounds and the call's final stream synchronise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "aos_ctx.h"
#include "field_passes.h"
#include "reach.h"
#include "reach_state.h"

namespace aos {

using rch::kBatch;
using rch::kTile;
using rch::kTileTB;

constexpr int kRcPitch = kTile + 2;                        // the tile with its halo, LDS words per row
constexpr int kRcPer = kTile * kTile / kTileTB;            // cells per thread
constexpr int kRcRowStep = kTileTB / kTile;                // rows between a thread's cells
constexpr uint32_t kRcInf = 0x80000000u;                   // none inside LDS: above every finite cost, and + 7 does not wrap
static_assert(kTile * kTile % kTileTB == 0 && kTileTB % kTile == 0 && kTileTB % 64 == 0, "a thread's cells share a column");

// the words of the device statistics block (ReachState::stats)
enum { kStPassable = 0 /* 64 bits */, kStReached = 2 /* 64 bits */, kStRuns = 4 /* 64 bits */, kStMaxCost = 6, kStUsed = 7,
       kStRounds = 8, kStWords = 10 };

// pass[c] = the cell is passable; cost[c] = none. d2 null: min_d2 <= 1. st[kStPassable] += the passable cells.
__global__ void __launch_bounds__(kFieldTB) k_rc_mask(const int8_t *grid, const uint32_t *d2, uint32_t min_d2, size_t C,
                                                      uint8_t *pass, uint32_t *cost, unsigned *st) {
    const size_t c = (size_t)blockIdx.x * kFieldTB + threadIdx.x;
    bool p = false;
    if (c < C) {
        p = grid[c] != 100 && (!d2 || d2[c] >= min_d2);
        pass[c] = p;
        cost[c] = rch::kNone;
    }
    const unsigned long long m = __ballot(p);
    if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(reinterpret_cast<unsigned long long *>(st + kStPassable), (unsigned long long)__popcll(m));
}

// One thread per source: a source with a passable cell zeroes it and flags the tiles within one tile of its own (a
// source on a tile's border is a changed border cell for the neighbours). st[kStUsed] += the sources kept.
__global__ void __launch_bounds__(kFieldTB) k_rc_seed(clr::Grid g, const double2 *src, int n, const uint8_t *pass, uint32_t *cost,
                                                      int ntx, int nty, int *flags, unsigned *st) {
    const int i = blockIdx.x * kFieldTB + threadIdx.x;
    bool used = false;
    if (i < n) {
        const double2 p = src[i];
        int mx, my;
        if (clr::cell_of(g, p.x, p.y, mx, my) && pass[(size_t)my * g.W + mx]) {
            used = true;
            cost[(size_t)my * g.W + mx] = 0;
            const int tx = mx / kTile, ty = my / kTile;
            for (int y = max(ty - 1, 0); y <= min(ty + 1, nty - 1); ++y)
                for (int x = max(tx - 1, 0); x <= min(tx + 1, ntx - 1); ++x) flags[(size_t)y * ntx + x] = 1;
        }
    }
    const unsigned long long m = __ballot(used);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st[kStUsed], (unsigned)__popcll(m));
}

// One round. grid (ntx, nty): workgroup (bx, by) owns the cells [bx * kTile, +kTile) x [by * kTile, +kTile) and writes
// no other. It reads its halo from the neighbours' cells while they may be writing them: a word is read whole, every
// value a cell ever holds is the cost of a real path, and a neighbour whose border cell falls flags this tile for the
// next round, so a stale word costs a round, never the result. Inside LDS the same holds between threads: the loop ends
// after a pass in which no thread stored, and such a pass read only final words.
__global__ void __launch_bounds__(kTileTB) k_rc_round(uint32_t *cost, const uint8_t *pass, int W, int H, int ntx, int nty,
                                                      int *cur, int *next, int *ran, unsigned *st) {
    __shared__ uint32_t s_cost[kRcPitch * kRcPitch];
    __shared__ uint8_t s_pass[kRcPitch * kRcPitch];
    __shared__ int s_flag;
    __shared__ unsigned s_dirs;
    const int tid = threadIdx.x, bx = blockIdx.x, by = blockIdx.y;
    const size_t t = (size_t)by * ntx + bx;
    if (tid == 0) {   // one reader of the flag, so the whole workgroup takes the same way
        const int f = cur[t];
        s_flag = f;
        s_dirs = 0;
        if (f) {
            cur[t] = 0;
            *ran = 1;
            atomicAdd(reinterpret_cast<unsigned long long *>(st + kStRuns), 1ull);
        }
    }
    __syncthreads();
    if (!s_flag) return;
    const int x0 = bx * kTile - 1, y0 = by * kTile - 1;   // the window's first cell
    for (int i = tid; i < kRcPitch * kRcPitch; i += kTileTB) {
        const int wy = i / kRcPitch, wx = i - wy * kRcPitch;
        const int gx = x0 + wx, gy = y0 + wy;
        uint32_t v = kRcInf;
        uint8_t p = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t c = (size_t)gy * W + gx;
            p = pass[c];
            const uint32_t cv = cost[c];
            if (cv != rch::kNone) v = cv;
        }
        s_cost[i] = v;
        s_pass[i] = p;
    }
    __syncthreads();
    // the thread's cells: column lx, rows ly + k * kRcRowStep
    const int lx = tid % kTile, ly = tid / kTile;
    uint32_t orig[kRcPer];
    unsigned ok[kRcPer];   // bit 0: the cell is passable; bits 1..4: the diagonal (+,+), (-,+), (+,-), (-,-) is allowed
#pragma unroll
    for (int k = 0; k < kRcPer; ++k) {
        const int li = (ly + k * kRcRowStep + 1) * kRcPitch + lx + 1;
        orig[k] = s_cost[li];
        const unsigned r = s_pass[li + 1], l = s_pass[li - 1], d = s_pass[li + kRcPitch], u = s_pass[li - kRcPitch];
        ok[k] = s_pass[li] ? (1u | (r & d) << 1 | (l & d) << 2 | (r & u) << 3 | (l & u) << 4) : 0u;
    }
    volatile uint32_t *sc = s_cost;
    for (;;) {
        bool fell = false;
#pragma unroll
        for (int k = 0; k < kRcPer; ++k) {
            if (!ok[k]) continue;
            const int li = (ly + k * kRcRowStep + 1) * kRcPitch + lx + 1;
            const uint32_t mine = sc[li];
            const uint32_t axis = min(min(sc[li + 1], sc[li - 1]), min(sc[li + kRcPitch], sc[li - kRcPitch]));
            uint32_t diag = kRcInf;
            if (ok[k] & 2u) diag = min(diag, sc[li + kRcPitch + 1]);
            if (ok[k] & 4u) diag = min(diag, sc[li + kRcPitch - 1]);
            if (ok[k] & 8u) diag = min(diag, sc[li - kRcPitch + 1]);
            if (ok[k] & 16u) diag = min(diag, sc[li - kRcPitch - 1]);
            const uint32_t best = min(axis + rch::kAxis, diag + rch::kDiag);
            if (best < mine) {
                sc[li] = best;
                fell = true;
            }
        }
        if (!__syncthreads_or(fell)) break;
    }
    // write back what fell; a border cell that fell flags the tiles behind that border (bit (dy + 1) * 3 + dx + 1)
    unsigned dirs = 0;
#pragma unroll
    for (int k = 0; k < kRcPer; ++k) {
        const int cy = ly + k * kRcRowStep;
        const uint32_t v = s_cost[(cy + 1) * kRcPitch + lx + 1];
        if (v >= orig[k]) continue;
        cost[(size_t)(y0 + 1 + cy) * W + (x0 + 1 + lx)] = v;   // (a cell that fell is passable, so it lies in the grid)
        const unsigned xs = 2u | (lx == 0 ? 1u : 0u) | (lx == kTile - 1 ? 4u : 0u);        // bit dx + 1
        const unsigned ys = 2u | (cy == 0 ? 1u : 0u) | (cy == kTile - 1 ? 4u : 0u);
        for (int dy = 0; dy < 3; ++dy)
            if (ys >> dy & 1u) dirs |= xs << (3 * dy);
    }
    dirs &= ~(1u << 4);
    if (dirs) atomicOr(&s_dirs, dirs);
    __syncthreads();
    if (tid < 9 && (s_dirs >> tid & 1u)) {
        const int nx = bx + tid % 3 - 1, ny = by + tid / 3 - 1;
        if (nx >= 0 && nx < ntx && ny >= 0 && ny < nty) next[(size_t)ny * ntx + nx] = 1;
    }
}

// After a batch of nb rounds: h[0] = a tile ran in the batch's last round; st[kStRounds] += the rounds of the batch in
// which one ran; the batch's words are cleared for the next. One thread; h: pinned host memory.
__global__ void k_rc_peek(int *ran, int nb, unsigned *st, uint32_t *h) {
    unsigned n = 0;
    for (int k = 0; k < nb; ++k) {
        n += ran[k] != 0;
        if (k == nb - 1) h[0] = (uint32_t)ran[k];
        ran[k] = 0;
    }
    st[kStRounds] += n;
}

// st[kStReached] += the cells with a finite cost; st[kStMaxCost] = their maximum (0 before)
__global__ void __launch_bounds__(kFieldTB) k_rc_stats(const uint32_t *cost, size_t C, unsigned *st) {
    const size_t c = (size_t)blockIdx.x * kFieldTB + threadIdx.x;
    const uint32_t v = c < C ? cost[c] : rch::kNone;
    const bool reached = v != rch::kNone;
    const unsigned long long m = __ballot(reached);
    const unsigned wm = wave_max_u32(reached ? v : 0u);
    if ((threadIdx.x & 63) == 0 && m) {
        atomicAdd(reinterpret_cast<unsigned long long *>(st + kStReached), (unsigned long long)__popcll(m));
        atomicMax(&st[kStMaxCost], wm);
    }
}

// One thread per point; out: pinned host memory, n words. st (nullable): the statistics block, copied to h_stats by the
// first thread.
__global__ void __launch_bounds__(kFieldTB) k_rc_sample(clr::Grid g, const uint32_t *cost, const double2 *pts, int n,
                                                        uint32_t *out, const unsigned *st, uint32_t *h_stats) {
    const int i = blockIdx.x * kFieldTB + threadIdx.x;
    if (i == 0 && st)
        for (int k = 0; k < kStWords; ++k) h_stats[k] = st[k];
    if (i >= n) return;
    const double2 p = pts[i];
    int mx, my;
    out[i] = clr::cell_of(g, p.x, p.y, mx, my) ? cost[(size_t)my * g.W + mx] : rch::kNone;
}

// One wave walks down from cell (x, y), whose cost is finite: lanes 0..7 read the eight neighbours in the definition's
// order, the first admissible one is the next cell. At most max_len cells (cost / 5 + 1: every step lowers the cost by
// 5 at least); the first cap of them are stored. *n_out (pinned) = the length.
__global__ void __launch_bounds__(64) k_rc_descend(const uint32_t *cost, int W, int H, int x, int y, uint32_t *cells,
                                                   unsigned long long cap, unsigned long long max_len,
                                                   unsigned long long *n_out) {
    const int lane = threadIdx.x;
    const int dxs[8] = {1, -1, 0, 0, 1, -1, 1, -1}, dys[8] = {0, 0, 1, -1, 1, 1, -1, -1};
    const int dx = dxs[lane & 7], dy = dys[lane & 7];
    auto at = [&](int ax, int ay) {
        return ax < 0 || ax >= W || ay < 0 || ay >= H ? rch::kNone : cost[(size_t)ay * W + ax];
    };
    uint32_t here = at(x, y);
    unsigned long long len = 0;
    while (here != rch::kNone && len < max_len) {
        if (lane == 0 && len < cap) cells[len] = (uint32_t)y * (uint32_t)W + (uint32_t)x;
        ++len;
        if (here == 0) break;
        uint32_t v = rch::kNone;
        bool ok = false;
        if (lane < 8) {
            v = at(x + dx, y + dy);
            ok = v != rch::kNone && v + (lane < 4 ? rch::kAxis : rch::kDiag) == here;
            if (ok && lane >= 4) ok = at(x + dx, y) != rch::kNone && at(x, y + dy) != rch::kNone;
        }
        const unsigned long long m = __ballot(ok);
        if (!m) break;   // (no fixed point has such a cell)
        const int k = __ffsll((long long)m) - 1;
        x += dxs[k];
        y += dys[k];
        here = (uint32_t)__shfl((int)v, k);
    }
    if (lane == 0) *n_out = len;
}

void rc_launch_descend(const ReachState &S, int x, int y, uint32_t *cells, unsigned long long cap,
                       unsigned long long max_len, unsigned long long *n_out, hipStream_t s) {
    k_rc_descend<<<1, 64, 0, s>>>(S.cost.as<uint32_t>(), S.g.W, S.g.H, x, y, cells, cap, max_len, n_out);
    AOS_HIP(hipGetLastError());
}

namespace {

ReachState &reach_state(aos_ctx *c) {
    ReachState &S = c->reach_state.get<ReachState>();
    for (hipEvent_t &e : S.ev) if (!e) AOS_HIP(hipEventCreate(&e));
    return S;
}

}  // namespace

}  // namespace aos

using namespace aos;

extern "C" int aos_gvd_reach(aos_ctx *c, const aos_path_graph *graph, const int8_t *grid, int grid_on_device,
                             const aos_grid_info *info, const double *sources_xy, int32_t n_sources,
                             const aos_reach_opts *opts, aos_reach_out *out) {
    if (!c || !out) return fail(AOS_E_INVALID, "aos_gvd_reach: null argument");
    if (grid && !info) return fail(AOS_E_INVALID, "aos_gvd_reach: grid without grid info");
    if (grid)
        if (const char *m = clr::check_info(*info)) return fail(AOS_E_INVALID, std::string("aos_gvd_reach: ") + m);
    if (graph)
        if (const char *m = clr::check_graph(graph->nodes_xy, graph->num_nodes, nullptr, 0))
            return fail(AOS_E_INVALID, std::string("aos_gvd_reach: ") + m);
    if (const char *m = rch::check_reach(sources_xy, n_sources)) return fail(AOS_E_INVALID, std::string("aos_gvd_reach: ") + m);
    const uint32_t min_d2 = opts ? opts->min_d2 : 0u;
    const int max_rounds = opts ? opts->max_rounds : 0;
    return guarded("reach", "aos_gvd_reach", [&]() -> int {
        DeviceScope dev_scope(c->device);
        if (!graph || !grid) c->gvd_view_settle();
        // the graph (only its nodes are read) and the grid; the handle's own are checked like a caller's
        const aos_path_graph g = c->plan_graph(graph).g;
        const double *nodes_xy = g.nodes_xy;
        const int32_t nn = g.num_nodes;
        if (!graph)
            if (const char *m = clr::check_graph(nodes_xy, nn, nullptr, 0)) throw std::invalid_argument(m);
        ReachState &S = reach_state(c);
        hipStream_t s = c->stream;
        const aos_ctx::PlanGrid pg = c->plan_grid(grid, grid_on_device, info, S.d_grid);
        const int8_t *d_grid = pg.d_grid;
        const aos_grid_info gi = pg.info;
        if (!grid)
            if (const char *m = clr::check_info(gi)) throw std::invalid_argument(m);
        S.have = false;
        S.info = gi;
        S.g = clr::Grid{gi.origin_x, gi.origin_y, (double)gi.resolution, (int)gi.width, (int)gi.height};
        const int W = S.g.W, H = S.g.H;
        const size_t C = (size_t)W * H;
        // pinned outputs: the nodes' costs, then the statistics words
        uint32_t *h_node = static_cast<uint32_t *>(S.h_out.ensure(sizeof(uint32_t) * ((size_t)nn + kStWords)));
        uint32_t *h_stats = h_node + nn;
        float ms[3] = {0.0f, 0.0f, 0.0f};
        if (C == 0) {   // no launch on an empty grid
            std::fill(h_node, h_node + nn, rch::kNone);
            std::fill(h_stats, h_stats + kStWords, 0u);
        } else {
            const int ntx = cdiv(W, kTile), nty = cdiv(H, kTile);
            const size_t nt = (size_t)ntx * nty;
            double2 *d_nodes = S.nodes.ensure_n<double2>(nn);
            double2 *d_src = S.src.ensure_n<double2>(n_sources);
            if (nn) AOS_HIP(hipMemcpyAsync(d_nodes, nodes_xy, sizeof(double2) * (size_t)nn, hipMemcpyHostToDevice, s));
            if (n_sources)
                AOS_HIP(hipMemcpyAsync(d_src, sources_xy, sizeof(double2) * (size_t)n_sources, hipMemcpyHostToDevice, s));
            unsigned *st = S.stats.ensure_n<unsigned>(kStWords);
            int *flags = S.flags.ensure_n<int>(2 * nt), *ran = S.ran.ensure_n<int>(kBatch);
            uint8_t *pass = S.pass.ensure_n<uint8_t>(C);
            uint32_t *cost = S.cost.ensure_n<uint32_t>(C);
            uint32_t *h_peek = static_cast<uint32_t *>(S.h_peek.ensure(sizeof(uint32_t)));
            AOS_HIP(hipMemsetAsync(st, 0, sizeof(unsigned) * kStWords, s));
            AOS_HIP(hipMemsetAsync(flags, 0, sizeof(int) * 2 * nt, s));
            AOS_HIP(hipMemsetAsync(ran, 0, sizeof(int) * kBatch, s));
            AOS_HIP(hipEventRecord(S.ev[0], s));
            // 1. the mask and the sources
            if (min_d2 >= 2) clr_launch_field(S.f, d_grid, W, H, s);
            k_rc_mask<<<cdiv(C, kFieldTB), kFieldTB, 0, s>>>(d_grid, min_d2 >= 2 ? S.f.d2.as<uint32_t>() : nullptr, min_d2, C, pass,
                                                         cost, st);
            if (n_sources)
                k_rc_seed<<<cdiv(n_sources, kFieldTB), kFieldTB, 0, s>>>(S.g, d_src, n_sources, pass, cost, ntx, nty, flags, st);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipEventRecord(S.ev[1], s));
            // 2. rounds to the fixed point, a batch between two looks at the pinned word
            int issued = 0;
            for (bool settled = n_sources == 0; !settled;) {
                const int nb = max_rounds > 0 ? std::min(kBatch, max_rounds - issued) : kBatch;
                for (int k = 0; k < nb; ++k, ++issued)
                    k_rc_round<<<dim3(ntx, nty), kTileTB, 0, s>>>(cost, pass, W, H, ntx, nty, flags + (size_t)(issued & 1) * nt,
                                                                 flags + (size_t)(~issued & 1) * nt, ran + k, st);
                k_rc_peek<<<1, 1, 0, s>>>(ran, nb, st, h_peek);
                AOS_HIP(hipGetLastError());
                AOS_HIP(hipStreamSynchronize(s));
                settled = *h_peek == 0;
                if (!settled && max_rounds > 0 && issued >= max_rounds)
                    throw std::runtime_error("reach did not converge in " + std::to_string(max_rounds) + " rounds");
            }
            AOS_HIP(hipEventRecord(S.ev[2], s));
            // 3. the statistics and the nodes
            k_rc_stats<<<cdiv(C, kFieldTB), kFieldTB, 0, s>>>(cost, C, st);
            k_rc_sample<<<std::max(1, cdiv(nn, kFieldTB)), kFieldTB, 0, s>>>(S.g, cost, d_nodes, nn, h_node, st, h_stats);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipEventRecord(S.ev[3], s));
            AOS_HIP(hipStreamSynchronize(s));
            for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&ms[k], S.ev[k], S.ev[k + 1]);
        }
        S.node_m.resize(nn);
        rch::to_metres(h_node, nn, S.g.res, S.node_m.data());
        S.have = true;
        auto u64 = [&](int k) { return (uint64_t)h_stats[k] | ((uint64_t)h_stats[k + 1] << 32); };
        std::memset(out, 0, sizeof(*out));
        out->info = gi;
        out->n_passable = u64(kStPassable);
        out->n_reached = u64(kStReached);
        out->n_sources_used = (int32_t)h_stats[kStUsed];
        out->max_cost = out->n_reached ? h_stats[kStMaxCost] : rch::kNone;
        out->cost_device = C ? S.cost.as<uint32_t>() : nullptr;
        out->num_nodes = nn;
        out->node_cost = h_node;
        out->node_metres = S.node_m.data();
        out->n_rounds = (int32_t)h_stats[kStRounds];
        out->n_tile_runs = u64(kStRuns);
        out->ms_mask = ms[0]; out->ms_wave = ms[1]; out->ms_graph = ms[2];
        return AOS_OK;
    });
}

extern "C" int aos_reach_field_copy(aos_ctx *c, uint32_t *dst, uint64_t capacity_cells) {
    if (!c) return fail(AOS_E_INVALID, "aos_reach_field_copy: null handle");
    const ReachState *S = c->reach_state.peek<ReachState>();
    if (!S || !S->have) return fail(AOS_E_STATE, "aos_reach_field_copy: no aos_gvd_reach on this handle yet");
    const uint64_t C = (uint64_t)S->g.W * (uint64_t)S->g.H;
    if (capacity_cells < C) return fail(AOS_E_INVALID, "aos_reach_field_copy: capacity below width x height");
    if (C && !dst) return fail(AOS_E_INVALID, "aos_reach_field_copy: null destination");
    return guarded("reach", "aos_reach_field_copy", [&]() -> int {
        DeviceScope dev_scope(c->device);
        if (C) {
            AOS_HIP(hipMemcpyAsync(dst, S->cost.p, sizeof(uint32_t) * C, hipMemcpyDeviceToHost, c->stream));
            AOS_HIP(hipStreamSynchronize(c->stream));
        }
        return AOS_OK;
    });
}

extern "C" int aos_reach_points(aos_ctx *c, const double *xy, int32_t n, uint32_t *cost_out, float *metres_out) {
    if (!c) return fail(AOS_E_INVALID, "aos_reach_points: null handle");
    if (n < 0) return fail(AOS_E_INVALID, "aos_reach_points: negative count");
    if (n > 0 && !xy) return fail(AOS_E_INVALID, "aos_reach_points: null points behind a count above 0");
    ReachState *S = c->reach_state.peek<ReachState>();
    if (!S || !S->have) return fail(AOS_E_STATE, "aos_reach_points: no aos_gvd_reach on this handle yet");
    if (n == 0) return AOS_OK;
    return guarded("reach", "aos_reach_points", [&]() -> int {
        DeviceScope dev_scope(c->device);
        uint32_t *h = static_cast<uint32_t *>(S->h_pts.ensure(sizeof(uint32_t) * (size_t)n));
        if ((size_t)S->g.W * S->g.H == 0) std::fill(h, h + n, rch::kNone);
        else {
            double2 *d_pts = S->pts.ensure_n<double2>(n);
            AOS_HIP(hipMemcpyAsync(d_pts, xy, sizeof(double2) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            k_rc_sample<<<cdiv(n, kFieldTB), kFieldTB, 0, c->stream>>>(S->g, S->cost.as<uint32_t>(), d_pts, n, h, nullptr, nullptr);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipStreamSynchronize(c->stream));
        }
        if (cost_out) std::memcpy(cost_out, h, sizeof(uint32_t) * (size_t)n);
        if (metres_out) rch::to_metres(h, n, S->g.res, metres_out);
        return AOS_OK;
    });
}

extern "C" int aos_reach_descend(aos_ctx *c, const double start_xy[2], uint32_t *cells, double *xy, uint64_t capacity_cells,
                                 uint64_t *n_cells) {
    if (!c) return fail(AOS_E_INVALID, "aos_reach_descend: null handle");
    if (!start_xy || !n_cells) return fail(AOS_E_INVALID, "aos_reach_descend: null argument");
    if (capacity_cells > 0 && !cells) return fail(AOS_E_INVALID, "aos_reach_descend: null cells behind a capacity above 0");
    ReachState *S = c->reach_state.peek<ReachState>();
    if (!S || !S->have) return fail(AOS_E_STATE, "aos_reach_descend: no aos_gvd_reach on this handle yet");
    *n_cells = 0;
    int mx, my;
    if ((size_t)S->g.W * S->g.H == 0 || !clr::cell_of(S->g, start_xy[0], start_xy[1], mx, my)) return AOS_OK;
    return guarded("reach", "aos_reach_descend", [&]() -> int {
        DeviceScope dev_scope(c->device);
        hipStream_t s = c->stream;
        const int W = S->g.W;
        // the start's cost bounds the length, and so the device buffer
        unsigned long long *h = static_cast<unsigned long long *>(S->h_path.ensure(sizeof(unsigned long long) * 2));
        uint32_t start_cost = rch::kNone;
        AOS_HIP(hipMemcpyAsync(&start_cost, S->cost.as<uint32_t>() + (size_t)my * W + mx, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        AOS_HIP(hipStreamSynchronize(s));
        if (start_cost == rch::kNone) return AOS_OK;
        const unsigned long long max_len = (unsigned long long)start_cost / rch::kAxis + 1;
        const unsigned long long cap = std::min<unsigned long long>(capacity_cells, max_len);
        uint32_t *d_cells = S->path.ensure_n<uint32_t>(cap);
        rc_launch_descend(*S, mx, my, d_cells, cap, max_len, h, s);
        AOS_HIP(hipStreamSynchronize(s));
        const unsigned long long len = h[0], wrote = std::min(len, cap);
        if (wrote) AOS_HIP(hipMemcpy(cells, d_cells, sizeof(uint32_t) * wrote, hipMemcpyDeviceToHost));
        if (xy)
            for (unsigned long long k = 0; k < wrote; ++k) rch::cell_centre(S->g, cells[k], xy[2 * k], xy[2 * k + 1]);
        *n_cells = len;
        return AOS_OK;
    });
}
