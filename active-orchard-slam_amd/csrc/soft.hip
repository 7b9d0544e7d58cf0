// aos_gvd_soft: the cost-to-go field that pays for driving close to obstacles. It is reach's wavefront with a weight per
// cell that rises towards the obstacles (soft.h and include/aos_gpu.h have the definitions): a move costs 5 or 7 times
// the greatest weight over the cells it touches. Also the values at a GvdGraph's nodes and at arbitrary points, and
// descent paths on the field. Everything is integer, and the field is the unique fixed point of
// cost[c] = min(cost[c], cost[n] + w(n, c)) over the allowed moves: any relaxation order ends at the same words.
//
// What runs where:
//   mask, weight  GPU  clearance.hip's field passes on this state's own buffers when min_d2 >= 2 or a weight can exceed
//                      1 (clr_launch_field); k_sf_weight: one byte per cell, 0 impassable, else the weight; every cost
//                      word set to none; the passable and weighted counts and the greatest weight (eight cells per
//                      thread, one atomic each per wave); k_sf_seed: one thread per source, zeroes its cell and flags
//                      the 3 x 3 tiles around it
//   bound         host 7 * max_weight * n_passable < 2^31, read back only when the options and the grid's size allow the
//                      product to get there at all
//   rounds        GPU  k_sf_round, one plain launch per round, one workgroup per kTile x kTile tile: a tile that is not
//                      flagged leaves at once; a flagged one loads its costs and weight bytes with a one-cell halo into
//                      LDS, forms the eight move costs of each of its cells once, relaxes in LDS until nothing changes,
//                      writes back the words that fell and flags the neighbours (8, corners included) behind every
//                      border cell that fell. Flags, batches and the peek are reach's protocol.
//   statistics    GPU  k_sf_stats: one pass over the field, eight cells per thread, the reached count and the maximum
//                      per wave
//   sampling      GPU  k_sf_sample: one thread per node or point, stored into pinned host memory by the kernel
//   descent       GPU  k_sf_descend: one wave; lanes 0..7 form the eight moves' costs from the weight bytes and read the
//                      eight neighbours, a ballot picks the first admissible
//   centres, plain_cost, checks    host (soft_host.cpp)
// Host waits: one for the bound where it can bind, one per batch of rounds and the call's final stream synchronise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "aos_ctx.h"
#include "field_passes.h"
#include "soft.h"
#include "soft_state.h"

namespace aos {

using rch::kBatch;
using rch::kTile;
using rch::kTileTB;

constexpr int kSfPitch = kTile + 2;                        // the tile with its halo, LDS words (and bytes) per row
constexpr int kSfPer = kTile * kTile / kTileTB;            // cells per thread
constexpr int kSfRowStep = kTileTB / kTile;                // rows between a thread's cells
constexpr uint32_t kSfInf = 0x80000000u;                   // none inside LDS: above every finite cost, + 7 * 255 does not wrap
constexpr unsigned long long kSfPathGuess = 1ull << 20;    // a descent's first device buffer, in cells
constexpr int kSfCellsPer = 8;                             // cells per thread of the weight and statistics passes
static_assert(kTile * kTile % kTileTB == 0 && kTileTB % kTile == 0 && kTileTB % 64 == 0, "a thread's cells share a column");
static_assert((uint64_t)kSfInf == sft::kCostLimit, "finite costs stay below none inside LDS");

// the words of the device statistics block (SoftState::stats)
enum { kSsPassable = 0 /* 64 bits */, kSsReached = 2 /* 64 bits */, kSsRuns = 4 /* 64 bits */, kSsMaxCost = 6, kSsUsed = 7,
       kSsRounds = 8, kSsMaxWeight = 9, kSsSoft = 10 /* 64 bits */, kSsWords = 12 };

// wt[c] = 0 where the cell is impassable, else its weight; cost[c] = none. d2 null: min_d2 <= 1 and every weight is 1.
// st[kSsPassable] += the passable cells, st[kSsSoft] += those with a weight above 1, st[kSsMaxWeight] = the greatest.
// A workgroup takes kFieldTB * kSfCellsPer cells, a thread kSfCellsPer of them kFieldTB apart (width.hip's statistics
// pass measured what same-address atomics cost at one cell per thread); one atomic each per wave, and none for a
// maximum that the word already passed (it only rises, so a stale read is safe).
__global__ void __launch_bounds__(kFieldTB) k_sf_weight(const int8_t *grid, const uint32_t *d2, uint32_t min_d2,
                                                        uint32_t soft_cells, uint32_t gain, size_t C, uint8_t *wt,
                                                        uint32_t *cost, unsigned *st) {
    const size_t c0 = (size_t)blockIdx.x * (kFieldTB * kSfCellsPer) + threadIdx.x;
    unsigned np = 0, ns = 0, wm = 0;
#pragma unroll
    for (int j = 0; j < kSfCellsPer; ++j) {
        const size_t c = c0 + (size_t)j * kFieldTB;
        if (c >= C) break;
        uint32_t w = 0;
        if (grid[c] != 100) {
            if (!d2) w = 1;
            else {
                const uint32_t v = d2[c];
                if (v >= min_d2) w = sft::weight(v, soft_cells, gain);
            }
        }
        wt[c] = (uint8_t)w;
        cost[c] = sft::kNone;
        np += w != 0;
        ns += w > 1;
        wm = max(wm, w);
    }
    wm = wave_max_u32(wm);
    for (int o = 32; o > 0; o >>= 1) {
        np += (unsigned)__shfl_xor((int)np, o);
        ns += (unsigned)__shfl_xor((int)ns, o);
    }
    if ((threadIdx.x & 63) == 0 && np) {
        atomicAdd(reinterpret_cast<unsigned long long *>(st + kSsPassable), (unsigned long long)np);
        if (ns) atomicAdd(reinterpret_cast<unsigned long long *>(st + kSsSoft), (unsigned long long)ns);
        if (wm > __atomic_load_n(&st[kSsMaxWeight], __ATOMIC_RELAXED)) atomicMax(&st[kSsMaxWeight], wm);
    }
}

// One thread per source: a source with a passable cell zeroes it and flags the tiles within one tile of its own (a
// source on a tile's border is a changed border cell for the neighbours). st[kSsUsed] += the sources kept.
__global__ void __launch_bounds__(kFieldTB) k_sf_seed(clr::Grid g, const double2 *src, int n, const uint8_t *wt, uint32_t *cost,
                                                      int ntx, int nty, int *flags, unsigned *st) {
    const int i = blockIdx.x * kFieldTB + threadIdx.x;
    bool used = false;
    if (i < n) {
        const double2 p = src[i];
        int mx, my;
        if (clr::cell_of(g, p.x, p.y, mx, my) && wt[(size_t)my * g.W + mx]) {
            used = true;
            cost[(size_t)my * g.W + mx] = 0;
            const int tx = mx / kTile, ty = my / kTile;
            for (int y = max(ty - 1, 0); y <= min(ty + 1, nty - 1); ++y)
                for (int x = max(tx - 1, 0); x <= min(tx + 1, ntx - 1); ++x) flags[(size_t)y * ntx + x] = 1;
        }
    }
    const unsigned long long m = __ballot(used);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st[kSsUsed], (unsigned)__popcll(m));
}

// One round. grid (ntx, nty): workgroup (bx, by) owns the cells [bx * kTile, +kTile) x [by * kTile, +kTile) and writes
// no other. It reads its halo from the neighbours' cells while they may be writing them: a word is read whole, every
// value a cell ever holds is the cost of a real path, and a neighbour whose border cell falls flags this tile for the
// next round, so a stale word costs a round, never the result. Inside LDS the same holds between threads: the loop ends
// after a pass in which no thread stored, and such a pass read only final words. The weights never change, so the
// halo's bytes, corners included (the side cells of a diagonal move across a tile corner), are final when read. Cells
// outside the grid have weight 0 and cost none.
__global__ void __launch_bounds__(kTileTB) k_sf_round(uint32_t *cost, const uint8_t *wt, int W, int H, int ntx, int nty,
                                                      int *cur, int *next, int *ran, unsigned *st) {
    __shared__ uint32_t s_cost[kSfPitch * kSfPitch];
    __shared__ uint8_t s_wt[kSfPitch * kSfPitch];
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
            atomicAdd(reinterpret_cast<unsigned long long *>(st + kSsRuns), 1ull);
        }
    }
    __syncthreads();
    if (!s_flag) return;
    const int x0 = bx * kTile - 1, y0 = by * kTile - 1;   // the window's first cell
    for (int i = tid; i < kSfPitch * kSfPitch; i += kTileTB) {
        const int wy = i / kSfPitch, wx = i - wy * kSfPitch;
        const int gx = x0 + wx, gy = y0 + wy;
        uint32_t v = kSfInf;
        uint8_t p = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t c = (size_t)gy * W + gx;
            p = wt[c];
            const uint32_t cv = cost[c];
            if (cv != sft::kNone) v = cv;
        }
        s_cost[i] = v;
        s_wt[i] = p;
    }
    __syncthreads();
    // the thread's cells: column lx, rows ly + k * kSfRowStep
    const int lx = tid % kTile, ly = tid / kTile;
    uint32_t orig[kSfPer];
    // the eight moves' costs in the descent's order: (+,0), (-,0), (0,+), (0,-), (+,+), (-,+), (+,-), (-,-). An axis
    // move to an impassable cell keeps a cost: that cell's word stays none, and none + the cost is above every word.
    // A diagonal that is not allowed has cost 0. own 0: the cell is impassable.
    uint32_t mv[kSfPer][8];
    bool own[kSfPer];
#pragma unroll
    for (int k = 0; k < kSfPer; ++k) {
        const int li = (ly + k * kSfRowStep + 1) * kSfPitch + lx + 1;
        orig[k] = s_cost[li];
        const uint32_t c = s_wt[li];
        const uint32_t r = s_wt[li + 1], l = s_wt[li - 1], d = s_wt[li + kSfPitch], u = s_wt[li - kSfPitch];
        const uint32_t rd = s_wt[li + kSfPitch + 1], ld = s_wt[li + kSfPitch - 1];
        const uint32_t ru = s_wt[li - kSfPitch + 1], lu = s_wt[li - kSfPitch - 1];
        own[k] = c != 0;
        mv[k][0] = rch::kAxis * max(c, r);
        mv[k][1] = rch::kAxis * max(c, l);
        mv[k][2] = rch::kAxis * max(c, d);
        mv[k][3] = rch::kAxis * max(c, u);
        mv[k][4] = r && d && rd ? rch::kDiag * max(max(c, rd), max(r, d)) : 0u;
        mv[k][5] = l && d && ld ? rch::kDiag * max(max(c, ld), max(l, d)) : 0u;
        mv[k][6] = r && u && ru ? rch::kDiag * max(max(c, ru), max(r, u)) : 0u;
        mv[k][7] = l && u && lu ? rch::kDiag * max(max(c, lu), max(l, u)) : 0u;
    }
    volatile uint32_t *sc = s_cost;
    for (;;) {
        bool fell = false;
#pragma unroll
        for (int k = 0; k < kSfPer; ++k) {
            if (!own[k]) continue;
            const int li = (ly + k * kSfRowStep + 1) * kSfPitch + lx + 1;
            const uint32_t mine = sc[li];
            uint32_t best = min(min(sc[li + 1] + mv[k][0], sc[li - 1] + mv[k][1]),
                                min(sc[li + kSfPitch] + mv[k][2], sc[li - kSfPitch] + mv[k][3]));
            if (mv[k][4]) best = min(best, sc[li + kSfPitch + 1] + mv[k][4]);
            if (mv[k][5]) best = min(best, sc[li + kSfPitch - 1] + mv[k][5]);
            if (mv[k][6]) best = min(best, sc[li - kSfPitch + 1] + mv[k][6]);
            if (mv[k][7]) best = min(best, sc[li - kSfPitch - 1] + mv[k][7]);
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
    for (int k = 0; k < kSfPer; ++k) {
        const int cy = ly + k * kSfRowStep;
        const uint32_t v = s_cost[(cy + 1) * kSfPitch + lx + 1];
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

// After a batch of nb rounds: h[0] = a tile ran in the batch's last round; st[kSsRounds] += the rounds of the batch in
// which one ran; the batch's words are cleared for the next. One thread; h: pinned host memory.
__global__ void k_sf_peek(int *ran, int nb, unsigned *st, uint32_t *h) {
    unsigned n = 0;
    for (int k = 0; k < nb; ++k) {
        n += ran[k] != 0;
        if (k == nb - 1) h[0] = (uint32_t)ran[k];
        ran[k] = 0;
    }
    st[kSsRounds] += n;
}

// st[kSsReached] += the cells with a finite cost; st[kSsMaxCost] = their maximum (0 before). The cells per thread
// and the atomics are k_sf_weight's.
__global__ void __launch_bounds__(kFieldTB) k_sf_stats(const uint32_t *cost, size_t C, unsigned *st) {
    const size_t c0 = (size_t)blockIdx.x * (kFieldTB * kSfCellsPer) + threadIdx.x;
    unsigned n = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < kSfCellsPer; ++j) {
        const size_t c = c0 + (size_t)j * kFieldTB;
        const uint32_t v = c < C ? cost[c] : sft::kNone;
        if (v != sft::kNone) {
            ++n;
            hi = max(hi, v);
        }
    }
    hi = wave_max_u32(hi);
    for (int o = 32; o > 0; o >>= 1) n += (unsigned)__shfl_xor((int)n, o);
    if ((threadIdx.x & 63) == 0 && n) {
        atomicAdd(reinterpret_cast<unsigned long long *>(st + kSsReached), (unsigned long long)n);
        if (hi > __atomic_load_n(&st[kSsMaxCost], __ATOMIC_RELAXED)) atomicMax(&st[kSsMaxCost], hi);
    }
}

// One thread per point; out: pinned host memory, n words. st (nullable): the statistics block, copied to h_stats by the
// first thread.
__global__ void __launch_bounds__(kFieldTB) k_sf_sample(clr::Grid g, const uint32_t *cost, const double2 *pts, int n,
                                                        uint32_t *out, const unsigned *st, uint32_t *h_stats) {
    const int i = blockIdx.x * kFieldTB + threadIdx.x;
    if (i == 0 && st)
        for (int k = 0; k < kSsWords; ++k) h_stats[k] = st[k];
    if (i >= n) return;
    const double2 p = pts[i];
    int mx, my;
    out[i] = clr::cell_of(g, p.x, p.y, mx, my) ? cost[(size_t)my * g.W + mx] : sft::kNone;
}

// One wave walks down from cell (x, y), whose cost is finite: lanes 0..7 form the eight moves' costs from the weight
// bytes and read the eight neighbours in the definition's order, the first admissible one is the next cell. At most
// max_len cells (cost / 5 + 1: every step lowers the cost by 5 at least); the first cap of them are stored. *n_out
// (pinned) = the length.
__global__ void __launch_bounds__(64) k_sf_descend(const uint32_t *cost, const uint8_t *wt, int W, int H, int x, int y,
                                                   uint32_t *cells, unsigned long long cap, unsigned long long max_len,
                                                   unsigned long long *n_out) {
    const int lane = threadIdx.x;
    const int dxs[8] = {1, -1, 0, 0, 1, -1, 1, -1}, dys[8] = {0, 0, 1, -1, 1, 1, -1, -1};
    const int dx = dxs[lane & 7], dy = dys[lane & 7];
    auto inside = [&](int ax, int ay) { return ax >= 0 && ax < W && ay >= 0 && ay < H; };
    auto weight_at = [&](int ax, int ay) { return inside(ax, ay) ? (uint32_t)wt[(size_t)ay * W + ax] : 0u; };
    uint32_t here = inside(x, y) ? cost[(size_t)y * W + x] : sft::kNone;
    unsigned long long len = 0;
    while (here != sft::kNone && len < max_len) {
        if (lane == 0 && len < cap) cells[len] = (uint32_t)y * (uint32_t)W + (uint32_t)x;
        ++len;
        if (here == 0) break;
        uint32_t v = sft::kNone;
        bool ok = false;
        if (lane < 8) {
            const uint32_t a = weight_at(x, y), b = weight_at(x + dx, y + dy);
            uint32_t w = max(a, b);
            bool allowed = a && b;
            if (allowed && lane >= 4) {
                const uint32_t s = weight_at(x + dx, y), t = weight_at(x, y + dy);
                allowed = s && t;
                w = max(w, max(s, t));
            }
            if (allowed) {
                v = cost[(size_t)(y + dy) * W + (x + dx)];
                ok = v != sft::kNone && v + w * (lane < 4 ? rch::kAxis : rch::kDiag) == here;
            }
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

namespace {

SoftState &soft_state(aos_ctx *c) {
    SoftState &S = c->soft_state.get<SoftState>();
    for (hipEvent_t &e : S.ev) if (!e) AOS_HIP(hipEventCreate(&e));
    return S;
}

}  // namespace

}  // namespace aos

using namespace aos;

extern "C" int aos_gvd_soft(aos_ctx *c, const aos_path_graph *graph, const int8_t *grid, int grid_on_device,
                            const aos_grid_info *info, const double *sources_xy, int32_t n_sources,
                            const aos_soft_opts *opts, aos_soft_out *out) {
    if (!c || !out) return fail(AOS_E_INVALID, "aos_gvd_soft: null argument");
    if (grid && !info) return fail(AOS_E_INVALID, "aos_gvd_soft: grid without grid info");
    if (grid)
        if (const char *m = clr::check_info(*info)) return fail(AOS_E_INVALID, std::string("aos_gvd_soft: ") + m);
    if (graph)
        if (const char *m = clr::check_graph(graph->nodes_xy, graph->num_nodes, nullptr, 0))
            return fail(AOS_E_INVALID, std::string("aos_gvd_soft: ") + m);
    const uint32_t min_d2 = opts ? opts->min_d2 : 0u;
    const int32_t soft_cells = opts ? opts->soft_cells : 0, gain = opts ? opts->gain : 0;
    const int max_rounds = opts ? opts->max_rounds : 0;
    if (const char *m = sft::check_soft(sources_xy, n_sources, soft_cells, gain))
        return fail(AOS_E_INVALID, std::string("aos_gvd_soft: ") + m);
    return guarded("soft", "aos_gvd_soft", [&]() -> int {
        DeviceScope dev_scope(c->device);
        if (!graph || !grid) c->gvd_view_settle();
        // the graph (only its nodes are read) and the grid; the handle's own are checked like a caller's
        const aos_path_graph g = c->plan_graph(graph).g;
        const double *nodes_xy = g.nodes_xy;
        const int32_t nn = g.num_nodes;
        if (!graph)
            if (const char *m = clr::check_graph(nodes_xy, nn, nullptr, 0)) throw std::invalid_argument(m);
        SoftState &S = soft_state(c);
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
        uint32_t *h_node = static_cast<uint32_t *>(S.h_out.ensure(sizeof(uint32_t) * ((size_t)nn + kSsWords)));
        uint32_t *h_stats = h_node + nn;
        float ms[3] = {0.0f, 0.0f, 0.0f};
        if (C == 0) {   // no launch on an empty grid
            std::fill(h_node, h_node + nn, sft::kNone);
            std::fill(h_stats, h_stats + kSsWords, 0u);
        } else {
            const int ntx = cdiv(W, kTile), nty = cdiv(H, kTile);
            const size_t nt = (size_t)ntx * nty;
            double2 *d_nodes = S.nodes.ensure_n<double2>(nn);
            double2 *d_src = S.src.ensure_n<double2>(n_sources);
            if (nn) AOS_HIP(hipMemcpyAsync(d_nodes, nodes_xy, sizeof(double2) * (size_t)nn, hipMemcpyHostToDevice, s));
            if (n_sources)
                AOS_HIP(hipMemcpyAsync(d_src, sources_xy, sizeof(double2) * (size_t)n_sources, hipMemcpyHostToDevice, s));
            unsigned *st = S.stats.ensure_n<unsigned>(kSsWords);
            int *flags = S.flags.ensure_n<int>(2 * nt), *ran = S.ran.ensure_n<int>(kBatch);
            uint8_t *wt = S.wt.ensure_n<uint8_t>(C);
            uint32_t *cost = S.cost.ensure_n<uint32_t>(C);
            uint32_t *h_peek = static_cast<uint32_t *>(S.h_peek.ensure(sizeof(uint32_t) * kSsWords));
            AOS_HIP(hipMemsetAsync(st, 0, sizeof(unsigned) * kSsWords, s));
            AOS_HIP(hipMemsetAsync(flags, 0, sizeof(int) * 2 * nt, s));
            AOS_HIP(hipMemsetAsync(ran, 0, sizeof(int) * kBatch, s));
            AOS_HIP(hipEventRecord(S.ev[0], s));
            // 1. the mask and weights, the bound, the sources
            const bool field = min_d2 >= 2 || sft::weighted(soft_cells, gain);
            if (field) clr_launch_field(S.f, d_grid, W, H, s);
            k_sf_weight<<<cdiv(C, kFieldTB * kSfCellsPer), kFieldTB, 0, s>>>(d_grid, field ? S.f.d2.as<uint32_t>() : nullptr, min_d2,
                                                           (uint32_t)soft_cells, (uint32_t)gain, C, wt, cost, st);
            AOS_HIP(hipGetLastError());
            if (!sft::check_bound(sft::weight_bound(soft_cells, gain), C).empty()) {   // the counts can bind: look at them
                AOS_HIP(hipMemcpyAsync(h_peek, st, sizeof(unsigned) * kSsWords, hipMemcpyDeviceToHost, s));
                AOS_HIP(hipStreamSynchronize(s));
                const uint64_t n_passable = (uint64_t)h_peek[kSsPassable] | ((uint64_t)h_peek[kSsPassable + 1] << 32);
                const std::string m = sft::check_bound(h_peek[kSsMaxWeight], n_passable);
                if (!m.empty()) throw std::invalid_argument(m);
            }
            if (n_sources)
                k_sf_seed<<<cdiv(n_sources, kFieldTB), kFieldTB, 0, s>>>(S.g, d_src, n_sources, wt, cost, ntx, nty, flags, st);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipEventRecord(S.ev[1], s));
            // 2. rounds to the fixed point, a batch between two looks at the pinned word
            int issued = 0;
            for (bool settled = n_sources == 0; !settled;) {
                const int nb = max_rounds > 0 ? std::min(kBatch, max_rounds - issued) : kBatch;
                for (int k = 0; k < nb; ++k, ++issued)
                    k_sf_round<<<dim3(ntx, nty), kTileTB, 0, s>>>(cost, wt, W, H, ntx, nty, flags + (size_t)(issued & 1) * nt,
                                                                 flags + (size_t)(~issued & 1) * nt, ran + k, st);
                k_sf_peek<<<1, 1, 0, s>>>(ran, nb, st, h_peek);
                AOS_HIP(hipGetLastError());
                AOS_HIP(hipStreamSynchronize(s));
                settled = *h_peek == 0;
                if (!settled && max_rounds > 0 && issued >= max_rounds)
                    throw std::runtime_error("soft did not converge in " + std::to_string(max_rounds) + " rounds");
            }
            AOS_HIP(hipEventRecord(S.ev[2], s));
            // 3. the statistics and the nodes
            k_sf_stats<<<cdiv(C, kFieldTB * kSfCellsPer), kFieldTB, 0, s>>>(cost, C, st);
            k_sf_sample<<<std::max(1, cdiv(nn, kFieldTB)), kFieldTB, 0, s>>>(S.g, cost, d_nodes, nn, h_node, st, h_stats);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipEventRecord(S.ev[3], s));
            AOS_HIP(hipStreamSynchronize(s));
            for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&ms[k], S.ev[k], S.ev[k + 1]);
        }
        S.have = true;
        auto u64 = [&](int k) { return (uint64_t)h_stats[k] | ((uint64_t)h_stats[k + 1] << 32); };
        std::memset(out, 0, sizeof(*out));
        out->info = gi;
        out->n_passable = u64(kSsPassable);
        out->n_reached = u64(kSsReached);
        out->n_soft = u64(kSsSoft);
        out->n_sources_used = (int32_t)h_stats[kSsUsed];
        out->max_cost = out->n_reached ? h_stats[kSsMaxCost] : sft::kNone;
        out->max_weight = h_stats[kSsMaxWeight];
        out->cost_device = C ? S.cost.as<uint32_t>() : nullptr;
        out->num_nodes = nn;
        out->node_cost = h_node;
        out->n_rounds = (int32_t)h_stats[kSsRounds];
        out->n_tile_runs = u64(kSsRuns);
        out->ms_mask = ms[0]; out->ms_wave = ms[1]; out->ms_graph = ms[2];
        return AOS_OK;
    });
}

extern "C" int aos_soft_field_copy(aos_ctx *c, uint32_t *dst, uint64_t capacity_cells) {
    if (!c) return fail(AOS_E_INVALID, "aos_soft_field_copy: null handle");
    const SoftState *S = c->soft_state.peek<SoftState>();
    if (!S || !S->have) return fail(AOS_E_STATE, "aos_soft_field_copy: no aos_gvd_soft on this handle yet");
    const uint64_t C = (uint64_t)S->g.W * (uint64_t)S->g.H;
    if (capacity_cells < C) return fail(AOS_E_INVALID, "aos_soft_field_copy: capacity below width x height");
    if (C && !dst) return fail(AOS_E_INVALID, "aos_soft_field_copy: null destination");
    return guarded("soft", "aos_soft_field_copy", [&]() -> int {
        DeviceScope dev_scope(c->device);
        if (C) {
            AOS_HIP(hipMemcpyAsync(dst, S->cost.p, sizeof(uint32_t) * C, hipMemcpyDeviceToHost, c->stream));
            AOS_HIP(hipStreamSynchronize(c->stream));
        }
        return AOS_OK;
    });
}

extern "C" int aos_soft_points(aos_ctx *c, const double *xy, int32_t n, uint32_t *cost_out) {
    if (!c) return fail(AOS_E_INVALID, "aos_soft_points: null handle");
    if (n < 0) return fail(AOS_E_INVALID, "aos_soft_points: negative count");
    if (n > 0 && !xy) return fail(AOS_E_INVALID, "aos_soft_points: null points behind a count above 0");
    SoftState *S = c->soft_state.peek<SoftState>();
    if (!S || !S->have) return fail(AOS_E_STATE, "aos_soft_points: no aos_gvd_soft on this handle yet");
    if (n == 0) return AOS_OK;
    return guarded("soft", "aos_soft_points", [&]() -> int {
        DeviceScope dev_scope(c->device);
        uint32_t *h = static_cast<uint32_t *>(S->h_pts.ensure(sizeof(uint32_t) * (size_t)n));
        if ((size_t)S->g.W * S->g.H == 0) std::fill(h, h + n, sft::kNone);
        else {
            double2 *d_pts = S->pts.ensure_n<double2>(n);
            AOS_HIP(hipMemcpyAsync(d_pts, xy, sizeof(double2) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            k_sf_sample<<<cdiv(n, kFieldTB), kFieldTB, 0, c->stream>>>(S->g, S->cost.as<uint32_t>(), d_pts, n, h, nullptr, nullptr);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipStreamSynchronize(c->stream));
        }
        if (cost_out) std::memcpy(cost_out, h, sizeof(uint32_t) * (size_t)n);
        return AOS_OK;
    });
}

extern "C" int aos_soft_descend(aos_ctx *c, const double start_xy[2], uint32_t *cells, double *xy, uint64_t capacity_cells,
                                uint64_t *n_cells, uint32_t *plain_cost) {
    if (!c) return fail(AOS_E_INVALID, "aos_soft_descend: null handle");
    if (!start_xy || !n_cells) return fail(AOS_E_INVALID, "aos_soft_descend: null argument");
    if (capacity_cells > 0 && !cells) return fail(AOS_E_INVALID, "aos_soft_descend: null cells behind a capacity above 0");
    SoftState *S = c->soft_state.peek<SoftState>();
    if (!S || !S->have) return fail(AOS_E_STATE, "aos_soft_descend: no aos_gvd_soft on this handle yet");
    *n_cells = 0;
    if (plain_cost) *plain_cost = 0;
    int mx, my;
    if ((size_t)S->g.W * S->g.H == 0 || !clr::cell_of(S->g, start_xy[0], start_xy[1], mx, my)) return AOS_OK;
    return guarded("soft", "aos_soft_descend", [&]() -> int {
        DeviceScope dev_scope(c->device);
        hipStream_t s = c->stream;
        const int W = S->g.W, H = S->g.H;
        // the start's cost bounds the length
        unsigned long long *h = static_cast<unsigned long long *>(S->h_path.ensure(sizeof(unsigned long long) * 2));
        uint32_t start_cost = sft::kNone;
        AOS_HIP(hipMemcpyAsync(&start_cost, S->cost.as<uint32_t>() + (size_t)my * W + mx, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        AOS_HIP(hipStreamSynchronize(s));
        if (start_cost == sft::kNone) return AOS_OK;
        const unsigned long long max_len = (unsigned long long)start_cost / rch::kAxis + 1;
        // With plain_cost the whole descent comes to the host, whatever the caller's capacity: the sum runs over all of
        // it. A weighted cost overstates the length, so the first buffer is a guess and a longer descent is walked
        // again. Without plain_cost only the caller's cells are stored and copied; a length query copies nothing.
        unsigned long long room = plain_cost ? std::min(max_len, kSfPathGuess) : std::min<unsigned long long>(capacity_cells, max_len);
        unsigned long long len = 0;
        for (;;) {
            uint32_t *d_cells = S->path.ensure_n<uint32_t>(room);
            k_sf_descend<<<1, 64, 0, s>>>(S->cost.as<uint32_t>(), S->wt.as<uint8_t>(), W, H, mx, my, d_cells, room, max_len, h);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipStreamSynchronize(s));
            len = h[0];
            if (!plain_cost || len <= room) break;
            room = len;
        }
        const unsigned long long have = std::min(len, room);
        S->cells.resize(have);
        if (have) {
            AOS_HIP(hipMemcpyAsync(S->cells.data(), S->path.p, sizeof(uint32_t) * have, hipMemcpyDeviceToHost, s));
            AOS_HIP(hipStreamSynchronize(s));
        }
        const unsigned long long wrote = std::min<unsigned long long>(have, capacity_cells);
        if (wrote) std::memcpy(cells, S->cells.data(), sizeof(uint32_t) * wrote);
        if (xy)
            for (unsigned long long k = 0; k < wrote; ++k) rch::cell_centre(S->g, cells[k], xy[2 * k], xy[2 * k + 1]);
        *n_cells = len;
        if (plain_cost) *plain_cost = sft::plain_cost(S->cells.data(), len, W);   // (have == len here)
        return AOS_OK;
    });
}
