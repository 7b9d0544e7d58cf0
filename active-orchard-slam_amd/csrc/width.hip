// aos_gvd_width: for every cell of a grid the widest robot that can get there from a set of sources, as the squared
// clearance it keeps on the best way (width.h and include/aos_gpu.h have the definitions), and the values at a
// GvdGraph's nodes and at arbitrary points. Everything is integer, and the field is the unique fixed point of
// width[c] = max(width[c], min(width[n], bottleneck(n -> c))) over the moves with width = cap at the source cells: any
// relaxation order ends at the same words.
//
// What runs where:
//   cap           GPU  clearance.hip's field passes on this state's own buffers (clr_launch_field), always;
//                      k_wd_cap: cap (0 where the byte is 100, else d2), every width word 0, the free count (one atomic
//                      per wave); k_wd_seed: one thread per source, width = cap at its cell and the 3 x 3 tiles around
//                      it flagged
//   rounds        GPU  k_wd_round, one plain launch per round, one workgroup per kTile x kTile tile: a tile that is not
//                      flagged leaves at once; a flagged one loads its widths and caps with a one-cell halo into LDS,
//                      relaxes there until nothing rises, writes back the words that rose and flags the neighbours (8,
//                      corners included) behind every border cell that rose. The flags are double buffered as reach's.
//                      Rounds go out kBatch at a time; k_wd_peek then stores "did a tile run in the batch's last round"
//                      into pinned memory, and the host stops at zero. No workgroup waits for another.
//   statistics    GPU  k_wd_stats: one pass over the field, the reached count, the minimum and the maximum per wave
//   sampling      GPU  k_wd_sample: one thread per node or point, stored into pinned host memory by the kernel
//   radii, checks      host (width_host.cpp)
// Host waits: one per batch of rounds and the call's final stream synchronise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "aos_ctx.h"
#include "field_passes.h"
#include "width.h"
#include "width_state.h"

namespace aos {

using rch::kBatch;
using rch::kTile;
using rch::kTileTB;

constexpr int kWdPitch = kTile + 2;                        // the tile with its halo, LDS words per row
constexpr int kWdPer = kTile * kTile / kTileTB;            // cells per thread
constexpr int kWdRowStep = kTileTB / kTile;                // rows between a thread's cells
static_assert(kTile * kTile % kTileTB == 0 && kTileTB % kTile == 0 && kTileTB % 64 == 0, "a thread's cells share a column");

// the words of the device statistics block (WidthState::stats)
enum { kWsFree = 0 /* 64 bits */, kWsReached = 2 /* 64 bits */, kWsRuns = 4 /* 64 bits */, kWsMin = 6, kWsMax = 7, kWsUsed = 8,
       kWsRounds = 9, kWsWords = 10 };

// cap[c] = 0 where the byte is 100, else d2[c]; width[c] = none. st[kWsFree] += the cells with cap > 0.
__global__ void __launch_bounds__(kFieldTB) k_wd_cap(const int8_t *grid, const uint32_t *d2, size_t C, uint32_t *cap,
                                                     uint32_t *width, unsigned *st) {
    const size_t c = (size_t)blockIdx.x * kFieldTB + threadIdx.x;
    bool is_free = false;
    if (c < C) {
        const uint32_t v = grid[c] == 100 ? 0u : d2[c];
        is_free = v != 0;
        cap[c] = v;
        width[c] = wd::kNone;
    }
    const unsigned long long m = __ballot(is_free);
    if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(reinterpret_cast<unsigned long long *>(st + kWsFree), (unsigned long long)__popcll(m));
}

// One thread per source: a source whose cell has cap > 0 stores the cap as the cell's width (equal stores to one cell
// race harmlessly) and flags the tiles within one tile of its own. st[kWsUsed] += the sources kept.
__global__ void __launch_bounds__(kFieldTB) k_wd_seed(clr::Grid g, const double2 *src, int n, const uint32_t *cap,
                                                      uint32_t *width, int ntx, int nty, int *flags, unsigned *st) {
    const int i = blockIdx.x * kFieldTB + threadIdx.x;
    bool used = false;
    if (i < n) {
        const double2 p = src[i];
        int mx, my;
        if (clr::cell_of(g, p.x, p.y, mx, my)) {
            const size_t c = (size_t)my * g.W + mx;
            const uint32_t v = cap[c];
            if (v) {
                used = true;
                width[c] = v;
                const int tx = mx / kTile, ty = my / kTile;
                for (int y = max(ty - 1, 0); y <= min(ty + 1, nty - 1); ++y)
                    for (int x = max(tx - 1, 0); x <= min(tx + 1, ntx - 1); ++x) flags[(size_t)y * ntx + x] = 1;
            }
        }
    }
    const unsigned long long m = __ballot(used);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st[kWsUsed], (unsigned)__popcll(m));
}

// One round. grid (ntx, nty): workgroup (bx, by) owns the cells [bx * kTile, +kTile) x [by * kTile, +kTile) and writes
// no other. It reads its halo from the neighbours' cells while they may be writing them: a word is read whole, every
// value a cell ever holds is the value of a real path, and a neighbour whose border cell rises flags this tile for the
// next round, so a stale word costs a round, never the result. Inside LDS the same holds between threads: the loop ends
// after a pass in which no thread stored, and such a pass read only final words. Cells outside the grid have width 0
// and cap 0: nothing passes through them and they never rise.
__global__ void __launch_bounds__(kTileTB) k_wd_round(uint32_t *width, const uint32_t *cap, int W, int H, int ntx, int nty,
                                                      int *cur, int *next, int *ran, unsigned *st) {
    __shared__ uint32_t s_w[kWdPitch * kWdPitch];
    __shared__ uint32_t s_cap[kWdPitch * kWdPitch];
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
            atomicAdd(reinterpret_cast<unsigned long long *>(st + kWsRuns), 1ull);
        }
    }
    __syncthreads();
    if (!s_flag) return;
    const int x0 = bx * kTile - 1, y0 = by * kTile - 1;   // the window's first cell
    for (int i = tid; i < kWdPitch * kWdPitch; i += kTileTB) {
        const int wy = i / kWdPitch, wx = i - wy * kWdPitch;
        const int gx = x0 + wx, gy = y0 + wy;
        uint32_t v = 0, p = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t c = (size_t)gy * W + gx;
            p = cap[c];
            v = width[c];
        }
        s_w[i] = v;
        s_cap[i] = p;
    }
    __syncthreads();
    // the thread's cells: column lx, rows ly + k * kWdRowStep
    const int lx = tid % kTile, ly = tid / kTile;
    uint32_t orig[kWdPer], own[kWdPer];
    uint32_t dcap[kWdPer][4];   // the bottleneck of the diagonal (+,+), (-,+), (+,-), (-,-) without the far cell's own cap
#pragma unroll
    for (int k = 0; k < kWdPer; ++k) {
        const int li = (ly + k * kWdRowStep + 1) * kWdPitch + lx + 1;
        orig[k] = s_w[li];
        const uint32_t c = s_cap[li];
        const uint32_t r = s_cap[li + 1], l = s_cap[li - 1], d = s_cap[li + kWdPitch], u = s_cap[li - kWdPitch];
        own[k] = c;
        dcap[k][0] = min(c, min(r, d));
        dcap[k][1] = min(c, min(l, d));
        dcap[k][2] = min(c, min(r, u));
        dcap[k][3] = min(c, min(l, u));
    }
    volatile uint32_t *sw = s_w;
    for (;;) {
        bool rose = false;
#pragma unroll
        for (int k = 0; k < kWdPer; ++k) {
            if (!own[k]) continue;
            const int li = (ly + k * kWdRowStep + 1) * kWdPitch + lx + 1;
            const uint32_t mine = sw[li];
            const uint32_t axis = max(max(sw[li + 1], sw[li - 1]), max(sw[li + kWdPitch], sw[li - kWdPitch]));
            uint32_t best = min(axis, own[k]);
            best = max(best, min(sw[li + kWdPitch + 1], dcap[k][0]));
            best = max(best, min(sw[li + kWdPitch - 1], dcap[k][1]));
            best = max(best, min(sw[li - kWdPitch + 1], dcap[k][2]));
            best = max(best, min(sw[li - kWdPitch - 1], dcap[k][3]));
            if (best > mine) {
                sw[li] = best;
                rose = true;
            }
        }
        if (!__syncthreads_or(rose)) break;
    }
    // write back what rose; a border cell that rose flags the tiles behind that border (bit (dy + 1) * 3 + dx + 1)
    unsigned dirs = 0;
#pragma unroll
    for (int k = 0; k < kWdPer; ++k) {
        const int cy = ly + k * kWdRowStep;
        const uint32_t v = s_w[(cy + 1) * kWdPitch + lx + 1];
        if (v <= orig[k]) continue;
        width[(size_t)(y0 + 1 + cy) * W + (x0 + 1 + lx)] = v;   // (a cell that rose has cap > 0, so it lies in the grid)
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

// After a batch of nb rounds: h[0] = a tile ran in the batch's last round; st[kWsRounds] += the rounds of the batch in
// which one ran; the batch's words are cleared for the next. One thread; h: pinned host memory.
__global__ void k_wd_peek(int *ran, int nb, unsigned *st, uint32_t *h) {
    unsigned n = 0;
    for (int k = 0; k < nb; ++k) {
        n += ran[k] != 0;
        if (k == nb - 1) h[0] = (uint32_t)ran[k];
        ran[k] = 0;
    }
    st[kWsRounds] += n;
}

// st[kWsReached] += the cells with width > 0; st[kWsMin], st[kWsMax] = their minimum (all ones before) and maximum (0).
// A workgroup takes kFieldTB * kWdStatPer cells, a thread kWdStatPer of them kFieldTB apart; one atomic each per wave,
// and none for a minimum or maximum that the word already passed (it only falls, or only rises: a stale read is safe).
constexpr int kWdStatPer = 8;
__global__ void __launch_bounds__(kFieldTB) k_wd_stats(const uint32_t *width, size_t C, unsigned *st) {
    const size_t c0 = (size_t)blockIdx.x * (kFieldTB * kWdStatPer) + threadIdx.x;
    unsigned n = 0, hi = 0, lo = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < kWdStatPer; ++j) {
        const size_t c = c0 + (size_t)j * kFieldTB;
        const uint32_t v = c < C ? width[c] : wd::kNone;
        if (v != wd::kNone) {
            ++n;
            hi = max(hi, v);
            lo = min(lo, v);
        }
    }
    hi = wave_max_u32(hi);
    lo = wave_min_u32(lo);
    for (int o = 32; o > 0; o >>= 1) n += (unsigned)__shfl_xor((int)n, o);
    if ((threadIdx.x & 63) == 0 && n) {
        atomicAdd(reinterpret_cast<unsigned long long *>(st + kWsReached), (unsigned long long)n);
        if (hi > __atomic_load_n(&st[kWsMax], __ATOMIC_RELAXED)) atomicMax(&st[kWsMax], hi);
        if (lo < __atomic_load_n(&st[kWsMin], __ATOMIC_RELAXED)) atomicMin(&st[kWsMin], lo);
    }
}

// One thread per point; out: pinned host memory, n words. st (nullable): the statistics block, copied to h_stats by the
// first thread.
__global__ void __launch_bounds__(kFieldTB) k_wd_sample(clr::Grid g, const uint32_t *width, const double2 *pts, int n,
                                                        uint32_t *out, const unsigned *st, uint32_t *h_stats) {
    const int i = blockIdx.x * kFieldTB + threadIdx.x;
    if (i == 0 && st)
        for (int k = 0; k < kWsWords; ++k) h_stats[k] = st[k];
    if (i >= n) return;
    const double2 p = pts[i];
    int mx, my;
    out[i] = clr::cell_of(g, p.x, p.y, mx, my) ? width[(size_t)my * g.W + mx] : wd::kNone;
}

namespace {

WidthState &width_state(aos_ctx *c) {
    WidthState &S = c->width_state.get<WidthState>();
    for (hipEvent_t &e : S.ev) if (!e) AOS_HIP(hipEventCreate(&e));
    return S;
}

}  // namespace

}  // namespace aos

using namespace aos;

extern "C" int aos_gvd_width(aos_ctx *c, const aos_path_graph *graph, const int8_t *grid, int grid_on_device,
                             const aos_grid_info *info, const double *sources_xy, int32_t n_sources,
                             const aos_width_opts *opts, aos_width_out *out) {
    if (!c || !out) return fail(AOS_E_INVALID, "aos_gvd_width: null argument");
    if (grid && !info) return fail(AOS_E_INVALID, "aos_gvd_width: grid without grid info");
    if (grid)
        if (const char *m = clr::check_info(*info)) return fail(AOS_E_INVALID, std::string("aos_gvd_width: ") + m);
    if (graph)
        if (const char *m = clr::check_graph(graph->nodes_xy, graph->num_nodes, nullptr, 0))
            return fail(AOS_E_INVALID, std::string("aos_gvd_width: ") + m);
    if (const char *m = wd::check_width(sources_xy, n_sources)) return fail(AOS_E_INVALID, std::string("aos_gvd_width: ") + m);
    const int max_rounds = opts ? opts->max_rounds : 0;
    return guarded("width", "aos_gvd_width", [&]() -> int {
        DeviceScope dev_scope(c->device);
        if (!graph || !grid) c->gvd_view_settle();
        // the graph (only its nodes are read) and the grid; the handle's own are checked like a caller's
        const aos_path_graph g = c->plan_graph(graph).g;
        const double *nodes_xy = g.nodes_xy;
        const int32_t nn = g.num_nodes;
        if (!graph)
            if (const char *m = clr::check_graph(nodes_xy, nn, nullptr, 0)) throw std::invalid_argument(m);
        WidthState &S = width_state(c);
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
        // pinned outputs: the nodes' widths, then the statistics words
        uint32_t *h_node = static_cast<uint32_t *>(S.h_out.ensure(sizeof(uint32_t) * ((size_t)nn + kWsWords)));
        uint32_t *h_stats = h_node + nn;
        float ms[3] = {0.0f, 0.0f, 0.0f};
        if (C == 0) {   // no launch on an empty grid
            std::fill(h_node, h_node + nn, wd::kNone);
            std::fill(h_stats, h_stats + kWsWords, 0u);
        } else {
            const int ntx = cdiv(W, kTile), nty = cdiv(H, kTile);
            const size_t nt = (size_t)ntx * nty;
            double2 *d_nodes = S.nodes.ensure_n<double2>(nn);
            double2 *d_src = S.src.ensure_n<double2>(n_sources);
            if (nn) AOS_HIP(hipMemcpyAsync(d_nodes, nodes_xy, sizeof(double2) * (size_t)nn, hipMemcpyHostToDevice, s));
            if (n_sources)
                AOS_HIP(hipMemcpyAsync(d_src, sources_xy, sizeof(double2) * (size_t)n_sources, hipMemcpyHostToDevice, s));
            unsigned *st = S.stats.ensure_n<unsigned>(kWsWords);
            int *flags = S.flags.ensure_n<int>(2 * nt), *ran = S.ran.ensure_n<int>(kBatch);
            uint32_t *cap = S.cap.ensure_n<uint32_t>(C);
            uint32_t *width = S.width.ensure_n<uint32_t>(C);
            uint32_t *h_peek = static_cast<uint32_t *>(S.h_peek.ensure(sizeof(uint32_t)));
            AOS_HIP(hipMemsetAsync(st, 0, sizeof(unsigned) * kWsWords, s));
            AOS_HIP(hipMemsetAsync(st + kWsMin, 0xFF, sizeof(unsigned), s));
            AOS_HIP(hipMemsetAsync(flags, 0, sizeof(int) * 2 * nt, s));
            AOS_HIP(hipMemsetAsync(ran, 0, sizeof(int) * kBatch, s));
            AOS_HIP(hipEventRecord(S.ev[0], s));
            // 1. cap and the sources
            clr_launch_field(S.f, d_grid, W, H, s);
            k_wd_cap<<<cdiv(C, kFieldTB), kFieldTB, 0, s>>>(d_grid, S.f.d2.as<uint32_t>(), C, cap, width, st);
            if (n_sources)
                k_wd_seed<<<cdiv(n_sources, kFieldTB), kFieldTB, 0, s>>>(S.g, d_src, n_sources, cap, width, ntx, nty, flags, st);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipEventRecord(S.ev[1], s));
            // 2. rounds to the fixed point, a batch between two looks at the pinned word
            int issued = 0;
            for (bool settled = n_sources == 0; !settled;) {
                const int nb = max_rounds > 0 ? std::min(kBatch, max_rounds - issued) : kBatch;
                for (int k = 0; k < nb; ++k, ++issued)
                    k_wd_round<<<dim3(ntx, nty), kTileTB, 0, s>>>(width, cap, W, H, ntx, nty, flags + (size_t)(issued & 1) * nt,
                                                                 flags + (size_t)(~issued & 1) * nt, ran + k, st);
                k_wd_peek<<<1, 1, 0, s>>>(ran, nb, st, h_peek);
                AOS_HIP(hipGetLastError());
                AOS_HIP(hipStreamSynchronize(s));
                settled = *h_peek == 0;
                if (!settled && max_rounds > 0 && issued >= max_rounds)
                    throw std::runtime_error("width did not converge in " + std::to_string(max_rounds) + " rounds");
            }
            AOS_HIP(hipEventRecord(S.ev[2], s));
            // 3. the statistics and the nodes
            k_wd_stats<<<cdiv(C, kFieldTB * kWdStatPer), kFieldTB, 0, s>>>(width, C, st);
            k_wd_sample<<<std::max(1, cdiv(nn, kFieldTB)), kFieldTB, 0, s>>>(S.g, width, d_nodes, nn, h_node, st, h_stats);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipEventRecord(S.ev[3], s));
            AOS_HIP(hipStreamSynchronize(s));
            for (int k = 0; k < 3; ++k) (void)hipEventElapsedTime(&ms[k], S.ev[k], S.ev[k + 1]);
        }
        S.node_r.resize(nn);
        wd::to_radius(h_node, nn, S.g.res, S.node_r.data());
        S.have = true;
        auto u64 = [&](int k) { return (uint64_t)h_stats[k] | ((uint64_t)h_stats[k + 1] << 32); };
        std::memset(out, 0, sizeof(*out));
        out->info = gi;
        out->n_free = u64(kWsFree);
        out->n_reached = u64(kWsReached);
        out->n_sources_used = (int32_t)h_stats[kWsUsed];
        out->min_width = out->n_reached ? h_stats[kWsMin] : 0u;
        out->max_width = h_stats[kWsMax];
        out->width_device = C ? S.width.as<uint32_t>() : nullptr;
        out->num_nodes = nn;
        out->node_width = h_node;
        out->node_radius_m = S.node_r.data();
        out->n_rounds = (int32_t)h_stats[kWsRounds];
        out->n_tile_runs = u64(kWsRuns);
        out->ms_field = ms[0]; out->ms_wave = ms[1]; out->ms_graph = ms[2];
        return AOS_OK;
    });
}

extern "C" int aos_width_field_copy(aos_ctx *c, uint32_t *dst, uint64_t capacity_cells) {
    if (!c) return fail(AOS_E_INVALID, "aos_width_field_copy: null handle");
    const WidthState *S = c->width_state.peek<WidthState>();
    if (!S || !S->have) return fail(AOS_E_STATE, "aos_width_field_copy: no aos_gvd_width on this handle yet");
    const uint64_t C = (uint64_t)S->g.W * (uint64_t)S->g.H;
    if (capacity_cells < C) return fail(AOS_E_INVALID, "aos_width_field_copy: capacity below width x height");
    if (C && !dst) return fail(AOS_E_INVALID, "aos_width_field_copy: null destination");
    return guarded("width", "aos_width_field_copy", [&]() -> int {
        DeviceScope dev_scope(c->device);
        if (C) {
            AOS_HIP(hipMemcpyAsync(dst, S->width.p, sizeof(uint32_t) * C, hipMemcpyDeviceToHost, c->stream));
            AOS_HIP(hipStreamSynchronize(c->stream));
        }
        return AOS_OK;
    });
}

extern "C" int aos_width_points(aos_ctx *c, const double *xy, int32_t n, uint32_t *width_out, float *radius_out) {
    if (!c) return fail(AOS_E_INVALID, "aos_width_points: null handle");
    if (n < 0) return fail(AOS_E_INVALID, "aos_width_points: negative count");
    if (n > 0 && !xy) return fail(AOS_E_INVALID, "aos_width_points: null points behind a count above 0");
    WidthState *S = c->width_state.peek<WidthState>();
    if (!S || !S->have) return fail(AOS_E_STATE, "aos_width_points: no aos_gvd_width on this handle yet");
    if (n == 0) return AOS_OK;
    return guarded("width", "aos_width_points", [&]() -> int {
        DeviceScope dev_scope(c->device);
        uint32_t *h = static_cast<uint32_t *>(S->h_pts.ensure(sizeof(uint32_t) * (size_t)n));
        if ((size_t)S->g.W * S->g.H == 0) std::fill(h, h + n, wd::kNone);
        else {
            double2 *d_pts = S->pts.ensure_n<double2>(n);
            AOS_HIP(hipMemcpyAsync(d_pts, xy, sizeof(double2) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            k_wd_sample<<<cdiv(n, kFieldTB), kFieldTB, 0, c->stream>>>(S->g, S->width.as<uint32_t>(), d_pts, n, h, nullptr, nullptr);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipStreamSynchronize(c->stream));
        }
        if (width_out) std::memcpy(width_out, h, sizeof(uint32_t) * (size_t)n);
        if (radius_out) wd::to_radius(h, n, S->g.res, radius_out);
        return AOS_OK;
    });
}
