// aos_reach_sight: which cells a straight segment between two cell centres touches and how many of them the last
// aos_gvd_reach's passable mask refuses; aos_reach_pull: the descent from a start pulled taut into the greedy
// farthest-visible waypoints (sight.h and include/aos_gpu.h have the definitions). Everything the kernels decide is
// integer, and the one value several workgroups write is a maximum of integers: no output depends on arrival order.
//
// What runs where:
//   sight         GPU  k_sg_sight: one wave per segment, kSegsPerWG segments per workgroup. The wave's lanes take the
//                      columns of the major axis 64 at a time; a lane derives its column's interval of minor offsets
//                      (sgt::walk_column), reads those mask bytes and counts; two wave sums; lane 0 stores into pinned
//                      host memory. Work per segment: the columns of the major axis, not the bounding box.
//   descent       GPU  reach.hip's k_rc_descend into this call's own buffer
//   anchor steps  GPU  k_sg_step, one plain launch per step s: it reads the anchor wp[s] from device memory and leaves at
//                      once when that is the descent's last step; else one wave per candidate j (kCandsPerWG per
//                      workgroup) walks the segment anchor -> j as above, stops at the first column with an
//                      impassable cell, and a free candidate is offered to wp[s + 1] with atomicMax. wp[s + 1] was 0
//                      before, and j = anchor + 1 is always free, so after the launch it is the next anchor. The list
//                      of anchors is the list of waypoint steps.
//                      Steps go out kPullBatch at a time; k_sg_peek then stores "how many waypoints, if the last step
//                      has been reached" into pinned memory. No workgroup waits for another.
//   lengths, centres, checks    host (sight_host.cpp)
// Host waits: aos_reach_sight one; aos_reach_pull one for the start's cost, one for the descent's length, one per batch
// of steps and one for the copy of the cells and steps.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "aos_ctx.h"
#include "reach_state.h"
#include "sight.h"

namespace aos {

using sgt::kCandsPerWG;
using sgt::kPullBatch;
using sgt::kSegsPerWG;
using sgt::kSightTB;

__device__ __forceinline__ unsigned sg_wave_sum(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}

// The lane's column t of the walk: touched += its cells, blocked += those that are not passable. (Every cell lies in
// the two ends' bounding box, so inside the grid.)
__device__ __forceinline__ void sg_column(const sgt::Walk &w, int t, const uint8_t *pass, int W, unsigned &touched,
                                          unsigned &blocked) {
    int lo, hi;
    sgt::walk_column(w, t, lo, hi);
    for (int o = lo; o <= hi; ++o) {
        int x, y;
        sgt::walk_cell(w, t, o, x, y);
        ++touched;
        blocked += pass[(size_t)y * W + x] ? 0u : 1u;
    }
}

// One wave per segment. n_touched / n_blocked: pinned host memory, n words each.
__global__ void __launch_bounds__(kSightTB) k_sg_sight(clr::Grid g, const uint8_t *pass, const double2 *from,
                                                       const double2 *to, int n, uint32_t *n_touched, uint32_t *n_blocked) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * kSegsPerWG + (threadIdx.x >> 6);
    if (k >= n) return;   // (the whole wave)
    const double2 p = from[k], q = to[k];
    int ax, ay, bx, by;
    if (!clr::cell_of(g, p.x, p.y, ax, ay) || !clr::cell_of(g, q.x, q.y, bx, by)) {
        if (lane == 0) {
            n_touched[k] = 0;
            n_blocked[k] = sgt::kNone;
        }
        return;
    }
    const sgt::Walk w = sgt::make_walk(ax, ay, bx, by);
    unsigned touched = 0, blocked = 0;
    for (int t = lane; t <= w.A; t += 64) sg_column(w, t, pass, g.W, touched, blocked);
    touched = sg_wave_sum(touched);
    blocked = sg_wave_sum(blocked);
    if (lane == 0) {
        n_touched[k] = touched;
        n_blocked[k] = blocked;
    }
}

// Anchor step s of a descent of m cells (m >= 2): wp[s] is the anchor (wp[0] = 0), wp[s + 1] is 0 before the launch and
// the farthest free candidate after it. span: max_span, <= 0 for none. Nothing is done once the anchor is m - 1 (or
// wp[s] is a 0 behind the end of the list).
__global__ void __launch_bounds__(kSightTB) k_sg_step(const uint8_t *pass, int W, const uint32_t *cells, unsigned m, int span,
                                                      unsigned *wp, int s) {
    const unsigned a = wp[s];
    if (a >= m - 1 || (s > 0 && a == 0)) return;
    const unsigned hi = span > 0 ? min(m - 1, a + (unsigned)span) : m - 1;
    const unsigned j = a + 1 + blockIdx.x * kCandsPerWG + (threadIdx.x >> 6);
    if (j > hi) return;   // (the whole wave)
    const int lane = threadIdx.x & 63;
    const uint32_t ca = cells[a], cj = cells[j];
    const sgt::Walk w = sgt::make_walk((int)(ca % (uint32_t)W), (int)(ca / (uint32_t)W), (int)(cj % (uint32_t)W),
                                       (int)(cj / (uint32_t)W));
    for (int t0 = 0; t0 <= w.A; t0 += 64) {   // (uniform bounds: every lane takes part in the ballot)
        unsigned touched = 0, blocked = 0;
        if (t0 + lane <= w.A) sg_column(w, t0 + lane, pass, W, touched, blocked);
        if (__any(blocked != 0)) return;
    }
    if (lane == 0) atomicMax(&wp[s + 1], j);
}

// After the steps [s0, s1): h[0] = the number of waypoints if one of wp[s0 .. s1] is the last step m - 1, else 0.
// One thread; h: pinned host memory.
__global__ void k_sg_peek(const unsigned *wp, unsigned m, int s0, int s1, uint32_t *h) {
    uint32_t n = 0;
    for (int k = s0; k <= s1; ++k)
        if (wp[k] == m - 1) { n = (uint32_t)k + 1; break; }
    h[0] = n;
}

namespace {

ReachState *sight_state(aos_ctx *c) {
    ReachState *S = c->reach_state.peek<ReachState>();
    return S && S->have ? S : nullptr;
}

}  // namespace

}  // namespace aos

using namespace aos;

extern "C" int aos_reach_sight(aos_ctx *c, const double *from_xy, const double *to_xy, int32_t n, uint32_t *n_touched,
                               uint32_t *n_blocked) {
    if (!c) return fail(AOS_E_INVALID, "aos_reach_sight: null handle");
    if (const char *m = sgt::check_sight(from_xy, to_xy, n)) return fail(AOS_E_INVALID, std::string("aos_reach_sight: ") + m);
    ReachState *S = sight_state(c);
    if (!S) return fail(AOS_E_STATE, "aos_reach_sight: no aos_gvd_reach on this handle yet");
    if (n == 0) return AOS_OK;
    return guarded("sight", "aos_reach_sight", [&]() -> int {
        DeviceScope dev_scope(c->device);
        hipStream_t s = c->stream;
        SightBufs &B = S->sight;
        uint32_t *h = static_cast<uint32_t *>(B.h_sight.ensure(sizeof(uint32_t) * 2 * (size_t)n));
        if ((size_t)S->g.W * S->g.H == 0) {   // no end has a cell
            std::fill(h, h + n, 0u);
            std::fill(h + n, h + 2 * (size_t)n, sgt::kNone);
        } else {
            double2 *d_from = B.from.ensure_n<double2>(n), *d_to = B.to.ensure_n<double2>(n);
            AOS_HIP(hipMemcpyAsync(d_from, from_xy, sizeof(double2) * (size_t)n, hipMemcpyHostToDevice, s));
            AOS_HIP(hipMemcpyAsync(d_to, to_xy, sizeof(double2) * (size_t)n, hipMemcpyHostToDevice, s));
            k_sg_sight<<<cdiv(n, kSegsPerWG), kSightTB, 0, s>>>(S->g, S->pass.as<uint8_t>(), d_from, d_to, n, h, h + n);
            AOS_HIP(hipGetLastError());
            AOS_HIP(hipStreamSynchronize(s));
        }
        if (n_touched) std::memcpy(n_touched, h, sizeof(uint32_t) * (size_t)n);
        if (n_blocked) std::memcpy(n_blocked, h + n, sizeof(uint32_t) * (size_t)n);
        return AOS_OK;
    });
}

extern "C" int aos_reach_pull(aos_ctx *c, const double start_xy[2], const aos_pull_opts *opts, aos_pull_out *out) {
    if (!c) return fail(AOS_E_INVALID, "aos_reach_pull: null handle");
    if (!start_xy || !out) return fail(AOS_E_INVALID, "aos_reach_pull: null argument");
    ReachState *S = sight_state(c);
    if (!S) return fail(AOS_E_STATE, "aos_reach_pull: no aos_gvd_reach on this handle yet");
    const int32_t max_span = opts ? opts->max_span : 0;
    return guarded("sight", "aos_reach_pull", [&]() -> int {
        DeviceScope dev_scope(c->device);
        hipStream_t s = c->stream;
        SightBufs &B = S->sight;
        for (hipEvent_t &e : B.ev) if (!e) AOS_HIP(hipEventCreate(&e));
        B.steps.clear();
        B.cells.clear();
        B.xy.clear();
        std::memset(out, 0, sizeof(*out));
        out->start_cost = sgt::kNone;
        out->descent_m = INFINITY;
        const int W = S->g.W;
        int mx = 0, my = 0;
        uint32_t start_cost = sgt::kNone;
        if ((size_t)W * S->g.H != 0 && clr::cell_of(S->g, start_xy[0], start_xy[1], mx, my)) {
            AOS_HIP(hipMemcpyAsync(&start_cost, S->cost.as<uint32_t>() + (size_t)my * W + mx, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            AOS_HIP(hipStreamSynchronize(s));
        }
        if (start_cost == sgt::kNone) return AOS_OK;   // m = 0
        // 1. the descent; the kernel reports the full length, so one above the limit shows without room for it
        const unsigned long long max_len = (unsigned long long)start_cost / rch::kAxis + 1;
        const unsigned long long cap = std::min<unsigned long long>(max_len, sgt::kMaxDescent);
        uint32_t *d_cells = B.path.ensure_n<uint32_t>(cap);
        unsigned long long *h_len = static_cast<unsigned long long *>(B.h_len.ensure(sizeof(unsigned long long)));
        AOS_HIP(hipEventRecord(B.ev[0], s));
        rc_launch_descend(*S, mx, my, d_cells, cap, max_len, h_len, s);
        AOS_HIP(hipEventRecord(B.ev[1], s));
        AOS_HIP(hipStreamSynchronize(s));
        const unsigned long long m = *h_len;
        if (const char *msg = sgt::check_pull(m)) throw std::invalid_argument(msg);
        // 2. the anchor steps, a batch between two looks at the pinned word
        unsigned *wp = B.wp.ensure_n<unsigned>(m + 1);
        uint32_t n_wp = 1;
        int issued = 0;
        if (m > 1) {
            uint32_t *h_peek = static_cast<uint32_t *>(B.h_peek.ensure(sizeof(uint32_t)));
            AOS_HIP(hipMemsetAsync(wp, 0, sizeof(unsigned) * (m + 1), s));
            const unsigned long long most = max_span > 0 ? std::min<unsigned long long>(m - 1, (unsigned long long)max_span) : m - 1;
            const int wgs = cdiv((long long)most, kCandsPerWG);
            for (n_wp = 0; n_wp == 0;) {
                if ((unsigned long long)issued >= m - 1) throw std::runtime_error("the anchors did not reach the descent's end");
                const int nb = (int)std::min<unsigned long long>(kPullBatch, m - 1 - (unsigned long long)issued);
                for (int k = 0; k < nb; ++k)
                    k_sg_step<<<wgs, kSightTB, 0, s>>>(S->pass.as<uint8_t>(), W, d_cells, (unsigned)m, max_span, wp, issued + k);
                k_sg_peek<<<1, 1, 0, s>>>(wp, (unsigned)m, issued, issued + nb, h_peek);
                AOS_HIP(hipGetLastError());
                AOS_HIP(hipStreamSynchronize(s));
                issued += nb;
                n_wp = *h_peek;
            }
        }
        AOS_HIP(hipEventRecord(B.ev[2], s));
        // 3. the cells and the steps to the host
        uint32_t *h = static_cast<uint32_t *>(B.h_pull.ensure(sizeof(uint32_t) * (m + n_wp)));
        AOS_HIP(hipMemcpyAsync(h, d_cells, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, s));
        if (m > 1) AOS_HIP(hipMemcpyAsync(h + m, wp, sizeof(uint32_t) * n_wp, hipMemcpyDeviceToHost, s));
        AOS_HIP(hipStreamSynchronize(s));
        if (m == 1) h[m] = 0;
        const uint32_t *steps = h + m;
        for (uint32_t i = 0; i < n_wp; ++i)
            if (steps[i] >= m || (i > 0 && steps[i] <= steps[i - 1])) throw std::runtime_error("the anchors do not advance");
        B.steps.assign(steps, steps + n_wp);
        B.cells.resize(n_wp);
        B.xy.resize(2 * (size_t)n_wp);
        for (uint32_t i = 0; i < n_wp; ++i) {
            B.cells[i] = h[steps[i]];
            rch::cell_centre(S->g, B.cells[i], B.xy[2 * i], B.xy[2 * i + 1]);
        }
        sgt::PullCounts pc;
        sgt::pull_finish(S->g, h, m, start_cost, steps, n_wp, max_span, pc);
        float ms[2] = {0.0f, 0.0f};
        for (int k = 0; k < 2; ++k) (void)hipEventElapsedTime(&ms[k], B.ev[k], B.ev[k + 1]);
        out->n_cells = m;
        out->start_cost = start_cost;
        out->n_waypoints = (int32_t)n_wp;
        out->waypoint_steps = B.steps.data();
        out->waypoint_cells = B.cells.data();
        out->waypoints_xy = B.xy.data();
        out->length_m = pc.length_m;
        out->descent_m = pc.descent_m;
        out->n_steps_launched = issued;
        out->n_sight_tests = pc.n_sight_tests;
        out->ms_descend = ms[0];
        out->ms_pull = ms[1];
        return AOS_OK;
    });
}
