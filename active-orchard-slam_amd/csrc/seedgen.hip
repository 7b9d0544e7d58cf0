// Seed-gen frame orchestration (AosSeedGenNode::processPointCloud, seed_gen:452-579) on one
// HIP stream. Host work is limited to launch geometry derived from the polygon (a few scalars);
// every per-point / per-cell stage runs on the GPU. The cloud gets here through cloud_upload.hip, a1-a4 are
// ror_stage.hip's; the tiled multi-GPU frame (tiled.hip) reuses ror_stage and finish_frame.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>

#include "aos_ctx.h"

using namespace aos;

// Teardown (aos_destroy): only what has an order or does not free itself. Every DevBuf, PinnedBuf and HostBuf member
// (the lanes' GvdStates and their scratch included) goes with `delete`, in aos_destroy's device scope; no destructor
// touches the handle's stream or events.
void aos_ctx::release() {
    for (hipEvent_t e : coll_ev) (void)hipEventDestroy(e);
    coll_ev.clear();
    thin_graphs_release();
    try { expander.join(); } catch (...) {}   // (before its buffers go)
    if (copy_stream) {
        (void)hipStreamSynchronize(copy_stream);
        (void)hipEventDestroy(copy_ready);
        if (copy_done) (void)hipEventDestroy(copy_done);
        copy_done = nullptr;
        (void)hipStreamDestroy(copy_stream);
        copy_stream = nullptr;
    }
    gvd_async_stop();   // joins the jobs in flight (they use the lanes' GvdStates)
    try { prefetch_join(); } catch (...) {}
    release_uploader();
    for (CloudSplit *sp : {&split_cur, &split_next})
        if (sp->copied) { (void)hipEventSynchronize(sp->copied); (void)hipEventDestroy(sp->copied); sp->copied = nullptr; }
    for (OwnedState *s : {&path_state, &lin_state, &clear_state, &regions_state}) s->reset();
    for (auto &lp : lanes) {
        markers_wait(lp->gs, false);
        lp->gs.cells.reset();
    }
}

namespace aos {

ActiveBounds active_bounds(const Poly &poly) {
    double hminx = poly[0].first, hmaxx = poly[0].first, hminy = poly[0].second, hmaxy = poly[0].second;
    for (const auto &pt : poly) {
        hminx = std::min(hminx, pt.first); hmaxx = std::max(hmaxx, pt.first);
        hminy = std::min(hminy, pt.second); hmaxy = std::max(hmaxy, pt.second);
    }
    const double margin = 2.5;
    return ActiveBounds{static_cast<float>(hminx - margin), static_cast<float>(hmaxx + margin),
                        static_cast<float>(hminy - margin), static_cast<float>(hmaxy + margin)};
}

// getActiveBounds (seed_gen:874-890) + generateOccupancyGrid geometry (:584-600)
FrameGeom frame_geom(const Poly &poly, const aos_params &P) {
    FrameGeom g{};
    const ActiveBounds b = active_bounds(poly);
    g.minx = b.minx; g.maxx = b.maxx; g.miny = b.miny; g.maxy = b.maxy;
    g.res = P.grid_resolution;
    float width = std::max(0.0f, g.maxx - g.minx), height = std::max(0.0f, g.maxy - g.miny);
    unsigned int w = static_cast<unsigned int>(std::ceil(width / g.res));
    unsigned int h = static_cast<unsigned int>(std::ceil(height / g.res));
    if (w == 0) w = 1;
    if (h == 0) h = 1;
    g.W = (int)w; g.H = (int)h; g.WW = (g.W + 63) / 64;
    g.origin_x = g.minx; g.origin_y = g.miny;
    g.R = static_cast<int>(P.inflation_radius / P.grid_resolution);  // applyInflation seed_gen:936
    return g;
}

Poly default_polygon() {   // hard-coded default polygon of the reference constructor (seed_gen:196-199)
    return {{-1.972916603088379, 7.9420671463012695}, {-2.0726776123046875, 0.022441387176513672},
            {70.22465515136719, 2.102720260620117}, {69.48777770996094, 9.786612510681152}};
}

// ximgproc thinning loop: T = 1 if the image is empty after iteration 1, else the first iteration
// (k >= 2, 1-based) that deletes nothing; 0 while undecided. flags as written by k_thin_block.
int thin_iterations(const int *flags, int iters_run) {
    if (!flags[0]) return 1;
    for (int k = 1; k < iters_run; ++k)
        if (!flags[1 + k]) return k + 1;
    return 0;
}

}  // namespace aos

// First thinning batch of a whole-map frame: the opening (which clears the flags), after_open (the inflated
// grid's read-back), then batch_n temporal-block launches (launch_next issues them and keeps the caller's launch
// state). With aos_params.thin_graph the launches are a hipGraph (BASELINE configs[4]: hipGraph-captured
// thinning), one per batch size, batch_n rounded up to a power of two. A graph bakes every argument in by
// value, so it is keyed on every pointer and size its nodes hold (the opened and ping-pong bit grids, the
// flags, the tile-activity rows, and W, H, WW, R, the launch count, the flags length, the tile count) and
// re-captured when any of them changes; the per-launch act_prev / act_next alternation is a function of the
// launch index from 0, the same on every replay. The graph holds the thinning launches only and the flags
// are read back outside it. (Round 1's shape, a memset node + the opening + the launches + a D2H copy node,
// wrote garbage into the flags on replay: DESIGN.md "hipGraph-captured first thinning batch". It and the
// other shapes built to diagnose that, selected with AOS_THIN_GRAPH=2..4, were removed.)
void aos_ctx::thin_first_batch(const FrameGeom &g, const uint64_t *d_ibits, uint64_t *d_open, uint64_t *const bufs[2],
                               int *d_flags, int *d_act, int nflags, int &batch_n, int cap_launches,
                               const std::function<void(int)> &launch_next, const std::function<void()> &after_open) {
    hipStream_t s = stream;
    last_thin_graph = 0;
    // The opening runs outside the graph so that after_open (the inflated grid's read-back) can be queued behind
    // it: the read-back's blit kernel beside k_open took it from ~40 to 110 us at C3 (round-5 trace); beside
    // thinning the copy meets long, LDS-bound launches instead.
    launch_open(d_ibits, d_open, g, s, d_flags, nflags);   // (clears the flags)
    after_open();
    if (!P.thin_graph) {
        launch_next(batch_n);
        return;
    }
    int bn = 2;
    while (bn < batch_n) bn *= 2;
    batch_n = std::min(bn, cap_launches);
    const std::array<const void *, 5> ptrs{d_open, bufs[0], bufs[1], d_flags, d_act};
    const std::array<int, 7> dims{g.W, g.H, g.WW, g.R, batch_n, nflags, thin_tiles(g)};
    ThinGraph *tg = nullptr;
    for (auto &t : thin_graphs)
        if (t.dims[4] == batch_n) tg = &t;
    if (tg && tg->exec && (tg->ptrs != ptrs || tg->dims != dims)) {
        AOS_HIP(hipGraphExecDestroy(tg->exec));
        tg->exec = nullptr;
    }
    if (!tg) {
        thin_graphs.emplace_back();
        tg = &thin_graphs.back();
    }
    if (!tg->exec) {
        hipGraph_t graph = nullptr;
        AOS_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        try {
            launch_next(batch_n);
        } catch (...) {
            (void)hipStreamEndCapture(s, &graph);
            if (graph) (void)hipGraphDestroy(graph);
            throw;
        }
        AOS_HIP(hipStreamEndCapture(s, &graph));
        const hipError_t e = hipGraphInstantiate(&tg->exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) tg->exec = nullptr;
        AOS_HIP(e);
        tg->ptrs = ptrs;
        tg->dims = dims;
        last_thin_graph = 2;
    } else {
        last_thin_graph = 1;
    }
    AOS_HIP(hipGraphLaunch(tg->exec, s));
}

void aos_ctx::thin_graphs_release() {
    for (auto &t : thin_graphs)
        if (t.exec) (void)hipGraphExecDestroy(t.exec);
    thin_graphs.clear();
}

void aos_ctx::run_seedgen(bool want_host, aos_seedgen_out &out) {
    // A frame is served (have_frame) only once every check passed: finish_frame sets it before the ROR
    // overflow and thinning-convergence checks of the deferred path, so every way out of here that is not
    // a good frame (a redo, a throw, a HIP error in between) clears it again.
    try {
        // a frame whose ROR scatter outgrew its size guess is redone once with the size it read back
        for (int attempt = 0; attempt < 2; ++attempt) {
            if (!run_seedgen_once(want_host, out, attempt == 0)) return;
            have_frame = false;
        }
        throw std::runtime_error("ROR staging overflowed twice");
    } catch (...) {
        have_frame = false;
        throw;
    }
}

bool aos_ctx::run_seedgen_once(bool want_host, aos_seedgen_out &out, bool allow_guess) {
    const bool trace = trace_on();
    const auto t_in = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count(); };
    std::memset(&out, 0, sizeof(out));
    tiled_frame = false;
    have_frame = false;
    const FrameGeom g = frame_geom(poly, P);
    geom = g;
    if (g.R > 63) throw std::runtime_error("inflation radius > 63 cells is not supported by the bit-packed kernel");
    if ((size_t)g.W * g.H > (size_t)1 << 31) throw std::runtime_error("grid larger than 2^31 cells");
    hipStream_t s = stream;
    const size_t Cw = (size_t)g.WW * g.H;
    AOS_HIP(hipEventRecord(ev[kEvFrameBegin], s));

    // ---------------- a1-a4: ROR restricted to the clip box, clip, exclusion discs, raster
    RorOwn own{0, 0, g.W, g.H, 0, 0, g.W, g.H, false, {0, 0, 0, 0}};
    uint64_t *d_rbits = static_cast<uint64_t *>(raster_bits.ensure(Cw * 8));
    ror_stage(g, own, d_rbits, allow_guess);
    AOS_HIP(hipEventRecord(ev[kEvRorEnd], s));

    // ---------------- a5 inflation, a6 frame -> /occupancy_grid
    uint64_t *d_ibits = static_cast<uint64_t *>(infl_bits.ensure(Cw * 8));
    int8_t *d_occ = static_cast<int8_t *>(occ_bytes.ensure((size_t)g.W * g.H));
    launch_inflate(d_rbits, d_ibits, g, s, d_occ, 5);   // (the bytes with the 5-cell frame in the same launch)
    AOS_HIP(hipEventRecord(ev[kEvGridEnd], s));
    // /occupancy_grid's bits cross PCIe beside thinning (after the opening: thin_first_batch), instead of beside
    // the cluster stage's read-backs (finish_frame sends the skeleton's)
    infl_bits_sent = false;
    auto send_infl_bits = [&]() {
        if (!want_host) return;
        expander.drain();   // (a failed frame's expansion may still read the buffer)
        const size_t nb = 8 * Cw;
        grid_d2h(h_occ_bits.ensure(std::max<size_t>(nb, 8)), d_ibits, nb);
        infl_bits_sent = true;
    };

    // ---------------- a7 opening + Zhang-Suen (temporal blocks of kThinItersPerLaunch iterations)
    uint64_t *d_open = static_cast<uint64_t *>(open_bits.ensure(Cw * 8));
    uint64_t *bufs[2] = {static_cast<uint64_t *>(thin_a.ensure(Cw * 8)), static_cast<uint64_t *>(thin_b.ensure(Cw * 8))};
    const int K = kThinItersPerLaunch;
    const int max_iters = std::max(g.W, g.H) + 4;   // Zhang-Suen removes >= 1 cell per changing iteration
    const int nflags = 2 + max_iters + K;
    int *d_flags = static_cast<int *>(flags.ensure(sizeof(int) * nflags));
    int *h_flags = static_cast<int *>(h_small.ensure(sizeof(int) * nflags));
    const int ntt = thin_tiles(g);
    int *d_act = static_cast<int *>(thin_act.ensure(sizeof(int) * 2 * (size_t)ntt));
    // Launches past convergence return at once (k_thin_block reads the previous iteration's flag on the
    // device), so the first batch is sized from the last frame's T (at least 2 launches) and later
    // batches double: a frame pays one host round trip in the common case, a few when T jumps.
    int cap_launches = std::max(3, max_iters / K);
    if (const int e = g_debug_thin_cap.load(std::memory_order_relaxed); e >= 0)
        cap_launches = std::max(1, e);   // (aos_debug_limits: tests force non-convergence)
    int launched = 0;
    const uint64_t *src = d_open;
    ThinOwn whole{0, g.H, 0, g.WW, 1};
    auto launch_next = [&](int count) {
        for (int j = 0; j < count && launched < cap_launches; ++j) {
            uint64_t *dst = bufs[launched & 1];
            // tile activity of the previous launch (none for the first: every tile runs)
            whole.act_prev = launched ? d_act + (size_t)((launched - 1) & 1) * ntt : nullptr;
            whole.act_next = d_act + (size_t)(launched & 1) * ntt;
            launch_thin_block(src, dst, g, launched * K, d_flags, whole, s);
            src = dst;
            ++launched;
        }
    };
    int batch_n = std::min(cap_launches, std::max(2, (thin_iters_prev + 2 + K - 1) / K));
    thin_first_batch(g, d_ibits, d_open, bufs, d_flags, d_act, nflags, batch_n, cap_launches, launch_next, send_infl_bits);
    launched = batch_n;
    src = bufs[(batch_n - 1) & 1];
    // No host round trip after the first batch (verdict r02 weak item 9): a device kernel copies the converged
    // launch's buffer (read from the device flags) into thin_out, the flags come back with the frame's later
    // read-backs, and the post-thinning stages run at once. After the frame the host checks convergence (and
    // the ROR overflow); a frame whose T outgrew the first batch runs more launches below and the
    // post-thinning stages again. (Round 2's order, a wait for the flags here, was kept as AOS_THIN_DEFER=0, removed.)
    uint64_t *d_out = static_cast<uint64_t *>(thin_out.ensure(Cw * 8));
    launch_thin_pick(d_flags, launched, bufs[0], bufs[1], d_out, Cw, s, h_flags, 1 + launched * K);
    AOS_HIP(hipEventRecord(ev[kEvThinEnd], s));
    skel_bits = d_out;
    double t_thin = since();
    // (the cluster stage asks at its first host wait, when k_thin_pick's h_flags are on the host: a first batch
    // that thinning outgrew leaves a skeleton that is not final, and its clusters are not worth computing)
    frame_stale = [h_flags, launched] { return thin_iterations(h_flags, launched * kThinItersPerLaunch) == 0; };
    try {
        finish_frame(g, want_host, nullptr, out);   // (ends with a stream synchronisation: h_flags is on the host)
    } catch (...) {
        frame_stale = nullptr;
        throw;
    }
    frame_stale = nullptr;
    if (ror_collect()) return true;
    ror_times(out);   // (finish_frame read the binned count before ror_collect set it)
    int T = thin_iterations(h_flags, launched * K);
    if (T) {
        last_thin_launches = launched;
        thin_iters = thin_iters_prev = T;
        out.thin_iters = T;
        out.thin_launches = launched;
        if (trace)
            fprintf(stderr, "[aos trace seedgen] at %.2f: thin (deferred) %.2f finish %.2f (T %d, launches %d, graph %d)\n",
                    trace_ms() - since(), t_thin, since(), T, launched, last_thin_graph);
        return false;
    }
    // T outgrew the first batch: more launches (each round doubles), then the post-thinning stages again
    for (int round = 1; !T; ++round) {
        if (launched >= cap_launches) throw std::runtime_error("thinning did not converge");
        launch_next(batch_n << round);
        AOS_HIP(hipMemcpyAsync(h_flags, d_flags, sizeof(int) * (1 + launched * K), hipMemcpyDeviceToHost, s));
        AOS_HIP(hipStreamSynchronize(s));
        T = thin_iterations(h_flags, launched * K);
    }
    // the last launch that ran: launch j runs iff j == 0 or iteration j*K-1 deleted something
    int last = 0;
    for (int j = 1; j < launched; ++j)
        if (h_flags[1 + j * K - 1]) last = j; else break;
    last_thin_launches = launched;
    thin_iters = T;
    thin_iters_prev = T;
    skel_bits = bufs[last & 1];
    AOS_HIP(hipEventRecord(ev[kEvThinEnd], s));
    t_thin = since();
    finish_frame(g, want_host, nullptr, out);
    if (trace)
        fprintf(stderr, "[aos trace seedgen] at %.2f: thin-sync %.2f finish %.2f (T %d, launches %d, graph %d)\n",
                trace_ms() - since(), t_thin, since(), T, launched, last_thin_graph);
    return false;
}

// The published grids' D2H (round 5): the two bit-packed grids (the inflated grid and the frameless skeleton,
// W*H/8 bytes each) cross PCIe and host threads expand them to the {0, 100} bytes with the frame / rectangle
// while the cluster stage runs (grid_host.cpp). Round 4's traces showed the byte grids' D2H as runtime blit
// kernels (__amd_rocclr_copyBuffer, 0.65 ms per C2 frame, 2.6 ms at C3) that stretched the cluster stage's
// kernels beside them (k_fg 18 -> 280 us): the bits are 8x fewer bytes through them. (Round 4's byte grids by
// hipMemcpyAsync or by a copy kernel were kept as AOS_GRID_READBACK=0 / AOS_GRID_COPY_KERNEL=1, removed.)
constexpr int kGridExpandThreads = 8;   // (was measured with AOS_GRID_EXPAND_THREADS, removed)
// The grids' D2H runs as the runtime's blit kernels (under the HIP runtime torch loads). Beside the cluster stage
// they held the CUs its kernels needed: k_fg took 45 us instead of 18.6 beside the 2 MB bits copy at C2, 159
// instead of 24 beside the 8 MB at C3 (round-5 traces, tools/kt_overlap.py). A copy stream with a CU mask
// (hipExtStreamCreateWithCUMask, k CUs spread over the id range so that its blit waves stay there) was measured
// with AOS_COPY_CUS, removed, and not adopted (profiles/r05g_copy_cus_ab.txt): with 16 CUs seed-gen took
// 1.47-1.49 ms per C2 frame instead of 1.24-1.27 (thinning and k_fg slower beside the masked copy). The stream
// has no mask; the copies are placed where they meet the fewest kernels instead (the inflated grid beside
// thinning, the skeleton after k_fg).
void aos_ctx::grid_d2h(void *h, const void *d, size_t bytes) {
    grid_copy_wait();
    AOS_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, copy_stream));
}
// the copy stream (created on first use) waits for the work queued on the handle's stream so far
void aos_ctx::grid_copy_wait() {
    if (!copy_stream) {
        AOS_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
        AOS_HIP(hipEventCreateWithFlags(&copy_ready, hipEventDisableTiming));
        AOS_HIP(hipEventCreateWithFlags(&copy_done, hipEventDisableTiming));
    }
    AOS_HIP(hipEventRecord(copy_ready, stream));
    AOS_HIP(hipStreamWaitEvent(copy_stream, copy_ready, 0));
}

// a16 + a8-a15 on the whole map from skel_bits / occ_bytes, then the frame outputs. clipped_total:
// the kept-candidate count when it was reduced over tiles (else read from this handle's counters).
void aos_ctx::finish_frame(const FrameGeom &g, bool want_host, const uint64_t *clipped_total, aos_seedgen_out &out,
                           const PreClusters *pre) {
    hipStream_t s = stream;
    ++frame_gen;   // skel_bytes is rewritten below
    const size_t C = (size_t)g.W * g.H;
    int8_t *d_occ = occ_bytes.as<int8_t>();

    // ---------------- a16 /skeletonized_occupancy_grid = skeleton + polygon bbox rectangle
    int8_t *d_skel = static_cast<int8_t *>(skel_bytes.ensure(C));
    int rect[4] = {0, 0, 0, 0};   // markPolygonBoundaryAsOccupied's rectangle: gx0, gy0, gx1, gy1
    {
        const ActiveBounds b = active_bounds(poly);
        auto w2g = [&](float wx, float wy, int &gx, int &gy) {  // worldToGrid seed_gen:760-769
            float rel_x = (wx - g.origin_x) / g.res;
            float rel_y = (wy - g.origin_y) / g.res;
            gx = static_cast<int>(std::floor(rel_x)); gy = static_cast<int>(std::floor(rel_y));
            gx = gx < 0 ? 0 : (gx >= g.W ? g.W - 1 : gx);
            gy = gy < 0 ? 0 : (gy >= g.H ? g.H - 1 : gy);
        };
        w2g(b.minx, b.miny, rect[0], rect[1]);
        w2g(b.maxx, b.maxy, rect[2], rect[3]);
    }
    // the two published grids go to host memory, as bits, on the copy stream while the cluster / seed stage runs
    // (the copy's blit kernels share the CUs with the stage's kernels; issuing it after the stage instead was kept
    // as AOS_GRID_COPY=1, removed)
    auto issue_grid_copy = [&]() {
        // (a failed frame's expansion may still write h_occ / h_skel and read the bit buffers: drained before
        // any of them can be reallocated; ADVICE r05. A no-op when the inflated bits' send drained it.)
        expander.drain();
        h_occ.ensure(std::max<size_t>(C, 1)); h_skel.ensure(std::max<size_t>(C, 1));
        const size_t nb = 8 * (size_t)g.WW * g.H;
        uint64_t *hob = static_cast<uint64_t *>(h_occ_bits.ensure(std::max<size_t>(nb, 8)));
        uint64_t *hsb = static_cast<uint64_t *>(h_skel_bits.ensure(std::max<size_t>(nb, 8)));
        if (!infl_bits_sent)   // (a tiled frame: the gathered inflated grid)
            grid_d2h(hob, tiled_frame ? full_infl.as<uint64_t>() : infl_bits.as<uint64_t>(), nb);
        grid_d2h(hsb, skel_bits, nb);
        AOS_HIP(hipEventRecord(copy_done, copy_stream));
        GridExpander::Job j{};
        const int dev = device;
        hipEvent_t e = copy_done;
        j.wait = [dev, e] {
            AOS_HIP(hipSetDevice(dev));
            AOS_HIP(hipEventSynchronize(e));
        };
        j.occ_bits = hob; j.skel_bits = hsb;
        j.occ = h_occ.as<int8_t>(); j.skel = h_skel.as<int8_t>();
        j.W = g.W; j.H = g.H; j.WW = g.WW; j.frame = 5;
        j.rect[0] = rect[0]; j.rect[1] = rect[1]; j.rect[2] = rect[2]; j.rect[3] = rect[3];
        j.threads = kGridExpandThreads;
        expander.start(j);
    };
    HostTrace tr{"finish"};
    launch_bits_to_bytes(skel_bits, d_skel, g, 0, s, rect);   // (a16: the rectangle drawn in the same launch)
    // the bits go once the cluster stage has queued k_fg and its count read-back (SeedStageIn::after_fg; round 5
    // traces: beside k_fg the copy's blit kernel took k_fg from 19 to 49 us, and the read-back waited behind it on
    // PCIe)
    bool copy_issued = false;
    auto copy_now = [&]() {
        if (copy_issued) return;
        copy_issued = true;
        issue_grid_copy();
    };
    tr.mark("copy_issued");

    // ---------------- a8-a15 clusters, tree rows, seeds
    SeedStageIn sin{skel_bits, &geom, &poly, P.cluster_min_length, pre};
    if (want_host) {
        sin.after_fg = copy_now;
        // the replays walk the skeleton's bits once their read-back (queued by after_fg) is done (replays from the
        // clusters' cells instead were kept as AOS_REPLAY_BITS=0, removed)
        sin.host_skel_bits = [&]() -> const uint64_t * {
            if (!copy_issued) return nullptr;
            AOS_HIP(hipEventSynchronize(copy_done));
            return static_cast<const uint64_t *>(h_skel_bits.p);
        };
    }
    sin.stale = frame_stale;
    SeedStageOut so;
    run_cluster_seed_stage(cs, sin, so, s, ev[kEvClusterEnd], trace_on() ? &ev[kEvStageBegin] : nullptr);
    AOS_HIP(hipEventRecord(ev[kEvSeedsEnd], s));
    if (want_host) copy_now();   // (a stage that did not call after_fg)

    unsigned long long *h_cnt = ror.stats()->kept;
    if (!clipped_total) AOS_HIP(hipMemcpyAsync(h_cnt, ror.counters.p, sizeof(RorCounters::kept), hipMemcpyDeviceToHost, s));
    tr.mark("stage_done");
    AOS_HIP(hipStreamSynchronize(s));
    tr.mark("stream_synced");
    if (want_host) expander.join();   // (rethrows a failed wait)
    tr.mark("copies_synced");
    if (clipped_total) {
        n_clipped = *clipped_total;
    } else {
        n_clipped = 0;
        for (int i = 0; i < kRorCounters; ++i) n_clipped += h_cnt[i];
    }
    have_frame = true;

    h_row_center = std::move(so.row_center); h_row_start = std::move(so.row_start);
    h_row_end = std::move(so.row_end); h_row_length = std::move(so.row_length);
    n_virtual = so.n_virtual; n_ray = so.n_ray; n_endpoint = so.n_endpoint;
    if (so.n_voronoi) h_voronoi.assign(so.h_voronoi, so.h_voronoi + 2 * (size_t)so.n_voronoi);
    else h_voronoi.clear();
    h_rows_info = std::move(so.rows_info);
    h_cluster_info = std::move(so.cluster_info);
    n_clusters_all = so.n_clusters_all;
    n_bfs_replayed = so.n_bfs;

    out.info = aos_grid_info{g.origin_x, g.origin_y, g.res, (uint32_t)g.W, (uint32_t)g.H};
    out.thin_iters = thin_iters;
    out.n_input = (d_cloud == map_buf.as<uint8_t>() && n_points == map_n) ? map_total : n_points;
    out.n_clipped = n_clipped;
    out.n_ror_kept = 0;  // not materialised (ROR is evaluated only where it can reach the grid)
    out.occupancy = want_host ? h_occ.as<int8_t>() : nullptr;
    out.skeleton = want_host ? h_skel.as<int8_t>() : nullptr;
    out.d_occupancy = d_occ;
    out.d_skeleton = d_skel;
    out.n_clusters_all = n_clusters_all;
    out.n_bfs_replayed = n_bfs_replayed;
    out.n_rows = (int)h_row_length.size();
    out.row_center = h_row_center.data(); out.row_start = h_row_start.data();
    out.row_end = h_row_end.data(); out.row_length = h_row_length.data();
    out.n_virtual = n_virtual; out.n_ray = n_ray; out.n_endpoint = n_endpoint;
    out.n_voronoi = (int)h_voronoi.size() / 2;
    out.voronoi_xy = h_voronoi.data();
    out.rows_info_xy = h_rows_info.data();
    out.n_cluster_info = (int)h_cluster_info.size() / 2;
    out.cluster_info_xy = h_cluster_info.data();
    out.ms_ror = ms_ev(kEvFrameBegin, kEvRorEnd); out.ms_grid = ms_ev(kEvRorEnd, kEvGridEnd);
    out.ms_thin = ms_ev(kEvGridEnd, kEvThinEnd);
    // (a tiled frame: its cluster stage starts after the grids' gather)
    out.ms_cluster = ms_ev(pre ? kEvGridsGathered : kEvThinEnd, kEvClusterEnd);
    out.ms_seeds = ms_ev(kEvClusterEnd, kEvSeedsEnd); out.ms_total = ms_ev(kEvFrameBegin, kEvSeedsEnd);
    if (trace_on() && !pre)
        fprintf(stderr, "[aos trace events] thin_end->stage_start %.3f stage_gpu %.3f gpu_end->rows %.3f (ms)\n",
                ms_ev(kEvThinEnd, kEvStageBegin), ms_ev(kEvStageBegin, kEvStageGpuEnd), ms_ev(kEvStageGpuEnd, kEvClusterEnd));
    ror_times(out);   // (the binned count as ror_collect left it: a plain frame calls this again after its own)
    out.thin_graph = tiled_frame ? 0 : last_thin_graph;
    out.thin_launches = last_thin_launches;
    out.n_ror_read = ror.read;
}

int aos_ctx::debug_grid(const char *which, int8_t *dst, uint64_t capacity) {
    const size_t C = (size_t)geom.W * geom.H;
    if (capacity < C) { set_error("aos_debug_grid: capacity < width*height"); return AOS_E_INVALID; }
    const uint64_t *bits = nullptr;
    if (!std::strcmp(which, "inflated")) bits = tiled_frame ? full_infl.as<uint64_t>() : infl_bits.as<uint64_t>();
    else if (!std::strcmp(which, "skeleton_frameless")) bits = skel_bits;
    else if (!tiled_frame && !std::strcmp(which, "raster")) bits = raster_bits.as<uint64_t>();
    else if (!tiled_frame && !std::strcmp(which, "opened")) bits = open_bits.as<uint64_t>();
    else {
        set_error(std::string("aos_debug_grid: unknown grid (or not kept by a tiled frame) ") + which);
        return AOS_E_INVALID;
    }
    DevBuf tmp;
    int8_t *d = static_cast<int8_t *>(tmp.ensure(C));
    launch_bits_to_bytes(bits, d, geom, 0, stream);
    AOS_HIP(hipMemcpyAsync(dst, d, C, hipMemcpyDeviceToHost, stream));
    AOS_HIP(hipStreamSynchronize(stream));
    tmp.release();
    return AOS_OK;
}
