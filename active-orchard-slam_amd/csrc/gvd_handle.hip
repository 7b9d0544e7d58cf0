// The handle's GVD methods: the synchronous calls (external inputs, the last seed-gen frame) and the pipelined lanes
// (aos_gvd_from_seedgen_async / aos_gvd_wait), all around run_gvd_stage (gvd.hip). No device code.
#include <algorithm>
#include <cstring>
#include <stdexcept>

#include "aos_ctx.h"

// ------------------------------------------------------------------ handle methods
using namespace aos;

static void fill_gvd_out(const aos_ctx &c, const GvdState &G, const aos_grid_info &info, bool published, aos_gvd_out &out) {
    std::memset(&out, 0, sizeof(out));
    out.published = published ? 1 : 0;
    out.resolution = info.resolution;  // GvdGraph.resolution = skeleton info.resolution (gvd:903)
    out.origin_x = info.origin_x; out.origin_y = info.origin_y;
    out.num_nodes = (int32_t)G.labels.size();
    out.num_edges = (int32_t)G.lengths.size();
    out.nodes_xy = G.nodes_xy.data();
    out.node_labels = G.labels.data(); out.node_cluster_indices = G.cluster_idx.data();
    out.node_label_counts = G.label_counts.data();
    out.n_label_entries = (int32_t)G.label_clusters.size();
    out.node_label_clusters = G.label_clusters.data(); out.node_label_types = G.label_types.data();
    out.edges = G.edges_out.data(); out.edge_lengths = G.lengths.data(); out.edge_clearances = G.clearances.data();
    out.n_merged_seeds = G.n_merged; out.n_voronoi_edges = G.n_vor_edges; out.n_boundary_points = G.n_bpts;
    out.ms_merge = G.ms_merge; out.ms_delaunay = G.ms_delaunay; out.ms_graph = G.ms_graph; out.ms_total = G.ms_total;
    out.ms_cells = 0.0f;   // the cells job may still run: aos_gvd_markers.ms_cells
    (void)c;
}

void aos_ctx::run_gvd_external(const aos_gvd_in &in, aos_gvd_out &out) {
    gvd_async_drop();
    GvdState &G = gs();
    const size_t C = (size_t)in.info.width * in.info.height;
    int8_t *d_sk = static_cast<int8_t *>(G.skel.ensure(std::max<size_t>(C, 1)));
    if (C && in.skeleton) AOS_HIP(hipMemcpyAsync(d_sk, in.skeleton, C, hipMemcpyHostToDevice, stream));
    GvdStageIn gi{in.seeds_xy, in.n_seeds, in.rows_info_xy, in.n_rows_poses, in.info, d_sk};
    have_gvd = false;
    const bool pub = run_gvd_stage(G, P, gi, stream, ev.data());
    have_gvd = true; gvd_from_frame = false; gvd_skel = d_sk; gvd_info = in.info; ++gvd_gen;
    fill_gvd_out(*this, G, in.info, pub, out);
}

void aos_ctx::run_gvd_from_frame(aos_gvd_out &out) {
    gvd_async_drop();
    GvdState &G = gs();
    aos_grid_info info{geom.origin_x, geom.origin_y, geom.res, (uint32_t)geom.W, (uint32_t)geom.H};
    GvdStageIn gi{h_voronoi.data(), (int)(h_voronoi.size() / 2), h_rows_info.data(), (int)(h_rows_info.size() / 2), info,
                  skel_bytes.as<int8_t>()};
    have_gvd = false;
    const bool pub = run_gvd_stage(G, P, gi, stream, ev.data());
    have_gvd = true; gvd_from_frame = true; gvd_frame_gen = frame_gen; gvd_skel = gi.d_skeleton; gvd_info = info; ++gvd_gen;
    fill_gvd_out(*this, G, info, pub, out);
}

// ------------------------------------------------------------------ pipelined GVD
// aos_gvd_from_seedgen_async: snapshot the frame's GVD inputs (host seeds and rows, a device copy of
// the skeleton ordered on the seed-gen stream) into a free lane, whose worker runs the same
// run_gvd_stage on the lane's stream. The next seed-gen frame may run meanwhile; it rewrites only
// seed-gen state. Frames are independent, so with aos_gvd_pipeline_depth(D) up to D jobs run at once
// (each Subdiv2D replay on its own host core); aos_gvd_wait collects them in start order.
void aos_ctx::gvd_lanes_ensure() {
    if (lanes.empty()) lanes.emplace_back(new GvdLane());
    while ((int)lanes.size() < gvd_depth + 1) lanes.emplace_back(new GvdLane());
}

void aos_ctx::lane_join(int l) {
    AsyncGvd &A = lanes[l]->ag;
    if (!A.worker.joinable()) return;
    std::unique_lock<std::mutex> lk(A.mu);
    A.cv.wait(lk, [&A] { return !A.busy; });
}

void aos_ctx::lane_apply(int l) {
    lanes[l]->ag.applied = true;
    cur_lane = l;
    have_gvd = true; gvd_from_frame = false; gvd_skel = lanes[l]->gs.skel.as<int8_t>(); gvd_info = lanes[l]->ag.info;
    ++gvd_gen;
}

void aos_ctx::gvd_async_start() {
    gvd_lanes_ensure();
    // D jobs in flight already: the oldest is superseded (joined, its result dropped)
    while ((int)inflight.size() >= gvd_depth) {
        const int l = inflight.front();
        inflight.pop_front();
        lane_join(l);
        std::lock_guard<std::mutex> lk(lanes[l]->ag.mu);
        lanes[l]->ag.done = false;
        lanes[l]->ag.err = nullptr;
    }
    int L = -1;   // a lane that holds neither the current result nor a job
    for (int i = 0; i < (int)lanes.size() && L < 0; ++i)
        if (i != cur_lane && std::find(inflight.begin(), inflight.end(), i) == inflight.end()) L = i;
    if (L < 0) throw std::logic_error("gvd_async_start: no free lane");
    GvdLane &ln = *lanes[L];
    AsyncGvd &A = ln.ag;
    if (!gvd_stream) AOS_HIP(hipStreamCreateWithFlags(&gvd_stream, hipStreamNonBlocking));
    if (!A.stream) {
        // every lane queues its GPU work on the handle's one GVD stream (few streams for the GPU's 4 hardware
        // queues: no false dependencies behind unrelated streams); each lane waits on its own events
        A.stream = gvd_stream;
        for (auto &e : A.ev) AOS_HIP(hipEventCreate(&e));
        AOS_HIP(hipEventCreateWithFlags(&A.ready, hipEventDisableTiming));
    }
    A.seeds = h_voronoi;
    A.rows = h_rows_info;
    A.P = P;   // snapshot on the caller's thread: aos_gvd_set_markers may change P while the job runs
    A.applied = false;
    A.info = aos_grid_info{geom.origin_x, geom.origin_y, geom.res, (uint32_t)geom.W, (uint32_t)geom.H};
    const size_t C = (size_t)geom.W * geom.H;
    int8_t *d_sk = static_cast<int8_t *>(ln.gs.skel.ensure(std::max<size_t>(C, 1)));
    AOS_HIP(hipMemcpyAsync(d_sk, skel_bytes.p, C, hipMemcpyDeviceToDevice, stream));
    AOS_HIP(hipEventRecord(A.ready, stream));
    AOS_HIP(hipStreamWaitEvent(A.stream, A.ready, 0));
    if (!A.worker.joinable())
        A.worker = std::thread([this, &ln]() {
            AsyncGvd &W = ln.ag;
            std::unique_lock<std::mutex> l(W.mu);
            for (;;) {
                W.cv.wait(l, [&W] { return W.busy || W.quit; });
                if (W.quit) return;
                l.unlock();
                std::exception_ptr e;
                bool pub = false;
                try {
                    AOS_HIP(hipSetDevice(device));
                    GvdStageIn gi{W.seeds.data(), (int)(W.seeds.size() / 2), W.rows.data(), (int)(W.rows.size() / 2),
                                  W.info, ln.gs.skel.as<int8_t>()};
                    gi.hook_arg = &W;
                    gi.on_host_phase = [](void *p) {
                        AsyncGvd *A = static_cast<AsyncGvd *>(p);
                        { std::lock_guard<std::mutex> g(A->mu); A->prefix = true; }
                        A->cv.notify_all();
                    };
                    pub = run_gvd_stage(ln.gs, W.P, gi, W.stream, W.ev.data());
                } catch (...) { e = std::current_exception(); }
                l.lock();
                W.err = e;
                W.pub = pub;
                W.busy = false;
                W.done = true;
                W.cv.notify_all();
            }
        });
    {
        std::lock_guard<std::mutex> l(A.mu);
        A.err = nullptr;
        A.done = false;
        A.prefix = false;
        A.busy = true;
    }
    A.cv.notify_all();
    inflight.push_back(L);
    view_newest = true;
    // Return once the job's short GPU prefix (seed merge) is done and its host replay runs: a
    // seed-gen frame launched earlier would occupy the GPU and hold the prefix back, and the replay
    // would start late instead of overlapping it.
    std::unique_lock<std::mutex> l(A.mu);
    A.cv.wait(l, [&A] { return A.prefix || !A.busy; });
}

// aos_gvd_wait: collects the oldest job in flight (raising its error if rethrow); its lane becomes
// the handle's current result (markers, planning).
bool aos_ctx::gvd_async_wait(bool rethrow) {
    if (inflight.empty()) return false;
    const int l = inflight.front();
    inflight.pop_front();
    view_newest = false;
    lane_join(l);
    AsyncGvd &A = lanes[l]->ag;
    std::exception_ptr e;
    {
        std::lock_guard<std::mutex> lk(A.mu);
        A.done = false;
        e = A.err;
        A.err = nullptr;
    }
    if (e) {
        if (rethrow) std::rethrow_exception(e);
        return false;
    }
    // a settle (markers / planning before this wait) already made this lane current: same graph, so the
    // path planner's graph cache (keyed on gvd_gen) stays valid
    if (!(cur_lane == l && A.applied && have_gvd)) lane_apply(l);
    return true;
}

// Markers and planning on the handle's own graph: right after aos_gvd_wait they see the collected
// job; with no wait since the last start they see the newest job (waited for, still collectable).
void aos_ctx::gvd_view_settle() {
    if (!view_newest || inflight.empty()) return;
    const int l = inflight.back();
    lane_join(l);
    AsyncGvd &A = lanes[l]->ag;
    bool ok;
    {
        std::lock_guard<std::mutex> lk(A.mu);
        ok = A.done && !A.err;
    }
    if (ok && (cur_lane != l || !have_gvd)) lane_apply(l);
}

// The planner calls' graph: the caller's, or the current result's (the caller has settled which one that is), every
// array of it, with load_graph's cache key; markers_wait first, as every reader of gs() on the caller's thread does.
aos_ctx::PlanGraph aos_ctx::plan_graph(const aos_path_graph *graph) {
    if (graph) return {*graph, nullptr, 0};
    if (!have_gvd) throw std::runtime_error("no GVD graph on this handle");
    GvdState &G = gs();
    markers_wait(G, false);
    aos_path_graph own{};
    own.num_nodes = (int32_t)G.labels.size(); own.nodes_xy = G.nodes_xy.data();
    own.node_labels = G.labels.data(); own.node_cluster_indices = G.cluster_idx.data();
    own.node_label_counts = G.label_counts.data();
    own.n_label_entries = (int32_t)G.label_clusters.size();
    own.node_label_clusters = G.label_clusters.data(); own.node_label_types = G.label_types.data();
    own.num_edges = (int32_t)G.lengths.size(); own.edges = G.edges_out.data(); own.edge_lengths = G.lengths.data();
    return {own, &G, gvd_gen};
}

// The planner calls' grid on the device: the caller's device pointer as it is, the caller's host grid copied into
// staging on the handle's stream (never null: staging holds a byte at least), or the skeleton of the current GVD
// result while it is still the one that call used.
aos_ctx::PlanGrid aos_ctx::plan_grid(const int8_t *grid, int on_device, const aos_grid_info *info, DevBuf &staging) {
    if (grid) {
        if (on_device) return {grid, *info};
        const size_t C = (size_t)info->width * info->height;
        int8_t *d = staging.ensure_n<int8_t>(C);
        if (C) AOS_HIP(hipMemcpyAsync(d, grid, C, hipMemcpyHostToDevice, stream));
        return {d, *info};
    }
    if (!have_gvd) throw std::runtime_error("no grid given and no GVD call on this handle");
    if (gvd_from_frame && gvd_frame_gen != frame_gen)
        throw std::runtime_error("the GVD graph's skeleton was replaced by a later seed-gen frame; pass the grid");
    return {gvd_skel, gvd_info};
}

// A synchronous GVD call (or the handle's release) supersedes every job in flight.
void aos_ctx::gvd_async_drop() {
    gvd_lanes_ensure();
    for (int l : inflight) {
        lane_join(l);
        std::lock_guard<std::mutex> lk(lanes[l]->ag.mu);
        lanes[l]->ag.done = false;
        lanes[l]->ag.err = nullptr;
    }
    inflight.clear();
    view_newest = false;
}

void aos_ctx::gvd_async_stop() {
    for (auto &lp : lanes) {
        AsyncGvd &A = lp->ag;
        if (A.worker.joinable()) {
            { std::lock_guard<std::mutex> l(A.mu); A.quit = true; }
            A.cv.notify_all();
            A.worker.join();
        }
        if (A.stream) {
            (void)hipStreamSynchronize(A.stream);
            for (auto &e : A.ev) (void)hipEventDestroy(e);
            (void)hipEventDestroy(A.ready);
            A.stream = nullptr;   // (the shared gvd_stream)
        }
    }
    if (gvd_stream) {
        (void)hipStreamDestroy(gvd_stream);
        gvd_stream = nullptr;
    }
    inflight.clear();
    view_newest = false;
}

int aos::gvd_wait_out(aos_ctx *c, aos_gvd_out *out) {   // aos_gvd_wait (api.hip)
    if (!c->gvd_async_wait(true)) return 0;
    const aos_ctx::GvdLane &ln = *c->lanes[c->cur_lane];
    fill_gvd_out(*c, ln.gs, ln.ag.info, ln.ag.pub, *out);
    return 1;
}
