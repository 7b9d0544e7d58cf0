// Per-handle state of libaos_gpu.so. Not part of the ABI. Every buffer member frees itself with the handle;
// release() (seedgen.hip) stops the threads and destroys the streams and events first.
// Methods by file: seedgen.hip the frame (release, run_seedgen*, the thinning driver, the grid copies, finish_frame,
// debug_grid); cloud_upload.hip the cloud upload, the prefetch and the streaming map's ingest; ror_stage.hip the
// ROR stage; tiled.hip the tiled frame; gvd_handle.hip the GVD and the planner calls' graph and grid (plan_graph,
// plan_grid); path.hip the planner (linearize.hip, clearance.hip, regions.hip, reach.hip, width.hip and soft.hip have no
// method: their states are the OwnedState members lin_state, clear_state, regions_state, reach_state, width_state and
// soft_state).
#pragma once
#include <array>
#include <condition_variable>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "aos_internal.h"
#include "cluster_seed.h"
#include "grid_host.h"
#include "gvd.h"
#include "host_pool.h"
#include "ror.h"

// Indices of aos_ctx::ev, recorded on the handle's stream in frame order unless said otherwise. AsyncGvd::ev uses
// the kEvGvd* four only (run_gvd_stage). The numbers are the ones the code grew up with.
enum FrameEvent : int {
    kEvFrameBegin = 0,       // before the frame's first launch
    kEvRorEnd = 1,           // a1-a4 done: the raster bits are complete
    kEvGridEnd = 2,          // a5-a6: inflated (a tiled frame: after the raster halo exchange)
    kEvThinEnd = 3,          // a7: the skeleton is picked
    kEvClusterEnd = 4,       // a8-a10 (run_cluster_seed_stage records it; a non-root tiled rank: its frame's end)
    kEvSeedsEnd = 5,         // a11-a15: the frame's end
    kEvGridsGathered = 6,    // a tiled frame: the grids are on the root, the distributed cluster stage begins ...
    kEvGvdBegin = 6,         // ... and, later, on the same handle: run_gvd_stage begins (never both in flight)
    kEvGvdMerged = 7,        // the seeds are merged
    kEvGvdEdges = 8,         // the Voronoi edges are on the device: the graph kernels begin
    kEvGvdEnd = 9,           // the graph's outputs are gathered
    kEvRorTilesBegin = 10,   // the ROR scatter is done, the tile pass begins
    kEvRorTilesEnd = 11,     // the tile pass (k_rt_ror, a streaming map's merge and sum included) is done
    kEvRorCountBegin = 12,   // the count pass (count + column scan) begins
    kEvRorCountEnd = 13,
    kEvRorScatterBegin = 14, // after the sizing read-back, if the frame needed one
    kEvUploadGate = 15,      // the uploader's streams wait for it: the work queued before a host cloud is overwritten
    kEvStageBegin = 16,      // 16, 17: AOS_TRACE splits of the cluster stage (run_cluster_seed_stage takes the pair)
    kEvStageGpuEnd = 17,
    kEvCount
};

struct aos_ctx {
    aos_params P{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::array<hipEvent_t, kEvCount> ev{};
    // elapsed ms between two of them (both recorded and reached)
    float ms_ev(FrameEvent a, FrameEvent b) const { float t = 0; (void)hipEventElapsedTime(&t, ev[a], ev[b]); return t; }
    aos::Poly poly;

    // ---- last cloud (reprocess reuses it: seed_gen:244, 283-285)
    bool have_cloud = false, have_frame = false;
    const uint8_t *d_cloud = nullptr;  // device view (own copy or caller's device buffer)
    uint64_t n_points = 0;
    uint32_t step = 16, ox = 0, oy = 4, oz = 8;
    int is_dense = 1;

    // ---- streaming map (aos_map_append): float4 x, y, z, 0
    aos::DevBuf map_buf, scan_stage;
    uint64_t map_n = 0;
    int map_dense = 1;
    // tiled streaming map (aos_tiled_map_append): the rank's map holds only the points of its points
    // box; map_total counts every point appended (the frame's n_input, as on one GPU)
    bool map_boxed = false;
    float map_box[4] = {0, 0, 0, 0};
    uint64_t map_total = 0;
    aos::DevBuf map_count;
    aos::PinnedBuf h_map_count;
    // ---- device buffers
    aos::DevBuf cloud_copy;
    aos::DevBuf raster_bits, infl_bits, open_bits, thin_a, thin_b, thin_act, occ_bytes, skel_bytes, flags;
    aos::DevBuf thin_out;   // the converged skeleton bits, picked on the device (launch_thin_pick)
    aos::DevBuf full_infl, full_skel;      // tiled frames: the whole map, assembled on the root rank
    aos::PinnedBuf h_small;
    // Host -> device upload of a large pageable buffer (a PointCloud2 message): kUpThreads host
    // threads copy 2 MB chunks into rings of pinned slots, each DMA'd on the thread's stream (tools/upload_ab.py:
    // 4-8 threads and 1-8 MB chunks all upload C2's 120 MB in 3-4 ms on the box, the H2D DMA's ~40 GB/s).
    static constexpr int kUpThreads = 16;   // capacity; up_threads() of them gather (AOS_UP_THREADS, default 16)
    static int up_threads();
    static constexpr int kUpSlots = 4;      // pinned slots per thread (a ring: gather one while others DMA)
    struct Uploader {
        aos::PinnedBuf slot[kUpThreads][kUpSlots];
        hipStream_t st[kUpThreads] = {};
        hipEvent_t ev[kUpThreads][kUpSlots] = {}, done[kUpThreads] = {};
        bool used[kUpThreads][kUpSlots] = {};
    } up;
    aos::HostPool up_pool;                  // the gather threads (upload_pack)
    // A host cloud is split while it is gathered (upload_pack): the points inside `box`, the ROR stage's
    // binned box for the polygon and parameters current at upload time (ror_stage: no point outside it
    // can be binned), go to the device, packed at the front of the cloud buffer in chunk-arrival order (the
    // ROR results do not depend on point order); the others stay in `rest` (pageable host memory: it is copied
    // only when the polygon grows, so it holds no page-locked memory — 2 x 12 n bytes at C2 with a prefetch —
    // ADVICE r04; thread t's run at byte rbeg[t], rn[t] points). A frame whose binned box is not inside `box`
    // (the polygon changed: aos_seedgen_reprocess) first copies the rest behind the front (cloud_for_box).
    struct CloudSplit {
        aos::HostBuf rest;
        uint64_t rbeg[kUpThreads] = {}, rn[kUpThreads] = {};
        int nth = 0;
        uint64_t n_front = 0, n_all = 0;
        float box[6] = {};          // bminx, bmaxx, bminy, bmaxy, bminz, bmaxz
        bool on = false;            // split (else all n_all points are on the device)
        bool whole = false;         // the rest was copied behind the front
        hipEvent_t copied = nullptr;   // that copy (recorded on the handle's stream; rest is rewritten after it)
        bool copy_pending = false;
        void swap_with(CloudSplit &o);
    } split_cur, split_next;
    static bool split_enabled();    // AOS_UP_SPLIT (default 1)
    bool split_box(const aos::Poly &poly, float box[6]) const;   // false: do not split
    uint64_t cloud_for_box(const float b[6]);   // device points the ROR stage reads for binned box b
    // prefetch = true (aos_cloud_prefetch): dst is not read by queued work and the handle's stream is not
    // made to wait; the consumer waits for up.done[] (set_cloud). sp: the split's state (box[] and on set
    // by the caller; on = false: no split)
    void upload_pack(void *dst, const aos_cloud_view &v, CloudSplit &sp, bool prefetch = false);
    void release_uploader();
    // aos_cloud_prefetch: the next frame's cloud uploaded into cloud_next on a background thread
    struct Prefetch {
        std::thread th;
        aos_cloud_view view{};
        const void *src = nullptr;
        size_t bytes = 0;
        bool active = false;
        std::exception_ptr err;
        float box[6] = {};
        bool split = false;
    } pf;
    aos::DevBuf cloud_next;
    void prefetch_start(const aos_cloud_view &v);
    bool prefetch_join();   // true: a prefetch was in flight and succeeded
    const uint64_t *skel_bits = nullptr;   // final thinning buffer (thin_a / thin_b, or full_skel)
    aos::FrameGeom geom{};                 // the whole map
    bool tiled_frame = false;
    int thin_iters = 0, thin_iters_prev = 0;   // (the previous frame's T sizes the first thinning batch)
    // set while finish_frame runs ahead of the thinning flags: true once they show that thinning had not converged
    // (SeedStageIn::stale)
    std::function<bool()> frame_stale;
    // First thinning batch (n temporal-block launches; the opening, which clears the flags, runs just before it so the
    // inflated grid's read-back can be queued behind it) as hipGraphs, one per batch
    // size n (a power of two), captured on first use and replayed while every pointer and size baked into
    // the graph is unchanged (seedgen.hip thin_first_batch). aos_params.thin_graph = 0: plain launches.
    struct ThinGraph {
        hipGraphExec_t exec = nullptr;
        std::array<const void *, 5> ptrs{};   // every device pointer a node holds
        std::array<int, 7> dims{};            // W, H, WW, R, launches, flag ints, tiles
    };
    std::vector<ThinGraph> thin_graphs;
    int last_thin_graph = 0, last_thin_launches = 0;
    void thin_graphs_release();
    void thin_first_batch(const aos::FrameGeom &g, const uint64_t *d_ibits, uint64_t *d_open, uint64_t *const bufs[2],
                          int *d_flags, int *d_act, int nflags, int &batch_n, int cap_launches,
                          const std::function<void(int)> &launch_next, const std::function<void()> &after_open);
    uint64_t n_ror_kept = 0, n_clipped = 0;

    // ---- ROR stage, a1-a4 (ror.h; ror_stage.hip: these methods)
    aos::RorStage ror;
    // a1-a4 into the bit window rbits for the cells o owns; allow_guess: the frame may be redone (ror_collect)
    void ror_stage(const aos::FrameGeom &g, const aos::RorOwn &o, uint64_t *rbits, bool allow_guess);
    // after the frame's sync: true if the attempt failed (an overflow, a big tile, a stuck look-back)
    bool ror_collect(bool throw_stuck = true);
    void ror_stats_to_host(const int *d_staged_total, const aos::RorStatus *d_st);   // queues the stats' read-back
    void ror_stage_append(aos::RorLaunch L, uint64_t *rbits);   // streaming map: one scan on the tile store
    aos::LookBack ror_lookback(const aos::RorLaunch &L, int G, aos::RorStatus *d_st);
    void ror_stage_unchanged();   // streaming map: no new points since the committed store
    void ror_times(aos_seedgen_out &out);   // n_binned and the three ms_ror_* of a collected frame

    // ---- cluster / row / seed stage (cluster_seed.hip); tiled frames: distributed a8-a10 (cluster_dist.hip)
    aos::ClusterSeedState cs;
    aos::ClusterDistState cdist;
    aos::ClusterDistStats cdist_stats;

    // ---- host-side outputs of the last frame
    aos::PinnedBuf h_occ, h_skel;   // the two OccupancyGrids (pinned: the D2H runs at DMA speed)
    aos::PinnedBuf h_occ_bits, h_skel_bits;   // their bit-packed device grids (the default read-back, grid_host.h)
    aos::GridExpander expander;               // expands them on host threads beside the cluster / seed stage
    hipStream_t copy_stream = nullptr;   // their D2H, beside the cluster / seed stage
    hipEvent_t copy_ready = nullptr, copy_done = nullptr;
    bool infl_bits_sent = false;         // this frame's inflated-grid bits are already on the copy stream
    void grid_d2h(void *h, const void *d, size_t bytes);   // on the copy stream, after the work queued so far
    void grid_copy_wait();
    std::vector<double> h_row_center, h_row_start, h_row_end, h_row_length, h_voronoi, h_rows_info, h_cluster_info;
    int n_virtual = 0, n_ray = 0, n_endpoint = 0, n_clusters_all = 0, n_bfs_replayed = 0;

    // ---- GVD (gvd.hip: the stage; gvd_handle.hip: these methods)
    bool have_gvd = false, gvd_from_frame = false;
    uint64_t frame_gen = 0, gvd_frame_gen = 0, gvd_gen = 0;   // seed-gen frames / GVD calls so far
    const int8_t *gvd_skel = nullptr;                          // the skeleton the last GVD call used
    aos_grid_info gvd_info{};

    // ---- pipelined GVD (aos_gvd_from_seedgen_async): the reference runs seed-gen and the GVD as two
    // nodes, so frame k + 1's seed-gen overlaps frame k's graph. The GVD of a snapshot of the frame
    // (seeds, rows, skeleton) runs on a lane: a GvdState with a persistent worker thread and its own
    // stream. Frames are independent, so up to gvd_depth jobs may be in flight on gvd_depth lanes
    // (aos_gvd_pipeline_depth); one more lane holds the handle's current result (markers, planning).
    struct AsyncGvd {
        std::thread worker;
        std::mutex mu;
        std::condition_variable cv;
        bool busy = false, quit = false, pub = false, done = false, prefix = false;
        std::exception_ptr err;
        hipStream_t stream = nullptr;
        std::array<hipEvent_t, kEvGvdEnd + 1> ev{};   // (FrameEvent: the kEvGvd* four)
        hipEvent_t ready = nullptr;               // the snapshot copy on the seed-gen stream
        std::vector<double> seeds, rows;          // snapshot of h_voronoi / h_rows_info
        aos_grid_info info{};
        aos_params P{};                           // the handle's parameters when the job started (markers incl.)
        bool applied = false;                     // its result was made current by a settle (gvd_view_settle)
    };
    struct alignas(128) GvdLane {
        aos::GvdState gs;
        AsyncGvd ag;
    };
    std::vector<std::unique_ptr<GvdLane>> lanes{};   // lanes[cur_lane] holds the current result
    int cur_lane = 0, gvd_depth = 1;
    hipStream_t gvd_stream = nullptr;                // the lanes' shared GPU stream
    std::deque<int> inflight;                        // lanes with uncollected jobs, oldest first
    bool view_newest = false;                        // no aos_gvd_wait since the last job started
    aos::GvdState &gs() { return lanes[cur_lane]->gs; }
    void gvd_lanes_ensure();
    void gvd_async_start();
    bool gvd_async_wait(bool rethrow);   // aos_gvd_wait: collect the oldest job; false if none
    void gvd_view_settle();              // markers / planning: settle which result is current
    // The planner calls' inputs, from their arguments or from the current result (aos_path_plan, aos_gvd_clearance,
    // aos_gvd_regions, aos_gvd_reach, aos_gvd_width, aos_gvd_soft; each settles by its own rule first). graph null: the handle's own graph, with (key, gen) for
    // the planner's graph cache; throws without one. grid null: the current result's skeleton; a host grid is copied
    // into staging on the handle's stream.
    struct PlanGraph { aos_path_graph g; const void *key; uint64_t gen; };
    struct PlanGrid { const int8_t *d_grid; aos_grid_info info; };
    PlanGraph plan_graph(const aos_path_graph *graph);
    PlanGrid plan_grid(const int8_t *grid, int on_device, const aos_grid_info *info, aos::DevBuf &staging);
    void gvd_async_drop();               // a synchronous GVD call supersedes every job in flight
    void gvd_async_stop();
    void lane_join(int l);               // waits for lane l's job (no bookkeeping)
    void lane_apply(int l);              // lane l's finished job becomes the current result

    // ---- the planner calls' states, each defined in its file and created on first use: path planning (path.hip:
    // PathState), /aos/path -> /plan (linearize.hip: LinState), the distance field and GvdGraph clearances
    // (clearance.hip: ClearState), nearest-obstacle regions and the grid GVD ridge (regions.hip: RegionsState), the
    // clearance-limited cost-to-go field (reach.hip: ReachState), the widest-robot field (width.hip: WidthState), the
    // clearance-weighted cost-to-go field (soft.hip: SoftState)
    aos::OwnedState path_state, lin_state, clear_state, regions_state, reach_state, width_state, soft_state;

    // ---- cloud upload, prefetch and streaming map ingest (cloud_upload.hip)
    void set_cloud(const aos_cloud_view &v);
    void map_append(const aos_cloud_view &scan);
    void map_append_box(const aos_cloud_view &scan, const float box[4]);   // tiled streaming map
    void map_grow(uint64_t n);
    // ---- the frame (seedgen.hip; tiled.hip: run_tiled*, tile_halo_exchange)
    void finish_frame(const aos::FrameGeom &g, bool want_host, const uint64_t *clipped_total, aos_seedgen_out &out,
                      const aos::PreClusters *pre = nullptr);
    void run_seedgen(bool want_host, aos_seedgen_out &out);
    bool run_seedgen_once(bool want_host, aos_seedgen_out &out, bool allow_guess);   // true: redo
    void run_tiled(const aos_comm &cm, int tiles_x, int tiles_y, int root, bool want_host, aos_seedgen_out &out);
    void run_tiled_frame(aos::FrameComm &fc, int tiles_x, int tiles_y, int root, bool want_host, aos_seedgen_out &out);
    aos_tiled_stats tstats{};   // the last tiled frame's breakdown (aos_tiled_stats_get)
    std::vector<hipEvent_t> coll_ev;   // FrameComm: begin / end events of the frame's enqueued collectives
    aos::DevBuf coll_red;              // FrameComm: the reduced thinning flags
    aos::LookBackScratch debug_lb;     // aos_debug_scan
    void tile_halo_exchange(uint64_t *win, const aos::TilePlan &t, aos::FrameComm &fc);
    void run_gvd_external(const aos_gvd_in &in, aos_gvd_out &out);
    void run_gvd_from_frame(aos_gvd_out &out);
    void run_path_plan(const aos_path_graph *graph, const int8_t *skeleton, int skeleton_on_device,
                       const aos_grid_info *info, const aos_path_query &q, aos_path_out &out);
    int debug_grid(const char *which, int8_t *dst, uint64_t capacity);
    void release();
};

namespace aos {
// aos_gvd_wait: collects the pipelined GVD job's graph into out; 0 if no job was started (gvd_handle.hip)
int gvd_wait_out(aos_ctx *c, aos_gvd_out *out);
}  // namespace aos
