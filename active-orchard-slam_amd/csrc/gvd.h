// GVD stage state: the facet builder's buffers, the markers' cells job, the per-lane GvdState and the stage's entry
// points (gvd.hip: kernels and run_gvd_stage; gvd_markers.hip: the cells' host worker; gvd_handle.hip: the handle's
// methods). Not part of the ABI.
#pragma once
#include <condition_variable>
#include <exception>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "aos_internal.h"
#include "cluster_seed.h"
#include "dev_prims.h"
#include "subdiv2d.h"

namespace aos {

// ------------------------------------------------------------------ GVD
// publishMarkers' Voronoi cells, computed by a worker thread next to the main Subdiv2D replay. It
// lives in its own cache-line-aligned heap object: the two replays write their state on every step,
// and sharing lines with the main replay's fields slowed both down by ~40 % on the EPYC host.
// Device buffers of the facet builder (calcVoronoi + getVoronoiFacetList on the GPU, gvd.hip).
// raw = the exported Subdiv2D state in one buffer (quad-edges | points | firstEdge | type), one H2D copy
struct FacetBufs { DevBuf raw, face, cnt, off; LookBackScratch lb; PinnedBuf h_stage; int *qe = nullptr, *vf = nullptr, *vt = nullptr; };

struct alignas(128) CellsWork {
    Subdiv2D sd;                               // extractCellBoundaries' Subdiv2D
    std::vector<double> seeds;                 // VoronoiDiagram::seeds_ (finite merged seeds)
    std::vector<double> cell_xy, cell_center;
    std::vector<int32_t> cell_off;
    std::vector<float> cell_rgba;
    float ms = 0;
    // One persistent worker per handle: it sleeps between frames and keeps its core (and the
    // replay's ~6 MB of quad-edges in that core's caches); a thread per frame landed on a cold core.
    std::thread worker;
    std::mutex mu;
    std::condition_variable cv;
    bool busy = false, quit = false;
    int rect_mode = 0;
    std::exception_ptr err;     // the last job's error (markers_wait raises or discards it)
    CellsWork() = default;
    CellsWork(const CellsWork &) = delete;
    CellsWork &operator=(const CellsWork &) = delete;
    ~CellsWork() {
        if (worker.joinable()) {
            { std::lock_guard<std::mutex> l(mu); quit = true; }
            cv.notify_all();
            worker.join();
        }
    }
};

struct GvdScratch;   // the stage's device scratch (gvd.hip)

struct GvdState {
    GvdState();
    ~GvdState();   // (both in gvd.hip, where GvdScratch is complete: a constructor unwinds its members too)
    DedupScratch dedup;
    DevBuf skel;         // the framed skeleton of an external call or a lane's snapshot (gvd_handle.hip)
    PinnedBuf h_misc;
    std::unique_ptr<GvdScratch> scratch;   // allocated by the first run_gvd_stage
    PinnedBuf h_seeds;   // seeds in / merged seeds out (g1)
    PinnedBuf h_out;     // the GvdGraph arrays, gathered into it by one kernel (k_gather_words)
    PinnedBuf h_evals;   // the graph searches' work counters (aos_params.gvd_count_evals)
    aos_gvd_evals evals{};
    SyncEvent sev;       // host waits of this state's GVD calls (the stream may be shared by several lanes)
    Subdiv2D subdiv;   // host insert replay; kept across frames to reuse its allocations
    // host outputs
    std::vector<double> nodes_xy;
    std::vector<int32_t> labels, cluster_idx, label_counts, label_clusters, label_types, edges_out;
    std::vector<float> lengths, clearances;
    int n_merged = 0, n_vor_edges = 0, n_bpts = 0;
    int pairs_cap = 0;   // capacity of the g6 pair lists (from the last frame's pair count)
    float ms_merge = 0, ms_delaunay = 0, ms_graph = 0, ms_total = 0;
    // markers (aos_gvd_markers)
    bool have_markers = false;
    bool graph_ok = false;     // the last GVD call produced a graph (markers can be computed on demand)
    int rect_mode = 0;         // its Subdiv2D rectangle mode
    std::vector<double> merged_xy, row_label_xy;
    std::vector<int32_t> row_label_valid;
    std::unique_ptr<CellsWork> cells;   // the worker thread's own heap object (no false sharing)
};

struct GvdStageIn {
    const double *seeds_host;  int n_seeds;     // /voronoi_seeds (x, y)
    const double *rows_info;   int n_rows_poses;
    aos_grid_info info;
    const int8_t *d_skeleton;                   // framed skeleton bytes on device
    // called once the merged seeds are on the host, when the GPU prefix is done and the host
    // Subdiv2D replay starts (the pipelined caller lets the next seed-gen frame go from here)
    void (*on_host_phase)(void *) = nullptr;
    void *hook_arg = nullptr;
};
bool run_gvd_stage(GvdState &G, const aos_params &P, const GvdStageIn &in, hipStream_t stream, hipEvent_t *ev);
// The Subdiv2D of VoronoiDiagram::compute (voronoi_diagram.cpp:27-89: the main graph) and of extractCellBoundaries
// (:209-311: the markers' cells), the same float expressions in both: orders the bounds, widens an extent under
// 1.0 to 1.0 about its centre, takes the rectangle one unit beyond them and inserts every finite (x, y) of xy[2 n],
// clamped to the rectangle less 0.1f. False (nothing built) when the rectangle is empty. (gvd.hip)
bool subdiv_build(Subdiv2D &sd, double min_x, double max_x, double min_y, double max_y, const double *xy, int n,
                  int rect_mode);
// Starts the markers' cells job on G.merged_xy (the cells' worker thread; gvd_markers.hip).
void markers_start(GvdState &G, int rect_mode);
// Joins the markers' cells job of the last GVD call; rethrow: raise its error (else discard it).
void markers_wait(GvdState &G, bool rethrow);
// aos_gvd_markers_get on a frame whose GVD ran without markers: compute them now (and wait)
void markers_on_demand(GvdState &G);

}  // namespace aos
