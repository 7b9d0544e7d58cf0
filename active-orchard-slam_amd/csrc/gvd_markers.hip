// The GVD markers' Voronoi cells (publishMarkers, src/aos_gvd_node.cpp:1098-1194): host work on the merged seeds, on
// a worker thread of its own next to the main graph's Subdiv2D replay (gvd.hip). No device code.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>

#include "gvd.h"

namespace aos {

// publishMarkers' Voronoi cells (gvd:1098-1194): VoronoiDiagram::extractCellBoundaries
// (voronoi_diagram.cpp:209-311), a second Subdiv2D over the finite merged seeds with their own
// bounding box as the rectangle, then cell i = facet i (i < seeds, facets) with >= 3 points, closed
// when its ends are more than 1 cm apart, paired with seeds_[i] and coloured from hue = i / cells.
// Pure host work on the merged seeds: it runs on a worker thread next to the main replay.
static void cells_colours(CellsWork &W, const std::vector<double> &seeds, int ncell);

static void compute_cells(CellsWork &W, int rect_mode) {
    const auto t0 = std::chrono::steady_clock::now();
    struct CellTrace {
        const double t = trace_on() ? trace_ms() : 0.0;
        ~CellTrace() { if (trace_on()) fprintf(stderr, "[aos trace cells] %.2f -> %.2f\n", t, trace_ms()); }
    } ctr;
    W.cell_off.assign(1, 0);
    W.cell_xy.clear(); W.cell_center.clear(); W.cell_rgba.clear();
    const std::vector<double> &seeds = W.seeds;   // VoronoiDiagram::seeds_ = the finite merged seeds
    const int ns = (int)seeds.size() / 2;
    if (ns == 0) return;
    double min_x = std::numeric_limits<double>::max(), max_x = std::numeric_limits<double>::lowest();
    double min_y = min_x, max_y = max_x;
    for (int i = 0; i < ns; ++i) {
        min_x = std::min(min_x, seeds[2 * i]); max_x = std::max(max_x, seeds[2 * i]);
        min_y = std::min(min_y, seeds[2 * i + 1]); max_y = std::max(max_y, seeds[2 * i + 1]);
    }
    // (subdiv_build's bound swap and finite test do nothing here: the bounds are a min / max over the seeds, and
    // markers_start kept only the finite ones; extractCellBoundaries has neither. Insertion failures are skipped,
    // voronoi_diagram.cpp:280-285)
    Subdiv2D &sd = W.sd;
    if (!subdiv_build(sd, min_x, max_x, min_y, max_y, seeds.data(), ns, rect_mode)) return;
    // getVoronoiFacetList on the worker's own core (calcVoronoi + the facet walk of subdiv2d.cpp, the host
    // reference of the main graph's GPU builder, bit-identical to it): the markers job needs no stream, pinned
    // buffers or GPU time of its own; the walk costs the worker a few ms next to its replay. (The markers'
    // facets on the GPU builder were kept as AOS_MARKERS_GPU_FACETS=1, removed.)
    std::vector<int> off;
    std::vector<float> xy;
    sd.voronoi_facets(off, xy);
    int ncell = 0;
    for (size_t f = 0; f + 1 < off.size() && (int)f < ns; ++f) {
        const int b0 = off[f], n = off[f + 1] - b0;
        if (n < 3) continue;
        for (int j = 0; j < n; ++j) { W.cell_xy.push_back(xy[2 * (b0 + j)]); W.cell_xy.push_back(xy[2 * (b0 + j) + 1]); }
        const double dx = (double)xy[2 * b0] - (double)xy[2 * (b0 + n - 1)];
        const double dy = (double)xy[2 * b0 + 1] - (double)xy[2 * (b0 + n - 1) + 1];
        if (std::sqrt(dx * dx + dy * dy) > 0.01) { W.cell_xy.push_back(xy[2 * b0]); W.cell_xy.push_back(xy[2 * b0 + 1]); }
        W.cell_off.push_back((int32_t)(W.cell_xy.size() / 2));
        ++ncell;
    }
    cells_colours(W, seeds, ncell);
    W.ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// cell i's centre and colour (gvd:1117-1145, float arithmetic as written)
static void cells_colours(CellsWork &W, const std::vector<double> &seeds, int ncell) {
    for (int i = 0; i < ncell; ++i) {
        W.cell_center.push_back(seeds[2 * i]); W.cell_center.push_back(seeds[2 * i + 1]);
        float hue = static_cast<float>(i) / std::max(1.0f, static_cast<float>(ncell));
        float saturation = 0.7f, value = 0.9f;
        float cc = value * saturation;
        float x = cc * (1.0f - std::abs(std::fmod(hue * 6.0f, 2.0f) - 1.0f));
        float m = value - cc;
        float r = 0.0f, g = 0.0f, b = 0.0f;
        if (hue < 1.0f / 6.0f) { r = cc; g = x; b = 0.0f; }
        else if (hue < 2.0f / 6.0f) { r = x; g = cc; b = 0.0f; }
        else if (hue < 3.0f / 6.0f) { r = 0.0f; g = cc; b = x; }
        else if (hue < 4.0f / 6.0f) { r = 0.0f; g = x; b = cc; }
        else if (hue < 5.0f / 6.0f) { r = x; g = 0.0f; b = cc; }
        else { r = cc; g = 0.0f; b = x; }
        W.cell_rgba.push_back(r + m); W.cell_rgba.push_back(g + m); W.cell_rgba.push_back(b + m); W.cell_rgba.push_back(0.4f);
    }
}

// The cells' worker thread. publishMarkers runs after publishGraph (gvd:310-313), so the graph is
// returned as soon as it is ready and the cells finish in the background: aos_gvd_markers_get, the
// next GVD call and release() join the job (markers_wait). An error of the job is raised by
// aos_gvd_markers_get; a job nobody asked about is discarded by the next call.
void markers_start(GvdState &G, int rect_mode) {
    if (!G.cells) G.cells.reset(new CellsWork());
    CellsWork &W = *G.cells;
    W.seeds.clear();
    for (size_t i = 0; i + 1 < G.merged_xy.size(); i += 2)
        if (std::isfinite(G.merged_xy[i]) && std::isfinite(G.merged_xy[i + 1])) {
            W.seeds.push_back(G.merged_xy[i]); W.seeds.push_back(G.merged_xy[i + 1]);
        }
    if (!W.worker.joinable())
        W.worker = std::thread([&W]() {
            std::unique_lock<std::mutex> l(W.mu);
            for (;;) {
                W.cv.wait(l, [&W] { return W.busy || W.quit; });
                if (W.quit) return;
                l.unlock();
                std::exception_ptr e;
                try { compute_cells(W, W.rect_mode); } catch (...) { e = std::current_exception(); }
                l.lock();
                W.err = e;
                W.busy = false;
                W.cv.notify_all();
            }
        });
    {
        std::lock_guard<std::mutex> l(W.mu);
        W.rect_mode = rect_mode;
        W.err = nullptr;
        W.busy = true;
    }
    W.cv.notify_all();
}

void markers_on_demand(GvdState &G) {
    markers_start(G, G.rect_mode);
    markers_wait(G, true);
    G.have_markers = true;
}

void markers_wait(GvdState &G, bool rethrow) {
    if (!G.cells) return;
    CellsWork &W = *G.cells;
    std::unique_lock<std::mutex> l(W.mu);
    W.cv.wait(l, [&W] { return !W.busy; });
    if (W.err) {
        std::exception_ptr e = W.err;
        W.err = nullptr;
        G.have_markers = false;
        if (rethrow) std::rethrow_exception(e);
    }
}

}  // namespace aos
