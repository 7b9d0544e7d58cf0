// Stand-alone driver of the product's host sight code (csrc/sight_host.cpp with csrc/sight.h, csrc/reach_host.cpp and
// csrc/clearance_host.cpp):
//   sight_host_main IN OUT [REPS]
// IN:  int32 scene count, then per scene int32 W, H, S, Q, K, uint32 min_d2, double origin_x, origin_y, float
//      resolution, W * H int8 cells, S x 2 doubles (sources), Q x 2 doubles (segment starts), Q x 2 doubles (segment
//      ends), then K pulls of 2 doubles (the start) and int32 max_span.
// OUT: per scene int32 status (0, or -1 where the library returns AOS_E_INVALID: nothing more follows for it), Q uint32
//      (n_touched), Q uint32 (n_blocked), then per pull uint64 n_cells, uint32 start_cost, uint32 n_waypoints,
//      n_waypoints uint32 (steps), n_waypoints uint32 (cells), n_waypoints x 2 doubles (centres), double length_m,
//      double descent_m, uint64 n_sight_tests.
// Before the scenes the refusals of the two check functions are tried, the 65536-cell limit among them.
// REPS > 0: each scene's sight queries and pulls are also run REPS times and "ms sight <scene> <Q> <median ms>" and
// "ms pull <scene> <pull> <median ms>" are printed (the bench tool's host column). Built by test_sight_cpu.py with
// ASan + UBSan; no GPU, no HIP.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sight.h"

using namespace aos;

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

template <class F> static double median_ms(int reps, F &&f) {
    std::vector<double> ms;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        f();
        const auto t1 = std::chrono::steady_clock::now();
        ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: sight_host_main IN OUT [REPS]\n"); return 2; }
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    {
        const double p[2] = {0.0, 0.0};
        const bool ok = sgt::check_sight(nullptr, nullptr, -1) && sgt::check_sight(nullptr, p, 1) && sgt::check_sight(p, nullptr, 1) &&
                        !sgt::check_sight(nullptr, nullptr, 0) && !sgt::check_sight(p, p, 1) && !sgt::check_pull(0) &&
                        !sgt::check_pull(sgt::kMaxDescent) && sgt::check_pull(sgt::kMaxDescent + 1) && sgt::kMaxDescent == 65536;
        if (!ok) { fprintf(stderr, "a check function accepts or refuses wrongly\n"); return 2; }
        printf("sight_host_main checks ok\n");
    }
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    int32_t count = 0;
    if (!rd(fi, &count, sizeof(count)) || count < 0) { fprintf(stderr, "short input\n"); return 2; }
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[5];
        uint32_t min_d2;
        double org[2];
        float resolution;
        if (!rd(fi, head, sizeof(head)) || !rd(fi, &min_d2, sizeof(min_d2)) || !rd(fi, org, sizeof(org)) ||
            !rd(fi, &resolution, sizeof(resolution)) || head[0] < 0 || head[1] < 0 || head[2] < 0 || head[3] < 0 ||
            head[4] < 0) { fprintf(stderr, "short input\n"); return 2; }
        const int32_t W = head[0], H = head[1], S = head[2], Q = head[3], K = head[4];
        const size_t C = (size_t)W * (size_t)H;
        std::vector<int8_t> cells(C);
        std::vector<double> src(2 * (size_t)S), from(2 * (size_t)Q), to(2 * (size_t)Q), starts(2 * (size_t)K);
        std::vector<int32_t> spans(K);
        bool ok = rd(fi, cells.data(), C) && rd(fi, src.data(), sizeof(double) * src.size()) &&
                  rd(fi, from.data(), sizeof(double) * from.size()) && rd(fi, to.data(), sizeof(double) * to.size());
        for (int32_t i = 0; ok && i < K; ++i) ok = rd(fi, &starts[2 * (size_t)i], 2 * sizeof(double)) && rd(fi, &spans[i], sizeof(int32_t));
        if (!ok) { fprintf(stderr, "short input\n"); return 2; }
        aos_grid_info info{org[0], org[1], resolution, (uint32_t)W, (uint32_t)H};
        int32_t status = 0;
        if (clr::check_info(info) || rch::check_reach(S ? src.data() : nullptr, S) ||
            sgt::check_sight(Q ? from.data() : nullptr, Q ? to.data() : nullptr, Q))
            status = -1;
        fwrite(&status, sizeof(status), 1, fo);
        if (status) continue;
        const clr::Grid g{info.origin_x, info.origin_y, (double)info.resolution, W, H};
        std::vector<uint32_t> cost(C);
        std::vector<uint8_t> pass(C);
        rch::Counts n;
        rch::reach_host(cells.data(), g, src.data(), S, min_d2, cost.data(), n);
        sgt::sight_host_mask(cells.data(), g, min_d2, pass.data());
        std::vector<uint32_t> nt(Q), nb(Q);
        sgt::sight_host(g, pass.data(), from.data(), to.data(), Q, nt.data(), nb.data());
        if (Q) fwrite(nt.data(), sizeof(uint32_t), Q, fo);
        if (Q) fwrite(nb.data(), sizeof(uint32_t), Q, fo);
        if (reps > 0 && Q)
            printf("ms sight %d %d %.4f\n", (int)k, (int)Q, median_ms(reps, [&] {
                       sgt::sight_host(g, pass.data(), from.data(), to.data(), Q, nt.data(), nb.data());
                   }));
        for (int32_t i = 0; i < K; ++i) {
            const double sx = starts[2 * (size_t)i], sy = starts[2 * (size_t)i + 1];
            const uint64_t m = rch::reach_host_descend(g, cost.data(), sx, sy, nullptr, 0);
            if (sgt::check_pull(m)) { fprintf(stderr, "a scene's descent is above the limit\n"); return 2; }
            std::vector<uint32_t> path(m), steps(m), wc;
            std::vector<double> xy;
            uint32_t nw = 0;
            auto run = [&] {
                rch::reach_host_descend(g, cost.data(), sx, sy, path.data(), m);
                nw = sgt::pull_host(pass.data(), W, path.data(), m, spans[i], steps.data());
            };
            run();
            sgt::PullCounts pc;
            sgt::pull_finish(g, path.data(), m, m ? cost[path[0]] : sgt::kNone, steps.data(), nw, spans[i], pc);
            wc.resize(nw);
            xy.resize(2 * (size_t)nw);
            for (uint32_t j = 0; j < nw; ++j) {
                wc[j] = path[steps[j]];
                rch::cell_centre(g, wc[j], xy[2 * (size_t)j], xy[2 * (size_t)j + 1]);
            }
            fwrite(&pc.n_cells, sizeof(uint64_t), 1, fo);
            fwrite(&pc.start_cost, sizeof(uint32_t), 1, fo);
            fwrite(&nw, sizeof(uint32_t), 1, fo);
            if (nw) fwrite(steps.data(), sizeof(uint32_t), nw, fo);
            if (nw) fwrite(wc.data(), sizeof(uint32_t), nw, fo);
            if (nw) fwrite(xy.data(), sizeof(double), 2 * (size_t)nw, fo);
            fwrite(&pc.length_m, sizeof(double), 1, fo);
            fwrite(&pc.descent_m, sizeof(double), 1, fo);
            fwrite(&pc.n_sight_tests, sizeof(uint64_t), 1, fo);
            if (reps > 0) printf("ms pull %d %d %.4f\n", (int)k, (int)i, median_ms(reps, run));
        }
    }
    fclose(fi);
    if (fclose(fo) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    printf("sight_host_main ok %d scenes\n", (int)count);
    return 0;
}
