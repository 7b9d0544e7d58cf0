// Stand-alone driver of the product's host regions code (csrc/regions_host.cpp and csrc/clearance_host.cpp with
// csrc/regions.h and csrc/clearance.h):
//   regions_host_main IN OUT [REPS]
// IN:  int32 scene count, then per scene int32 W, H, N, has_labels, min_component_cells, want_ridge_distance, double
//      origin_x, origin_y, float resolution, W * H int8 cells, W * H int32 labels if has_labels, N x 2 doubles (nodes).
// OUT: per scene int32 status (0, or -1 where the library returns AOS_E_INVALID: nothing more follows for it), uint64
//      n_occupied, n_sites, n_ridge, int64 n_components, n_regions, uint32 max_d2, then W * H uint32 (site), W * H int32
//      (region), W * H int8 (ridge), W * H uint32 (ridge_d2, only if wanted), then N words each of node site, region,
//      d2, ridge_d2 and N floats (ridge offset, metres).
// REPS > 0: each scene is also run REPS times and "ms <scene> <cells> <median ms>" is printed (the bench tool's host
// column). Built by test_regions_cpu.py with ASan + UBSan; no GPU, no HIP.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "regions.h"

using namespace aos;

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
template <class T> static void wr(FILE *f, const std::vector<T> &v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: regions_host_main IN OUT [REPS]\n"); return 2; }
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    int32_t count = 0;
    if (!rd(fi, &count, sizeof(count)) || count < 0) { fprintf(stderr, "short input\n"); return 2; }
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[6];
        double org[2];
        float resolution;
        if (!rd(fi, head, sizeof(head)) || !rd(fi, org, sizeof(org)) || !rd(fi, &resolution, sizeof(resolution)) ||
            head[0] < 0 || head[1] < 0 || head[2] < 0) { fprintf(stderr, "short input\n"); return 2; }
        const int32_t W = head[0], H = head[1], N = head[2];
        const bool has_labels = head[3] != 0, want_rd = head[5] != 0;
        const aos_regions_opts opts{head[4], head[5]};
        const size_t C = (size_t)W * (size_t)H;
        std::vector<int8_t> cells(C);
        std::vector<int32_t> labels(has_labels ? C + 1 : 0);   // (one more: an empty grid's labels are still an array)
        std::vector<double> nodes(2 * (size_t)N);
        if (!rd(fi, cells.data(), C) || !rd(fi, labels.data(), has_labels ? sizeof(int32_t) * C : 0) ||
            !rd(fi, nodes.data(), sizeof(double) * nodes.size())) { fprintf(stderr, "short input\n"); return 2; }
        aos_grid_info info{org[0], org[1], resolution, (uint32_t)W, (uint32_t)H};
        int32_t status = 0;
        if (clr::check_info(info) || clr::check_graph(N ? nodes.data() : nullptr, N, nullptr, 0) ||
            rgn::check_regions(true, has_labels, &opts)) status = -1;
        fwrite(&status, sizeof(status), 1, fo);
        if (status) continue;
        const clr::Grid g{info.origin_x, info.origin_y, (double)info.resolution, W, H};
        std::vector<uint32_t> site(C), rd2(want_rd ? C : 0), n_site(N), n_d2(N), n_rd2(N);
        std::vector<int32_t> region(C), n_region(N);
        std::vector<int8_t> ridge(C);
        std::vector<float> n_m(N);
        rgn::Counts n;
        auto run = [&] {
            rgn::regions_host(cells.data(), has_labels ? labels.data() : nullptr, W, H, opts.min_component_cells, site.data(),
                              region.data(), ridge.data(), want_rd ? rd2.data() : nullptr, n);
            rgn::regions_host_points(g, site.data(), region.data(), want_rd ? rd2.data() : nullptr, nodes.data(), N,
                                     n_site.data(), n_region.data(), n_d2.data(), n_rd2.data());
            clr::to_metres(n_rd2.data(), n_rd2.size(), g.res, n_m.data());
        };
        run();
        fwrite(&n.n_occupied, 8, 1, fo); fwrite(&n.n_sites, 8, 1, fo); fwrite(&n.n_ridge, 8, 1, fo);
        fwrite(&n.n_components, 8, 1, fo); fwrite(&n.n_regions, 8, 1, fo); fwrite(&n.max_d2, 4, 1, fo);
        wr(fo, site); wr(fo, region); wr(fo, ridge); wr(fo, rd2);
        wr(fo, n_site); wr(fo, n_region); wr(fo, n_d2); wr(fo, n_rd2); wr(fo, n_m);
        if (reps > 0) {
            std::vector<double> ms;
            for (int r = 0; r < reps; ++r) {
                const auto t0 = std::chrono::steady_clock::now();
                run();
                ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            printf("ms %d %zu %.4f\n", (int)k, C, ms[ms.size() / 2]);
        }
    }
    fclose(fi);
    if (fclose(fo) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    printf("regions_host_main ok %d scenes\n", (int)count);
    return 0;
}
