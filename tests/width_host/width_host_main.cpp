// Stand-alone driver of the product's host width code (csrc/width_host.cpp with csrc/width.h and
// csrc/clearance_host.cpp):
//   width_host_main IN OUT [REPS]
// IN:  int32 scene count, then per scene int32 W, H, N, S, K, double origin_x, origin_y, float resolution, W * H int8
//      cells, N x 2 doubles (nodes), S x 2 doubles (sources), K x 2 doubles (points).
// OUT: per scene int32 status (0, or -1 where the library returns AOS_E_INVALID: nothing more follows for it), uint64
//      n_free, n_reached, int32 n_sources_used, uint32 min_width, max_width, W * H uint32 (the field), N uint32
//      (node_width), N floats (node_radius_m), K uint32 and K floats (the points' width and radius_m).
// REPS > 0: each scene's field is also computed REPS times and "ms <scene> <cells> <median ms>" is printed (the bench
// tool's host column). Built by test_width_cpu.py with ASan + UBSan; no GPU, no HIP.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "width.h"

using namespace aos;

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: width_host_main IN OUT [REPS]\n"); return 2; }
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    int32_t count = 0;
    if (!rd(fi, &count, sizeof(count)) || count < 0) { fprintf(stderr, "short input\n"); return 2; }
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[5];
        double org[2];
        float resolution;
        if (!rd(fi, head, sizeof(head)) || !rd(fi, org, sizeof(org)) || !rd(fi, &resolution, sizeof(resolution)) ||
            head[0] < 0 || head[1] < 0 || head[2] < 0 || head[3] < 0 || head[4] < 0) {
            fprintf(stderr, "short input\n");
            return 2;
        }
        const int32_t W = head[0], H = head[1], N = head[2], S = head[3], K = head[4];
        const size_t C = (size_t)W * (size_t)H;
        std::vector<int8_t> cells(C);
        std::vector<double> nodes(2 * (size_t)N), src(2 * (size_t)S), pts(2 * (size_t)K);
        if (!rd(fi, cells.data(), C) || !rd(fi, nodes.data(), sizeof(double) * nodes.size()) ||
            !rd(fi, src.data(), sizeof(double) * src.size()) || !rd(fi, pts.data(), sizeof(double) * pts.size())) {
            fprintf(stderr, "short input\n");
            return 2;
        }
        aos_grid_info info{org[0], org[1], resolution, (uint32_t)W, (uint32_t)H};
        int32_t status = 0;
        if (clr::check_info(info) || clr::check_graph(N ? nodes.data() : nullptr, N, nullptr, 0) ||
            wd::check_width(S ? src.data() : nullptr, S))
            status = -1;
        fwrite(&status, sizeof(status), 1, fo);
        if (status) continue;
        const clr::Grid g{info.origin_x, info.origin_y, (double)info.resolution, W, H};
        std::vector<uint32_t> width(C), nw(N), pw(K);
        std::vector<float> nr(N), pr(K);
        wd::Counts n;
        wd::width_host(cells.data(), g, src.data(), S, width.data(), n);
        if (C) {
            wd::width_host_points(g, width.data(), nodes.data(), N, nw.data());
            wd::width_host_points(g, width.data(), pts.data(), K, pw.data());
        } else {
            std::fill(nw.begin(), nw.end(), wd::kNone);
            std::fill(pw.begin(), pw.end(), wd::kNone);
        }
        wd::to_radius(nw.data(), nw.size(), g.res, nr.data());
        wd::to_radius(pw.data(), pw.size(), g.res, pr.data());
        fwrite(&n.n_free, sizeof(uint64_t), 1, fo);
        fwrite(&n.n_reached, sizeof(uint64_t), 1, fo);
        fwrite(&n.n_sources_used, sizeof(int32_t), 1, fo);
        fwrite(&n.min_width, sizeof(uint32_t), 1, fo);
        fwrite(&n.max_width, sizeof(uint32_t), 1, fo);
        if (C) fwrite(width.data(), sizeof(uint32_t), C, fo);
        if (N) fwrite(nw.data(), sizeof(uint32_t), N, fo);
        if (N) fwrite(nr.data(), sizeof(float), N, fo);
        if (K) fwrite(pw.data(), sizeof(uint32_t), K, fo);
        if (K) fwrite(pr.data(), sizeof(float), K, fo);
        if (reps > 0) {
            std::vector<double> ms;
            for (int r = 0; r < reps; ++r) {
                const auto t0 = std::chrono::steady_clock::now();
                wd::width_host(cells.data(), g, src.data(), S, width.data(), n);
                const auto t1 = std::chrono::steady_clock::now();
                ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            printf("ms %d %zu %.4f\n", (int)k, C, ms[ms.size() / 2]);
        }
    }
    fclose(fi);
    if (fclose(fo) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    printf("width_host_main ok %d scenes\n", (int)count);
    return 0;
}
