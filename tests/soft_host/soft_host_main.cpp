// Stand-alone driver of the product's host soft code (csrc/soft_host.cpp with csrc/soft.h and
// csrc/clearance_host.cpp):
//   soft_host_main IN OUT [REPS]
// IN:  int32 scene count, then per scene int32 W, H, N, S, K, uint32 min_d2, int32 soft_cells, gain, double origin_x,
//      origin_y, float resolution, W * H int8 cells, N x 2 doubles (nodes), S x 2 doubles (sources), K x 2 doubles
//      (descent starts).
// OUT: per scene int32 status (0, or -1 where the library returns AOS_E_INVALID, the 2^31 bound included: nothing more
//      follows for it), uint64 n_passable, n_reached, n_soft, int32 n_sources_used, uint32 max_cost, max_weight, W * H
//      uint32 (the field), N uint32 (node_cost), then per start uint64 length, uint32 plain_cost, length uint32 (cells),
//      length x 2 doubles (centres).
// REPS > 0: each scene's field is also computed REPS times and "ms <scene> <cells> <median ms>" is printed (the bench
// tool's host column). Built by test_soft_cpu.py with ASan + UBSan; no GPU, no HIP.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "soft.h"

using namespace aos;

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: soft_host_main IN OUT [REPS]\n"); return 2; }
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    int32_t count = 0;
    if (!rd(fi, &count, sizeof(count)) || count < 0) { fprintf(stderr, "short input\n"); return 2; }
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[5], soft[2];
        uint32_t min_d2;
        double org[2];
        float resolution;
        if (!rd(fi, head, sizeof(head)) || !rd(fi, &min_d2, sizeof(min_d2)) || !rd(fi, soft, sizeof(soft)) ||
            !rd(fi, org, sizeof(org)) || !rd(fi, &resolution, sizeof(resolution)) || head[0] < 0 || head[1] < 0 ||
            head[2] < 0 || head[3] < 0 || head[4] < 0) { fprintf(stderr, "short input\n"); return 2; }
        const int32_t W = head[0], H = head[1], N = head[2], S = head[3], K = head[4];
        const size_t C = (size_t)W * (size_t)H;
        std::vector<int8_t> cells(C);
        std::vector<double> nodes(2 * (size_t)N), src(2 * (size_t)S), starts(2 * (size_t)K);
        if (!rd(fi, cells.data(), C) || !rd(fi, nodes.data(), sizeof(double) * nodes.size()) ||
            !rd(fi, src.data(), sizeof(double) * src.size()) || !rd(fi, starts.data(), sizeof(double) * starts.size())) {
            fprintf(stderr, "short input\n");
            return 2;
        }
        aos_grid_info info{org[0], org[1], resolution, (uint32_t)W, (uint32_t)H};
        int32_t status = 0;
        if (clr::check_info(info) || clr::check_graph(N ? nodes.data() : nullptr, N, nullptr, 0) ||
            sft::check_soft(S ? src.data() : nullptr, S, soft[0], soft[1]))
            status = -1;
        const clr::Grid g{info.origin_x, info.origin_y, (double)info.resolution, W, H};
        std::vector<uint8_t> wt(status ? 0 : C);
        std::vector<uint32_t> cost(status ? 0 : C), nc(N);
        sft::Counts n;
        if (!status && !sft::soft_host(cells.data(), g, src.data(), S, min_d2, soft[0], soft[1], wt.data(), cost.data(), n)) {
            if (sft::check_bound(n.max_weight, n.n_passable).empty()) { fprintf(stderr, "refused without a message\n"); return 2; }
            status = -1;
        }
        fwrite(&status, sizeof(status), 1, fo);
        if (status) continue;
        if (C) sft::soft_host_points(g, cost.data(), nodes.data(), N, nc.data());
        else std::fill(nc.begin(), nc.end(), sft::kNone);
        fwrite(&n.n_passable, sizeof(uint64_t), 1, fo);
        fwrite(&n.n_reached, sizeof(uint64_t), 1, fo);
        fwrite(&n.n_soft, sizeof(uint64_t), 1, fo);
        fwrite(&n.n_sources_used, sizeof(int32_t), 1, fo);
        fwrite(&n.max_cost, sizeof(uint32_t), 1, fo);
        fwrite(&n.max_weight, sizeof(uint32_t), 1, fo);
        if (C) fwrite(cost.data(), sizeof(uint32_t), C, fo);
        if (N) fwrite(nc.data(), sizeof(uint32_t), N, fo);
        for (int32_t i = 0; i < K; ++i) {
            // the length first, with no room at all; then the cells into a buffer of exactly that length
            const uint64_t len = sft::soft_host_descend(g, wt.data(), cost.data(), starts[2 * i], starts[2 * i + 1], nullptr, 0);
            std::vector<uint32_t> path(len);
            std::vector<double> xy(2 * len);
            if (sft::soft_host_descend(g, wt.data(), cost.data(), starts[2 * i], starts[2 * i + 1], path.data(), len) != len) {
                fprintf(stderr, "descent lengths differ\n");
                return 2;
            }
            for (uint64_t j = 0; j < len; ++j) rch::cell_centre(g, path[j], xy[2 * j], xy[2 * j + 1]);
            const uint32_t plain = sft::plain_cost(path.data(), len, W);
            fwrite(&len, sizeof(len), 1, fo);
            fwrite(&plain, sizeof(plain), 1, fo);
            if (len) fwrite(path.data(), sizeof(uint32_t), len, fo);
            if (len) fwrite(xy.data(), sizeof(double), 2 * len, fo);
        }
        if (reps > 0) {
            std::vector<double> ms;
            for (int r = 0; r < reps; ++r) {
                const auto t0 = std::chrono::steady_clock::now();
                sft::soft_host(cells.data(), g, src.data(), S, min_d2, soft[0], soft[1], wt.data(), cost.data(), n);
                const auto t1 = std::chrono::steady_clock::now();
                ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            printf("ms %d %zu %.4f\n", (int)k, C, ms[ms.size() / 2]);
        }
    }
    fclose(fi);
    if (fclose(fo) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    printf("soft_host_main ok %d scenes\n", (int)count);
    return 0;
}
