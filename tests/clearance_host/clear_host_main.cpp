// Stand-alone driver of the product's host clearance code (csrc/clearance_host.cpp with csrc/clearance.h):
//   clear_host_main IN OUT [REPS]
// IN:  int32 scene count, then per scene int32 W, H, N, E, double origin_x, origin_y, float resolution, W * H int8
//      cells, N x 2 doubles (nodes), E x 2 int32 (edges).
// OUT: per scene int32 status (0, or -1 where the library returns AOS_E_INVALID: nothing more follows for it), uint64
//      n_occupied, uint32 max_d2, then W * H uint32 (the field), N + E uint32 (node_d2, edge_d2), N + E floats (metres).
// REPS > 0: each scene is also run REPS times and "ms <scene> <cells> <median field ms> <median graph ms>" is printed
// (the bench tool's host column). Built by test_clearance_cpu.py with ASan + UBSan; no GPU, no HIP.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "clearance.h"

using namespace aos::clr;

static bool rd(FILE *f, void *p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: clear_host_main IN OUT [REPS]\n"); return 2; }
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    int32_t count = 0;
    if (!rd(fi, &count, sizeof(count)) || count < 0) { fprintf(stderr, "short input\n"); return 2; }
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[4];
        double org[2];
        float resolution;
        if (!rd(fi, head, sizeof(head)) || !rd(fi, org, sizeof(org)) || !rd(fi, &resolution, sizeof(resolution)) ||
            head[0] < 0 || head[1] < 0 || head[2] < 0 || head[3] < 0) { fprintf(stderr, "short input\n"); return 2; }
        const int32_t W = head[0], H = head[1], N = head[2], E = head[3];
        const size_t C = (size_t)W * (size_t)H;
        std::vector<int8_t> cells(C);
        std::vector<double> nodes(2 * (size_t)N);
        std::vector<int32_t> edges(2 * (size_t)E);
        if (!rd(fi, cells.data(), C) || !rd(fi, nodes.data(), sizeof(double) * nodes.size()) ||
            !rd(fi, edges.data(), sizeof(int32_t) * edges.size())) { fprintf(stderr, "short input\n"); return 2; }
        aos_grid_info info{org[0], org[1], resolution, (uint32_t)W, (uint32_t)H};
        int32_t status = 0;
        if (check_info(info) || check_graph(N ? nodes.data() : nullptr, N, E ? edges.data() : nullptr, E)) status = -1;
        fwrite(&status, sizeof(status), 1, fo);
        if (status) continue;
        const Grid g{info.origin_x, info.origin_y, (double)info.resolution, W, H};
        std::vector<uint32_t> d2(C), nd(N), ed(E);
        std::vector<float> nm(N), em(E);
        uint32_t max_d2 = 0;
        const uint64_t n_occ = clear_host_field(cells.data(), W, H, d2.data(), &max_d2);
        clear_host_graph(g, d2.data(), nodes.data(), N, edges.data(), E, nd.data(), ed.data());
        to_metres(nd.data(), nd.size(), g.res, nm.data());
        to_metres(ed.data(), ed.size(), g.res, em.data());
        fwrite(&n_occ, sizeof(n_occ), 1, fo);
        fwrite(&max_d2, sizeof(max_d2), 1, fo);
        if (C) fwrite(d2.data(), sizeof(uint32_t), C, fo);
        if (N) fwrite(nd.data(), sizeof(uint32_t), N, fo);
        if (E) fwrite(ed.data(), sizeof(uint32_t), E, fo);
        if (N) fwrite(nm.data(), sizeof(float), N, fo);
        if (E) fwrite(em.data(), sizeof(float), E, fo);
        if (reps > 0) {
            std::vector<double> msf, msg;
            for (int r = 0; r < reps; ++r) {
                const auto t0 = std::chrono::steady_clock::now();
                clear_host_field(cells.data(), W, H, d2.data(), &max_d2);
                const auto t1 = std::chrono::steady_clock::now();
                clear_host_graph(g, d2.data(), nodes.data(), N, edges.data(), E, nd.data(), ed.data());
                to_metres(nd.data(), nd.size(), g.res, nm.data());
                to_metres(ed.data(), ed.size(), g.res, em.data());
                const auto t2 = std::chrono::steady_clock::now();
                msf.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
                msg.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count());
            }
            std::sort(msf.begin(), msf.end());
            std::sort(msg.begin(), msg.end());
            printf("ms %d %zu %.4f %.4f\n", (int)k, C, msf[msf.size() / 2], msg[msg.size() / 2]);
        }
    }
    fclose(fi);
    if (fclose(fo) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    printf("clear_host_main ok %d scenes\n", (int)count);
    return 0;
}
