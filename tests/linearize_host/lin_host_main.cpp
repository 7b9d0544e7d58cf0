// Stand-alone driver of the product's host linearization (csrc/linearize_host.cpp) with the host split search:
//   lin_host_main IN OUT [REPS]
// IN:  int32 scene count, then per scene int32 n and n x 4 doubles (x, y, qz, qw).
// OUT: per scene int32 status (0, or -1 where the library returns AOS_E_INVALID), published, long_distance,
//      n_split_searches, n_breakpoints, n_poses, then the breakpoints (int32) and the poses (4 doubles each).
// REPS > 0: each scene is also run REPS times and "ms <scene> <n> <median ms>" is printed per scene (the bench
// tool's host column). Built by test_linearize_cpu.py with ASan + UBSan; no GPU, no HIP.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "linearize.h"

using namespace aos::lin;

static void run(const std::vector<double> &poses, int n, Result &R) {
    const double *p = poses.data();
    linearize(p, n, [p](int s, int e) { return host_search(p, s, e); }, R);
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: lin_host_main IN OUT [REPS]\n"); return 2; }
    const int reps = argc > 3 ? atoi(argv[3]) : 0;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open files\n"); return 2; }
    int32_t count = 0;
    if (fread(&count, sizeof(count), 1, fi) != 1 || count < 0) { fprintf(stderr, "short input\n"); return 2; }
    for (int32_t k = 0; k < count; ++k) {
        int32_t n = 0;
        if (fread(&n, sizeof(n), 1, fi) != 1 || n < 0) { fprintf(stderr, "short input\n"); return 2; }
        std::vector<double> poses(4 * (size_t)n);
        if (n && fread(poses.data(), sizeof(double), poses.size(), fi) != poses.size()) { fprintf(stderr, "short input\n"); return 2; }
        Result R;
        int32_t status = 0;
        try {
            run(poses, n, R);
        } catch (const std::invalid_argument &) {
            status = -1;
            R = Result{};
        }
        const int32_t head[6] = {status, R.published, R.long_distance, R.n_split_searches, (int32_t)R.breakpoints.size(),
                                 (int32_t)(R.poses.size() / 4)};
        fwrite(head, sizeof(int32_t), 6, fo);
        if (!R.breakpoints.empty()) fwrite(R.breakpoints.data(), sizeof(int32_t), R.breakpoints.size(), fo);
        if (!R.poses.empty()) fwrite(R.poses.data(), sizeof(double), R.poses.size(), fo);
        if (reps > 0 && status == 0) {
            std::vector<double> ms;
            for (int r = 0; r < reps; ++r) {
                Result T;
                const auto t0 = std::chrono::steady_clock::now();
                run(poses, n, T);
                ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            printf("ms %d %d %.4f\n", (int)k, (int)n, ms[ms.size() / 2]);
        }
    }
    fclose(fi);
    if (fclose(fo) != 0) { fprintf(stderr, "write failed\n"); return 2; }
    printf("lin_host_main ok %d scenes\n", (int)count);
    return 0;
}
