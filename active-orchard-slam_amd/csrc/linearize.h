// aos_path_linearization_node's convertToLinearSegments (src/aos_path_linearization_node.cpp:248-370) without its
// split search: the regression, the recursion, the breakpoints, the 5 cm interpolation and the forward pass, in
// plain C++ (no HIP types; linearize_host.cpp). The search is a callable, so the library hands in the GPU search
// (linearize.hip) and the tests' stand-alone program the host one. Not part of the ABI.
#pragma once
#include <cmath>
#include <cstdint>
#include <functional>
#include <vector>

#ifdef __HIP__
#define AOS_LIN_HD __host__ __device__ inline
#else
#define AOS_LIN_HD inline
#endif

namespace aos {
namespace lin {

constexpr int kMaxPosesIn = 65536;
constexpr double kSpacing = 0.05;
constexpr double kMaxSegment = 4194304.0 * kSpacing;   // 2^22 intermediates: floor(distance / 0.05) stays inside int
constexpr double kMaxPosesOut = 4194304.0;
constexpr double kDblMax = 1.7976931348623157e308;

struct Fit { double slope, intercept, error; };

// linearRegression (:50-96) over poses [s, e] of an array with `Stride` doubles per pose (x, y first): four running
// sums in index order, every product rounded on its own (the files that include this are built without FMA
// contraction), then the mean squared error in a second pass.
template <int Stride>
AOS_LIN_HD Fit fit(const double *p, int s, int e) {
    Fit r{0.0, 0.0, 0.0};
    if (e <= s || e - s < 2) return r;
    const double n = (double)(e - s + 1);
    double sum_x = 0.0, sum_y = 0.0, sum_xy = 0.0, sum_x2 = 0.0;
    for (int i = s; i <= e; ++i) {
        const double x = p[(size_t)i * Stride], y = p[(size_t)i * Stride + 1];
        sum_x += x;
        sum_y += y;
        sum_xy += x * y;
        sum_x2 += x * x;
    }
    const double den = n * sum_x2 - sum_x * sum_x;
    if (fabs(den) < 1e-9) {
        r.slope = 0.0;
        r.intercept = sum_y / n;
    } else {
        r.slope = (n * sum_xy - sum_x * sum_y) / den;
        r.intercept = (sum_y - r.slope * sum_x) / n;
    }
    double total = 0.0;
    for (int i = s; i <= e; ++i) {
        const double x = p[(size_t)i * Stride], y = p[(size_t)i * Stride + 1];
        const double predicted = r.slope * x + r.intercept;
        const double err = y - predicted;
        total += err * err;
    }
    r.error = total / n;
    return r;
}

// The weighted error of splitting [s, e] at `split` (findBestSplitPoint's loop body, :110-116).
template <int Stride>
AOS_LIN_HD double split_total(const double *p, int s, int e, int split) {
    const Fit f1 = fit<Stride>(p, s, split);
    const Fit f2 = fit<Stride>(p, split, e);
    const int n1 = split - s + 1, n2 = e - split + 1;
    return (f1.error * (double)n1 + f2.error * (double)n2) / (double)(n1 + n2);
}

// (start, end) -> split: findBestSplitPoint over the poses handed to linearize(), end > start + 1
using SplitSearch = std::function<int(int, int)>;

struct Result {
    int published = 0, long_distance = 0, n_split_searches = 0;
    std::vector<int32_t> breakpoints;
    std::vector<double> poses;   // x, y, qz, qw
};

// The node's own search (:99-125) on the host: the tests' stand-alone program and the bench tool's yardstick.
int host_search(const double *poses, int s, int e);

// pathCallback + convertToLinearSegments on n poses (x, y, qz, qw). Throws std::invalid_argument for a non-finite
// position, a segment longer than kMaxSegment or an output above kMaxPosesOut (checked in double before the
// node's cast to int and before the output grows).
void linearize(const double *poses, int n, const SplitSearch &search, Result &out);

}  // namespace lin
}  // namespace aos
