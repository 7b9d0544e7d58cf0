// aos_path_linearize: aos_path_linearization_node's pathCallback + convertToLinearSegments
// (src/aos_path_linearization_node.cpp:372-395, 248-370), the /aos/path -> /plan step.
//
// What runs where:
//   findBestSplitPoint (:99-125)    GPU  k_lin_split: the node tries every interior pose of the range as a split
//                                        and runs two two-pass regressions per candidate, O(n^2) per search. The
//                                        candidates are independent, so one thread takes one candidate and runs
//                                        both regressions itself in index order (linearize.h's fit, the code the
//                                        host uses): a search is one serial pass of about 2 n steps. Each
//                                        workgroup reduces its candidates to the first minimum and stores the
//                                        pair into pinned host memory; the host takes the first strict minimum
//                                        over the workgroups in workgroup order.
//   everything else                 host linearize_host.cpp: the whole-range fits, the recursion, the breakpoints,
//                                        the interpolation (libm atan2 / cos / sin) and the forward pass
// The poses are read from global memory, not staged in LDS: a range may hold 65536 poses (1 MiB of positions,
// more than a CU's LDS), the first regression's loads are wave-uniform and the second's are consecutive across
// lanes, and one path serves every size.
#include <hip/hip_runtime.h>

#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "aos_ctx.h"
#include "linearize.h"

namespace aos {

constexpr int kLinThreads = 256;   // candidates per workgroup (tests/linearize_scenes.py WORKGROUP)

// (total, split) pairs order by value, then by index; a candidate whose total is not below DBL_MAX is
// (inf, INT_MAX) and loses to every other
__device__ __forceinline__ bool lin_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// Candidate c of the search over [s, e] is the split s + 1 + c, c in [0, e - s - 1). Workgroup g stores the first
// minimum of its candidates into best_total[g], best_split[g] (pinned host memory).
__global__ void __launch_bounds__(kLinThreads) k_lin_split(const double2 *xy, int s, int e, double *best_total,
                                                           int *best_split) {
    __shared__ double sd[kLinThreads];
    __shared__ int si[kLinThreads];
    const int c = blockIdx.x * kLinThreads + threadIdx.x;
    double total = INFINITY;
    int split = INT_MAX;
    if (c < e - s - 1) {
        const double t = lin::split_total<2>(reinterpret_cast<const double *>(xy), s, e, s + 1 + c);
        if (t < lin::kDblMax) { total = t; split = s + 1 + c; }
    }
    sd[threadIdx.x] = total;
    si[threadIdx.x] = split;
    __syncthreads();
    for (int h = kLinThreads / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h && lin_less(sd[threadIdx.x + h], si[threadIdx.x + h], sd[threadIdx.x], si[threadIdx.x])) {
            sd[threadIdx.x] = sd[threadIdx.x + h];
            si[threadIdx.x] = si[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { best_total[blockIdx.x] = sd[0]; best_split[blockIdx.x] = si[0]; }
}

struct LinState {
    DevBuf d_xy;
    PinnedBuf h_xy, h_best;
    lin::Result res;
};

namespace {

// findBestSplitPoint over [s, e] of the n uploaded poses, e > s + 1: one launch and one host wait
int gpu_search(LinState &S, int n, int s, int e, hipStream_t stream) {
    if (s < 0 || e >= n || e <= s + 1) throw std::runtime_error("aos_path_linearize: search range out of bounds");
    const int ncand = e - s - 1;
    const int groups = (ncand + kLinThreads - 1) / kLinThreads;
    const size_t split_off = (sizeof(double) * (size_t)groups + 63) / 64 * 64;
    char *h = static_cast<char *>(S.h_best.ensure(split_off + sizeof(int) * (size_t)groups));
    double *h_total = reinterpret_cast<double *>(h);
    int *h_split = reinterpret_cast<int *>(h + split_off);
    k_lin_split<<<groups, kLinThreads, 0, stream>>>(S.d_xy.as<double2>(), s, e, h_total, h_split);
    AOS_HIP(hipGetLastError());
    AOS_HIP(hipStreamSynchronize(stream));
    int best = s + 1;
    double min_total = lin::kDblMax;
    for (int g = 0; g < groups; ++g)
        if (h_total[g] < min_total) { min_total = h_total[g]; best = h_split[g]; }
    return best;
}

}  // namespace

}  // namespace aos

using namespace aos;

extern "C" int aos_path_linearize(aos_ctx *c, const double *poses, int32_t n_poses, aos_linear_path_out *out) {
    if (!c || !out) return fail(AOS_E_INVALID, "aos_path_linearize: null argument");
    if (n_poses < 0) return fail(AOS_E_INVALID, "aos_path_linearize: negative pose count");
    if (!poses && n_poses > 0) return fail(AOS_E_INVALID, "aos_path_linearize: null poses behind a count above 0");
    if (n_poses > lin::kMaxPosesIn) return fail(AOS_E_INVALID, "aos_path_linearize: more than 65536 poses");
    return guarded("linearize", nullptr, [&]() -> int {
        const auto t0 = std::chrono::steady_clock::now();
        DeviceScope dev_scope(c->device);
        int n = n_poses;
        if (!poses) {   // the fused form: the last aos_path_plan's poses (its arrays are only read)
            if (!path_last_poses(c->path_state, &poses, &n))
                return fail(AOS_E_STATE, "aos_path_linearize: no aos_path_plan on this handle yet");
            if (n > lin::kMaxPosesIn) return fail(AOS_E_INVALID, "aos_path_linearize: more than 65536 poses");
        }
        LinState &S = c->lin_state.get<LinState>();
        bool uploaded = false;
        const lin::SplitSearch search = [&](int s, int e) {
            if (!uploaded) {   // the positions, once per call
                double2 *h = static_cast<double2 *>(S.h_xy.ensure(sizeof(double2) * (size_t)n));
                for (int i = 0; i < n; ++i) h[i] = make_double2(poses[4 * i], poses[4 * i + 1]);
                double2 *d = static_cast<double2 *>(S.d_xy.ensure(sizeof(double2) * (size_t)n));
                AOS_HIP(hipMemcpyAsync(d, h, sizeof(double2) * (size_t)n, hipMemcpyHostToDevice, c->stream));
                uploaded = true;
            }
            return gpu_search(S, n, s, e, c->stream);
        };
        lin::Result res;
        lin::linearize(poses, n, search, res);   // (throws before the last result is touched)
        S.res = std::move(res);
        std::memset(out, 0, sizeof(*out));
        out->published = S.res.published;
        out->long_distance = S.res.long_distance;
        out->n_breakpoints = (int32_t)S.res.breakpoints.size(); out->breakpoints = S.res.breakpoints.data();
        out->n_poses = (int32_t)(S.res.poses.size() / 4); out->poses = S.res.poses.data();
        out->n_split_searches = S.res.n_split_searches;
        out->ms_linearize = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return AOS_OK;
    });
}
