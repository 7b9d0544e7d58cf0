// Host half of aos_path_linearize (linearize.h): everything of aos_path_linearization_node's
// convertToLinearSegments (src/aos_path_linearization_node.cpp:248-370) except the split search, which the caller
// hands in. Doubles in the node's operand order; built without FMA contraction.
#include "linearize.h"

#include <algorithm>
#include <stdexcept>

namespace aos {
namespace lin {

namespace {

struct Pose { double x, y, qz, qw; };

// The reference is built without optimisation, so cos and sin of the half yaw are separate libm calls; an
// optimising compiler fuses them into one sincos, whose results can differ by an ulp (as in path.hip).
__attribute__((noinline)) double half_sin(double yaw) { return std::sin(yaw / 2.0); }
__attribute__((noinline)) double half_cos(double yaw) { return std::cos(yaw / 2.0); }

Pose pose_at(const double *poses, int i) { return {poses[4 * i], poses[4 * i + 1], poses[4 * i + 2], poses[4 * i + 3]}; }

double segment_length(const Pose &a, const Pose &b) {   // (:195-198, dz = 0)
    const double dx = b.x - a.x, dy = b.y - a.y;
    return std::sqrt(dx * dx + dy * dy);
}

// The limits that keep interpolateSegment's static_cast<int>(floor(distance / spacing)) (:212) defined, for the
// segments between the consecutive poses idx names; `bound` counts at least the poses they produce.
void check_segments(const double *poses, const std::vector<int32_t> &idx) {
    double bound = 1.0;
    for (size_t i = 0; i + 1 < idx.size(); ++i) {
        const double d = segment_length(pose_at(poses, idx[i]), pose_at(poses, idx[i + 1]));
        if (!(d <= kMaxSegment)) throw std::invalid_argument("aos_path_linearize: a segment is longer than 2^22 x 0.05 m");
        bound += std::floor(d / kSpacing) + 1.0;
    }
    if (bound > kMaxPosesOut) throw std::invalid_argument("aos_path_linearize: the output would exceed 2^22 poses");
}

void interpolate(const Pose &p1, const Pose &p2, std::vector<Pose> &out, bool skip_start) {   // :190-245
    const double dx = p2.x - p1.x, dy = p2.y - p1.y;
    const double distance = std::sqrt(dx * dx + dy * dy);
    if (distance < 1e-6) {
        if (!skip_start) out.push_back(p1);
        return;
    }
    const double yaw = std::atan2(dy, dx);
    const int num_intermediate = static_cast<int>(std::floor(distance / kSpacing));
    const double qw = half_cos(yaw), qz = half_sin(yaw);
    if (!skip_start) out.push_back({p1.x, p1.y, qz, qw});
    for (int i = 1; i <= num_intermediate; i++) {
        const double t = static_cast<double>(i) * kSpacing / distance;
        if (t >= 1.0) break;
        out.push_back({p1.x + t * dx, p1.y + t * dy, qz, qw});
    }
    out.push_back({p2.x, p2.y, qz, qw});
}

struct Splitter {   // splitPathRecursive (:128-177)
    const double *poses;
    const SplitSearch &search;
    int max_segments;
    std::vector<int32_t> bps;
    int n_searches = 0;

    void run(int s, int e) {
        if (e <= s || max_segments <= 1) return;
        const Fit f = fit<4>(poses, s, e);
        double max_distance = 0.0;
        for (int i = s + 1; i < e; ++i) {
            const double predicted = f.slope * poses[4 * i] + f.intercept;
            const double distance = std::fabs(poses[4 * i + 1] - predicted);
            if (distance > max_distance) max_distance = distance;
        }
        if (max_distance < 0.1 || (int)bps.size() >= max_segments - 1) return;
        // (e > s + 1 here: a range without interior poses has max_distance 0)
        const int best = search(s, e);
        n_searches++;
        if (std::find(bps.begin(), bps.end(), best) == bps.end()) {
            bps.push_back(best);
            std::sort(bps.begin(), bps.end());
        }
        if ((int)bps.size() < max_segments - 1) {
            run(s, best);
            run(best, e);
        }
    }
};

}  // namespace

int host_search(const double *poses, int s, int e) {   // findBestSplitPoint (:99-125)
    if (e <= s + 1) return e;
    int best = s + 1;
    double min_total = kDblMax;
    for (int split = s + 1; split < e; ++split) {
        const double total = split_total<4>(poses, s, e, split);
        if (total < min_total) { min_total = total; best = split; }
    }
    return best;
}

void linearize(const double *poses, int n, const SplitSearch &search, Result &R) {
    R = Result{};
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(poses[4 * i]) || !std::isfinite(poses[4 * i + 1]))
            throw std::invalid_argument("aos_path_linearize: non-finite pose position");
    if (n <= 0) return;   // pathCallback returns (:373-375)
    R.published = 1;
    const Pose first = pose_at(poses, 0), last = pose_at(poses, n - 1);
    R.long_distance = std::fabs(last.x) < 1e-6 && std::fabs(last.y) < 1e-6;
    std::vector<Pose> out;
    if (n == 1) {
        out.push_back(first);
    } else if (n <= 4) {   // no regression: consecutive poses (:270-293)
        for (int i = 0; i < n; ++i) R.breakpoints.push_back(i);
        check_segments(poses, R.breakpoints);
        for (int i = 0; i + 1 < n; ++i) interpolate(pose_at(poses, i), pose_at(poses, i + 1), out, i > 0);
        if (!out.empty()) { out[0] = first; out.back() = last; }
    } else {
        Splitter sp{poses, search, R.long_distance ? 10 : 4, {}};
        sp.run(0, n - 1);
        R.n_split_searches = sp.n_searches;
        std::vector<int32_t> &b = sp.bps;
        if (b.empty() || b[0] != 0) b.insert(b.begin(), 0);
        if (b.back() != n - 1) b.push_back(n - 1);
        std::sort(b.begin(), b.end());
        b.erase(std::unique(b.begin(), b.end()), b.end());
        R.breakpoints = b;
        check_segments(poses, b);
        for (size_t i = 0; i + 1 < b.size(); ++i) interpolate(pose_at(poses, b[i]), pose_at(poses, b[i + 1]), out, i > 0);
        if (!out.empty()) { out[0] = first; out.back() = last; }
        if (out.size() > 2) {   // the forward-direction pass (:335-369)
            std::vector<Pose> ordered;
            ordered.push_back(out[0]);
            for (size_t i = 1; i < out.size(); ++i) {
                if (i > 1) {
                    const Pose &pp = ordered[ordered.size() - 2], &pv = ordered.back(), &cur = out[i];
                    const double dx1 = pv.x - pp.x, dy1 = pv.y - pp.y;
                    const double dx2 = cur.x - pv.x, dy2 = cur.y - pv.y;
                    const double dot = dx1 * dx2 + dy1 * dy2;
                    if (dot < -0.01) continue;
                }
                ordered.push_back(out[i]);
            }
            ordered.back() = last;
            out.swap(ordered);
        }
    }
    R.poses.reserve(4 * out.size());
    for (const Pose &p : out) { R.poses.push_back(p.x); R.poses.push_back(p.y); R.poses.push_back(p.qz); R.poses.push_back(p.qw); }
}

}  // namespace lin
}  // namespace aos
