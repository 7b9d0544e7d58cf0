"""aos_path_linearization_node's pathCallback + convertToLinearSegments (src/aos_path_linearization_node.cpp:372-395,
248-370) restated in Python floats: the checker of aos_path_linearize. Every sum runs in index order with each
product rounded on its own, as the node's unoptimised doubles do; atan2 / sin / cos are the C library's, which
the product's host code calls too. search_numpy is a second statement of the split search, vectorised over the
candidates: step k of every candidate's loop at once, element-wise adds only.
"""
import math

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
SPACING = 0.05
MAX_POSES_IN = 65536
MAX_SEGMENT = float(2 ** 22) * SPACING   # floor(distance / 0.05) stays far inside int
MAX_POSES_OUT = float(2 ** 22)


def fit(xy, s, e):
    """linearRegression (:50-96) over poses [s, e] -> (slope, intercept, error)."""
    if e <= s or e - s < 2:
        return 0.0, 0.0, 0.0
    n = e - s + 1
    sx = sy = sxy = sx2 = 0.0
    for i in range(s, e + 1):
        x, y = xy[i]
        sx += x
        sy += y
        sxy += x * y
        sx2 += x * x
    den = n * sx2 - sx * sx
    if abs(den) < 1e-9:
        slope, icpt = 0.0, sy / n
    else:
        slope = (n * sxy - sx * sy) / den
        icpt = (sy - slope * sx) / n
    tot = 0.0
    for i in range(s, e + 1):
        x, y = xy[i]
        err = y - (slope * x + icpt)
        tot += err * err
    return slope, icpt, tot / n


def candidate_totals(xy, s, e):
    """The weighted error of every split in (s, e), in split order (:109-116)."""
    out = []
    for split in range(s + 1, e):
        e1, e2 = fit(xy, s, split)[2], fit(xy, split, e)[2]
        n1, n2 = split - s + 1, e - split + 1
        out.append((e1 * n1 + e2 * n2) / (n1 + n2))
    return out


def pick(totals, s):
    """The first strictly smallest total below DBL_MAX (:105-122); s + 1 if there is none."""
    best, m = s + 1, DBL_MAX
    for k, t in enumerate(totals):
        if t < m:
            m, best = t, s + 1 + k
    return best


def search(xy, s, e):
    """findBestSplitPoint (:99-125)."""
    if e <= s + 1:
        return e
    return pick(candidate_totals(xy, s, e), s)


def _fit_errors_numpy(x, y, first, count, steps):
    """The error of one regression per candidate: candidate c fits `count[c]` poses from index first[c]."""
    nc = len(first)
    sx, sy, sxy, sx2 = (np.zeros(nc) for _ in range(4))
    last = len(x) - 1
    for k in range(steps):
        on = k < count
        idx = np.minimum(first + k, last)
        xk, yk = x[idx], y[idx]
        sx = np.where(on, sx + xk, sx)
        sy = np.where(on, sy + yk, sy)
        sxy = np.where(on, sxy + xk * yk, sxy)
        sx2 = np.where(on, sx2 + xk * xk, sx2)
    n = count.astype(np.float64)
    den = n * sx2 - sx * sx
    flat = np.abs(den) < 1e-9
    with np.errstate(all="ignore"):
        slope = np.where(flat, 0.0, (n * sxy - sx * sy) / den)
        icpt = np.where(flat, sy / n, (sy - slope * sx) / n)
        tot = np.zeros(nc)
        for k in range(steps):
            on = k < count
            idx = np.minimum(first + k, last)
            err = y[idx] - (slope * x[idx] + icpt)
            tot = np.where(on, tot + err * err, tot)
        return np.where(count < 3, 0.0, tot / n)


def candidate_totals_numpy(xy, s, e):
    a = np.asarray(xy, np.float64).reshape(-1, 2)
    x, y = np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])
    split = np.arange(s + 1, e)
    n1, n2 = split - s + 1, e - split + 1
    with np.errstate(all="ignore"):
        e1 = _fit_errors_numpy(x, y, np.full(len(split), s), n1, e - s)
        e2 = _fit_errors_numpy(x, y, split, n2, e - s)
        return (e1 * n1 + e2 * n2) / (n1 + n2).astype(np.float64)


def search_numpy(xy, s, e):
    if e <= s + 1:
        return e
    return pick(candidate_totals_numpy(xy, s, e).tolist(), s)


def _interpolate(p1, p2, out, skip_start):
    """interpolateSegment (:190-245); poses are (x, y, qz, qw)."""
    dx, dy = p2[0] - p1[0], p2[1] - p1[1]
    dist = math.sqrt(dx * dx + dy * dy)
    if dist < 1e-6:
        if not skip_start:
            out.append(tuple(p1))
        return
    yaw = math.atan2(dy, dx)
    qw, qz = math.cos(yaw / 2.0), math.sin(yaw / 2.0)
    num = int(math.floor(dist / SPACING))
    if not skip_start:
        out.append((p1[0], p1[1], qz, qw))
    for i in range(1, num + 1):
        t = float(i) * SPACING / dist
        if t >= 1.0:
            break
        out.append((p1[0] + t * dx, p1[1] + t * dy, qz, qw))
    out.append((p2[0], p2[1], qz, qw))


def _check_segments(poses, idx):
    """The limits that keep static_cast<int>(floor(distance / 0.05)) defined (:212), in double."""
    bound = 1.0
    for a, b in zip(idx[:-1], idx[1:]):
        dx, dy = poses[b][0] - poses[a][0], poses[b][1] - poses[a][1]
        with np.errstate(all="ignore"):
            dist = float(np.sqrt(np.float64(dx) * dx + np.float64(dy) * dy))
        if not dist <= MAX_SEGMENT:
            raise ValueError("segment too long")
        bound += math.floor(dist / SPACING) + 1.0
    if bound > MAX_POSES_OUT:
        raise ValueError("output too long")


def linearize(poses, search_fn=search):
    """-> dict(published, long_distance, breakpoints, poses (m x 4), n_split_searches, searches [(s, e, split)]).
    ValueError where aos_path_linearize returns AOS_E_INVALID."""
    P = [tuple(float(v) for v in p) for p in np.asarray(poses, np.float64).reshape(-1, 4)]
    n = len(P)
    if n > MAX_POSES_IN:
        raise ValueError("too many poses")
    if any(not (math.isfinite(p[0]) and math.isfinite(p[1])) for p in P):
        raise ValueError("non-finite position")
    res = {"published": int(n > 0), "long_distance": 0, "breakpoints": np.zeros(0, np.int32),
           "poses": np.zeros((0, 4)), "n_split_searches": 0, "searches": []}
    if n == 0:
        return res
    res["long_distance"] = int(abs(P[-1][0]) < 1e-6 and abs(P[-1][1]) < 1e-6)
    max_segments = 10 if res["long_distance"] else 4
    out = []
    if n == 1:
        out = [P[0]]
        bps = []
    elif n <= 4:
        bps = list(range(n))
        _check_segments(P, bps)
        for i in range(n - 1):
            _interpolate(P[i], P[i + 1], out, i > 0)
        if out:
            out[0], out[-1] = P[0], P[-1]
    else:
        xy = [(p[0], p[1]) for p in P]
        bps = []

        def rec(s, e):   # splitPathRecursive (:128-177)
            if e <= s:
                return
            slope, icpt, _ = fit(xy, s, e)
            worst = 0.0
            for i in range(s + 1, e):
                d = abs(xy[i][1] - (slope * xy[i][0] + icpt))
                if d > worst:
                    worst = d
            if worst < 0.1 or len(bps) >= max_segments - 1:
                return
            split = search_fn(xy, s, e)
            res["searches"].append((s, e, split))
            if split not in bps:
                bps.append(split)
                bps.sort()
            if len(bps) < max_segments - 1:
                rec(s, split)
                rec(split, e)

        rec(0, n - 1)
        bps = sorted(set(bps + [0, n - 1]))
        _check_segments(P, bps)
        for i in range(len(bps) - 1):
            _interpolate(P[bps[i]], P[bps[i + 1]], out, i > 0)
        if out:
            out[0], out[-1] = P[0], P[-1]
        if len(out) > 2:   # the forward-direction pass (:335-369)
            kept = [out[0]]
            for i in range(1, len(out)):
                if i > 1:
                    a, b, c = kept[-2], kept[-1], out[i]
                    if (b[0] - a[0]) * (c[0] - b[0]) + (b[1] - a[1]) * (c[1] - b[1]) < -0.01:
                        continue
                kept.append(out[i])
            kept[-1] = P[-1]
            out = kept
    res["breakpoints"] = np.array(bps, np.int32)
    res["poses"] = np.array(out, np.float64).reshape(-1, 4)
    res["n_split_searches"] = len(res["searches"])
    return res
