"""Designed /aos/path inputs for aos_path_linearize (poses x, y, qz, qw), each built for one regime of the
linearization node: the n <= 4 paths without regression, the smallest regressed path, the 4- and 10-segment caps,
a search on a range that starts past pose 0, the |den| < 1e-9 branch, exact ties between neighbouring candidates
(at the workgroup and wave boundaries of the split kernel), and search sizes around the kernel's workgroup size.
test_linearize_cpu.py asserts each regime in the restatement (linearize_ref), so a scene that drifts out of its
regime fails there.
"""
import math

import numpy as np

WORKGROUP = 256   # k_lin_split's workgroup size (csrc/linearize.hip kLinThreads)


def with_yaw(xy, last=None):
    """Poses oriented along the next step, as aos_path_gen_node publishes them; the last one like its predecessor
    unless given."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = len(xy)
    out = np.zeros((n, 4))
    out[:, :2] = xy
    out[:, 3] = 1.0
    for i in range(n - 1):
        yaw = math.atan2(xy[i + 1, 1] - xy[i, 1], xy[i + 1, 0] - xy[i, 0])
        out[i, 2:] = math.sin(yaw / 2.0), math.cos(yaw / 2.0)
    if n > 1:
        out[-1, 2:] = out[-2, 2:] if last is None else (math.sin(last / 2.0), math.cos(last / 2.0))
    return out


def small():
    """n = 0 ... 4: a repeated pose, and orientations that differ from the segments' yaw."""
    q = lambda yaw: (math.sin(yaw / 2.0), math.cos(yaw / 2.0))   # noqa: E731
    return {
        "n0": np.zeros((0, 4)),
        "n1": np.array([[1.5, -2.0, *q(0.7)]]),
        "n2": np.array([[0.0, 0.0, *q(1.0)], [0.3, 0.4, *q(-2.0)]]),
        "n2_same": np.array([[2.0, 1.0, *q(0.3)], [2.0, 1.0, *q(0.9)]]),
        "n3": np.array([[0.0, 0.0, *q(0.2)], [0.12, 0.0, *q(0.4)], [0.12, 0.1, *q(3.0)]]),
        "n3_repeat": np.array([[1.0, 1.0, *q(0.5)], [1.0, 1.0, *q(0.6)], [1.0, 1.2, *q(-1.0)]]),
        "n4": np.array([[0.0, 0.0, *q(0.0)], [0.2, 0.0, *q(0.1)], [0.2, 0.0, *q(0.2)], [0.0, -0.07, *q(2.5)]]),
        "n4_origin": np.array([[1.0, 0.0, *q(3.0)], [0.5, 0.0, *q(3.1)], [0.2, 0.1, *q(3.0)], [0.0, 0.0, *q(1.0)]]),
    }


def five():
    return with_yaw([(0, 0), (1, .05), (2, 1), (3, .05), (4, .1)])


def straight9():
    return with_yaw([(0.2 * i, 1.0 + 0.1 * i) for i in range(9)])


def ell():
    return with_yaw([(0.2 * i, 0.0) for i in range(11)] + [(2.0, 0.2 * j) for j in range(1, 11)])


def zigzag_xy(legs=8, per_leg=10, step=0.2):
    d = step / math.sqrt(2.0)
    pts, y = [], 0.0
    for k in range(legs * per_leg):
        pts.append((d * k, y))
        y += d if (k // per_leg) % 2 == 0 else -d
    return np.array(pts)


def zigzag(n_legs=8, per_leg=10):
    return with_yaw(zigzag_xy(n_legs, per_leg))


def zigzag_ending_at(x, y, n_legs=8, per_leg=10):
    """zigzag shifted so that its last pose is exactly (x, y)."""
    xy = zigzag_xy(n_legs, per_leg)
    xy = xy - xy[-1]
    xy[-1] = (0.0, 0.0)
    xy = xy + np.array([x, y])
    xy[-1] = (x, y)
    return with_yaw(xy)


def home():
    return zigzag_ending_at(0.0, 0.0)


def vertical():
    return with_yaw([(3.0, 0.2 * i) for i in range(12)])


def hairpin(m, step, y0=0.0):
    """m poses along +x at y = y0, two poses up, then m poses back. The shape is its own mirror image with the pose
    order reversed, so splits m and m + 1 (the two poses of the turn) have the same error in exact arithmetic;
    at step 0.25 the coordinate sums are exact, and for the y0 of HAIRPIN_TIES the two rounded totals are
    equal too and the smallest of the search (asserted in test_linearize_cpu.py)."""
    pts = [(step * i, y0) for i in range(m)]
    pts += [(step * (m - 1), y0 + step), (step * (m - 1), y0 + 2 * step)]
    pts += [(step * (m - 1 - i), y0 + 3 * step) for i in range(m)]
    return with_yaw(pts)


# m -> y0 at which hairpin(m, 0.25, y0)'s full-range search ties exactly between splits m and m + 1: candidates
# m - 1 and m, the last thread of one 256-thread workgroup and the first of the next (m = 256), or of one wave and
# the next (m = 64)
HAIRPIN_TIES = {256: -0.25, 64: 0.25}


def arc(n_candidates):
    """A quarter-circle-like bend of n_candidates + 2 poses: its full-range search has n_candidates candidates."""
    n = n_candidates + 2
    r = 0.2 * n / (math.pi / 2.0)
    return with_yaw([(r * math.sin(math.pi / 2.0 * i / (n - 1)), r * (1.0 - math.cos(math.pi / 2.0 * i / (n - 1))))
                     for i in range(n)])


def dup():
    pts = [(1.0, 2.0)] * 3 + [(1.0 + 0.2 * i, 2.0 + 0.05 * i * i) for i in range(1, 20)]
    return with_yaw(pts)


def random_walks(count=40, seed=20240611):
    rng = np.random.default_rng(seed)
    out = {}
    for k in range(count):
        n = int(rng.integers(5, 301))
        heading = rng.uniform(-math.pi, math.pi)
        xy = np.zeros((n, 2))
        for i in range(1, n):
            heading += rng.normal(0.0, 0.25) + (rng.uniform(-2.0, 2.0) if rng.random() < 0.03 else 0.0)
            xy[i] = xy[i - 1] + 0.2 * np.array([math.cos(heading), math.sin(heading)])
        xy += rng.uniform(-20.0, 20.0, 2)
        if k % 2:
            xy = xy - xy[-1]
            xy[-1] = (0.0, 0.0)
        out[f"walk{k:02d}_n{n}" + ("_home" if k % 2 else "")] = with_yaw(xy, last=float(rng.uniform(-3.0, 3.0)))
    return out


def all_scenes():
    B = WORKGROUP
    s = dict(small())
    s.update({"five": five(), "straight9": straight9(), "ell": ell(), "zigzag": zigzag(), "home": home(),
              "zigzag_end_1e-6": zigzag_ending_at(1e-6, 0.0), "zigzag_end_9e-7": zigzag_ending_at(9e-7, -9e-7),
              "vertical": vertical(), "dup": dup()})
    for m in sorted({B, 64}):
        s[f"hairpin{m}"] = hairpin(m, 0.25, HAIRPIN_TIES[m])
    for nc in (B - 1, B, B + 1, 2 * B + 1):
        s[f"arc{nc}"] = arc(nc)
    s.update(random_walks())
    return s
