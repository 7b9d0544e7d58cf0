"""Plain Python / numpy restatement of the two device-side operations of aos_path_plan (csrc/path.hip) and nothing
else: trimPathNearOccupiedRegions' cut index (k_trim_check; src/aos_path_gen_node.cpp:1591-1617) and
findKNearestNodes / findNearestNode (k_nearest_k; :898-932). Every function takes variant=, one of the mistakes a
kernel could make; None is the reference's arithmetic. test_path_scenes_cpu.py holds the restatement against the
oracle on every scene of path_scenes.py and shows which variants a scene can tell from the reference's arithmetic,
and why the others cannot be told apart from it by any grid.
"""
import math
from fractions import Fraction

import numpy as np

SAFETY = 0.2
DBL_MAX = float(np.finfo(np.float64).max)
INT_LO, INT_HI = -2147483649.0, 2147483648.0   # static_cast<int> is defined (and exact truncation) strictly between

TRIM_VARIANTS = ("floor", "ge", "fma", "round", "nonzero", "pose0")
NEAREST_VARIANTS = ("fma", "larger-index")
NEAREST_ONE_VARIANTS = ("accept-inf",)


def fma(a, b, c):
    """a * b + c with one rounding, exactly (finite arguments)."""
    try:
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    except OverflowError:
        return math.inf if Fraction(a) * Fraction(b) + Fraction(c) > 0 else -math.inf


def grid_res(info):
    """OccupancyGrid's float32 resolution, widened."""
    return float(np.float32(info["resolution"]))


def radius_cells(res, variant=None):
    q = SAFETY / res
    return int(round(q)) if variant == "round" else int(math.ceil(q))


def offsets(res, variant=None):
    """The (dx, dy) the reference samples around a pose, in its loop order (:1593-1602)."""
    rc = radius_cells(res, variant)
    out = []
    for dx in range(-rc, rc + 1):
        for dy in range(-rc, rc + 1):
            dist = math.sqrt(dx * dx + dy * dy) * res
            if dist >= SAFETY if variant == "ge" else dist > SAFETY:
                continue
            out.append((dx, dy))
    return out


def cell(f, variant=None):
    """static_cast<int>(f): truncation toward zero; a quotient outside the int range (x86 gives INT_MIN) or a NaN is
    no cell. None: outside every grid."""
    if not (INT_LO < f < INT_HI):
        return None
    return math.floor(f) if variant == "floor" else int(f)


def sample_cell(x, y, dx, dy, info, variant=None):
    """(mx, my) of the sample (dx, dy) of a pose at (x, y), or None outside the grid."""
    res = grid_res(info)
    ox, oy = info["origin"]
    if variant == "fma":
        cx, cy = fma(dx, res, x), fma(dy, res, y)
    else:
        cx, cy = x + dx * res, y + dy * res
    mx, my = cell((cx - ox) / res, variant), cell((cy - oy) / res, variant)
    if mx is None or my is None or not (0 <= mx < info["width"] and 0 <= my < info["height"]):
        return None
    return mx, my


def trim_first(poses_xy, grid, info, variant=None):
    """The index trimPathNearOccupiedRegions cuts at (the path keeps poses [0, index)), or None. grid: the int8
    cells, row-major (height, width)."""
    g = np.asarray(grid, np.int8).reshape(info["height"], info["width"])
    offs = offsets(grid_res(info), variant)
    for i, (x, y) in enumerate(np.asarray(poses_xy, np.float64).reshape(-1, 2).tolist()):
        if i == 0 and variant != "pose0":
            continue
        for dx, dy in offs:
            c = sample_cell(x, y, dx, dy, info, variant)
            if c is None:
                continue
            v = int(g[c[1], c[0]])
            if v != 0 if variant == "nonzero" else v == 100:
                return i
    return None


def distances(nodes, p, variant=None):
    """distance(p, node) of :781-785 for every node: dx = p.x - n.x, sqrt(dx * dx + dy * dy); inf on overflow."""
    n = np.asarray(nodes, np.float64).reshape(-1, 2)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy = float(p[0]) - n[:, 0], float(p[1]) - n[:, 1]
        if variant == "fma":
            s = np.array([fma(a, a, b * b) if math.isfinite(a) and math.isfinite(b * b) else a * a + b * b
                          for a, b in zip(dx.tolist(), dy.tolist())], np.float64)
        else:
            s = dx * dx + dy * dy
        return np.sqrt(s)


def k_nearest(nodes, p, k, variant=None):
    """findKNearestNodes: sorted((distance, index))[:k]."""
    d = distances(nodes, p, variant).tolist()
    sign = -1 if variant == "larger-index" else 1
    return [i for _, _, i in sorted((v, sign * i, i) for i, v in enumerate(d))[:k]]


def nearest(nodes, p, variant=None):
    """findNearestNode: strict < from DBL_MAX, -1 when no node is nearer than that."""
    best, m = -1, DBL_MAX
    d = distances(nodes, p).tolist()
    for i, v in enumerate(d):
        if v < m:
            best, m = i, v
    if best < 0 and variant == "accept-inf" and d:
        best = k_nearest(nodes, p, 1)[0]
    return best
