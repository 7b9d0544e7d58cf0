"""aos_reach_sight and aos_reach_pull restated with numpy and fractions, from the definitions in include/aos_gpu.h alone,
on top of reach_ref.

The cells a segment between the centres of cells a and b touches, in three forms:
    touched_bbox     every cell of the bounding box against 2 |dx (y - ay) - dy (x - ax)| <= |dx| + |dy|
    touched_exact    every cell of the bounding box against an exact rational clip (Liang-Barsky over fractions) of the
                     closed segment to the cell's closed unit square; for small cases
    columns          per column of the major axis the interval of minor coordinates that satisfy the inequality, by
                     floor division, for many segments in one numpy pass; fast enough for the large scenes
Everything is an integer, so the library has to give these words exactly.
"""
from fractions import Fraction

import numpy as np

import clearance_ref as C
import reach_ref as R

COST_NONE = R.COST_NONE
MAX_DESCENT = 65536


def touched_bbox(a, b):
    """The set of touched cells (x, y), from the inequality over the bounding box."""
    (ax, ay), (bx, by) = a, b
    dx, dy = bx - ax, by - ay
    return {(x, y) for x in range(min(ax, bx), max(ax, bx) + 1) for y in range(min(ay, by), max(ay, by) + 1)
            if 2 * abs(dx * (y - ay) - dy * (x - ax)) <= abs(dx) + abs(dy)}


def square_meets_segment(x, y, p, q):
    """Does the closed square [x, x + 1] x [y, y + 1] meet the closed segment p -> q? Exact, over fractions."""
    t0, t1 = Fraction(0), Fraction(1)
    for p0, d, lo, hi in ((p[0], q[0] - p[0], x, x + 1), (p[1], q[1] - p[1], y, y + 1)):
        if d == 0:
            if p0 < lo or p0 > hi:
                return False
            continue
        ta, tb = Fraction(lo - p0) / d, Fraction(hi - p0) / d
        if ta > tb:
            ta, tb = tb, ta
        t0, t1 = max(t0, ta), min(t1, tb)
    return t0 <= t1


def touched_exact(a, b):
    (ax, ay), (bx, by) = a, b
    h = Fraction(1, 2)
    p, q = (ax + h, ay + h), (bx + h, by + h)
    return {(x, y) for x in range(min(ax, bx), max(ax, bx) + 1) for y in range(min(ay, by), max(ay, by) + 1)
            if square_meets_segment(x, y, p, q)}


def columns(ax, ay, bx, by):
    """Every touched cell of the segments (ax, ay)[k] -> (bx, by)[k], column by column: (k, x, y) int64 arrays, k the
    segment's index. For a column at signed major offset u the minor offsets v satisfy |D v - N| <= S with D = 2 * the
    major delta, N = 2 * the minor delta * u and S = |dx| + |dy|; dividing by |D| gives the interval."""
    ax, ay, bx, by = (np.asarray(v, np.int64).reshape(-1) for v in (ax, ay, bx, by))
    dx, dy = bx - ax, by - ay
    xmaj = np.abs(dx) >= np.abs(dy)
    dM, dm = np.where(xmaj, dx, dy), np.where(xmaj, dy, dx)       # the major and the minor delta
    n = np.abs(dM) + 1
    k = np.repeat(np.arange(len(ax)), n)
    first = np.cumsum(n) - n
    u = (np.arange(int(n.sum())) - first[k]) * np.sign(dM)[k]     # the signed major offset of the column
    S, D = (np.abs(dx) + np.abs(dy))[k], 2 * dM[k]
    N = 2 * dm[k] * u
    aD, sN = np.maximum(np.abs(D), 1), N * np.where(D < 0, -1, 1)   # |aD v - sN| <= S   (D = 0: the single cell)
    lo, hi = -((S - sN) // aD), (S + sN) // aD
    lo, hi = np.maximum(lo, np.minimum(dm, 0)[k]), np.minimum(hi, np.maximum(dm, 0)[k])
    assert (hi >= lo).all() and (hi - lo <= 2).all()
    kk, uu, vv = [], [], []
    for o in range(3):
        ok = lo + o <= hi
        kk.append(k[ok]); uu.append(u[ok]); vv.append((lo + o)[ok])
    k, u, v = np.concatenate(kk), np.concatenate(uu), np.concatenate(vv)
    return k, np.where(xmaj[k], ax[k] + u, ax[k] + v), np.where(xmaj[k], ay[k] + v, ay[k] + u)


def touched_columns(a, b):
    _, x, y = columns([a[0]], [a[1]], [b[0]], [b[1]])
    cells = set(zip(x.tolist(), y.tolist()))
    assert len(cells) == len(x)
    return cells


def sight_cells(mask, ax, ay, bx, by):
    """(n_touched, n_blocked) uint32 of segments between cells."""
    n = len(np.asarray(ax).reshape(-1))
    k, x, y = columns(ax, ay, bx, by)
    touched = np.bincount(k, minlength=n)
    blocked = np.bincount(k, weights=~mask[y, x], minlength=n).astype(np.int64)
    return touched.astype(np.uint32), blocked.astype(np.uint32)


def sight(mask, from_xy, to_xy, origin, resolution):
    """aos_reach_sight: (n_touched, n_blocked) of segments between world points."""
    H, W = mask.shape
    a, b = (np.asarray(v, np.float64).reshape(-1, 2) for v in (from_xy, to_xy))
    oka, ax, ay = C.cells_of(a[:, 0], a[:, 1], origin, resolution, W, H)
    okb, bx, by = C.cells_of(b[:, 0], b[:, 1], origin, resolution, W, H)
    ok = (oka & okb) if W * H else np.zeros(len(a), bool)
    touched, blocked = np.zeros(len(a), np.uint32), np.full(len(a), COST_NONE, np.uint32)
    if ok.any():
        touched[ok], blocked[ok] = sight_cells(mask, ax[ok], ay[ok], bx[ok], by[ok])
    return touched, blocked


def pull_steps(mask, cells, max_span=0):
    """The waypoint steps of a descent (linear cell indices) by the farthest-visible rule."""
    H, W = mask.shape
    m = len(cells)
    if m == 0:
        return np.zeros(0, np.uint32)
    cx, cy = np.asarray(cells, np.int64) % W, np.asarray(cells, np.int64) // W
    steps, k = [0], 0
    while k < m - 1:
        hi = m - 1 if max_span <= 0 else min(m - 1, k + max_span)
        j = np.arange(k + 1, hi + 1)
        _, blocked = sight_cells(mask, np.full(len(j), cx[k]), np.full(len(j), cy[k]), cx[j], cy[j])
        free = j[blocked == 0]
        assert len(free) and free[0] == k + 1   # the next cell is an allowed move
        k = int(free.max())
        steps.append(k)
    return np.array(steps, np.uint32)


def pull(fld, mask, start, origin, resolution, max_span=0):
    """Everything aos_reach_pull returns for a start on a reach_ref field."""
    H, W = fld.shape
    cells = R.descend(fld, mask, start, origin, resolution)
    m = len(cells)
    if m > MAX_DESCENT:
        raise ValueError("descent longer than 65536 cells")
    steps = pull_steps(mask, cells, max_span)
    wc = cells[steps] if m else np.zeros(0, np.uint32)
    res = C.res_of(resolution)
    x, y = wc.astype(np.int64) % max(W, 1), wc.astype(np.int64) // max(W, 1)
    total = 0.0
    for ddx, ddy in zip(np.diff(x).tolist(), np.diff(y).tolist()):
        total += float(np.sqrt(np.float64(ddx * ddx + ddy * ddy)))
    start_cost = int(fld.ravel()[cells[0]]) if m else COST_NONE
    tests = sum((m - 1 if max_span <= 0 else min(m - 1, int(k) + max_span)) - int(k) for k in steps[:-1]) if m else 0
    return {"n_cells": m, "start_cost": start_cost, "steps": steps, "cells": wc.astype(np.uint32),
            "xy": R.centres(wc, W, origin, resolution), "length_m": total * res,
            "descent_m": float(start_cost) * res / 5.0 if m else float("inf"), "n_sight_tests": tests,
            "descent": cells}


def leg_cells(mask, cells):
    """Every cell touched by every leg of the waypoint cells (linear indices): (x, y) arrays."""
    W = mask.shape[1]
    c = np.asarray(cells, np.int64)
    if len(c) < 2:
        return c % max(W, 1), c // max(W, 1)
    _, x, y = columns(c[:-1] % W, c[:-1] // W, c[1:] % W, c[1:] // W)
    return x, y
