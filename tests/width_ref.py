"""aos_gvd_width restated twice with numpy, heapq and scipy, from the definitions in include/aos_gpu.h alone.

cap = 0 where the byte is 100, else the clearance d2 (clearance_ref.field). A move goes to an 8-neighbour; its bottleneck
is the least cap of its two cells and, for a diagonal, of the two cells beside it. width = the greatest, over the move
paths from a kept source cell, of the least bottleneck on the path (a path of one cell: the cell's cap), 0 where none
is above 0.
  (a) dijkstra:        a max-heap bottleneck Dijkstra over the moves.
  (b) threshold_sweep: for every distinct cap value m, {width >= m} = the components of reach's move graph on the mask
                       cap >= m (test_reach_cpu.move_graph) that hold a kept source; no path is ever followed.
Everything is an integer, so the library has to give these words exactly.
"""
import heapq

import numpy as np

import clearance_ref as C

WIDTH_NONE = 0
D2_NONE = 0xFFFFFFFF
MAX_SOURCES = 1 << 20


def cap_of(grid):
    grid = np.asarray(grid, np.int8)
    if grid.size == 0:
        return np.zeros(grid.shape, np.uint32)
    return np.where(grid == 100, 0, C.field(grid)).astype(np.uint32)


def source_cells(sources, origin, resolution, cap):
    """(kept, linear cell) per source: kept iff the point has a cell and the cell's cap is above 0."""
    H, W = cap.shape
    xy = np.asarray(sources, np.float64).reshape(-1, 2)
    ok, mx, my = C.cells_of(xy[:, 0], xy[:, 1], origin, resolution, W, H)
    ok = ok.copy()
    if W * H:
        ok[ok] = cap[my[ok], mx[ok]] > 0
    return ok, np.where(ok, my * W + mx, -1)


def dijkstra(cap, cells, corner_rule=True):
    """width (H, W) uint32 from the linear source cells. corner_rule False: a diagonal's bottleneck leaves out the two
    cells beside it (the wrong answer the corner scenes are built to tell apart)."""
    H, W = cap.shape
    if W * H == 0:
        return np.zeros((H, W), np.uint32)
    cp = [int(v) for v in cap.ravel()]
    wd = [0] * (W * H)
    heap = []
    for c in sorted(set(int(c) for c in cells)):
        wd[c] = cp[c]
        heap.append((-cp[c], c))
    heapq.heapify(heap)
    pop, push = heapq.heappop, heapq.heappush
    while heap:
        v, c = pop(heap)
        v = -v
        if v != wd[c]:
            continue
        y, x = divmod(c, W)
        l, r, u, d = x > 0, x + 1 < W, y > 0, y + 1 < H
        for ok, n in ((r, c + 1), (l, c - 1), (d, c + W), (u, c - W)):
            if ok:
                b = min(v, cp[n])
                if b > wd[n]:
                    wd[n] = b
                    push(heap, (-b, n))
        for ok, n, s1, s2 in ((r and d, c + W + 1, c + 1, c + W), (l and d, c + W - 1, c - 1, c + W),
                              (r and u, c - W + 1, c + 1, c - W), (l and u, c - W - 1, c - 1, c - W)):
            if ok:
                b = min(v, cp[n], cp[s1], cp[s2]) if corner_rule else min(v, cp[n])
                if b > wd[n]:
                    wd[n] = b
                    push(heap, (-b, n))
    return np.array(wd, np.uint32).reshape(H, W)


def threshold_sweep(cap, cells):
    """Statement (b)."""
    from scipy.sparse.csgraph import connected_components

    from test_reach_cpu import move_graph
    H, W = cap.shape
    out = np.zeros(H * W, np.uint32)
    cells = np.unique(np.asarray(cells, np.int64))
    if W * H == 0 or len(cells) == 0:
        return out.reshape(H, W)
    flat = cap.ravel()
    top = int(flat[cells].max())   # no source survives a higher threshold
    for m in np.unique(flat):
        m = int(m)
        if m == 0 or m > top:
            continue
        mask = cap >= m
        _, label = connected_components(move_graph(mask), directed=False)
        kept = cells[flat[cells] >= m]
        inside = np.isin(label, np.unique(label[kept])) & mask.ravel()
        out[inside] = m   # (ascending m: the last threshold a cell survives stays)
    return out.reshape(H, W)


def radius(width, resolution):
    width = np.asarray(width, np.uint32)
    m = (np.sqrt(width.astype(np.float64)) * C.res_of(resolution)).astype(np.float32)
    return np.where(width == D2_NONE, np.float32(np.inf), m).astype(np.float32)


def at_points(fld, xy, origin, resolution):
    H, W = fld.shape
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ok, mx, my = C.cells_of(xy[:, 0], xy[:, 1], origin, resolution, W, H)
    out = np.zeros(len(xy), np.uint32)
    if W * H:
        out[ok] = fld[my[ok], mx[ok]]
    return out


def width(scene):
    """Everything aos_gvd_width and its companions return for a scene (width_scenes.scene), by statement (a)."""
    cap = cap_of(scene["grid"])
    kept, cells = source_cells(scene["sources"], scene["origin"], scene["resolution"], cap)
    fld = dijkstra(cap, cells[kept])
    reached = fld != WIDTH_NONE
    node_width = at_points(fld, scene["nodes"], scene["origin"], scene["resolution"])
    point_width = at_points(fld, scene["points"], scene["origin"], scene["resolution"])
    return {"field": fld, "cap": cap, "cells": cells[kept], "n_free": int((cap > 0).sum()), "n_reached": int(reached.sum()),
            "n_sources_used": int(kept.sum()), "min_width": int(fld[reached].min()) if reached.any() else 0,
            "max_width": int(fld[reached].max()) if reached.any() else 0, "node_width": node_width,
            "node_radius_m": radius(node_width, scene["resolution"]), "point_width": point_width,
            "point_radius_m": radius(point_width, scene["resolution"])}
