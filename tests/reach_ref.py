"""aos_gvd_reach restated with numpy and heapq, from the definitions in include/aos_gpu.h alone.

Passable: the byte is not 100 and the clearance d2 (clearance_ref.field) is at least min_d2. Moves: to a passable
8-neighbour, 5 along an axis, 7 diagonally and then only between two passable cells. cost = the least sum of move costs
from a source cell (a plain Dijkstra over a binary heap), COST_NONE where none arrives. The cell rule is
clearance_ref.cells_of. Everything is an integer, so the library has to give these words exactly.
"""
import heapq

import numpy as np

import clearance_ref as C

COST_NONE = 0xFFFFFFFF
AXIS, DIAG = 5, 7
MAX_SOURCES = 1 << 20
MOVES = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))   # the descent's order


def passable(grid, min_d2=0):
    grid = np.asarray(grid, np.int8)
    free = grid != 100
    if min_d2 >= 2 and grid.size:
        free &= C.field(grid).astype(np.uint64) >= min_d2   # (D2_NONE is above every min_d2)
    return free


def source_cells(sources, origin, resolution, mask):
    """(kept, linear cell) per source: kept iff the point has a cell and the cell is passable."""
    H, W = mask.shape
    xy = np.asarray(sources, np.float64).reshape(-1, 2)
    ok, mx, my = C.cells_of(xy[:, 0], xy[:, 1], origin, resolution, W, H)
    ok = ok.copy()
    if W * H:
        ok[ok] = mask[my[ok], mx[ok]]
    return ok, np.where(ok, my * W + mx, -1)


def allowed(mask, x, y, dx, dy):
    """The move from the passable cell (x, y) by (dx, dy)."""
    H, W = mask.shape
    nx, ny = x + dx, y + dy
    if nx < 0 or nx >= W or ny < 0 or ny >= H or not mask[ny, nx]:
        return False
    return dx == 0 or dy == 0 or bool(mask[y, nx] and mask[ny, x])


def dijkstra(mask, cells):
    """cost (H, W) uint32 from the linear source cells."""
    H, W = mask.shape
    out = np.full((H, W), COST_NONE, np.uint32)
    if W * H == 0:
        return out
    m = mask.ravel().tolist()
    INF = 1 << 62
    cost = [INF] * (W * H)
    heap = []
    for c in sorted(set(int(c) for c in cells)):
        cost[c] = 0
        heap.append((0, c))
    pop, push = heapq.heappop, heapq.heappush
    while heap:
        d, c = pop(heap)
        if d != cost[c]:
            continue
        y, x = divmod(c, W)
        l, r, u, dn = x > 0 and m[c - 1], x + 1 < W and m[c + 1], y > 0 and m[c - W], y + 1 < H and m[c + W]
        v = d + AXIS
        for ok, n in ((r, c + 1), (l, c - 1), (dn, c + W), (u, c - W)):
            if ok and v < cost[n]:
                cost[n] = v
                push(heap, (v, n))
        v = d + DIAG
        for ok, n in ((r and dn, c + W + 1), (l and dn, c + W - 1), (r and u, c - W + 1), (l and u, c - W - 1)):
            if ok and m[n] and v < cost[n]:
                cost[n] = v
                push(heap, (v, n))
    flat = np.array([COST_NONE if v == INF else v for v in cost], np.uint32)
    return flat.reshape(H, W)


def metres(cost, resolution):
    cost = np.asarray(cost, np.uint32)
    m = (cost.astype(np.float64) * C.res_of(resolution) / 5.0).astype(np.float32)
    return np.where(cost == COST_NONE, np.float32(np.inf), m).astype(np.float32)


def at_points(fld, xy, origin, resolution):
    H, W = fld.shape
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ok, mx, my = C.cells_of(xy[:, 0], xy[:, 1], origin, resolution, W, H)
    out = np.full(len(xy), COST_NONE, np.uint32)
    if W * H:
        out[ok] = fld[my[ok], mx[ok]]
    return out


def descend(fld, mask, start, origin, resolution):
    """The descent's linear cell indices (uint32) from the world point start."""
    H, W = fld.shape
    ok, mx, my = C.cells_of([start[0]], [start[1]], origin, resolution, W, H)
    if W * H == 0 or not ok[0] or fld[my[0], mx[0]] == COST_NONE:
        return np.zeros(0, np.uint32)
    x, y = int(mx[0]), int(my[0])
    cells = [y * W + x]
    while fld[y, x] != 0:
        here = int(fld[y, x])
        for dx, dy in MOVES:
            if allowed(mask, x, y, dx, dy) and int(fld[y + dy, x + dx]) + (AXIS if dx == 0 or dy == 0 else DIAG) == here:
                x, y = x + dx, y + dy
                break
        else:
            raise AssertionError("a reached cell without a descent neighbour: the field is no fixed point")
        cells.append(y * W + x)
    assert len(cells) <= int(fld[my[0], mx[0]]) // AXIS + 1
    return np.array(cells, np.uint32)


def centres(cells, W, origin, resolution):
    cells = np.asarray(cells, np.int64)
    res = C.res_of(resolution)
    return np.stack([origin[0] + ((cells % max(W, 1)).astype(np.float64) + 0.5) * res,
                     origin[1] + ((cells // max(W, 1)).astype(np.float64) + 0.5) * res], 1).reshape(-1, 2)


def reach(scene):
    """Everything aos_gvd_reach and its companions return for a scene (reach_scenes.scene)."""
    grid = np.asarray(scene["grid"], np.int8)
    H, W = grid.shape
    mask = passable(grid, scene["min_d2"])
    kept, cells = source_cells(scene["sources"], scene["origin"], scene["resolution"], mask)
    fld = dijkstra(mask, cells[kept])
    reached = fld != COST_NONE
    node_cost = at_points(fld, scene["nodes"], scene["origin"], scene["resolution"])
    paths = [descend(fld, mask, s, scene["origin"], scene["resolution"]) for s in scene["starts"]]
    return {"field": fld, "mask": mask, "n_passable": int(mask.sum()), "n_reached": int(reached.sum()),
            "n_sources_used": int(kept.sum()), "max_cost": int(fld[reached].max()) if reached.any() else COST_NONE,
            "node_cost": node_cost, "node_metres": metres(node_cost, scene["resolution"]), "descents": paths,
            "descent_xy": [centres(p, W, scene["origin"], scene["resolution"]) for p in paths]}
