"""aos_gvd_soft restated with numpy, from the definitions in include/aos_gpu.h alone, twice over.

Passable is reach_ref's rule. r = the integer square root of the clearance d2 (clearance_ref.field), wt = 1 + gain *
max(0, soft_cells - r) on passable cells (1 where d2 is none), 0 on the others. A move is reach's and costs 5 or 7 times
the largest wt over the cells it touches: its two cells, and for a diagonal the two cells beside it. cost = the least sum
of move costs from a source cell, COST_NONE where none arrives.
    dijkstra        walks cell by cell over a binary heap and forms each move's cost from the weight bytes
    dijkstra_scipy  builds the move graph with whole-array shifts (move_costs) and hands it to scipy
Everything is an integer, so the library has to give these words exactly.
"""
import heapq
import math

import numpy as np

import clearance_ref as C
import reach_ref as R

COST_NONE = R.COST_NONE
AXIS, DIAG, MOVES = R.AXIS, R.DIAG, R.MOVES
COST_LIMIT = 1 << 31


def options_ok(soft_cells, gain):
    """The options aos_gvd_soft accepts: both in range and the largest weight they can give within a byte."""
    return 0 <= soft_cells <= 255 and 0 <= gain <= 254 and 1 + gain * max(0, soft_cells - 1) <= 255


def weights(grid, min_d2=0, soft_cells=0, gain=0):
    """uint8 (H, W): 0 on impassable cells, else the weight."""
    grid = np.asarray(grid, np.int8)
    mask = R.passable(grid, min_d2)
    wt = mask.astype(np.int64)
    if grid.size and gain > 0 and soft_cells > 0:
        d2 = C.field(grid).astype(np.int64)
        vals, inv = np.unique(d2, return_inverse=True)   # math.isqrt is exact; one call per distinct value
        r = np.array([math.isqrt(int(v)) for v in vals], np.int64)[inv.reshape(-1)].reshape(d2.shape)
        pen = np.where(d2 == C.D2_NONE, 0, np.maximum(0, soft_cells - r))
        wt = np.where(mask, 1 + gain * pen, 0)
    assert wt.max(initial=0) <= 255
    return wt.astype(np.uint8)


def move_cost(wt, x, y, dx, dy):
    """The cost of the move from (x, y) by (dx, dy); 0: not allowed."""
    H, W = wt.shape
    nx, ny = x + dx, y + dy
    if nx < 0 or nx >= W or ny < 0 or ny >= H:
        return 0
    cells = [wt[y, x], wt[ny, nx]] + ([wt[y, nx], wt[ny, x]] if dx and dy else [])
    return 0 if min(cells) == 0 else (DIAG if dx and dy else AXIS) * int(max(cells))


def dijkstra(wt, cells):
    """cost (H, W) uint32 from the linear source cells, cell by cell."""
    H, W = wt.shape
    if W * H == 0:
        return np.full((H, W), COST_NONE, np.uint32)
    w = wt.ravel().tolist()
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
        a = w[c]
        l = w[c - 1] if x > 0 else 0
        r = w[c + 1] if x + 1 < W else 0
        u = w[c - W] if y > 0 else 0
        dn = w[c + W] if y + 1 < H else 0
        for b, n in ((r, c + 1), (l, c - 1), (dn, c + W), (u, c - W)):
            if b:
                v = d + AXIS * (a if a > b else b)
                if v < cost[n]:
                    cost[n] = v
                    push(heap, (v, n))
        for s, t, n in ((r, dn, c + W + 1), (l, dn, c + W - 1), (r, u, c - W + 1), (l, u, c - W - 1)):
            if s and t and w[n]:
                v = d + DIAG * max(a, w[n], s, t)
                if v < cost[n]:
                    cost[n] = v
                    push(heap, (v, n))
    return np.array([COST_NONE if v == INF else v for v in cost], np.uint32).reshape(H, W)


def shifted(a, dx, dy):
    """(the cells that have a neighbour by (dx, dy), that neighbour) as two views of a."""
    H, W = a.shape
    ys, yd = (slice(0, H - 1), slice(1, H)) if dy == 1 else (slice(1, H), slice(0, H - 1)) if dy == -1 else (slice(0, H),) * 2
    xs, xd = (slice(0, W - 1), slice(1, W)) if dx == 1 else (slice(1, W), slice(0, W - 1)) if dx == -1 else (slice(0, W),) * 2
    return (ys, xs), (yd, xd)


def move_costs(wt):
    """Per move (dx, dy) an (H, W) int64 array: the cost of that move from each cell, 0 where it is not allowed. Built
    with whole-array shifts."""
    w = wt.astype(np.int64)
    out = {}
    for dx, dy in MOVES:
        (ys, xs), (yd, xd) = shifted(w, dx, dy)
        touched = [w[ys, xs], w[yd, xd]] + ([w[ys, xd], w[yd, xs]] if dx and dy else [])
        lo, hi = np.minimum.reduce(touched), np.maximum.reduce(touched)
        full = np.zeros(w.shape, np.int64)
        full[ys, xs] = np.where(lo > 0, (DIAG if dx and dy else AXIS) * hi, 0)
        out[(dx, dy)] = full
    return out


def dijkstra_scipy(wt, cells):
    """The same field from scipy's Dijkstra on the move graph."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra as sp_dijkstra
    H, W = wt.shape
    cells = np.unique(np.asarray(cells, np.int64))
    if W * H == 0 or len(cells) == 0:
        return np.full((H, W), COST_NONE, np.uint32)
    idx = np.arange(H * W).reshape(H, W)
    rows, cols, vals = [], [], []
    for (dx, dy), mc in move_costs(wt).items():
        (ys, xs), (yd, xd) = shifted(idx, dx, dy)
        ok = mc[ys, xs] > 0
        rows.append(idx[ys, xs][ok]); cols.append(idx[yd, xd][ok]); vals.append(mc[ys, xs][ok])
    g = coo_matrix((np.concatenate(vals).astype(np.float64), (np.concatenate(rows), np.concatenate(cols))),
                   shape=(H * W, H * W)).tocsr()
    d = sp_dijkstra(g, directed=True, indices=cells, min_only=True)
    return np.where(np.isinf(d), COST_NONE, d).astype(np.uint32).reshape(H, W)


def descend(fld, wt, start, origin, resolution):
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
            w = move_cost(wt, x, y, dx, dy)
            if w and fld[y + dy, x + dx] != COST_NONE and int(fld[y + dy, x + dx]) + w == here:
                x, y = x + dx, y + dy
                break
        else:
            raise AssertionError("a reached cell without a descent neighbour: the field is no fixed point")
        cells.append(y * W + x)
    assert len(cells) <= int(fld[my[0], mx[0]]) // AXIS + 1
    return np.array(cells, np.uint32)


def plain_cost(cells, W):
    """The sum of 5 and 7 over the moves between consecutive cells."""
    c = np.asarray(cells, np.int64)
    if len(c) < 2:
        return 0
    diag = (np.diff(c % W) != 0) & (np.diff(c // W) != 0)
    return int(np.where(diag, DIAG, AXIS).sum())


def weighted_cost(cells, wt):
    """The sum of the moves' costs between consecutive cells."""
    H, W = wt.shape
    c = [int(v) for v in cells]
    return sum(move_cost(wt, a % W, a // W, b % W - a % W, b // W - a // W) for a, b in zip(c[:-1], c[1:]))


def bound_crossed(wt):
    return 7 * int(wt.max(initial=0)) * int((wt > 0).sum()) >= COST_LIMIT


def soft(scene, statement=None):
    """Everything aos_gvd_soft and its companions return for a scene (soft_scenes.scene). A scene the library refuses
    gives {"refused": ...}. statement None: the heap walk, or scipy for a scene marked "big"."""
    grid = np.asarray(scene["grid"], np.int8)
    H, W = grid.shape
    if not options_ok(scene["soft_cells"], scene["gain"]):
        return {"refused": "options"}
    wt = weights(grid, scene["min_d2"], scene["soft_cells"], scene["gain"])
    if bound_crossed(wt):
        return {"refused": "bound", "max_weight": int(wt.max()), "n_passable": int((wt > 0).sum())}
    mask = wt > 0
    kept, cells = R.source_cells(scene["sources"], scene["origin"], scene["resolution"], mask)
    statement = statement or (dijkstra_scipy if scene.get("big") else dijkstra)
    fld = statement(wt, cells[kept])
    reached = fld != COST_NONE
    paths = [descend(fld, wt, s, scene["origin"], scene["resolution"]) for s in scene["starts"]]
    return {"field": fld, "weights": wt, "mask": mask, "n_passable": int(mask.sum()), "n_reached": int(reached.sum()),
            "n_soft": int((wt > 1).sum()), "max_weight": int(wt.max(initial=0)), "n_sources_used": int(kept.sum()),
            "max_cost": int(fld[reached].max()) if reached.any() else COST_NONE,
            "node_cost": R.at_points(fld, scene["nodes"], scene["origin"], scene["resolution"]), "descents": paths,
            "descent_xy": [R.centres(p, W, scene["origin"], scene["resolution"]) for p in paths],
            "plain_costs": [plain_cost(p, W) for p in paths]}
