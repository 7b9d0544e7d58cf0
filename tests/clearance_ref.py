"""aos_gvd_clearance restated with numpy, from the definitions in include/aos_gpu.h alone.

Occupied cell: the byte is 100. Field: d2[y, x] = min over occupied (cx, cy) of (x - cx)^2 + (y - cy)^2, uint32 in cell
units, D2_NONE everywhere without an occupied cell. Two statements of it: brute force (every cell against every occupied
cell) for small grids, and a separable one (column distances, then every row's cells against every column of the row)
for mid-size grids; both are integer, so they have to agree word for word. The sampler and the conversions are plain
float64 operations in the order the header states them.
"""
import numpy as np

D2_NONE = 0xFFFFFFFF
MAX_DIM = 16384
MIN_LEN = 1e-6
BRUTE_MAX_PAIRS = 1 << 31   # cells x occupied cells a test may ask of the brute force


def occupied(grid):
    return np.asarray(grid, np.int8) == 100


def brute_field(grid):
    occ = occupied(grid)
    H, W = occ.shape
    out = np.full((H, W), D2_NONE, np.uint32)
    cy, cx = np.nonzero(occ)
    if len(cx) == 0 or W * H == 0:
        return out
    assert W * H * len(cx) <= BRUTE_MAX_PAIRS
    cx, cy = cx.astype(np.int64), cy.astype(np.int64)
    xs = np.arange(W, dtype=np.int64)
    rows = max(1, (1 << 24) // (W * len(cx)))
    for y0 in range(0, H, rows):
        ys = np.arange(y0, min(H, y0 + rows), dtype=np.int64)
        d = (xs[None, :, None] - cx[None, None, :]) ** 2 + (ys[:, None, None] - cy[None, None, :]) ** 2
        out[y0:y0 + len(ys)] = d.min(axis=2).astype(np.uint32)
    return out


def column_distance(grid):
    """g[y, x] = min over the column's occupied rows y' of |y - y'| (int64; INF = 1 << 20 without one)."""
    occ = occupied(grid)
    H, W = occ.shape
    INF = 1 << 20
    ys = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(occ, ys, -INF), axis=0)                    # nearest occupied row <= y
    below = np.minimum.accumulate(np.where(occ, ys, 2 * INF)[::-1], axis=0)[::-1]     # nearest occupied row >= y
    return np.minimum(np.minimum(ys - above, below - ys), INF)


def separable_field(grid):
    occ = occupied(grid)
    H, W = occ.shape
    out = np.full((H, W), D2_NONE, np.uint32)
    if W * H == 0 or not occ.any():
        return out
    g = column_distance(grid)
    INF = 1 << 20
    xs = np.arange(W, dtype=np.int64)
    dx2 = (xs[:, None] - xs[None, :]) ** 2          # [x, x']
    rows = max(1, (1 << 23) // (W * W))
    for y0 in range(0, H, rows):
        gg = g[y0:y0 + rows]
        v = (dx2[None, :, :] + (gg * gg)[:, None, :]).min(axis=2)
        out[y0:y0 + rows] = np.where(v >= INF * INF, D2_NONE, v).astype(np.uint32)
    return out


def field(grid):
    """The brute force where it is affordable, else the separable statement."""
    occ = occupied(grid)
    return brute_field(grid) if occ.size * max(1, int(occ.sum())) <= (1 << 26) else separable_field(grid)


def res_of(resolution):
    return float(np.float32(resolution))   # (double)info.resolution


def cells_of(px, py, origin, resolution, W, H):
    """occ_trunc's rule, vectorised: (has a cell, column, row)."""
    res = res_of(resolution)
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fx = (px - origin[0]) / res
        fy = (py - origin[1]) / res
        inside = (fx > -1.0) & (fx < float(W)) & (fy > -1.0) & (fy < float(H))
        mx = np.where(inside, np.trunc(np.where(inside, fx, 0.0)), -1).astype(np.int64)
        my = np.where(inside, np.trunc(np.where(inside, fy, 0.0)), -1).astype(np.int64)
    ok = inside & (mx >= 0) & (mx < W) & (my >= 0) & (my < H)
    return ok, mx, my


def edge_num(length, resolution):
    """num of edgePassesThroughOccupiedPixels: (int)(len / step) + 1, x86's INT_MIN out of range -> INT_MIN + 1."""
    step = res_of(resolution) * 0.5
    q = length / step
    if q > -2147483649.0 and q < 2147483647.0:
        return int(q) + 1
    return -(1 << 31) + 1


def edge_samples(s, e, resolution):
    """The sample points (px, py) of the edge from s to e, in order."""
    ex, ey = e[0] - s[0], e[1] - s[1]
    with np.errstate(over="ignore"):
        length = float(np.sqrt(np.float64(ex) * np.float64(ex) + np.float64(ey) * np.float64(ey)))
    if length < MIN_LEN:
        return np.array([s[0]], np.float64), np.array([s[1]], np.float64)
    num = edge_num(length, resolution)
    if num < 0:
        return np.zeros(0), np.zeros(0)
    ux, uy = ex / length, ey / length
    i = np.arange(num + 1, dtype=np.float64)
    t = i / float(num)
    t[num] = 1.0
    return s[0] + (t * ux) * length, s[1] + (t * uy) * length


def metres(d2, resolution):
    d2 = np.asarray(d2, np.uint32)
    m = (np.sqrt(d2.astype(np.float64)) * res_of(resolution)).astype(np.float32)
    return np.where(d2 == D2_NONE, np.float32(np.inf), m).astype(np.float32)


def at_points(fld, xy, origin, resolution):
    H, W = fld.shape
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ok, mx, my = cells_of(xy[:, 0], xy[:, 1], origin, resolution, W, H)
    out = np.full(len(xy), D2_NONE, np.uint32)
    if W * H:
        out[ok] = fld[my[ok], mx[ok]]
    return out


def graph_clearances(fld, nodes, edges, origin, resolution):
    """(node_d2, edge_d2) of a graph against a field."""
    nodes = np.asarray(nodes, np.float64).reshape(-1, 2)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    node_d2 = at_points(fld, nodes, origin, resolution)
    edge_d2 = np.full(len(edges), D2_NONE, np.uint32)
    for k, (a, b) in enumerate(edges):
        px, py = edge_samples(nodes[a], nodes[b], resolution)
        if len(px):
            edge_d2[k] = at_points(fld, np.stack([px, py], 1), origin, resolution).min()
    return node_d2, edge_d2


def clearance(scene, fld=None):
    """Everything aos_gvd_clearance returns for a scene (clearance_scenes.scene)."""
    grid = np.asarray(scene["grid"], np.int8)
    if fld is None:
        fld = field(grid)
    n_occ = int(occupied(grid).sum())
    node_d2, edge_d2 = graph_clearances(fld, scene["nodes"], scene["edges"], scene["origin"], scene["resolution"])
    return {"field": fld, "n_occupied": n_occ, "max_d2": int(fld.max()) if n_occ else D2_NONE,
            "node_d2": node_d2, "edge_d2": edge_d2, "node_clearances": metres(node_d2, scene["resolution"]),
            "edge_clearances": metres(edge_d2, scene["resolution"])}
