"""Designed scenes for aos_gvd_width: the smallest shapes at which its kernels can still go wrong.

A scene is {"grid": int8 (H, W), "origin", "resolution", "nodes": (n, 2), "sources": (s, 2), "points": (p, 2) world
points}. The sizes the kernels use are reach's (csrc/reach.h through csrc/width.h), which the sweeps run +-1 around:
    TILE = 32    a tile is TILE x TILE cells (kTile); its workgroup holds it with a one-cell halo
    BATCH = 16   rounds between two looks of the host at "did a tile run" (kBatch)
"""
import numpy as np

import clearance_scenes as CS

TILE, BATCH = 32, 16
ORIGIN, RES = (-1.0, -2.0), 0.25   # every cell corner and centre is an exact double
SWEEP = (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1)


def centre(x, y, origin=ORIGIN, res=RES):
    return (origin[0] + (x + 0.5) * res, origin[1] + (y + 0.5) * res)


def scene(grid, sources=(), nodes=None, points=None, origin=ORIGIN, resolution=RES, cells=True):
    """sources / nodes / points: cells (x, y) when cells, else world points. nodes None: the corner and centre cells'
    centres. points None: the nodes moved by a third of a cell, two points without a cell and two that are not finite."""
    grid = np.ascontiguousarray(grid, np.int8)
    H, W = grid.shape
    res = float(np.float32(resolution))
    to_xy = (lambda v: [centre(x, y, origin, res) for x, y in v]) if cells else (lambda v: v)
    nodes = CS.default_graph(W, H, origin, res)[0] if nodes is None else to_xy(nodes)
    nodes = np.ascontiguousarray(nodes, np.float64).reshape(-1, 2)
    if points is None:
        extra = [centre(-3, 1, origin, res), centre(W + 2, H + 2, origin, res), (np.nan, 0.0), (0.0, -np.inf)]
        points = np.concatenate([nodes + res / 3.0, np.array(extra, np.float64)])
    else:
        points = to_xy(points)
    return {"grid": grid, "origin": (float(origin[0]), float(origin[1])), "resolution": res, "nodes": nodes,
            "edges": np.zeros((0, 2), np.int32), "sources": np.array(to_xy(sources), np.float64).reshape(-1, 2),
            "points": np.ascontiguousarray(points, np.float64).reshape(-1, 2)}


def seeded(W, H, share, seed, free=()):
    g = CS.seeded(W, H, share, seed)
    for x, y in free:
        g[y, x] = 0
    return g


def corridor(W, H, rows, half):
    """Column x is free in the rows rows[x] - half[x] .. rows[x] + half[x] and occupied elsewhere."""
    g = np.full((H, W), 100, np.int8)
    for x in range(W):
        g[max(rows[x] - half[x], 0):rows[x] + half[x] + 1, x] = 0
    return g


STAIR_HALF = (3, 3, 3, 1, 1, 1, 2, 2, 2, 0, 0, 3, 3, 3)   # free rows either side of the centre row, per column


def staircase():
    """A corridor along row 4 of a 14 x 9 grid whose half width rises and falls. The centre row's cap is the least of
    (x - x')^2 + (half[x'] + 1)^2 over the columns x', by hand 13 8 5 4 4 4 5 5 2 1 1 2 5 10, and its width the running
    minimum of that from the source."""
    return corridor(len(STAIR_HALF), 9, [4] * len(STAIR_HALF), STAIR_HALF)


def neck(xn, yc, W=70, H=70, step=0):
    """A corridor seven cells wide along row yc whose columns xn and xn + 1 are one cell wide: the narrowest cell pair.
    step 1: the corridor's right part, from column xn + 1 on, lies one row lower, and the two cells (xn + 1, yc) and
    (xn, yc + 1) beside the diagonal are free, so the pair sits on the corner of four tiles when xn = yc = TILE - 1."""
    rows = [yc if x <= xn else yc + step for x in range(W)]
    half = [0 if x in (xn, xn + 1) else 3 for x in range(W)]
    g = corridor(W, H, rows, half)
    if step:
        g[yc, xn + 1] = g[yc + 1, xn] = 0
    return g


def two_routes():
    """Two rooms, the wall between them (columns 33 and 34) with a hole one cell high at row 10 and a gate nine cells
    high at rows 56 .. 64. The source sits beside the hole, so the right room first fills with the hole's cap and rises
    again when the way through the gate arrives."""
    g = np.zeros((70, 70), np.int8)
    g[:, 33:35] = 100
    g[10, 33:35] = 0
    g[56:65, 33:35] = 0
    return g


def wide_serpentine(W=70, lanes=28, hole=35):
    """Lanes three cells high (cap 4 on their centre row), a wall row between two lanes with a gate three cells wide
    alternately at its right and left end, and a hole one cell wide at column `hole` in every wall: the short way down
    through the holes has bottleneck 1, the long way along the lanes 4."""
    g = np.zeros((4 * lanes - 1, W), np.int8)
    for k in range(lanes - 1):
        y = 4 * k + 3
        g[y] = 100
        g[y, hole] = 0
        if k % 2 == 0:
            g[y, W - 3:] = 0
        else:
            g[y, :3] = 0
    return g


def corner(flip_x=False, flip_y=False, at=(5, 5), size=12):
    """a = at and b = at + (1, 1) with the obstacles (3, -1) and (-1, 3) from a: cap a = 10, cap b = 8, and the two
    cells beside the diagonal have cap 5, as every other way into b has. Only the corner rule gives width[b] = 5 from a
    source at a: without it the diagonal carries 8. Returns (grid, a, b), mirrored as asked."""
    g = np.zeros((size, size), np.int8)
    ax, ay = at
    g[ay - 1, ax + 3] = g[ay + 3, ax - 1] = 100
    a, b = (ax, ay), (ax + 1, ay + 1)
    if flip_x:
        g, a, b = g[:, ::-1], (size - 1 - a[0], a[1]), (size - 1 - b[0], b[1])
    if flip_y:
        g, a, b = g[::-1], (a[0], size - 1 - a[1]), (b[0], size - 1 - b[1])
    return np.ascontiguousarray(g), a, b


def ring():
    """A room with a block in its middle: the ways round it on either side have the same bottleneck."""
    g = np.zeros((41, 41), np.int8)
    g[0] = g[-1] = 100
    g[:, 0] = g[:, -1] = 100
    g[14:27, 14:27] = 100
    return g


def all_scenes():
    S = {}
    # sizes
    S["one_free"] = scene(np.zeros((1, 1)), [(0, 0)])
    S["one_occupied"] = scene(np.full((1, 1), 100), [(0, 0)])
    S["w70_h1"] = scene(seeded(70, 1, 0.05, 1, [(3, 0)]), [(3, 0)])
    S["w1_h70"] = scene(seeded(1, 70, 0.05, 2, [(0, 66)]), [(0, 66)])
    for n in SWEEP:
        S[f"sweep_{n}x5"] = scene(seeded(n, 5, 0.04, 100 + n, [(0, 0), (n - 1, 4)]), [(0, 0)])
        S[f"sweep_5x{n}"] = scene(seeded(5, n, 0.04, 200 + n, [(0, 0), (4, n - 1)]), [(4, n - 1)])
    for w, h in ((33, 65), (64, 31), (65, 33), (32, 32), (63, 64), (31, 63)):
        S[f"sweep_{w}x{h}"] = scene(seeded(w, h, 0.03, 300 + w, [(w - 1, h - 1), (0, 0)]), [(w - 1, h - 1), (0, 0)])
    S["wide_700x500"] = scene(seeded(700, 500, 0.02, 7, [(5, 5), (690, 490), (350, 250)]), [(5, 5), (690, 490), (350, 250)],
                              nodes=[(0, 0), (699, 499), (699, 0), (350, 100), (31, 31), (32, 32), (672, 480)])
    S["empty_70x5"] = scene(np.zeros((5, 70)), [(69, 4)])
    S["empty_65x65"] = scene(np.zeros((65, 65)), [(0, 0)])
    S["full_65x3"] = scene(np.full((3, 65), 100), [(0, 0), (64, 2)])
    g = np.array([[-128, -1, 0, 1, 99, 101, 127], [0, 0, 0, 0, 0, 0, 100], [99, 101, -100, 1, 2, 3, 4]])
    S["values"] = scene(g, [(0, 0)])
    S["no_cells_0x0"] = scene(np.zeros((0, 0)), [centre(1, 1)], nodes=[centre(1, 1), centre(2, 2)], cells=False,
                              points=[centre(0, 0), (np.nan, 1.0)])
    S["no_cells_5x0"] = scene(np.zeros((0, 5)), [centre(1, 1)], nodes=[centre(1, 1)], cells=False, points=[centre(0, 0)])
    S["no_cells_0x5"] = scene(np.zeros((5, 0)), [centre(1, 1)], nodes=[centre(1, 1)], cells=False, points=[centre(0, 0)])
    # sources
    g = seeded(70, 70, 0.02, 13, [(31, 31), (32, 32), (60, 5)])
    g[40, 40] = 100
    g[49:52, 50:53] = 100; g[50, 51] = 0   # a free cell walled in: a source of its own component
    bad = [centre(-5, -5), (np.nan, 0.0), (0.0, np.inf), centre(40, 40), centre(70, 3)]
    good = [centre(31, 31), centre(32, 32), centre(31, 31), centre(60, 5), centre(31, 31)]
    S["sources_mix"] = scene(g, good[:2] + bad[:3] + good[2:] + bad[3:], cells=False)
    S["sources_walled_in"] = scene(g, [(51, 50)], nodes=[(51, 50), (51, 49), (0, 0)])
    S["sources_none"] = scene(g, [])
    S["sources_all_dropped"] = scene(g, bad, cells=False)
    g = np.zeros((40, 66)); g[:, 30:33] = 100; g[7, 50] = g[30, 3] = 100
    S["two_components"] = scene(g, [(2, 2), (63, 37)], nodes=[(0, 0), (65, 39), (31, 20), (29, 20), (33, 20)])
    S["one_component_of_two"] = scene(g, [(63, 37)], nodes=[(0, 0), (65, 39), (31, 20), (29, 20), (33, 20)])
    # the neck: on the border between two tiles, one cell to either side of it, and on the corner of four tiles
    for xn in (TILE - 2, TILE - 1, TILE):
        S[f"neck_x{xn}"] = scene(neck(xn, 20), [(2, 20)], nodes=[(xn - 5, 20), (xn, 20), (xn + 1, 20), (xn + 6, 20), (67, 20)])
        S[f"neck_y{xn}"] = scene(neck(xn, 20).T, [(20, 2)], nodes=[(20, xn - 5), (20, xn), (20, xn + 1), (20, xn + 6), (20, 67)])
    S["neck_tile_corner"] = scene(neck(TILE - 1, TILE - 1, step=1), [(2, TILE - 1)],
                                  nodes=[(TILE - 6, TILE - 1), (TILE - 1, TILE - 1), (TILE, TILE), (TILE + 5, TILE), (67, TILE)])
    S["staircase"] = scene(staircase(), [(0, 4)], nodes=[(x, 4) for x in range(len(STAIR_HALF))])
    S["staircase_from_middle"] = scene(staircase(), [(7, 4)], nodes=[(x, 4) for x in range(len(STAIR_HALF))])
    S["two_routes"] = scene(two_routes(), [(30, 10)], nodes=[(37, 10), (60, 5), (34, 10), (34, 60), (60, 60), (2, 60)])
    S["wide_serpentine"] = scene(wide_serpentine(), [(1, 1)], nodes=[(1, 1), (35, 3), (35, 5), (1, 109), (68, 109), (35, 109)])
    for k, (fx, fy) in enumerate(((False, False), (True, False), (False, True), (True, True))):
        g, a, b = corner(fx, fy)
        S[f"corner_{k}"] = scene(g, [a], nodes=[a, b])
    g, a, b = corner(at=(TILE - 1, TILE - 1), size=70)
    S["corner_tile_corner"] = scene(g, [a], nodes=[a, b])
    S["ties"] = scene(ring(), [(7, 20)], nodes=[(33, 20), (20, 7), (20, 33), (7, 20)])
    # nodes on cell edges, at the border and outside (clearance_scenes' graph scenes)
    G = CS.graph_scenes()
    for k in ("on_cell_edges", "border_nodes", "outside_and_partly"):
        S[f"nodes_{k}"] = scene(G[k]["grid"], [centre(20, 15), centre(1, 28)], nodes=G[k]["nodes"], origin=G[k]["origin"],
                                resolution=G[k]["resolution"], cells=False, points=G[k]["nodes"] + 0.01)
    # the C0 golden skeleton, the sources its graph's nodes
    c0 = CS.c0_scene()
    S["c0"] = scene(c0["grid"], c0["nodes"], nodes=c0["nodes"], origin=c0["origin"], resolution=c0["resolution"], cells=False,
                    points=c0["nodes"][::7] + 0.3)
    return S


SMALL = 65   # the cross-check against aos_gvd_reach takes the scenes up to SMALL x SMALL, and C0
