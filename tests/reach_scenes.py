"""Designed scenes for aos_gvd_reach: the smallest shapes at which its kernels can still go wrong.

A scene is {"grid": int8 (H, W), "origin", "resolution", "nodes": (n, 2), "sources": (s, 2) world points, "min_d2": int,
"starts": (k, 2) world points whose descents are compared}. The sizes the kernels use (csrc/reach.h), which the sweeps
run +-1 around:
    TILE = 32    a tile is TILE x TILE cells (kTile); its workgroup holds it with a one-cell halo
    BATCH = 16   rounds between two looks of the host at "did a tile run" (kBatch)
"""
import numpy as np

import clearance_scenes as CS
import reach_ref as R

TILE, BATCH = 32, 16
ORIGIN, RES = (-1.0, -2.0), 0.25   # every cell corner and centre is an exact double
SWEEP = (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1)


def centre(x, y, origin=ORIGIN, res=RES):
    return (origin[0] + (x + 0.5) * res, origin[1] + (y + 0.5) * res)


def scene(grid, sources=(), min_d2=0, nodes=None, starts=None, origin=ORIGIN, resolution=RES, cells=True):
    """sources / starts: cells (x, y) when cells, else world points. nodes None: the corner and centre cells' centres;
    starts None: the nodes."""
    grid = np.ascontiguousarray(grid, np.int8)
    H, W = grid.shape
    res = float(np.float32(resolution))
    to_xy = (lambda v: [centre(x, y, origin, res) for x, y in v]) if cells else (lambda v: v)
    if nodes is None:
        nodes = CS.default_graph(W, H, origin, res)[0]
    nodes = np.ascontiguousarray(nodes, np.float64).reshape(-1, 2)
    starts = nodes if starts is None else np.array(to_xy(starts), np.float64).reshape(-1, 2)
    return {"grid": grid, "origin": (float(origin[0]), float(origin[1])), "resolution": res, "nodes": nodes,
            "edges": np.zeros((0, 2), np.int32), "sources": np.array(to_xy(sources), np.float64).reshape(-1, 2),
            "min_d2": int(min_d2), "starts": np.ascontiguousarray(starts, np.float64)}


def seeded(W, H, share, seed, free=()):
    g = CS.seeded(W, H, share, seed)
    for x, y in free:
        g[y, x] = 0
    return g


def serpentine(W, H, x0=0):
    """Odd rows occupied in columns [x0, W) except alternately column W - 1, then column x0; columns below x0 occupied."""
    g = np.zeros((H, W), np.int8)
    g[:, :x0] = 100
    for k, y in enumerate(range(1, H, 2)):
        g[y, x0:] = 100
        g[y, W - 1 if k % 2 == 0 else x0] = 0
    return g


def spiral(n):
    """A one-cell corridor winding inwards from (0, 0), one wall cell between its turns."""
    g = np.full((n, n), 100, np.int8)
    x = y = 0
    g[0, 0] = 0
    runs = [n - 1, n - 1, n - 1] + [v for L in range(n - 3, 0, -2) for v in (L, L)]
    for k, L in enumerate(runs):
        dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[k % 4]
        for _ in range(L):
            x, y = x + dx, y + dy
            g[y, x] = 0
    return g, (x, y)


def tie_scene(k):
    """A free 5 x 5 grid, the start at its centre, sources on the centre's neighbours k .. of the same kind (axis or
    diagonal) in the descent's order: they tie, and neighbour k is the first admissible."""
    hi = 4 if k < 4 else 8
    return scene(np.zeros((5, 5)), [(2 + dx, 2 + dy) for dx, dy in R.MOVES[k:hi]], starts=[(2, 2)])


def all_scenes():
    S = {}
    # the hand answers
    S["hand_3x3"] = scene(np.zeros((3, 3)), [(0, 0)])
    g = np.zeros((2, 2)); g[0, 1] = 100
    S["hand_2x2"] = scene(g, [(0, 0)])
    S["hand_17"] = scene(serpentine(17, 17), [(0, 0)], starts=[(16, 16), (0, 0), (16, 0)])
    # sizes
    S["one_free"] = scene(np.zeros((1, 1)), [(0, 0)])
    S["one_occupied"] = scene(np.full((1, 1), 100), [(0, 0)])
    S["w70_h1"] = scene(seeded(70, 1, 0.0, 1), [(3, 0)])
    S["w1_h70"] = scene(seeded(1, 70, 0.0, 1), [(0, 66)])
    for n in SWEEP:
        S[f"sweep_{n}x5"] = scene(seeded(n, 5, 0.2, 100 + n, [(0, 0), (n - 1, 4)]), [(0, 0)])
        S[f"sweep_5x{n}"] = scene(seeded(5, n, 0.2, 200 + n, [(0, 0), (4, n - 1)]), [(4, n - 1)])
    for w, h in ((33, 65), (64, 31), (65, 33), (32, 32), (63, 64)):
        S[f"sweep_{w}x{h}"] = scene(seeded(w, h, 0.25, 300 + w, [(w - 1, h - 1)]), [(w - 1, h - 1)])
    S["wide_700x500"] = scene(seeded(700, 500, 0.3, 7, [(5, 5), (690, 490), (350, 250)]), [(5, 5), (690, 490), (350, 250)],
                              starts=[(0, 0), (699, 499), (699, 0), (350, 100)])
    S["empty_70x5"] = scene(np.zeros((5, 70)), [(69, 4)])
    S["full_65x3"] = scene(np.full((3, 65), 100), [(0, 0), (64, 2)])
    g = np.array([[-128, -1, 0, 1, 99, 101, 127], [0, 0, 0, 0, 0, 0, 100], [99, 101, -100, 1, 2, 3, 4]])
    S["values"] = scene(g, [(0, 0)])
    # the corner rule
    g = np.zeros((40, 40)); g[10, 10] = g[11, 11] = 100
    S["diag_touch_inside"] = scene(g, [(10, 11)], starts=[(11, 10)])
    g = np.zeros((70, 70)); g[TILE - 1, TILE - 1] = g[TILE, TILE] = 100
    S["diag_touch_tile_corner"] = scene(g, [(TILE - 1, TILE)], starts=[(TILE, TILE - 1)])
    yy, xx = np.mgrid[0:9, 0:9]
    S["checkerboard"] = scene(np.where((xx + yy) % 2 == 1, 100, 0), [(0, 0), (4, 4)])
    g = np.zeros((12, 12)); g[5] = g[6] = 100; g[5, 6] = g[6, 7] = 0
    S["notch"] = scene(g, [(6, 0)], starts=[(6, 5), (7, 6), (6, 11)])
    # thresholds: rows 0 and 8 are walls, so the centre line y = 4 has d2 = 16 exactly and row 3 has 9
    g = np.zeros((9, 40)); g[0] = g[8] = 100
    for m in (15, 16, 17):
        S[f"corridor_min_d2_{m}"] = scene(g, [(0, 4), (5, 3)], m, starts=[(39, 4), (39, 3)])
    for m in (0, 1, 2):
        S[f"min_d2_{m}"] = scene(seeded(40, 30, 0.03, 11, [(1, 1)]), [(1, 1)], m)
    # long wavefronts
    S["serpentine"] = scene(serpentine(70, 61), [(0, 0)], starts=[(0, 60), (69, 60)])
    S["reenter"] = scene(serpentine(40, 31, 24), [(24, 0)], starts=[(24, 30), (39, 30)])
    g, end = spiral(41)
    S["spiral"] = scene(g, [(0, 0)], starts=[end])
    # a wall across: (11, 10) is two cells from the source at (9, 10) and is reached from (29, 10) alone
    g = np.zeros((20, 30)); g[:, 10] = 100
    S["far_source_wins"] = scene(g, [(9, 10), (29, 10)], starts=[(11, 10), (0, 0)])
    S["one_room_of_two"] = scene(g, [(29, 10)], starts=[(11, 10), (0, 0), (10, 10)])
    S["diagonals_20"] = scene(np.zeros((20, 20)), [(0, 0)], starts=[(19, 19), (19, 7), (7, 19), (0, 19)])
    # sources
    g = seeded(70, 70, 0.1, 13)
    for x, y in ((31, 31), (32, 32), (60, 5)):   # the good sources keep d2 >= 2
        g[y - 1:y + 2, x - 1:x + 2] = 0
    g[40, 40] = 100; g[50, 50:53] = 0; g[49, 51] = 100; g[48, 50:53] = g[49, 50] = g[49, 52] = 0
    bad = [centre(-5, -5), (np.nan, 0.0), (0.0, np.inf), centre(40, 40), centre(51, 50), centre(70, 3)]
    good = [centre(31, 31), centre(32, 32), centre(31, 31), centre(60, 5), centre(31, 31)]
    S["sources_mix"] = scene(g, good[:2] + bad[:3] + good[2:] + bad[3:], 2, cells=False)
    S["sources_none"] = scene(g, [], 2)
    S["sources_all_dropped"] = scene(g, bad, 2, cells=False)
    for k in range(8):
        S[f"tie_{k}"] = tie_scene(k)
    # nodes on cell edges, at the border and outside (clearance_scenes' graph scenes), starts without a cell
    G = CS.graph_scenes()
    for k in ("on_cell_edges", "border_nodes", "outside_and_partly"):
        S[f"nodes_{k}"] = scene(G[k]["grid"], [(20, 15), (1, 28)], nodes=G[k]["nodes"], origin=G[k]["origin"],
                                resolution=G[k]["resolution"])
    S["no_cells_0x0"] = scene(np.zeros((0, 0)), [centre(1, 1)], nodes=[centre(1, 1), centre(2, 2)], cells=False)
    S["no_cells_5x0"] = scene(np.zeros((0, 5)), [centre(1, 1)], 4, nodes=[centre(1, 1)], cells=False)
    # the C0 golden skeleton, the sources its graph's nodes: every free cell, and a robot that keeps nine cells away,
    # for which most nodes and some pockets of free space are out of reach
    c0 = CS.c0_scene()
    starts = [centre(x, y, c0["origin"], c0["resolution"]) for x, y in C0_STARTS]
    for m in (0, C0_MIN_D2):
        S[f"c0_min_d2_{m}"] = scene(c0["grid"], c0["nodes"], m, nodes=c0["nodes"], starts=starts, origin=c0["origin"],
                                    resolution=c0["resolution"], cells=False)
    return S


C0_MIN_D2 = 81
C0_STARTS = [(5, 5), (506, 506), (256, 256), (253, 110), (100, 400)]
