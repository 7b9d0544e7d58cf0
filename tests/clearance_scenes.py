"""Designed scenes for aos_gvd_clearance: the smallest shapes at which its kernels can still go wrong.

A scene is {"grid": int8 (H, W), "origin": (x, y), "resolution": float, "nodes": (n, 2) float64, "edges": (m, 2) int32}.
Field scenes carry a small default graph (the corner and centre cells, joined), graph scenes a graph built for one rule
of the sampler each. The sizes the kernels use (csrc/field_passes.h; kClrPer: clearance.hip), which the sweeps
run +-1 around:
    BAND = 64        rows per band of the column pass (kFieldBand)
    WORKGROUP = 256  threads per workgroup: columns per column-pass workgroup, cells per row-pass step, nodes or edges
                     per sampling workgroup (kFieldTB)
    BLOCK = 64       columns per block minimum of the row pass (kFieldBlock)
    ROUND = 2048     samples a sampling workgroup takes per round (kFieldTB * kClrPer)
"""
import json
import os

import numpy as np

BAND, WORKGROUP, BLOCK, ROUND = 64, 256, 64, 2048
SWEEP = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ORIGIN, RES = (-1.0, -2.0), 0.25   # graph scenes: every cell corner is an exact double


def default_graph(W, H, origin, res):
    """Nodes at the centres of the corner cells and the middle cell, joined corner to corner through the middle."""
    if W * H == 0:
        return np.zeros((0, 2)), np.zeros((0, 2), np.int32)
    cells = [(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1), (W // 2, H // 2)]
    nodes = np.array([(origin[0] + (x + 0.5) * res, origin[1] + (y + 0.5) * res) for x, y in cells], np.float64)
    edges = np.array([(0, 4), (4, 2), (1, 4), (4, 3), (0, 1), (3, 2)], np.int32)
    return nodes, edges


def scene(grid, nodes=None, edges=None, origin=(3.5, -7.25), resolution=0.05):
    grid = np.ascontiguousarray(grid, np.int8)
    H, W = grid.shape
    if nodes is None:
        nodes, edges = default_graph(W, H, origin, float(np.float32(resolution)))
    return {"grid": grid, "origin": (float(origin[0]), float(origin[1])), "resolution": float(np.float32(resolution)),
            "nodes": np.ascontiguousarray(nodes, np.float64).reshape(-1, 2),
            "edges": np.ascontiguousarray(edges, np.int32).reshape(-1, 2)}


def seeded(W, H, share, seed, force=None):
    rng = np.random.default_rng(seed)
    g = np.where(rng.random((H, W)) < share, 100, 0).astype(np.int8)
    if force is not None:
        g[force[1], force[0]] = 100
    return g


def c0_scene():
    g = np.load(os.path.join(GOLDEN, "c0_gvd.npz"))
    s = np.load(os.path.join(GOLDEN, "c0_seedgen.npz"))
    meta = json.loads(str(s["meta"]))
    W, H = meta["width"], meta["height"]
    sk = (np.unpackbits(s["grid_skeleton_framed"])[: W * H].astype(np.int8) * 100).reshape(H, W)
    return scene(sk, g["nodes"], g["edges"], tuple(float(v) for v in s["origin"]), float(s["resolution"]))


def field_scenes():
    S = {}
    S["one_occupied"] = scene(np.full((1, 1), 100))
    S["one_free"] = scene(np.zeros((1, 1)))
    g = np.zeros((130, 1)); g[[0, 77], 0] = 100
    S["w1_h130"] = scene(g)
    g = np.zeros((1, 130)); g[0, [3, 129]] = 100
    S["w130_h1"] = scene(g)
    S["empty_70x5"] = scene(np.zeros((5, 70)))
    S["full_65x3"] = scene(np.full((3, 65), 100))
    g = np.array([[-128, -1, 0, 1, 99, 101, 127], [0, 0, 0, 0, 0, 0, 100], [99, 101, -100, 1, 2, 3, 4]])
    S["values"] = scene(g)
    g = np.zeros((200, 300)); g[0, 0] = 100
    S["corner_300x200"] = scene(g)
    g = np.zeros((200, 300)); g[199, 299] = 100
    S["far_corner_300x200"] = scene(g)
    g = np.zeros((11, 130))
    for row, col in zip((0, 2, 4, 6, 8), (63, 64, 127, 128, 129)):
        g[row, col] = 100
    S["block_edges_130"] = scene(g)
    # (4, 4): its column's nearest occupied cell is 6 rows up (d2 36) and its row has none, but (1, 2) is nearer (13)
    g = np.zeros((12, 9)); g[10, 4] = 100; g[2, 1] = 100
    S["diagonal_wins"] = scene(g)
    g = np.zeros((9, 9)); g[4, 0] = g[4, 8] = g[0, 4] = g[8, 4] = 100   # (4, 4) is 16 from all four
    S["ties"] = scene(g)
    for n in SWEEP:
        S[f"sweep_{n}x5"] = scene(seeded(n, 5, 0.01, 1000 + n, force=(n - 1, 4)))
        S[f"sweep_5x{n}"] = scene(seeded(5, n, 0.01, 2000 + n, force=(4, n - 1)))
    for share in (0.001, 0.05, 0.6):
        S[f"mid_700x500_{share}"] = scene(seeded(700, 500, share, 7))
    S["c0"] = c0_scene()
    return S


def graph_grid(W=40, H=30):
    g = seeded(W, H, 0.03, 11)
    g[0, 0] = g[H - 1, W - 1] = 100
    return g


def _at(fx, fy):
    """The world point at cell coordinates (fx, fy) of the graph scenes' grid (exact for multiples of 1 / 64)."""
    return (ORIGIN[0] + fx * RES, ORIGIN[1] + fy * RES)


def graph_scenes():
    S = {}
    G = graph_grid()
    W, H = 40, 30
    gs = lambda nodes, edges, grid=G: scene(grid, nodes, edges, ORIGIN, RES)  # noqa: E731
    # a vertical edge on the grid line x = 7 cells and a horizontal one on y = 5: every sample has an integral fx / fy
    S["on_cell_edges"] = gs([_at(7, 2), _at(7, 20), _at(3, 5), _at(33, 5)], [(0, 1), (2, 3), (0, 3)])
    just_under = (np.nextafter(ORIGIN[0] + W * RES, -np.inf), np.nextafter(ORIGIN[1] + H * RES, -np.inf))
    S["border_nodes"] = gs([_at(-0.5, 3), _at(-1.0, 3), _at(W, 3), (just_under[0], _at(0, 3)[1]), _at(5, -0.5), _at(5, -1.0),
                            _at(5, H), (_at(5, 0)[0], just_under[1]), _at(-0.5, -0.5), just_under],
                           [(0, 3), (1, 2), (4, 7), (5, 6), (8, 9)])
    S["outside_and_partly"] = gs([_at(-20, -20), _at(-3, -9), _at(-10, 12), _at(15, 12), _at(60, 45), _at(20, 10)],
                                 [(0, 1), (2, 3), (5, 4), (0, 4)])
    S["long_1e4m"] = gs([(-5000.0, 0.5), (5000.0, 3.0), (2.0, -5000.0), (2.5, 5000.0)], [(0, 1), (2, 3), (1, 2)])
    S["overflow_1e9m"] = scene(G, [(-5e8, 0.3), (5e8, 0.4), (0.2, 0.2), (1.0, 1.0)], [(0, 1), (2, 3), (2, 1)],
                                 (-0.5, -0.25), 0.05)
    S["zero_and_self"] = gs([_at(9.5, 9.5), _at(9.5, 9.5), _at(12.25, 3.75), _at(-7, -7)],
                            [(0, 1), (2, 2), (3, 3), (1, 0), (0, 2)])
    S["no_graph"] = gs(np.zeros((0, 2)), np.zeros((0, 2), np.int32))
    S["nodes_only"] = gs([_at(1.5, 1.5), _at(38.5, 28.5)], np.zeros((0, 2), np.int32))
    S["one_edge"] = gs([_at(1.5, 1.5), _at(38.5, 28.5)], [(0, 1)])
    rng = np.random.default_rng(5)
    for ne in (WORKGROUP - 1, WORKGROUP, WORKGROUP + 1):
        nodes = np.stack([rng.uniform(-2.0, 10.0, ne + 1), rng.uniform(-3.0, 6.5, ne + 1)], 1)
        S[f"edges_{ne}"] = gs(nodes, np.stack([np.arange(ne), np.arange(1, ne + 1)], 1))
    # 255 edges of about 0.1 m and one across the whole of a 1200 x 40 field (about 2400 samples, more than ROUND) in
    # one workgroup: the long edge's samples are spread over every thread and take a second round
    big = seeded(1200, 40, 0.004, 9)
    base = np.stack([rng.uniform(-1.0, 299.0, 255), rng.uniform(-2.0, 8.0, 255)], 1)
    nodes = np.concatenate([base, base + rng.uniform(-0.1, 0.1, (255, 2)), [(-3.0, -4.0), (302.0, 11.0)]])
    edges = np.concatenate([np.stack([np.arange(255), np.arange(255, 510)], 1), [(510, 511)]])
    order = rng.permutation(256)
    S["short_255_long_1"] = scene(big, nodes, edges[order], ORIGIN, RES)
    S["no_cells_0x0"] = gs([_at(1, 1), _at(2, 2)], [(0, 1)], np.zeros((0, 0), np.int8))
    S["no_cells_5x0"] = gs([_at(1, 1), _at(2, 2)], [(0, 1), (1, 1)], np.zeros((0, 5), np.int8))
    return S


def all_scenes():
    return {**field_scenes(), **graph_scenes()}
