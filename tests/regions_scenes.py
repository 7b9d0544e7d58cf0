"""Designed scenes for aos_gvd_regions: the smallest shapes at which its kernels can still go wrong.

A scene is clearance_scenes.scene's dict (grid, origin, resolution, nodes, edges) with two optional keys: "labels"
(int32 (H, W): the caller-label form) and "min_component_cells". The sizes the kernels use (csrc/field_passes.h;
kCclChunk: cluster_seed.hip), which the sweeps run +-1 around:
    BAND = 64        rows per band of the column pass (kFieldBand)
    WORKGROUP = 256  threads per workgroup (kFieldTB): columns per column-pass workgroup, cells per row-pass step
    BLOCK = 64       columns per block minimum of the row pass (kFieldBlock), and cells per packed occupancy word
    CHUNK = 2048     occupied cells per block-local labelling chunk (kCclChunk)
"""
import numpy as np

import clearance_scenes as CS
from clearance_scenes import scene

BAND, WORKGROUP, BLOCK, CHUNK = 64, 256, 64, 2048
SWEEP = (63, 64, 65, 127, 128, 129, 255, 256, 257)
ORIGIN, RES = CS.ORIGIN, CS.RES
INT32_MAX = 2 ** 31 - 1


def with_opts(sc, labels=None, min_component_cells=None):
    sc = dict(sc)
    if labels is not None:
        sc["labels"] = np.ascontiguousarray(labels, np.int32).reshape(sc["grid"].shape)
    if min_component_cells is not None:
        sc["min_component_cells"] = int(min_component_cells)
    return sc


def grid_of(W, H, cells):
    """cells: (x, y) pairs."""
    g = np.zeros((H, W), np.int8)
    for x, y in cells:
        g[y, x] = 100
    return g


def size_scenes():
    S = {}
    S["one_occupied"] = scene(np.full((1, 1), 100))
    S["one_free"] = scene(np.zeros((1, 1)))
    S["w1_h130"] = scene(grid_of(1, 130, [(0, 0), (0, 77), (0, 78), (0, 129)]))
    S["w130_h1"] = scene(grid_of(130, 1, [(3, 0), (64, 0), (129, 0)]))
    S["empty_70x5"] = scene(np.zeros((5, 70)))
    S["full_65x3"] = scene(np.full((3, 65), 100))
    # three components of 1, 2 and 3 cells, all below the filter: occupied cells, no site
    S["no_sites_after_filter"] = with_opts(scene(grid_of(20, 9, [(1, 1), (8, 2), (9, 3), (15, 6), (16, 6), (17, 7)])),
                                           min_component_cells=4)
    S["one_component"] = scene(grid_of(30, 20, [(x, 9) for x in range(5, 25)] + [(24, y) for y in range(3, 9)]))
    S["no_cells_0x0"] = scene(np.zeros((0, 0), np.int8), [CS._at(1, 1)], np.zeros((0, 2), np.int32), ORIGIN, RES)
    S["no_cells_5x0"] = scene(np.zeros((0, 5), np.int8), [CS._at(1, 1), CS._at(2, 2)], np.zeros((0, 2), np.int32), ORIGIN, RES)
    return S


def alignment_scenes():
    S = {}
    for n in SWEEP:
        S[f"sweep_{n}x5"] = scene(CS.seeded(n, 5, 0.03, 3000 + n, force=(n - 1, 4)))
        S[f"sweep_5x{n}"] = scene(CS.seeded(5, n, 0.03, 4000 + n, force=(4, n - 1)))
    S["sweep_257x129"] = scene(CS.seeded(257, 129, 0.002, 77, force=(256, 128)))
    for share in (0.001, 0.05):
        S[f"mid_700x500_{share}"] = scene(CS.seeded(700, 500, share, 7))
    return S


def tie_scenes():
    """TIES[name] = ((x, y) of the tied cell, (x, y) of the site that has to win, the tied d2)."""
    S = {}
    S["tie_row"] = scene(grid_of(11, 7, [(2, 3), (8, 3)]))
    S["tie_col_band"] = scene(grid_of(3, 130, [(1, 0), (1, 128)]))            # rows 0 and 128 about row 64: two bands
    S["tie_row_blocks"] = scene(grid_of(129, 1, [(0, 0), (128, 0)]))           # columns 0 and 128 about 64: three blocks
    S["tie_square"] = scene(grid_of(9, 9, [(2, 2), (6, 2), (2, 6), (6, 6)]))
    # (4, 4): its column's sites lie 4 up and 4 down (the upper one is the column's candidate, d2 16), column 6 has a
    # nearer one (d2 4), which wins
    S["tie_up_down_beside_nearer"] = scene(grid_of(9, 9, [(4, 0), (4, 8), (6, 4)]))
    # (1, 4): column 1's sites 3 up and 3 down (d2 9) against (4, 4) at d2 9: three candidates, the upper one wins
    S["tie_up_down_and_row"] = scene(grid_of(9, 9, [(1, 1), (1, 7), (4, 4)]))
    # (70, 30) is in block 1; (85, 50) in its own block is met first at d2 625; (63, 6), the last column of block 0, has
    # block distance 7 and column distance 24: 49 + 576 = 625, a bound that only a strict prune lets through, and the
    # smaller index
    S["tie_strict_prune_wins"] = scene(grid_of(200, 60, [(85, 50), (63, 6)]))
    # the mirror: the block that a non-strict prune would skip holds the candidate that loses ((63, 54): larger index)
    S["tie_strict_prune_loses"] = scene(grid_of(200, 60, [(85, 10), (63, 54)]))
    # (70, 30): (77, 30) in its own block at d2 49, (63, 30) in block 0 at block distance 7: the walk may end only
    # where the squared block distance is greater than the best
    S["tie_strict_walk_end"] = scene(grid_of(200, 60, [(77, 30), (63, 30)]))
    # ... and to the right: (120, 30) against (120, 38) in its own block and (128, 30), the first column of block 2
    S["tie_strict_walk_end_right"] = scene(grid_of(200, 60, [(120, 38), (128, 30)]))
    return S


TIES = {"tie_row": ((5, 3), (2, 3), 9), "tie_col_band": ((1, 64), (1, 0), 64 * 64),
        "tie_row_blocks": ((64, 0), (0, 0), 64 * 64), "tie_square": ((4, 4), (2, 2), 8),
        "tie_up_down_and_row": ((1, 4), (1, 1), 9),
        "tie_strict_prune_wins": ((70, 30), (63, 6), 625), "tie_strict_prune_loses": ((70, 30), (85, 10), 625),
        "tie_strict_walk_end": ((70, 30), (63, 30), 49), "tie_strict_walk_end_right": ((120, 30), (128, 30), 64)}


def u_shape():
    """Two arms joined at the bottom; the right arm reaches higher, so the least index is on the arm a column-wise or
    left-first walk meets second."""
    return [(2, y) for y in range(3, 9)] + [(8, y) for y in range(1, 9)] + [(x, 8) for x in range(2, 9)]


def spiral(n=15):
    """A rectangular spiral one cell wide with one free cell between its turns, inwards from the top-right corner: its
    inner end is joined to its least cell, (0, 0), only through every turn."""
    g = np.zeros((n, n), np.int8)
    dirs = ((-1, 0), (0, 1), (1, 0), (0, -1))
    x, y, d, turns = n - 1, 0, 0, 0
    g[y, x] = 100
    while turns < 2:
        dx, dy = dirs[d]
        nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        free_ahead = 0 <= nx < n and 0 <= ny < n and not g[ny, nx] and not (0 <= fx < n and 0 <= fy < n and g[fy, fx])
        if free_ahead:
            x, y, turns = nx, ny, 0
            g[y, x] = 100
        else:
            d, turns = (d + 1) % 4, turns + 1
    return g


def component_scenes():
    S = {}
    # a staircase joined only by corners, and a second one: two components of 5 and 4 cells
    S["diagonal_only"] = scene(grid_of(14, 9, [(1 + k, 1 + k) for k in range(5)] + [(12 - k, 1 + k) for k in range(4)]))
    S["u_and_dot"] = scene(grid_of(16, 11, u_shape() + [(13, 5)]))
    g = np.zeros((17, 24), np.int8)
    g[1:16, 1:16] = spiral(15)
    g[8, 21] = 100
    S["spiral_and_dot"] = scene(g)
    # one component of two 2500-cell lines joined at their right ends, and one more line: the components cross the
    # labelling's chunks of 2048 occupied cells
    cells = [(x, 1) for x in range(20, 2520)] + [(x, 3) for x in range(20, 2520)] + [(2519, 2)] + [(x, 6) for x in range(0, 2600)]
    S["lines_over_chunks"] = scene(grid_of(2600, 8, cells))
    # components of 4 and 9 cells: the filter at size - 1, size, size + 1 of the smaller one
    cells = [(2, 2), (3, 2), (2, 3), (3, 3)] + [(10 + i, 5 + j) for i in range(3) for j in range(3)]
    for m in (3, 4, 5):
        S[f"filter_min_{m}"] = with_opts(scene(grid_of(18, 12, cells)), min_component_cells=m)
    S["filter_min_1"] = with_opts(scene(grid_of(18, 12, cells)), min_component_cells=1)
    S["filter_negative"] = with_opts(scene(grid_of(18, 12, cells)), min_component_cells=-7)
    return S


def label_scenes():
    S = {}
    rng = np.random.default_rng(21)
    # four blobs: A and B share a label, C is split into two labels on 4-adjacent cells, D is negative (no site);
    # free cells carry arbitrary labels, which must not be read
    cells = {"A": [(2, 2), (3, 2), (3, 3)], "B": [(20, 9), (21, 9)], "C": [(10, 5), (11, 5), (10, 6), (11, 6)], "D": [(15, 2), (16, 3)]}
    g = grid_of(26, 13, sum(cells.values(), []))
    lab = rng.integers(-5, 50, g.shape).astype(np.int32)
    for x, y in cells["A"] + cells["B"]:
        lab[y, x] = 7
    for x, y in cells["C"]:
        lab[y, x] = 3 if x == 10 else INT32_MAX
    for x, y in cells["D"]:
        lab[y, x] = -1 if x == 15 else -(2 ** 31)
    S["labels_mixed"] = with_opts(scene(g), labels=lab)
    S["labels_all_negative"] = with_opts(scene(g), labels=np.full(g.shape, -3))
    S["labels_zero_everywhere"] = with_opts(scene(g), labels=np.zeros(g.shape))
    S["labels_no_cells_0x0"] = with_opts(scene(np.zeros((0, 0), np.int8), [CS._at(1, 1)], np.zeros((0, 2), np.int32), ORIGIN, RES),
                                         labels=np.zeros((0, 0)))
    g = CS.seeded(130, 67, 0.02, 5)
    S["labels_random_130x67"] = with_opts(scene(g), labels=rng.integers(-2, 6, g.shape))
    return S


def wall_scenes():
    S = {}
    # vertical walls at x = 2, 7, 13, 15: four free columns (even), five (odd), and a single one, which is marked
    g = np.zeros((12, 19), np.int8)
    g[:, [2, 7, 13, 15]] = 100
    S["walls_vertical"] = scene(g)
    S["walls_horizontal"] = scene(np.ascontiguousarray(g.T))
    return S


def graph_scenes():
    """Nodes on cell edges, outside the grid and on ridge cells, against the vertical walls (exact corners)."""
    g = np.zeros((12, 19), np.int8)
    g[:, [2, 7, 13, 15]] = 100
    W, H = 19, 12
    just_under = (np.nextafter(ORIGIN[0] + W * RES, -np.inf), np.nextafter(ORIGIN[1] + H * RES, -np.inf))
    at = CS._at
    nodes = [at(7, 2), at(7.0, 5.0), at(3, 5), at(13, 0),                         # on cell edges and corners
             at(-0.5, 3), at(-1.0, 3), at(W, 3), at(5, -1.0), at(5, H), just_under, at(-20, -20), at(60, 45),
             at(14.5, 0.5), at(14.5, 6.5), at(14.0, 11.0), at(4.5, 3.5), at(5.5, 3.5), at(10.5, 7.5),   # ridge cells, but (5, 3)
             at(2.5, 2.5), at(15.5, 11.5)]                                        # site cells
    S = {"graph_nodes": scene(g, nodes, np.zeros((0, 2), np.int32), ORIGIN, RES),
         "graph_none": scene(g, np.zeros((0, 2)), np.zeros((0, 2), np.int32), ORIGIN, RES)}
    rng = np.random.default_rng(8)
    for n in (WORKGROUP - 1, WORKGROUP, WORKGROUP + 1):
        pts = np.stack([rng.uniform(-1.5, 4.5, n), rng.uniform(-2.5, 1.5, n)], 1)
        S[f"graph_{n}_nodes"] = scene(g, pts, np.zeros((0, 2), np.int32), ORIGIN, RES)
    return S


def all_scenes():
    S = {}
    for part in (size_scenes, alignment_scenes, tie_scenes, component_scenes, label_scenes, wall_scenes, graph_scenes):
        S.update(part())
    S["c0"] = CS.c0_scene()
    return S
