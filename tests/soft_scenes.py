"""Designed scenes for aos_gvd_soft: the smallest shapes at which its kernels can still go wrong.

A scene is reach_scenes' ({"grid", "origin", "resolution", "nodes", "sources", "min_d2", "starts"}) with "soft_cells" and
"gain"; "big" marks the one scene whose reference comes from scipy alone. The sizes the kernels use are reach's
(csrc/reach.h through csrc/soft.h), which the sweeps run +-1 around:
    TILE = 32    a tile is TILE x TILE cells (kTile); its workgroup holds it with a one-cell halo
    BATCH = 16   rounds between two looks of the host at "did a tile run" (kBatch)
"""
import numpy as np

import reach_scenes as RS
import width_scenes as WS

TILE, BATCH = RS.TILE, RS.BATCH
SWEEP = RS.SWEEP
centre = RS.centre


def scene(grid, sources=(), soft_cells=0, gain=0, min_d2=0, big=False, **kw):
    sc = RS.scene(grid, sources, min_d2, **kw)
    sc.update(soft_cells=int(soft_cells), gain=int(gain), big=bool(big))
    return sc


def soften(sc, soft_cells, gain, min_d2=None):
    """A reach scene with soft options."""
    out = dict(sc, soft_cells=int(soft_cells), gain=int(gain), big=False)
    if min_d2 is not None:
        out["min_d2"] = int(min_d2)
    return out


def wall_with_door(xw, W=70, H=40, door=(18, 21)):
    """A wall along column xw with a door: with soft_cells = 4 the weighted band is the three columns either side."""
    g = np.zeros((H, W), np.int8)
    g[:, xw] = 100
    g[door[0]:door[1], xw] = 0
    return g


def corridor(k, L):
    """Columns 1 .. 2k + 1 free between the walls in columns 0 and 2k + 2, L rows long."""
    g = np.zeros((L, 2 * k + 3), np.int8)
    g[:, 0] = g[:, -1] = 100
    return g


def side_only(flip_x=False, flip_y=False, at=(5, 5), size=12):
    """a = at, b = at + (1, 1); the one occupied cell (2, -1) from a is an 8-neighbour of the side cell (1, 0) alone, so
    with soft_cells = 2 that side cell is the only weighted one of the four the diagonal touches. Returns (grid, a, b),
    mirrored as asked."""
    g = np.zeros((size, size), np.int8)
    ax, ay = at
    g[ay - 1, ax + 2] = 100
    a, b = (ax, ay), (ax + 1, ay + 1)
    if flip_x:
        g, a, b = g[:, ::-1], (size - 1 - a[0], a[1]), (size - 1 - b[0], b[1])
    if flip_y:
        g, a, b = g[::-1], (a[0], size - 1 - a[1]), (b[0], size - 1 - b[1])
    return np.ascontiguousarray(g), a, b


# the 2^31 bound: 7 * 255 * n_passable is below 2^31 up to n_passable = 1 203 072 and reaches it with one cell more
BOUND_W, BOUND_H = 256, 4700
BOUND_LAST = ((1 << 31) - 1) // (7 * 255)
TWO_WAYS_GAINS = (2, 50)


def bound_grid(n_passable):
    g = np.zeros((BOUND_H, BOUND_W), np.int8)
    n_occ = BOUND_W * BOUND_H - n_passable
    assert 0 < n_occ <= BOUND_W
    g[0, :n_occ] = 100
    return g


def all_scenes():
    S = {}
    R = RS.all_scenes()
    # sizes
    S["one_free"] = scene(np.zeros((1, 1)), [(0, 0)], 4, 3)
    S["one_occupied"] = scene(np.full((1, 1), 100), [(0, 0)], 4, 3)
    for n in SWEEP:
        S[f"sweep_{n}x5"] = scene(RS.seeded(n, 5, 0.04, 100 + n, [(0, 0), (n - 1, 4)]), [(0, 0)], 3, 2)
        S[f"sweep_5x{n}"] = scene(RS.seeded(5, n, 0.04, 200 + n, [(0, 0), (4, n - 1)]), [(4, n - 1)], 3, 2)
    for w, h in ((33, 65), (64, 31), (65, 33), (32, 32), (63, 64), (31, 63)):
        S[f"sweep_{w}x{h}"] = scene(RS.seeded(w, h, 0.03, 300 + w, [(w - 1, h - 1), (0, 0)]), [(w - 1, h - 1)], 4, 3)
    S["wide_700x500"] = scene(RS.seeded(700, 500, 0.02, 7, [(5, 5), (690, 490), (350, 250)]), [(5, 5), (690, 490), (350, 250)],
                              5, 2, starts=[(0, 0), (699, 499), (699, 0), (350, 100)])
    # empty and full grids, every byte value, no cells, and every source case of the reach scenes
    for k in ("empty_70x5", "full_65x3", "values", "no_cells_0x0", "no_cells_5x0", "sources_mix", "sources_none",
              "sources_all_dropped", "far_source_wins", "one_room_of_two", "notch", "diag_touch_tile_corner",
              "nodes_on_cell_edges", "nodes_border_nodes", "nodes_outside_and_partly"):
        S[k] = soften(R[k], 4, 3)
    S["sources_mix_hard_only"] = soften(R["sources_mix"], 0, 0)
    for m in (15, 16, 17):
        S[f"corridor_min_d2_{m}"] = soften(R[f"corridor_min_d2_{m}"], 6, 2)
    # the weighted band (soft_cells 4: three columns beside the wall) across, at and off the border between two tiles
    for xw in (TILE - 4, TILE - 3, TILE - 2, TILE - 1):
        g = wall_with_door(xw)
        S[f"band_x{xw}"] = scene(g, [(xw + 12, 5)], 4, 3, starts=[(2, 35), (xw + 1, 30), (xw + 3, 2), (xw - 1, 19)])
        S[f"band_y{xw}"] = scene(g.T, [(5, xw + 12)], 4, 3, starts=[(35, 2), (30, xw + 1), (2, xw + 3), (19, xw - 1)])
    # a weight step on the corner shared by four tiles: one occupied cell two cells off the corner, in each quadrant
    for k, (ox, oy) in enumerate(((TILE - 3, TILE - 3), (TILE + 2, TILE - 3), (TILE - 3, TILE + 2), (TILE + 2, TILE + 2))):
        g = np.zeros((70, 70), np.int8)
        g[oy, ox] = 100
        sx, sy = (1 if ox < TILE else -1), (1 if oy < TILE else -1)   # from the occupied cell towards the corner
        far = (TILE + 20 * sx, TILE + 20 * sy)                        # the source lies across the corner from it
        S[f"corner_step_{k}"] = scene(g, [far], 4, 5, starts=[(ox + sx, oy + sy), (ox - sx, oy - sy), (ox, oy + 3 * sy),
                                                              (TILE - 25 * sx, TILE - 25 * sy)])
    # corridors of odd width: the descent steps to the centre column and stays there
    S["corridor_3"] = scene(corridor(1, 30), [(1, 29)], 2, 2, starts=[(1, 0)])
    S["corridor_7"] = scene(corridor(3, 40), [(1, 39)], 4, 1, starts=[(1, 0)])
    # two ways into one room: the hole one cell high beside the source, the gate nine cells high far away
    for gain in TWO_WAYS_GAINS:
        S[f"two_ways_gain_{gain}"] = scene(WS.two_routes(), [(30, 10)], 5, gain, starts=[(37, 10), (60, 60), (2, 60)])
    # diagonals whose side cell alone carries weight
    for k, (fx, fy) in enumerate(((False, False), (True, False), (False, True), (True, True))):
        g, a, b = side_only(fx, fy)
        S[f"side_only_{k}"] = scene(g, [a], 2, 3, starts=[b])
    g, a, b = side_only(at=(TILE - 1, TILE - 1), size=70)
    S["side_only_tile_corner"] = scene(g, [a], 2, 3, starts=[b])
    # ties
    for k in range(8):
        S[f"tie_{k}"] = soften(R[f"tie_{k}"], 3, 2)
    S["ties_ring"] = scene(WS.ring(), [(7, 20)], 4, 2, starts=[(33, 20), (20, 7), (20, 33)])
    # the largest weights
    g = RS.seeded(40, 30, 0.03, 11, [(1, 1)])
    S["weight_254"] = scene(g, [(1, 1)], 2, 253)
    S["weight_255"] = scene(g, [(1, 1)], 2, 254)
    S["weight_255_wide"] = scene(g, [(1, 1)], 255, 1)
    S["weight_127_steps"] = scene(g, [(1, 1)], 3, 127)
    # the 2^31 bound, met from below
    S["bound_last"] = scene(bound_grid(BOUND_LAST), [(BOUND_W - 1, BOUND_H - 1), (BOUND_W // 2, 2000), (3, 40)], 255, 1, big=True,
                            nodes=[centre(0, 1), centre(BOUND_W - 1, 0), centre(200, 4000)], cells=True,
                            starts=[(0, 1), (130, 0), (10, 3000)])
    # rounds: reach's serpentine, every lane one cell wide, so every passable cell has the weight 1 + 2 * 3
    S["serpentine"] = soften(R["serpentine"], 4, 2)
    # rounds with a band that is not uniform: width's serpentine of lanes three cells high with its holes closed, so the
    # one way runs along every lane; a lane's centre row weighs 3 and its side rows 5
    g = WS.wide_serpentine()
    g[3::4, 35] = 100
    S["serpentine_band"] = scene(g, [(1, 1)], 3, 2, starts=[(1, 109), (68, 109), (35, 57)])
    # the C0 golden skeleton, the sources its graph's nodes
    for m in (0, 16):
        S[f"c0_min_d2_{m}"] = soften(R["c0_min_d2_0"], 10, 2, m)
    return S


def refused_scenes():
    """Scenes the library must refuse with AOS_E_INVALID: {"name": (scene, a word of the message)}."""
    g = np.zeros((3, 4), np.int8)
    out = {"weight_256": (scene(g, [(0, 0)], 4, 85), "255"), "weight_257": (scene(g, [(0, 0)], 3, 128), "255"),
           "soft_cells_256": (scene(g, [(0, 0)], 256, 0), "soft_cells"), "soft_cells_negative": (scene(g, [(0, 0)], -1, 0), "soft_cells"),
           "gain_255": (scene(g, [(0, 0)], 0, 255), "gain"), "gain_negative": (scene(g, [(0, 0)], 2, -1), "gain")}
    out["bound_first"] = (scene(bound_grid(BOUND_LAST + 1), [(BOUND_W - 1, BOUND_H - 1)], 255, 1, big=True,
                                nodes=[centre(0, 1)], cells=True, starts=[(0, 1)]), "n_passable 1203073")
    return out
