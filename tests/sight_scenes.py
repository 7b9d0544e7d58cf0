"""Designed scenes for aos_reach_sight and aos_reach_pull, on top of reach_scenes: the smallest shapes at which their
kernels can still go wrong. The sizes the kernels use (csrc/sight.h), which the sweeps run +-1 around:
    SEGS_PER_WG = 4    segments per workgroup of the sight kernel, one wave each (kSegsPerWG)
    CANDS_PER_WG = 4   candidates per workgroup of an anchor step, one wave each (kCandsPerWG)
    PULL_BATCH = 16    anchor steps between two looks of the host at "done" (kPullBatch)
    LANES = 64         columns of the major axis a wave takes at a time

A scene is a reach_scenes scene. queries(scenes) gives, per scene name, the world segments (from_xy, to_xy) whose
sight is compared; pulls(scenes) gives the (scene name, start, max_span) whose pulled descents are compared.
"""
import numpy as np

import reach_scenes as RS
import sight_ref as G

SEGS_PER_WG, CANDS_PER_WG, PULL_BATCH, LANES = 4, 4, 16, 64
LENGTHS = (LANES - 1, LANES, LANES + 1, 2 * LANES - 1, 2 * LANES, 2 * LANES + 1)
SIGNS = ((1, 1), (-1, 1), (1, -1), (-1, -1))
BLOCKS = ("first", "last", "lane63", "lane64")
LANE_GRID, LANE_MINOR = 140, 3    # the lane scenes' grid side and their segments' minor delta


def pillar():
    """A free 24 x 12 grid with one occupied cell: along the descent from (23, 6) to (0, 0) the pillar hides three steps
    from the start and the steps behind them are visible again."""
    g = np.zeros((12, 24))
    g[5, 13] = 100
    return RS.scene(g, [(0, 0)], starts=[(23, 6)])


def lane_segments(L, along_x):
    """The four sign combinations of a segment with major delta L and minor delta LANE_MINOR: cells (a, b)."""
    out = []
    for i, (sM, sm) in enumerate(SIGNS):   # (a band of the minor axis each, so that none meets another's cell)
        M0, m0 = (5 if sM > 0 else LANE_GRID - 6), 20 + 30 * i
        a, b = (M0, m0), (M0 + sM * L, m0 + sm * LANE_MINOR)
        out.append((a, b) if along_x else (a[::-1], b[::-1]))
    return out


def lane_scene(L, along_x, block):
    """A free grid with one occupied cell on each of the four segments: in its first column, its last, or the column on
    either side of the first 64-column boundary of the walk."""
    g = np.zeros((LANE_GRID, LANE_GRID), np.int8)
    t = min(L, {"first": 0, "last": L, "lane63": LANES - 1, "lane64": LANES}[block])   # (L = 63 has no column 64)
    for a, b in lane_segments(L, along_x):
        major = 0 if along_x else 1
        col = sorted(c for c in G.touched_bbox(a, b) if abs(c[major] - a[major]) == t)
        x, y = col[0]
        g[y, x] = 100
    return RS.scene(g, [], starts=[])


def all_scenes(reach_scenes=None):
    S = dict(reach_scenes if reach_scenes is not None else RS.all_scenes())
    S["pillar"] = pillar()
    S["free_15"] = RS.scene(np.zeros((15, 15)), [(7, 7)], starts=[(0, 0)])
    S["seeded_15"] = RS.scene(RS.seeded(15, 15, 0.2, 5, [(7, 7)]), [(7, 7)], starts=[(0, 0), (14, 14)])
    # a straight corridor whose descents have lengths around the sweeps' sizes
    S["row_40"] = RS.scene(np.zeros((1, 40)), [(0, 0)], starts=[(m - 1, 0) for m in PULL_LENGTHS])
    for L in LENGTHS:
        for along_x in (True, False):
            for block in BLOCKS:
                S[f"lane_{'x' if along_x else 'y'}{L}_{block}"] = lane_scene(L, along_x, block)
    return S


# descents of these many cells: around one workgroup's candidates, and (with max_span 1, one step per cell) around
# one and two batches of steps
PULL_LENGTHS = (2, CANDS_PER_WG, CANDS_PER_WG + 1, CANDS_PER_WG + 2, PULL_BATCH, PULL_BATCH + 1, PULL_BATCH + 2,
                2 * PULL_BATCH, 2 * PULL_BATCH + 1, 2 * PULL_BATCH + 2)


def centres(sc, cells):
    return np.array([RS.centre(x, y, sc["origin"], sc["resolution"]) for x, y in cells], np.float64).reshape(-1, 2)


def queries(scenes):
    """{scene name: (from_xy, to_xy)}: every scene with cells gets seeded segments between its cells and the segments
    between its starts and its sources; the designed ones are added to theirs."""
    Q = {}

    def add(name, a, b, swap=True):
        a, b = np.asarray(a, np.float64).reshape(-1, 2), np.asarray(b, np.float64).reshape(-1, 2)
        if swap:   # both ends swapped: the answers must be equal
            a, b = np.concatenate([a, b]), np.concatenate([b, a])
        fa, fb = Q.get(name, (np.zeros((0, 2)), np.zeros((0, 2))))
        Q[name] = (np.concatenate([fa, a]), np.concatenate([fb, b]))

    for i, (name, sc) in enumerate(scenes.items()):
        H, W = sc["grid"].shape
        if W * H == 0:
            add(name, sc["nodes"], sc["nodes"][::-1])
            continue
        if name.startswith("lane_"):
            L, along_x = int(name.split("_")[1][1:]), name.split("_")[1][0] == "x"
            seg = lane_segments(L, along_x)
            add(name, centres(sc, [a for a, _ in seg]), centres(sc, [b for _, b in seg]))
            continue
        rng = np.random.default_rng(1000 + i)
        n = 24 if W * H < 100000 else 8
        a = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
        b = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
        add(name, centres(sc, a), centres(sc, b))
        if len(sc["starts"]) and len(sc["sources"]):
            add(name, sc["starts"], np.repeat(sc["sources"][:1], len(sc["starts"]), 0))
    # all 15 x 15 offsets from the centre
    for name in ("free_15", "seeded_15"):
        sc = scenes[name]
        ends = [(x, y) for y in range(15) for x in range(15)]
        add(name, centres(sc, [(7, 7)] * len(ends)), centres(sc, ends))
    # steep and shallow slopes, corner to corner
    sc = scenes["wide_700x500"]
    a = [(0, 0), (0, 499), (0, 0), (0, 0), (699, 499), (10, 0), (0, 250), (350, 0), (5, 5), (690, 490)]
    b = [(699, 499), (699, 0), (699, 1), (1, 499), (0, 498), (12, 499), (699, 251), (351, 499), (690, 490), (350, 250)]
    add("wide_700x500", centres(sc, a), centres(sc, b))
    # ends on cell edges, at the border, outside, not finite, equal; an end on an occupied cell
    sc = scenes["far_source_wins"]
    (ox, oy), r = sc["origin"], sc["resolution"]
    pts = [(ox, oy), (ox + 3 * r, oy + 4 * r), (ox + 30 * r, oy + 5 * r), (ox + 29.999 * r, oy + 19.999 * r),
           (ox - 0.5 * r, oy - 0.5 * r), (ox - 1.0 * r, oy), (ox - 5 * r, oy + 3 * r), (ox + 12 * r, oy + 25 * r),
           (np.nan, oy), (ox, np.inf), (-np.inf, np.nan), RS.centre(10, 10), RS.centre(9, 10), RS.centre(20, 3)]
    a = [p for p in pts for _ in pts]
    b = [q for _ in pts for q in pts]
    add("far_source_wins", a, b, swap=False)
    G_ = scenes["nodes_on_cell_edges"]
    add("nodes_on_cell_edges", G_["nodes"], np.roll(G_["nodes"], 1, 0))
    # the corridor: its centre line has d2 = 16 exactly
    for m in (15, 16, 17):
        sc = scenes[f"corridor_min_d2_{m}"]
        add(f"corridor_min_d2_{m}", centres(sc, [(0, 4), (0, 4), (0, 3)]), centres(sc, [(39, 4), (39, 3), (39, 3)]))
    # the diagonal between two obstacles that touch
    add("diag_touch_inside", centres(scenes["diag_touch_inside"], [(10, 11)]), centres(scenes["diag_touch_inside"], [(11, 10)]))
    return Q


def batch_sizes():
    """Segment counts around one workgroup's and two workgroups' segments."""
    return (1, SEGS_PER_WG - 1, SEGS_PER_WG, SEGS_PER_WG + 1, 2 * SEGS_PER_WG - 1, 2 * SEGS_PER_WG, 2 * SEGS_PER_WG + 1)


def pulls(scenes):
    """[(scene name, start (x, y), max_span)]: every start of every scene that has starts, at max_span 0; the pillar
    scene at 0, 1, 3 and 19; the corridor's lengths at 0 and 1."""
    P = []
    for name, sc in scenes.items():
        for s in sc["starts"]:
            P.append((name, (float(s[0]), float(s[1])), 0))
    s = scenes["pillar"]["starts"][0]
    P += [("pillar", (float(s[0]), float(s[1])), k) for k in (1, 3, 19)]
    P += [("row_40", (float(s[0]), float(s[1])), 1) for s in scenes["row_40"]["starts"]]
    P += [("hand_17", tuple(float(v) for v in scenes["hand_17"]["starts"][0]), k) for k in (15, 16, 17, 2)]
    return P
