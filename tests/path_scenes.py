"""Designed graphs, grids and queries for aos_path_plan (csrc/path.hip): k_trim_check, k_nearest_k and the host
planner around them. A scene is (name, family, graph, grid, query, regime); regime holds the facts the scene was built
for, which test_path_scenes_cpu.py asserts on the oracle and on the restatement (path_ref) without a GPU, so a scene
that drifts out of its regime fails there. test_gpu_path_scenes.py runs every scene through the library, bit for bit
against the oracle.

How a scene controls what the kernels see:
  trim     the poses are the nodes of a chain graph (edge lengths 0, BR on the first node, BL on the last, query
           target=1, previous=0: the path starts on node 0 and visits every node), or the initial straight line;
  nearest  the robot stands at P among isolated far nodes; only chosen near nodes have an edge to the goal G, so the
           node path names the candidate that won.

Regimes the planner cannot be brought into, and why no scene has them:
  * a sample offset whose distance is exactly 0.2 (`>=` for `>`), a rounded dx * res (a fused x + dx * res), and
    rc = round(0.2 / res): the resolution is a float32, so dx * res is exact in double and no product of it with an
    integer's root is 0.2 (test_path_scenes_cpu.py searches), and every offset within 0.2 m lies within
    floor(0.2 / res) cells, whichever way rc is rounded;
  * the last path node within / beyond 0.01 m of the target: the node path ends on the target's own node, so that
    distance is 0 (or the node is a repeat of the pose before it and was not added: still 0);
  * five winners in the last partial stride of k_nearest_k at n = 513, 1025, 2561, 5121: that stride holds one node.
    LAST_STRIDE_N has node counts whose last stride holds six, and at every n the last node is the nearest once.
"""
import collections
import math

import numpy as np

import path_ref as R
from test_path_oracle import graph

NEAR_THREADS = 512     # csrc/path.hip kNearThreads
NEAR_K = 5             # csrc/path.hip kNearK
TRIM_BLOCK = 128       # csrc/path.hip run_path_plan: k_trim_check's block
INF = math.inf

Scene = collections.namedtuple("Scene", "name family graph grid query regime")

RESOLUTIONS = (0.1, 0.05, 0.04, 0.0625, 0.025, 0.2, 0.25)   # float32 each (OccupancyGrid.info.resolution)


def grid(W, H, res, origin=(0.0, 0.0), cells=(), fill=0):
    sk = np.full((H, W), fill, np.int8)
    for x, y, *v in cells:
        sk[y, x] = v[0] if v else 100
    return {"origin": (float(origin[0]), float(origin[1])), "resolution": res, "width": W, "height": H,
            "skeleton_framed": sk.reshape(-1)}


def chain(poses):
    """A path graph whose node positions are the poses of the planned path, in order."""
    n = len(poses)
    assert n >= 2 and math.dist(poses[0], poses[-1]) > 0.2 + 1e-9
    e = [v for i in range(n - 1) for v in (i, i + 1)]
    return graph(poses, e, [0.0] * (n - 1), [(0, 0, 3), (n - 1, 0, 2)])


CHAIN_QUERY = dict(target=1, previous=0)
FAR = (-50.0, -50.0)   # a first pose outside every grid here (pose 0 never cuts; it only starts the chain)


def chain_scene(name, poses, gr, cut, **regime):
    poses = [(float(x), float(y)) for x, y in poses]
    return Scene(name, "trim", chain(poses), gr, CHAIN_QUERY, dict(regime, cut=cut, poses=poses))


# ------------------------------------------------------------------------------------------------ trim: offsets
def offset_extremes(res32):
    """(farthest kept, nearest skipped, the axis offset (rc, 0)) of a resolution; ties by the larger dx."""
    res = float(np.float32(res32))
    rc = R.radius_cells(res)
    kept = R.offsets(res)
    box = [(dx, dy) for dx in range(0, rc + 2) for dy in range(0, rc + 2)]
    d = lambda o: math.sqrt(o[0] * o[0] + o[1] * o[1]) * res   # noqa: E731
    far_kept = max((o for o in box if o in kept), key=lambda o: (d(o), o[0]))
    near_skipped = min((o for o in box if o not in kept), key=lambda o: (d(o), -o[0]))
    return far_kept, near_skipped, (rc, 0)


def offset_scenes():
    out = []
    for r in RESOLUTIONS:
        res = float(np.float32(r))
        kept, skipped, axis = offset_extremes(r)
        rc = axis[0]
        c = rc + 2                       # the pose's cell, in the middle of a (2 rc + 5)^2 grid
        W = 2 * rc + 5
        origin = (-3.0, 2.0)
        pose = (origin[0] + (c + 0.5) * res, origin[1] + (c + 0.5) * res)
        cases = [("kept", kept, 1), ("kept-neg", (-kept[0], -kept[1]), 1), ("kept-swap", (-kept[1], kept[0]), 1),
                 ("skipped", skipped, None), ("skipped-neg", (-skipped[0], -skipped[1]), None)]
        if axis != skipped:
            cases.append(("skipped-axis", axis, None))
        for what, (dx, dy), cut in cases:
            gr = grid(W, W, r, origin, [(c + dx, c + dy)])
            out.append(chain_scene(f"offset-{r}-{what}", [FAR, pose], gr, cut, offset=(dx, dy), res=res))
    return out


# ------------------------------------------------------------------------------------------------ trim: borders
def border_scenes():
    out = []
    o = (10.0, 10.0)
    for name, cells, pose, cut in [
            ("left-in", [(0, 4)], (9.9, 11.1), 1), ("left-out", [(0, 4)], (9.7, 11.1), None),
            ("below-in", [(4, 0)], (11.1, 9.9), 1), ("below-out", [(4, 0)], (11.1, 9.7), None),
            ("corner-in", [(0, 0)], (9.9, 9.9), 1), ("corner-out-x", [(0, 0)], (9.7, 9.9), None),
            ("corner-out-y", [(0, 0)], (9.9, 9.7), None)]:
        out.append(chain_scene(f"border-{name}", [FAR, pose], grid(8, 8, 0.25, o, cells), cut))
    # origin 0 and a power-of-two resolution: fx = x / 0.25 exactly, so one ulp of x is one ulp of fx
    dn = lambda v: float(np.nextafter(v, -INF))   # noqa: E731
    W, H = 8, 6
    for name, cells, pose, cut, f in [
            ("fx-W", [(7, 2)], (2.0, 0.6), None, (8.0, None)), ("fx-W-ulp", [(7, 2)], (dn(2.0), 0.6), 1, (dn(8.0), None)),
            ("fy-H", [(2, 5)], (0.6, 1.5), None, (None, 6.0)), ("fy-H-ulp", [(2, 5)], (0.6, dn(1.5)), 1, (None, dn(6.0))),
            ("int-int", [(3, 3)], (0.75, 0.75), 1, (3.0, 3.0)),
            ("ulp-int", [(3, 3)], (dn(0.75), 0.75), None, (dn(3.0), 3.0)),
            ("int-ulp", [(3, 3)], (0.75, dn(0.75)), None, (3.0, dn(3.0))),
            ("ulp-ulp", [(2, 2)], (dn(0.75), dn(0.75)), 1, (dn(3.0), dn(3.0))),
            ("int-int-below", [(2, 2)], (0.75, 0.75), None, (3.0, 3.0))]:
        out.append(chain_scene(f"edge-{name}", [FAR, pose], grid(W, H, 0.25, (0.0, 0.0), cells), cut, f=f))
    return out


# ------------------------------------------------------------------------------------------------ trim: range
def range_scenes():
    """Poses whose cell quotients leave the int range on a full grid, and two whose quotients are 2^32 + 5 and
    -2^32 + 5 exactly (a cast that wrapped would land in the grid)."""
    full = grid(16, 16, 0.25, (0.0, 0.0), fill=100)
    wrap = 2.0 ** 30 + 1.25       # / 0.25 = 2^32 + 5
    far = [(1.0e9, 1.0), (-1.0e9, 1.0), (1.0, -1.0e9), (2.0e10, 2.0e10), (-2.0e10, 1.0), (1.0, 2.0e10),
           (wrap, 1.0), (1.0, wrap - 2.0 ** 31)]
    assert wrap / 0.25 == 2.0 ** 32 + 5 and (wrap - 2.0 ** 31) / 0.25 == -2.0 ** 32 + 5
    return [chain_scene("range-far-only", [FAR] + far, full, None),
            chain_scene("range-far-then-inside", [FAR] + far + [(1.0, 1.0)], full, 1 + len(far))]


# ------------------------------------------------------------------------------------------------ trim: values
def value_scenes():
    out = []
    poses = [FAR, (0.6, 0.6), (1.1, 0.6), (1.1, 1.1)]
    for v in (99, 101, 127, -1, -100, 1):
        out.append(chain_scene(f"value-{v}", poses, grid(8, 8, 0.25, fill=v), None, fill=v))
        out.append(chain_scene(f"value-{v}-one-100", poses, grid(8, 8, 0.25, cells=[(4, 2)], fill=v), 2, fill=v))
    # pose 0 alone on an occupied cell
    out.append(chain_scene("pose0-only", [(0.6, 0.6), (1.1, 0.6), (1.1, 1.1)], grid(8, 8, 0.25, cells=[(2, 2)]), None))
    out.append(chain_scene("pose0-and-2", [(0.6, 0.6), (1.1, 0.6), (1.1, 1.1)],
                           grid(8, 8, 0.25, cells=[(2, 2), (4, 4)]), 2))
    return out


# ------------------------------------------------------------------------------------------------ trim: blocks
FIRST_CUTS = (1, 127, 128, 129, 255, 256)   # around k_trim_check's 128-thread blocks


def later(first, n):
    return sorted({i for i in (first + 3, first + 50, 2 * TRIM_BLOCK + 5, n - 1) if first < i < n})


def block_scenes():
    """300 poses 0.3 m apart at 0.25 m cells (only a pose's own cell is sampled): the first occupied pose and
    later ones, which other blocks' atomicMin must not let win."""
    out = []
    n = 300
    poses = [(0.3 * i + 0.1, 0.6) for i in range(n)]
    col = lambda i: int(poses[i][0] / 0.25)   # noqa: E731
    assert len({col(i) for i in range(n)}) == n
    for f in FIRST_CUTS:
        cells = [(col(i), 2) for i in [f] + later(f, n)]
        out.append(chain_scene(f"block-chain-{f}", poses, grid(col(n - 1) + 2, 4, 0.25, cells=cells), f))
    out.append(chain_scene("block-chain-none", poses, grid(col(n - 1) + 2, 4, 0.25, cells=[(col(5), 1), (col(5), 3)]), None))
    return out


def straight_poses(to):
    """planAndPublishPath's initial straight line from the origin (:989-1010)."""
    dx, dy = to
    total = math.sqrt(dx * dx + dy * dy)
    steps = int(math.ceil(total / 0.2))
    p = [(0.0 + i / steps * dx, 0.0 + i / steps * dy) for i in range(steps + 1)]
    p[-1] = (float(to[0]), float(to[1]))
    return p


def straight_scenes():
    """The same cuts through the initial straight line, 0.2 m steps at 0.1f cells: pose i lies in column 2 i and
    samples columns 2 i - 1 ... 2 i + 1, so column 2 f + 1 is first seen by pose f."""
    out = []
    L = 59.8
    one_node = graph([(0.0, 0.0)], [], [], [])
    for axis, firsts in (("x", FIRST_CUTS), ("y", (128, 256))):
        to = (L, 0.0) if axis == "x" else (0.0, L)
        poses = straight_poses(to)
        n = len(poses)
        assert n >= 300
        for f in firsts:
            along = [2 * i + 1 for i in [f] + later(f, n)]
            if axis == "x":
                gr = grid(2 * n + 2, 3, 0.1, (-0.05, -0.15), [(a, 1) for a in along])
            else:
                gr = grid(3, 2 * n + 2, 0.1, (-0.15, -0.05), [(1, a) for a in along])
            q = dict(initial_waypoint_reached=False, initial_waypoint=to)
            out.append(Scene(f"block-straight-{axis}-{f}", "trim", one_node, gr, q, dict(cut=f, poses=poses)))
    return out


# ------------------------------------------------------------------------------------------------ trim: shapes
def shape_scenes():
    out = [chain_scene("shape-1x1", [FAR, (0.1, 0.1)], grid(1, 1, 0.25, cells=[(0, 0)]), 1),
           chain_scene("shape-1x1-from-outside", [FAR, (-0.1, -0.1)], grid(1, 1, 0.25, cells=[(0, 0)]), 1),
           chain_scene("shape-1x1-free", [FAR, (0.1, 0.1)], grid(1, 1, 0.25), None),
           chain_scene("shape-w1-h300-last", [FAR, (0.1, 299 * 0.25 + 0.1)], grid(1, 300, 0.25, cells=[(0, 299)]), 1),
           chain_scene("shape-w1-h300-miss", [FAR, (0.1, 298 * 0.25 + 0.1)], grid(1, 300, 0.25, cells=[(0, 299)]), None),
           chain_scene("shape-w300-h1-last", [FAR, (299 * 0.25 + 0.1, 0.1)], grid(300, 1, 0.25, cells=[(299, 0)]), 1),
           chain_scene("shape-w300-h1-miss", [FAR, (298 * 0.25 + 0.1, 0.1)], grid(300, 1, 0.25, cells=[(299, 0)]), None)]
    W, H = 513, 257
    at = lambda x, y: (x * 0.25 + 0.1, y * 0.25 + 0.1)   # noqa: E731
    but = grid(W, H, 0.25, fill=100, cells=[(300, 200, 0)])
    out += [chain_scene("shape-513x257-only", [FAR, at(300, 200)], grid(W, H, 0.25, cells=[(300, 200)]), 1),
            chain_scene("shape-513x257-all-but", [FAR, at(300, 200)], but, None),
            chain_scene("shape-513x257-last", [FAR, at(0, 256), at(512, 0), at(512, 256)],
                        grid(W, H, 0.25, cells=[(512, 256)]), 3),
            # the cell that (x, y) would be with the rows H long: 300 + 200 * 257 = 100 * 513 + 400
            chain_scene("shape-513x257-transposed", [FAR, at(300, 200)], grid(W, H, 0.25, cells=[(400, 100)]), None)]
    return out


def trim_scenes():
    return (offset_scenes() + border_scenes() + range_scenes() + value_scenes() + block_scenes() + straight_scenes()
            + shape_scenes())


# ------------------------------------------------------------------------------------------------ nearest
P = (128.0, -64.0)
TIES = [(3, 4), (-3, 4), (3, -4), (-3, -4), (4, 3), (-4, 3), (4, -3), (-4, -3), (5, 0), (-5, 0), (0, 5), (0, -5)]
FAR13 = [(5, 12), (-5, 12), (5, -12), (-5, -12), (13, 0), (-13, 0)]
NEAR_N = (513, 1024, 1025, 2560, 2561, 5121)
LAST_STRIDE_N = (518, 1030, 2566)
GOAL = 0


def near_nodes(n, near, p=P):
    """n nodes: `near` {index: offset from p}, node GOAL far to the west, the others isolated and >= 1000 m away."""
    i = np.arange(n, dtype=np.float64)
    nodes = np.stack([p[0] + 1000.0 + i, p[1] + 2000.0 - 0.5 * i], 1)
    nodes[GOAL] = (p[0] - 3000.0, p[1])
    for k, (ox, oy) in near.items():
        assert 0 < k < n, (k, n)
        nodes[k] = (p[0] + ox, p[1] + oy)
    return nodes


def near_graph(nodes, edges):
    """edges: [(near node, length)] to GOAL; GOAL carries BR of cluster 0 (the one waypoint)."""
    e = [v for k, _ in edges for v in (k, GOAL)]
    return graph(nodes, e, [l for _, l in edges], [(GOAL, 0, 3)])


def merge_level(a, b):
    """The stride of k_nearest_k's LDS merge at which threads a and b's lists meet."""
    s = NEAR_THREADS // 2
    while s >= 1 and a % s != b % s:
        s //= 2
    return s


def near_patterns(n):
    """name -> {index: offset}; the twelve exact ties at distance 5 unless said otherwise."""
    tie = lambda idx: dict(zip(idx, TIES))   # noqa: E731
    rest = list(range(400, 406))
    pats = {}
    for s in (256, 128, 1):
        pats[f"apart-{s}"] = tie([20, 21, 22, 20 + s, 21 + s, 22 + s] + rest if s > 1 else list(range(20, 26)) + rest)
        pats[f"straddle-{s}"] = tie([3, 4, 5, 6, 40, 40 + s] + rest)
    tail = tie([3, 4, 5, 6, 40, 41] + rest)
    tail[n - 1] = (3, 0)                                   # the last node of all is the nearest
    pats["tail"] = tail
    t7 = [7 + NEAR_THREADS * m for m in range(6)]
    if n > 3005:
        pats["stride-six"] = tie(t7 + list(range(3000, 3006)))
        pats["stride-descending"] = dict(zip(t7, [(10, 0), (0, 9), (-8, 0), (0, -7), (6, 0), (0, 5)]))
    if n in LAST_STRIDE_N:
        last = list(range((n - 1) // NEAR_THREADS * NEAR_THREADS, n))
        assert len(last) == 6
        pats = {"last-stride": {**dict(zip(last, TIES[:4] + TIES[8:10])), **dict(zip(range(10, 16), FAR13))}}
    return pats


def nearest_scenes():
    out = []
    q = dict(target=0, current=P)
    for n in NEAR_N + LAST_STRIDE_N:
        for pname, near in near_patterns(n).items():
            nodes = near_nodes(n, near)
            d = R.distances(nodes, P)
            rank = sorted(near, key=lambda k: (d[k], k))
            reg = dict(near=near, rank=rank, n=n, pattern=pname, p=P)
            out.append(Scene(f"near-{n}-{pname}-all", "nearest", near_graph(nodes, [(k, 1.0) for k in sorted(near)]),
                             grid(4, 4, 0.25), q, dict(reg, node_path=[rank[0], GOAL], cands=rank[:NEAR_K])))
            for j in range(NEAR_K):
                g = near_graph(nodes, [(rank[j], 2.0), (rank[NEAR_K], 1.0)])
                out.append(Scene(f"near-{n}-{pname}-{j}", "nearest", g, grid(4, 4, 0.25), q,
                                 dict(reg, node_path=[rank[j], GOAL], cands=rank[:NEAR_K])))
    return out + overflow_near_scenes() + same_position_scenes() + [fma_pair_scene()]


def overflow_near_scenes():
    """Fewer than five nodes at a finite distance, the others at x = 1e200 (their distance overflows to inf): the
    candidates are the finite ones, then (inf, index) order. Only finite candidates can carry a path."""
    out = []
    q = dict(target=0, current=P)
    for n, fin in ((8, {3: (0, 2), 6: (1, 0), 5: (0, -3)}), (1025, {600: (0, 2), 5: (1, 0), 1000: (0, -3)}),
                   (7, {4: (2, 0)})):
        nodes = np.array([(1.0e200, float(i)) for i in range(n)])
        nodes[GOAL] = (P[0] - 3000.0, P[1])
        for k, (ox, oy) in fin.items():
            nodes[k] = (P[0] + ox, P[1] + oy)
        d = R.distances(nodes, P)
        rank = sorted(range(n), key=lambda k: (d[k], k))[:NEAR_K]
        finite = [k for k in rank if math.isfinite(d[k])]
        assert len(finite) == len(fin) + 1 and not math.isfinite(d[rank[-1]])    # (the goal is finite too)
        reg = dict(n=n, p=P, cands=rank, overflow=True)
        every = [(k, 1.0) for k in range(1, n)]
        out.append(Scene(f"near-overflow-{n}-all", "nearest", near_graph(nodes, every), grid(4, 4, 0.25), q,
                         dict(reg, node_path=[finite[0], GOAL])))
        only_inf = [(k, 1.0) for k in range(1, n) if not math.isfinite(d[k])]
        out.append(Scene(f"near-overflow-{n}-inf-edges-only", "nearest", near_graph(nodes, only_inf),
                         grid(4, 4, 0.25), q, dict(reg, status=0)))
    return out


def same_position_scenes():
    """n = 1 ... 6 nodes at one position, the robot 5 m away: the candidates are nodes 0 ... 4 by index; node 0 is the
    goal, and node 5's shorter edge is never used."""
    out = []
    for n in range(1, 7):
        nodes = [(1.0, 1.0)] * n
        edges = [(k, 0.5 if k == 5 else 1.0) for k in range(1, n)]
        reg = dict(n=n, p=(4.0, 5.0), cands=list(range(min(n, NEAR_K))))
        reg.update(dict(status=0) if n == 1 else dict(node_path=[1, 0], n_poses=2))
        out.append(Scene(f"near-same-position-{n}", "nearest", near_graph(np.array(nodes), edges), grid(4, 4, 0.25),
                         dict(target=0, current=(4.0, 5.0)), reg))
    return out


FMA_P = (0.3, -0.7)


def fma_pair(seed=20250131, count=1500, radius=7.3):
    """Two points a, b with distance(FMA_P, a) < distance(FMA_P, b) as the reference rounds dx * dx + dy * dy, and
    the other way round with the sum fused: the first such pair of a seeded ring of points."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-math.pi, math.pi, count)
    pts = np.stack([FMA_P[0] + radius * np.cos(t), FMA_P[1] + radius * np.sin(t)], 1)
    plain, fused = R.distances(pts, FMA_P), R.distances(pts, FMA_P, "fma")
    hit = np.argwhere((plain[:, None] < plain[None, :]) & (fused[:, None] > fused[None, :]))
    if len(hit):
        a, b = hit[0]
        return tuple(pts[a].tolist()), tuple(pts[b].tolist())
    raise AssertionError("no pair found")


def fma_pair_scene():
    a, b = fma_pair()
    n = 20
    nodes = near_nodes(n, {2: (1, 0), 3: (0, 2), 4: (-3, 0), 5: (0, -4)}, FMA_P)
    nodes[11], nodes[10] = a, b                                 # a has the larger index: the distance decides
    g = near_graph(nodes, [(11, 2.0), (10, 1.0)])
    return Scene("near-fma-pair", "nearest", g, grid(4, 4, 0.25), dict(target=0, current=FMA_P),
                 dict(n=n, p=FMA_P, cands=[2, 3, 4, 5, 11], node_path=[11, GOAL], fma_pair=(11, 10)))


# ------------------------------------------------------------------------------------------------ origin return
ORIGIN_QUERY = dict(target=1, previous=0, exploration_completed=True)


def origin_scenes():
    """findNearestNode from the origin: exact ties go to the smallest index (strict <); a graph whose nodes are all
    at an overflowing distance has no nearest node and the origin return fails."""
    out = []
    base = [(20.0, 0.0), (40.0, 40.0), (3.0, 4.0), (50.0, 50.0), (-5.0, 0.0), (0.0, -5.0), (4.0, -3.0)]
    ties = [2, 4, 5, 6]
    for name, perm in (("ties-a", [0, 1, 2, 3, 4, 5, 6]), ("ties-b", [0, 1, 6, 3, 5, 4, 2]), ("ties-c", [0, 4, 3, 1, 2, 5, 6])):
        nodes = [base[k] for k in perm]
        tied = [i for i, k in enumerate(perm) if k in ties]
        e = [v for t in tied for v in (0, t)]
        g = graph(nodes, e, [1.0] * len(tied), [(0, 0, 3)])
        out.append(Scene(f"origin-{name}", "origin", g, grid(4, 4, 0.25, (100.0, 100.0)), ORIGIN_QUERY,
                         dict(goal=min(tied), tied=tied, node_path=[0, min(tied)])))
    big = [(1.0e200, 0.0), (1.0e200, 1.0), (1.0e200, 2.0)]
    g = graph(big, [0, 1, 1, 2], [1.0, 1.0], [(2, 0, 3), (0, 0, 2)])
    q = dict(target=2, previous=1, exploration_completed=True)
    out.append(Scene("origin-all-overflow", "origin", g, grid(4, 4, 0.25, (100.0, 100.0)), q,
                     dict(goal=-1, status=0, target=2, n_waypoints=3)))
    g = graph(big + [(30.0, 40.0)], [0, 1, 1, 2, 2, 3], [1.0, 1.0, 1.0], [(2, 0, 3), (0, 0, 2)])
    out.append(Scene("origin-one-finite", "origin", g, grid(4, 4, 0.25, (100.0, 100.0)), q,
                     dict(goal=3, node_path=[0, 1, 2, 3], target=2)))
    return out


# ------------------------------------------------------------------------------------------------ host planner
def host_scenes():
    out = []
    free = grid(4, 4, 0.25, (1000.0, 1000.0))
    add = lambda name, g, q, **reg: out.append(Scene("host-" + name, "host", g, free, q, reg))   # noqa: E731

    # 6 x 6 grid graph, unit lengths: many equal-f pops
    nodes = [(float(i), float(j)) for j in range(6) for i in range(6)]
    e = []
    for j in range(6):
        for i in range(6):
            if i < 5:
                e += [6 * j + i, 6 * j + i + 1]
            if j < 5:
                e += [6 * j + i, 6 * j + i + 6]
    g66 = graph(nodes, e, [1.0] * (len(e) // 2), [(0, 0, 3), (35, 0, 2), (5, 0, 1)])
    for t, p in ((1, 0), (2, 1), (0, 2)):
        add(f"grid6x6-{t}", g66, dict(target=t, previous=p), n_waypoints=3)

    # two routes S-A-G and S-B-G; the pair (S, A) is listed twice (and self loops first)
    pos = [(0.0, 0.0), (100.0, 50.0), (100.0, -50.0), (200.0, 0.0)]
    lab = [(0, 0, 3), (3, 0, 2)]
    q = dict(target=1, previous=0)
    for name, e, l, path in (
            ("dup-long-first", [0, 1, 0, 1, 1, 3, 0, 2, 2, 3], [5.0, 0.1, 1.0, 1.0, 1.0], [0, 2, 3]),
            ("dup-short-first", [0, 1, 0, 1, 1, 3, 0, 2, 2, 3], [0.1, 5.0, 1.0, 1.0, 1.0], [0, 1, 3]),
            ("dup-reversed-long-first", [1, 0, 0, 1, 1, 3, 0, 2, 2, 3], [5.0, 0.1, 1.0, 1.0, 1.0], [0, 2, 3]),
            ("dup-reversed-short-first", [0, 1, 1, 0, 1, 3, 0, 2, 2, 3], [0.1, 5.0, 1.0, 1.0, 1.0], [0, 1, 3]),
            ("self-loops", [0, 0, 1, 1, 3, 3, 0, 1, 1, 3, 0, 2, 2, 2, 2, 3], [7.0, 0.0, 0.0, 0.1, 1.0, 1.0, 9.0, 1.0], [0, 1, 3]),
            ("self-loop-goal-only", [3, 3, 0, 1], [1.0, 1.0], None),
            ("len-zero", [0, 1, 1, 3, 0, 2, 2, 3], [0.0, 0.0, 0.0, 0.0], None),
            ("len-fltmax-inf", [0, 1, 1, 3, 0, 2, 2, 3], [float(np.finfo(np.float32).max), 0.0, INF, 0.0], None),
            ("len-all-inf", [0, 1, 1, 3, 0, 2, 2, 3], [INF, INF, INF, INF], None),
            ("len-inf-last", [0, 1, 1, 3], [1.0, INF], None)):
        add(name, graph(pos, e, l, lab), q, **({"node_path": path} if path else {}))

    # the goal is reachable only from the fifth candidate; the sixth has a shorter edge
    p = (10.0, 10.0)
    nodes = [(500.0, 500.0)] + [(p[0] + d, p[1]) for d in (1.0, 2.0, 3.0, 4.0, 5.0, 6.0)]
    add("fifth-candidate", graph(nodes, [5, 0, 6, 0], [2.0, 1.0], [(0, 0, 3)]), dict(target=0, current=p),
        node_path=[5, 0])

    # the start within / beyond 0.1 m of the first path node; within: the path begins on the node
    line = graph([(0.0, 0.0), (5.0, 0.0)], [0, 1], [1.0], [(1, 0, 3)])
    up = lambda v: float(np.nextafter(v, INF))   # noqa: E731
    dn = lambda v: float(np.nextafter(v, -INF))   # noqa: E731
    add("start-0.1", line, dict(target=0, current=(0.1, 0.0)), n_poses=2, eq=[(math.sqrt(0.1 * 0.1), 0.1)])
    add("start-0.1-ulp", line, dict(target=0, current=(up(0.1), 0.0)), n_poses=3, gt=[(math.sqrt(up(0.1) ** 2), 0.1)])

    # consecutive path nodes at one position, 1e-300 apart (dx * dx underflows: distance 0, dropped) and 1e-150
    for name, x, n_poses in (("repeat-same", 0.0, 3), ("repeat-1e-300", 1.0e-300, 3), ("repeat-1e-150", 1.0e-150, 4)):
        g = graph([(-3.0, 0.0), (0.0, 0.0), (x, 0.0), (0.0, 4.0)], [0, 1, 1, 2, 2, 3], [1.0, 1.0, 1.0], [(0, 0, 3), (3, 0, 2)])
        add(name, g, dict(target=1, previous=0), n_poses=n_poses, node_path=[0, 1, 2, 3])

    # waypoints exactly 0.2 m apart (dropped) and one ulp more (kept)
    for name, x, nw in (("waypoint-0.2", 0.2, 2), ("waypoint-0.2-ulp", up(0.2), 3)):
        g = graph([(0.0, 0.0), (x, 0.0), (0.0, 4.0)], [0, 1, 1, 2, 0, 2], [1.0, 1.0, 1.0], [(0, 0, 3), (1, 0, 2), (2, 0, 1)])
        add(name, g, dict(target=1, previous=0), n_waypoints=nw,
            **({"eq": [(math.sqrt(x * x), 0.2)]} if nw == 2 else {"gt": [(math.sqrt(x * x), 0.2)]}))

    # cluster ids, missing corners, repeated and invalid label entries on a 14-node line
    nodes = [(2.0 * i, 1.0 * (i % 3)) for i in range(14)]
    e = [v for i in range(13) for v in (i, i + 1)]
    lens = [1.0 + 0.25 * (i % 4) for i in range(13)]
    label_sets = {
        "ids-0-2-7": [(0, 0, 3), (1, 0, 2), (2, 2, 3), (3, 2, 2), (4, 7, 0), (5, 7, 1), (6, 7, 2), (7, 7, 3), (8, 0, 1)],
        "ids-odd-only": [(0, 1, 0), (1, 1, 1), (2, 3, 0), (3, 3, 1), (4, 3, 2), (5, 1, 2)],
        "ids-missing-corners": [(0, 0, 2), (3, 1, 1), (5, 2, 3), (6, 4, 1), (9, 5, 2)],
        "labels-repeated": [(2, 0, 3), (2, 0, 3), (5, 0, 3), (1, 0, 2), (9, 0, 2), (9, 0, 1), (4, 0, 1), (4, 0, 3)],
        "labels-invalid": [(0, 0, -1), (1, 0, 4), (2, -1, 3), (3, 0, 3), (4, -1, -1), (5, 0, 2), (6, 3, 7), (7, -5, 2)],
    }
    for name, lab in label_sets.items():
        g = graph(nodes, e, lens, lab)
        nw = {"ids-0-2-7": 7, "ids-odd-only": 5, "ids-missing-corners": 4, "labels-repeated": 3, "labels-invalid": 2}[name]
        for t in range(nw + 1):
            add(f"{name}-t{t}", g, dict(target=t, previous=t - 1), n_waypoints=nw)
    # label counts that run past n_label_entries: node 1 claims three entries more than there are in all
    g = graph(nodes, e, lens, label_sets["ids-0-2-7"])
    g["node_label_counts"] = g["node_label_counts"].copy()
    g["node_label_counts"][1] += 3
    g["node_label_counts"][12] += 40
    for t in range(3):
        add(f"label-counts-past-end-t{t}", g, dict(target=t, previous=t - 1), counts_past_end=True)

    # the bitmask fallback (no label entries): multi-bit masks, later nodes overwrite, bits >= 4 and masks <= 0 and
    # clusters < 0 are ignored
    g = graph(nodes, e, lens, [])
    g["node_labels"] = np.array([0b1100, 0b0011, 0b0110, 16, -1, 0b1000, 0b1111, 0b0100, 0, 0b10001, 0b0010, 5, 0, 0], np.int32)
    g["node_cluster_indices"] = np.array([0, 0, 1, 1, 1, 1, -1, 2, 2, 0, 2, -3, 0, 0], np.int32)
    for t in range(5):
        add(f"bitmask-t{t}", g, dict(target=t, previous=t - 1), fallback=True)

    # the saved target: nearest waypoint within 0.5 m wins, at exactly 0.5 m the saved index does
    g = graph(nodes, e, lens, label_sets["ids-0-2-7"])
    w0 = nodes[0]     # cluster 0's BR: the first waypoint
    assert w0 == (0.0, 0.0)
    add("saved-0.5", g, dict(target=2, previous=1, saved_target=(-0.5, 0.0)), target=2, eq=[(math.sqrt(0.5 * 0.5), 0.5)])
    add("saved-0.5-ulp", g, dict(target=2, previous=1, saved_target=(-dn(0.5), 0.0)), target=0,
        gt=[(0.5, math.sqrt(dn(0.5) * dn(0.5)))])
    add("saved-far-index-kept", g, dict(target=3, saved_target=(500.0, 500.0)), target=3)
    add("saved-far-index-out", g, dict(target=50, saved_target=(500.0, 500.0)), target=50, status=0)
    add("saved-far-index-negative", g, dict(target=-1, saved_target=(500.0, 500.0)), target=0)
    add("saved-completed-out", g, dict(target=50, saved_target=(500.0, 500.0), exploration_completed=True), target=7)
    return out


def all_scenes():
    s = trim_scenes() + nearest_scenes() + origin_scenes() + host_scenes()
    names = [x.name for x in s]
    assert len(set(names)) == len(names)
    return s


FAMILIES = ("trim", "nearest", "origin", "host")


def size(s):
    return len(s.graph["nodes"]) + s.grid["width"] * s.grid["height"] + 16 * len(s.regime.get("poses", ()))


def handle_order(scenes):
    """One handle's order through all scenes: the smallest, the largest, the second smallest, ... so the node, pose
    and grid buffers shrink and grow between every two plans."""
    by = sorted(scenes, key=size)
    out = []
    while by:
        out.append(by.pop(0))
        if by:
            out.append(by.pop())
    return out
