"""Non-orchard inputs for the GVD stage's parity tests (test infrastructure, imported like shapes.py).

SCENES[name] is (seeds, rows_info, grid): what O.gvd and Ctx.gvd take (no scene needs parameters of its own; the tests
set the resolution and the Subdiv2D rectangle mode). Every grid has resolution 0.25 and origin (100, 200), exact in
float32 and in double; its skeleton is all zero unless the scene sets one. Seeds are float64 (n, 2); rows_info is
(2 * rows, 2): each row's start and end. Scenes are built on first use, deterministically, and are read-only.

The regime predictors restate one branch condition of the library each, on an oracle result, every constant named with
its source; tests/test_gvd_scenes_cpu.py checks every scene against them without a GPU, and that the constants still
match csrc.
"""
import functools
from collections.abc import Mapping

import numpy as np

RES = 0.25
ORIGIN = (100.0, 200.0)

# the library's constants the predictors use
LF_TB = 256            # csrc/greedy.hip       kLfTB (candidates per k_lfmis block)
LF_LIST = 16           # csrc/greedy.hip       kLfList (listed earlier conflicting candidates; more: the `over` re-walk)
NODE_MATCH = 16        # csrc/gvd.hip          kNodeMatch (label points listed per node; more: the plain loop)
NEAR_THREADS = 512     # csrc/path.hip         kNearThreads (k_nearest_k's one block)
NEAR_K = 5             # csrc/path.hip         kNearK
MERGE_R = 0.5          # csrc/gvd.hip          kMergeRadius (merge_seeds, g1: kConflictLessEq, d <= 0.5)
MERGE_RANGE = 60.0     # csrc/gvd.hip          kMergeRange: g1's cell index spans the grid +- 60 m (points beyond: border cells)
BP_CELL = 0.5          # csrc/gvd.hip          kBpCell, kBpRange (graph_begin): g5's cell index: the grid +- 10 m in cells of 0.5 m
BP_RANGE = 10.0
BP_THR_SQ = 0.05 * 0.05   # csrc/gvd.hip       kBpThr squared, g5: the same 1 cm key, or d^2 < 0.0025
NODE_CELL = 5.01       # csrc/gvd.hip          kNodeCell, kNodeRange (graph_attempt): g8's node index: the grid +- 10 m in cells of 5.01 m
NODE_RANGE = 10.0
LABEL_CELL = 0.1       # csrc/gvd.hip          kLabelCell, kLabelRange (graph_attempt): g9's label point index: the grid +- 1 m in cells of 0.1 m
LABEL_RANGE = 1.0
CELLS_PER_ITEM = 2.0   # csrc/dev_prims.h      make_hash_n: at most max(HASH_MIN_CELLS, cells_per_item * n) cells
HASH_MIN_CELLS = 4096  # csrc/greedy.hip       make_hash_n
HASH_GROW = 1.25       # csrc/greedy.hip       make_hash_cap enlarges the cell by this factor until the cells fit
PAIR_CAP_MIN = 1024    # csrc/gvd.hip          kPairCapMin (run_gvd_stage): cap_first = max(1024, 2 * no); cap_next = max(1024, P + P / 4)
PAIR_MIN, PAIR_MAX = 1e-6, 0.5   # csrc/gvd.hip  kPairMin, kPairMax (pairs_of): the pairs: 1e-6 < d <= 0.5


# ---------------------------------------------------------------- grids
def grid(W, H, sk=None):
    if sk is None:
        sk = np.zeros((H, W), np.int8)
    sk = np.ascontiguousarray(sk, np.int8)
    assert sk.shape == (H, W)
    return {"origin": ORIGIN, "resolution": RES, "width": W, "height": H, "skeleton_framed": sk}


G_W, G_H = 200, 160          # "g": x in [100, 150], y in [200, 240]
BIG_W = BIG_H = 400          # "big": x in [100, 200], y in [200, 300]
WIDE_W, WIDE_H = 1600, 1400  # x in [100, 500], y in [200, 550]


def bars_skeleton():
    sk = np.zeros((BIG_H, BIG_W), np.int8)
    sk[100:300:40, 50:350] = 100
    return sk


def bounds(gr):
    x0, y0 = gr["origin"]
    res = float(np.float32(gr["resolution"]))
    return x0, x0 + gr["width"] * res, y0, y0 + gr["height"] * res


# ---------------------------------------------------------------- seed sets
def serpentine(rows=13, per_row=108, pitch=0.4, x0=102.0, y0=205.0):
    """Rows 1 m apart walked in alternating directions, two connecting seeds (1/3 m apart) at every turn: consecutive
    indices are never more than `pitch` apart, from the first seed to the last."""
    pts = []
    for r in range(rows):
        ks = range(per_row) if r % 2 == 0 else range(per_row - 1, -1, -1)
        pts += [(x0 + pitch * k, y0 + r) for k in ks]
        if r + 1 < rows:
            xe = pts[-1][0]
            pts += [(xe, y0 + r + 1.0 / 3.0), (xe, y0 + r + 2.0 / 3.0)]
    return np.array(pts, np.float64)


CLUMP_N = 48


def index_corner(gr_bounds, rng_m, cell, n, x, y):
    """The corner of the cell index (grid +- rng_m, cells of `cell` for n items) nearest to (x, y)."""
    x0, x1, y0, y1 = gr_bounds
    size = hash_geometry(x0 - rng_m, x1 + rng_m, y0 - rng_m, y1 + rng_m, cell, n)[0]
    return np.array([x0 - rng_m + round((x - (x0 - rng_m)) / size) * size,
                     y0 - rng_m + round((y - (y0 - rng_m)) / size) * size])


def chain_clump():
    """The serpentine, then two clumps of 48 seeds within +- 0.15 m of a corner of g1's cell index, so each clump lies
    in four cells. A clump's first seed is kept and owns the 47 others; it sits 0.1 m above and right of the corner in
    the first clump and 0.1 m below and left of it in the second: its members in the other cell row find it in the
    row above / below their own when they re-walk the cells."""
    rng = np.random.default_rng(11)
    ser = serpentine()
    gb = (ORIGIN[0], ORIGIN[0] + G_W * RES, ORIGIN[1], ORIGIN[1] + G_H * RES)
    parts = [ser]
    for (x, y), sgn in (((125.0, 232.0), 1.0), ((112.0, 232.0), -1.0)):
        c = index_corner(gb, MERGE_RANGE, MERGE_R, len(ser) + 2 * CLUMP_N, x, y)
        parts += [c[None] + sgn * 0.1, c + rng.uniform(-0.15, 0.15, (CLUMP_N - 1, 2))]
    return np.vstack(parts)


def circle(n, r, cx=125.0, cy=220.0, jitter=0.0, seed=0):
    t = 2 * np.pi * np.arange(n) / n
    p = np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1)
    if jitter:
        p += np.random.default_rng(seed).uniform(-jitter, jitter, p.shape)
    return p


def lattice(nx, ny, pitch, x0, y0):
    """Row-major lattice points (x fastest)."""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny))
    return np.stack([x0 + pitch * ix.ravel(), y0 + pitch * iy.ravel()], 1).astype(np.float64)


LATTICE_N, LATTICE_PITCH, LATTICE_X0, LATTICE_Y0 = 28, 2.0, 120.0, 220.0


def lattice_rows(seeds, n, start):
    """One 6 m row per every third lattice point of every second lattice line, along x and along y alternately,
    starting at the lattice point + start. With start = half a pitch both ways an endpoint sits on a Voronoi vertex
    (rejected: nearer than 0.5 m), and the two next vertices its quadrant admits are exactly one pitch away: a tie.
    (Rows that start on lattice points have a single nearest vertex per quadrant: no tie, measured.)"""
    rows = []
    k = 0
    for j in range(0, n, 2):
        for i in range(0, n, 3):
            s = seeds[j * n + i] + start
            d = (6.0, 0.0) if k % 2 == 0 else (0.0, 6.0)
            rows += [s, s + d]
            k += 1
    return np.array(rows, np.float64)


def uniform_seeds(n, x0, x1, y0, y1, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], 1)


def sparse_rows():
    """40 random rows of 0-30 m in big, a zero-length row, a vertical row (sx == ex) and a row wholly outside the grid."""
    rng = np.random.default_rng(23)
    s = np.stack([rng.uniform(102.0, 198.0, 40), rng.uniform(202.0, 298.0, 40)], 1)
    a, L = rng.uniform(0, 2 * np.pi, 40), rng.uniform(0.0, 30.0, 40)
    e = s + np.stack([L * np.cos(a), L * np.sin(a)], 1)
    rows = np.empty((80, 2))
    rows[0::2], rows[1::2] = s, e
    extra = np.array([[150.0, 250.0], [150.0, 250.0],      # zero length: ml < 1e-6
                      [160.0, 230.0], [160.0, 262.0],      # vertical: sx == ex
                      [230.0, 320.0], [250.0, 330.0]])     # outside the grid
    return np.vstack([rows, extra])


def _labels_sparse():
    return uniform_seeds(60, 110.0, 190.0, 210.0, 290.0, 5), sparse_rows(), grid(BIG_W, BIG_H, bars_skeleton())


def _labels_dup_rows():
    seeds, rows, gr = _labels_sparse()
    return seeds, np.vstack([rows[:4]] * 20 + [rows[4:]]), gr


def _lattice():
    seeds = lattice(LATTICE_N, LATTICE_N, LATTICE_PITCH, LATTICE_X0, LATTICE_Y0)
    half = np.array([LATTICE_PITCH / 2, LATTICE_PITCH / 2])
    return seeds, lattice_rows(seeds, LATTICE_N, half), grid(BIG_W, BIG_H, bars_skeleton())


def _tiny(n):
    return lambda: (lattice(LATTICE_N, LATTICE_N, LATTICE_PITCH, LATTICE_X0, LATTICE_Y0)[:n],
                    np.array([[118.0, 221.0], [124.0, 221.0]]), grid(G_W, G_H))


def _collinear(dy):
    def build():
        p = np.stack([105.0 + np.arange(40.0), np.full(40, 220.0)], 1)
        if dy:
            p[:, 1] += np.random.default_rng(3).uniform(-dy, dy, 40)
        return p, np.array([[110.0, 225.0], [130.0, 225.0]]), grid(G_W, G_H)
    return build


def _far_seeds():
    near = lattice(12, 10, 3.0, 108.0, 206.0)
    far = np.array([[1e6, 1e6], [-1e6, 220.0], [125.0, 5e5]])
    return np.vstack([near[:60], far[:1], near[60:], far[1:]]), np.array([[110.0, 207.5], [140.0, 207.5]]), grid(G_W, G_H)


def _wide_grid():
    seeds = uniform_seeds(30, 150.0, 450.0, 250.0, 500.0, 9)
    rng = np.random.default_rng(10)
    s = np.stack([rng.uniform(150.0, 450.0, 6), rng.uniform(250.0, 500.0, 6)], 1)
    rows = np.empty((12, 2))
    rows[0::2], rows[1::2] = s, s + rng.uniform(-40.0, 40.0, (6, 2))
    return seeds, rows, grid(WIDE_W, WIDE_H)


def _pairs(n, seed):
    return lambda: (uniform_seeds(n, 101.0, 149.0, 201.0, 239.0, seed),
                    np.array([[110.0, 210.0], [135.0, 214.0], [120.0, 230.0], [120.0, 236.0]]), grid(G_W, G_H))


_ONE_ROW_G = np.array([[110.0, 225.0], [140.0, 228.0]])


def _circle_jitter():
    """Centred on a corner of g5's cell index (the grid +- 10 m; with fewer than 2048 edge ends its cell budget is the
    minimum, whatever their number): the ~90 circumcentres within 0.1 m of the centre lie in four cells."""
    gb = (ORIGIN[0], ORIGIN[0] + G_W * RES, ORIGIN[1], ORIGIN[1] + G_H * RES)
    c = index_corner(gb, BP_RANGE, BP_CELL, 1, 125.0, 220.0)
    # (seed 3: of the seeds 0-11 tried, 3, 8 and 11 leave candidates that only the row above / only the row below decides)
    return circle(96, 12.0, cx=c[0], cy=c[1], jitter=2e-4, seed=3), _ONE_ROW_G, grid(G_W, G_H)

_BUILDERS = {
    "chain-clump": lambda: (chain_clump(), _ONE_ROW_G, grid(G_W, G_H)),
    "chain-clump-shuffled": lambda: (chain_clump()[np.random.default_rng(12).permutation(len(chain_clump()))], _ONE_ROW_G,
                                     grid(G_W, G_H)),
    "circle": lambda: (circle(64, 8.0), _ONE_ROW_G, grid(G_W, G_H)),
    "circle-centre": lambda: (np.vstack([circle(64, 8.0), [[125.0, 220.0]]]), _ONE_ROW_G, grid(G_W, G_H)),
    "circle-jitter": _circle_jitter,
    "lattice": _lattice,
    "collinear": _collinear(0.0),
    "near-collinear": _collinear(1e-3),
    "tiny-1": _tiny(1),
    "tiny-2": _tiny(2),
    "tiny-3": _tiny(3),
    "identical-50": lambda: (np.tile([[123.0, 219.0]], (50, 1)), _ONE_ROW_G, grid(G_W, G_H)),
    "far-seeds": _far_seeds,
    "labels-sparse": _labels_sparse,
    "labels-dup-rows": _labels_dup_rows,
    "no-rows": lambda: (_labels_sparse()[0], np.zeros((0, 2)), _labels_sparse()[2]),
    "wide-grid": _wide_grid,
    "pairs-small": _pairs(150, 31),
    "pairs-big": _pairs(4000, 32),
}

# the scenes that also run with subdiv_rect_mode = 1
RECT_MODE_SCENES = ("circle", "lattice", "collinear", "tiny-1", "tiny-2", "tiny-3", "far-seeds")

# the one-handle sequence (large and small frames alternate)
HANDLE_ORDER = ("pairs-small", "pairs-big", "tiny-1", "chain-clump", "no-rows", "labels-dup-rows", "pairs-small",
                "pairs-big", "circle", "wide-grid", "identical-50", "lattice")


@functools.lru_cache(maxsize=None)
def scene(name):
    """(seeds, rows_info, grid) of the scene; shared between the tests: leave the arrays unchanged."""
    seeds, rows, gr = _BUILDERS[name]()
    seeds, rows = np.ascontiguousarray(seeds, np.float64), np.ascontiguousarray(rows, np.float64)
    for a in (seeds, rows, gr["skeleton_framed"]):
        a.setflags(write=False)
    return seeds, rows, gr


class _Scenes(Mapping):
    """name -> (seeds, rows_info, grid), built on first use."""
    def __getitem__(self, name):
        return scene(name)

    def __iter__(self):
        return iter(_BUILDERS)

    def __len__(self):
        return len(_BUILDERS)


SCENES = _Scenes()


# ---------------------------------------------------------------- regime predictors (on an oracle result)
def _make_hash_n(minx, maxx, miny, maxy, cell, n, cells_per_item=CELLS_PER_ITEM):
    """make_hash_n (csrc/greedy.hip:34-57): (inv, nx, ny, nx * ny of the unenlarged cell, the cell budget)."""
    def make(c):
        inv = 1.0 / (c * (1.0 + 1e-9))
        nx, ny = (maxx - minx) * inv + 2.0, (maxy - miny) * inv + 2.0
        while nx * ny > 2.0e9:
            inv *= 0.5
            nx, ny = (maxx - minx) * inv + 2.0, (maxy - miny) * inv + 2.0
        return inv, max(1, int(nx)), max(1, int(ny))
    cap = max(float(HASH_MIN_CELLS), cells_per_item * max(n, 1))
    c = cell
    inv, nx, ny = make(c)
    first = nx * ny
    while nx * ny > cap:
        c *= HASH_GROW
        inv, nx, ny = make(c)
    return inv, nx, ny, first, cap


def hash_geometry(minx, maxx, miny, maxy, cell, n):
    """(cell size used, nx, ny, nx * ny of the unenlarged cell, the cell budget) of make_hash_n."""
    inv, nx, ny, first, cap = _make_hash_n(minx, maxx, miny, maxy, cell, n)
    return 1.0 / inv, nx, ny, first, cap


def index_cells(p, gr, rng_m, cell, n):
    """hash_cell (csrc/dev_prims_device.h:11-15) of every point in the index make_hash_n(grid +- rng_m, cell, n)."""
    x0, x1, y0, y1 = bounds(gr)
    inv, nx, ny, _, _ = _make_hash_n(x0 - rng_m, x1 + rng_m, y0 - rng_m, y1 + rng_m, cell, n)
    out = []
    for v, lo, m in ((p[:, 0], x0 - rng_m, nx), (p[:, 1], y0 - rng_m, ny)):
        f = (v - lo) * inv
        c = np.trunc(np.clip(np.nan_to_num(f, nan=0.0), 0.0, float(m))).astype(np.int64)
        out.append(np.where(~(f > 0.0), 0, np.where(f >= m - 1, m - 1, c)))
    return out[0], out[1]


def over_rows(p, cy, mode):
    """Replays the greedy de-duplication over the points p in order and looks at every removed candidate that takes
    k_lfmis' `over` branch (more than LF_LIST earlier conflicting candidates; g5: and no earlier identical one).
    mode "merge" (g1, OWNER): the index row of its owner, the smallest kept conflicting candidate, minus its own.
    mode "ends" (g5): the common row offset of all its kept conflicting candidates, if they share one.
    Returns the set of these offsets: -1 and +1 in it mean the re-walk's outer rows decide some candidate."""
    n = len(p)
    kept = np.zeros(n, bool)
    if mode == "ends":
        kx, ky = _trunc_key(p[:, 0]), _trunc_key(p[:, 1])
    out = set()
    for i in range(n):
        dx, dy = p[:i, 0] - p[i, 0], p[:i, 1] - p[i, 1]
        if mode == "merge":
            conf = np.sqrt(dx * dx + dy * dy) <= MERGE_R
            dup = False
        else:
            conf = ((kx[:i] == kx[i]) & (ky[:i] == ky[i])) | (dx * dx + dy * dy < BP_THR_SQ)
            dup = bool(((dx == 0) & (dy == 0)).any())
        kc = np.nonzero(conf & kept[:i])[0]
        kept[i] = len(kc) == 0
        if kept[i] or dup or np.count_nonzero(conf) <= LF_LIST:
            continue
        off = cy[kc] - cy[i]
        if mode == "merge":
            out.add(int(off[0]))
        elif (off == off[0]).all():
            out.add(int(off[0]))
    return out


def node_index_geometry(gr, og):
    x0, x1, y0, y1 = bounds(gr)
    r = NODE_RANGE
    return hash_geometry(x0 - r, x1 + r, y0 - r, y1 + r, NODE_CELL, 2 * len(og["vor_edges"]))


def earlier_conflicts_merge(seeds):
    """g1 (k_lfmis<OWNER>, kConflictLessEq): per seed, how many earlier seeds lie within 0.5 m (sqrt of the squared
    distance, as conflict() computes it)."""
    from scipy.spatial import cKDTree
    s = np.asarray(seeds, np.float64)
    fin = np.isfinite(s).all(1)
    out = np.zeros(len(s), np.int64)
    idx = np.nonzero(fin)[0]
    tree = cKDTree(s[idx])
    for a, nb in zip(idx, tree.query_ball_point(s[idx], MERGE_R + 1e-9)):
        j = idx[np.asarray(nb, np.int64)]
        j = j[j < a]
        d = s[j] - s[a]
        out[a] = np.count_nonzero(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) <= MERGE_R)
    return out


def longest_index_chain(seeds):
    """The longest run of consecutive indices with |s[i] - s[i - 1]| <= 0.5: k_lfmis decides them one after the other."""
    s = np.asarray(seeds, np.float64)
    d = s[1:] - s[:-1]
    c = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) <= MERGE_R
    best = run = 0
    for v in c:
        run = run + 1 if v else 0
        best = max(best, run)
    return best + 1 if best else 0


def _trunc_key(v):
    w = v * 100
    ok = (w > -2147483649.0) & (w < 2147483648.0)   # x86_trunc_i32 (csrc/greedy.hip:290)
    return np.where(ok, np.trunc(np.where(ok, w, 0.0)), -2147483648.0).astype(np.int64)


def earlier_conflicts_ends(og):
    """g5 (k_lfmis<false>, kConflictKeyOrSq) over the 2E edge ends in vor_edges order: per end, how many earlier
    non-identical ends conflict with it (the same 1 cm key, or d^2 < 0.0025), and whether an earlier end is identical
    (such an end is removed at once and never waits)."""
    e = og["vor_edges"].reshape(-1, 2)
    kx, ky = _trunc_key(e[:, 0]), _trunc_key(e[:, 1])
    n = len(e)
    cnt, dup = np.zeros(n, np.int64), np.zeros(n, bool)
    for i in range(1, n):
        dx, dy = e[:i, 0] - e[i, 0], e[:i, 1] - e[i, 1]
        same = (dx == 0) & (dy == 0)
        conf = ((kx[:i] == kx[i]) & (ky[:i] == ky[i])) | (dx * dx + dy * dy < BP_THR_SQ)
        cnt[i] = np.count_nonzero(conf & ~same)
        dup[i] = same.any()
    return cnt, dup


def pair_count(og):
    """P of run_gvd_stage: pairs i < j of the boundary points with 1e-6 < d <= 0.5 (csrc/gvd.hip, pairs_of)."""
    from scipy.spatial import cKDTree
    b = og["boundary_raw"]
    if len(b) < 2:
        return 0
    pr = cKDTree(b).query_pairs(PAIR_MAX + 1e-9, output_type="ndarray")
    d = b[pr[:, 0]] - b[pr[:, 1]]
    d = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    return int(np.count_nonzero((d <= PAIR_MAX) & (d > PAIR_MIN)))


def pair_cap_first(og):
    return max(PAIR_CAP_MIN, 2 * (2 * len(og["vor_edges"])))


def pair_cap_next(P):
    return max(PAIR_CAP_MIN, P + P // 4)


def rerun_pattern(results):
    """Per frame of one handle (oracle results in order): (P, capacity the frame starts with, whether it reruns).
    A frame that ends before g6 (not published, or no Voronoi edge) leaves the capacity as it was."""
    out, cap = [], 0
    for og in results:
        if not og["published"] or len(og["vor_edges"]) == 0:
            out.append((0, cap, False))
            continue
        P = pair_count(og)
        c = cap if cap > 0 else pair_cap_first(og)
        out.append((P, c, P > c))
        cap = pair_cap_next(P)
    return out


def label_jobs(rows_info):
    """run_gvd_stage's jobs (csrc/gvd.hip, label_jobs): (ex, ey, ox, oy, deg) per (row, label), 4 per row."""
    r = np.asarray(rows_info, np.float64).reshape(-1, 4)
    jobs = []
    for sx, sy, ex, ey in r:
        if sx > ex:
            sx, sy, ex, ey = ex, ey, sx, sy
        jobs += [(sx, sy, ex, ey, -90.0), (sx, sy, ex, ey, 90.0), (ex, ey, sx, sy, -90.0), (ex, ey, sx, sy, 90.0)]
    return np.array(jobs, np.float64).reshape(-1, 5)


def label_candidates(job, nodes, diag2):
    """k_label_points' test (csrc/gvd.hip, the `test` lambda) on every node: (valid mask, distances)."""
    ex, ey, ox, oy, deg = job
    mdx, mdy = ox - ex, oy - ey
    ml = np.sqrt(mdx * mdx + mdy * mdy)
    if ml < 1e-6:
        mdx, mdy = 1.0, 0.0
    else:
        mdx, mdy = mdx / ml, mdy / ml
    outx, outy, perx, pery = -mdx, -mdy, -mdy, mdx
    dx, dy = nodes[:, 0] - ex, nodes[:, 1] - ey
    z = dx * dx + dy * dy
    dist = np.sqrt(z)
    s = np.where(z > 0.0, dist, 1.0)
    nx, ny = dx / s, dy / s
    ok = ~((dist < 0.5) | (dist > max(9.0, diag2))) & ~(outx * nx + outy * ny < 0.0)
    dp = perx * nx + pery * ny
    ok &= ~(dp > 0.0) if deg < 0 else ~(dp < 0.0)
    return ok, dist


def label_regime(rows_info, gr, og):
    """Per valid label job: the class of its point and whether its arg-min is an exact tie.
    classes: 0 a node within pass 0's reach (z <= 25 (1 + 1e-12)); 1 a node nearer than pass 1's `two_cells`; 2 a node
    at `two_cells` or beyond (pass 2: the full scan); 3 no candidate (castRay)."""
    nodes = og["nodes"]
    x0, x1, y0, y1 = bounds(gr)
    diag2 = np.sqrt((x1 - x0) ** 2 + (y1 - y0) ** 2) * 2.0
    cell = node_index_geometry(gr, og)[0]
    two_cells = 2.0 * cell * (1.0 - 1e-9)    # csrc/gvd.hip, k_label_points (cell = 1 / cn.h.inv)
    jobs = label_jobs(rows_info)
    valid = og["row_label_valid"].reshape(-1)
    pts = og["row_label_pts"].reshape(-1, 2)
    assert len(valid) == len(jobs)
    cls, ties = np.full(len(jobs), -1), np.zeros(len(jobs), bool)
    for j, job in enumerate(jobs):
        if not valid[j]:
            continue
        ok, dist = label_candidates(job, nodes, diag2)
        if not ok.any():
            cls[j] = 3
            assert not (nodes == pts[j]).all(1).any(), (j, pts[j])   # castRay's point is not a node
            continue
        best = dist[ok].min()
        first = np.nonzero(ok & (dist == best))[0]
        assert np.array_equal(nodes[first[0]], pts[j]), (j, nodes[first[0]], pts[j])   # the predictor restates the oracle
        ties[j] = len(first) > 1
        cls[j] = 0 if best * best <= 25.0 * (1.0 + 1e-12) else 1 if best < two_cells else 2
    return cls, ties, two_cells


# ---------------------------------------------------------------- the regime each scene is for
def check_regime(name, og, oracle_of=None):
    """Asserts the scene's regime on its oracle result og (markers = 1); returns the figures. oracle_of(name): the
    oracle result of another scene, for the two scenes that are defined against one."""
    seeds, rows, gr = scene(name)
    x0, x1, y0, y1 = bounds(gr)
    inside = ((og["nodes"][:, 0] >= x0) & (og["nodes"][:, 0] <= x1) & (og["nodes"][:, 1] >= y0) &
              (og["nodes"][:, 1] <= y1)) if len(og["nodes"]) else np.zeros(0, bool)
    fig = {"published": og["published"], "seeds": len(seeds), "merged": len(og["merged"]),
           "vor_edges": len(og["vor_edges"]), "boundary": len(og["boundary_raw"]), "nodes": len(og["nodes"]),
           "edges": len(og["edges"]), "label_entries": len(og["node_label_clusters"])}
    assert og["published"], fig
    if name in ("chain-clump", "chain-clump-shuffled"):
        fig["earlier_conflicts_max"] = int(earlier_conflicts_merge(seeds).max())
        assert fig["earlier_conflicts_max"] > LF_LIST, fig
        assert fig["merged"] < fig["seeds"], fig
        if name == "chain-clump":
            fig["chain"] = longest_index_chain(seeds)
            assert fig["chain"] >= 4 * LF_TB, fig
            cy = index_cells(seeds, gr, MERGE_RANGE, MERGE_R, len(seeds))[1]
            fig["over_owner_rows"] = sorted(over_rows(seeds, cy, "merge"))
            assert {-1, 1} <= set(fig["over_owner_rows"]), fig
        else:
            other = oracle_of("chain-clump")["merged"]
            fig["merged_unshuffled"] = len(other)
            assert sorted(map(tuple, other)) != sorted(map(tuple, og["merged"])), fig
    elif name == "circle-centre":
        # With a seed at the centre no Voronoi vertex lies there: the vertices are the circumcentres of (centre, p_k,
        # p_k+1), 64 distinct points on a circle of half the radius, the corners of the centre's one facet. What the
        # scene has instead of `circle`'s coincident ends: one facet of 64 corners and the ring graph around it.
        cnt, dup = earlier_conflicts_ends(og)
        fig["earlier_conflicts_max"] = int(cnt[~dup].max())
        e = np.unique(og["vor_edges"].reshape(-1, 2), axis=0)
        r = np.hypot(e[:, 0] - 125.0, e[:, 1] - 220.0)
        fig["distinct_ends_on_inner_circle"] = int(np.count_nonzero(np.abs(r - 4.0 / np.cos(np.pi / 64)) < 0.01))
        fig["cell_corners_max"] = int(np.diff(og["cell_offsets"]).max())
        assert fig["distinct_ends_on_inner_circle"] == 64 and fig["cell_corners_max"] >= 64, fig
        assert fig["nodes"] == 64 and fig["edges"] == 64 and fig["earlier_conflicts_max"] <= LF_LIST, fig
    elif name in ("circle", "circle-jitter"):
        cnt, dup = earlier_conflicts_ends(og)
        fig["ends_over"] = int(np.count_nonzero((cnt > LF_LIST) & ~dup))
        fig["earlier_conflicts_max"] = int(cnt[~dup].max())
        assert fig["earlier_conflicts_max"] > LF_LIST, fig
        if name == "circle-jitter":
            assert fig["nodes"] > 1 and fig["edges"] > 0, fig
            ends = og["vor_edges"].reshape(-1, 2)
            assert 2 * len(ends) < HASH_MIN_CELLS   # (what _circle_jitter places its centre by)
            cy = index_cells(ends, gr, BP_RANGE, BP_CELL, len(ends))[1]
            fig["over_kept_rows"] = sorted(over_rows(ends, cy, "ends"))
            assert {-1, 1} <= set(fig["over_kept_rows"]), fig
        else:
            e = np.unique(og["vor_edges"].reshape(-1, 2), axis=0)
            fig["distinct_ends_near_centre"] = int(np.count_nonzero(np.hypot(e[:, 0] - 125.0, e[:, 1] - 220.0) < 0.05))
            assert fig["distinct_ends_near_centre"] >= 50, fig
    elif name == "lattice":
        cls, ties, _ = label_regime(rows, gr, og)
        fig["label_jobs"], fig["tied_jobs"] = int(np.count_nonzero(cls >= 0)), int(np.count_nonzero(ties))
        assert fig["tied_jobs"] >= 100, fig
        assert fig["nodes"] > NEAR_THREADS, fig
    elif name in ("collinear", "near-collinear"):
        fig["nodes_inside"] = int(np.count_nonzero(inside))
        fig["merged_y_extent"] = float(np.ptp(og["merged"][:, 1]))
        assert fig["nodes"] == 0 and fig["nodes_inside"] == 0, fig
        assert fig["merged_y_extent"] < 1.0, fig    # extractCellBoundaries widens the seeds' box to 1 m
    elif name in ("tiny-1", "tiny-2", "tiny-3", "identical-50"):
        want = {"tiny-1": 3, "tiny-2": 7, "tiny-3": 11, "identical-50": 3}[name]
        assert fig["vor_edges"] == want and fig["nodes"] == 0, fig
        if name == "identical-50":
            assert fig["merged"] == 1, fig
    elif name == "far-seeds":
        r = MERGE_RANGE
        far = (seeds[:, 0] < x0 - r) | (seeds[:, 0] > x1 + r) | (seeds[:, 1] < y0 - r) | (seeds[:, 1] > y1 + r)
        fig["far_seeds"] = int(np.count_nonzero(far))
        e = og["vor_edges"].reshape(-1, 2)
        r = BP_RANGE
        fig["ends_beyond_index"] = int(np.count_nonzero((e[:, 0] < x0 - r) | (e[:, 0] > x1 + r) | (e[:, 1] < y0 - r) |
                                                        (e[:, 1] > y1 + r)))
        assert fig["far_seeds"] == 3 and fig["ends_beyond_index"] > 0 and fig["nodes"] > 0, fig
    elif name == "labels-sparse":
        cls, ties, two = label_regime(rows, gr, og)
        fig["two_cells"] = two
        fig["classes"] = [int(np.count_nonzero(cls == k)) for k in range(4)]
        fig["invalid_jobs"] = int(np.count_nonzero(cls < 0))
        assert min(fig["classes"]) >= 8, fig
    elif name == "labels-dup-rows":
        fig["label_count_max"] = int(og["node_label_counts"].max())
        fig["nodes_over"] = int(np.count_nonzero(og["node_label_counts"] > NODE_MATCH))
        assert fig["nodes_over"] >= 1, fig
    elif name == "no-rows":
        assert fig["nodes"] > 0 and fig["label_entries"] == 0 and len(og["row_label_valid"]) == 0, fig
    elif name == "wide-grid":
        size, nx, ny, first, cap = node_index_geometry(gr, og)
        fig.update(node_cell=size, node_cells_unenlarged=first, node_cell_budget=cap)
        assert first > cap and size > NODE_CELL * (1.0 + 1e-9) * 1.2, fig
        nj = 2 * len(rows)
        lab = hash_geometry(x0 - LABEL_RANGE, x1 + LABEL_RANGE, y0 - LABEL_RANGE, y1 + LABEL_RANGE, LABEL_CELL, nj)
        r = BP_RANGE
        bp = hash_geometry(x0 - r, x1 + r, y0 - r, y1 + r, BP_CELL, 2 * fig["vor_edges"])
        fig.update(label_cell=lab[0], bp_cell=bp[0])
        assert lab[3] > lab[4] and bp[3] > bp[4], fig
        assert fig["nodes"] > 0 and fig["label_entries"] > 0, fig
    elif name in ("pairs-small", "pairs-big"):
        fig["P"], fig["cap_first"] = pair_count(og), pair_cap_first(og)
        fig["cap_next"] = pair_cap_next(fig["P"])
        if name == "pairs-small":
            assert fig["cap_next"] == PAIR_CAP_MIN and fig["P"] > 0, fig
        else:
            assert fig["P"] > PAIR_CAP_MIN, fig
    else:
        raise KeyError(name)
    return fig


# ---------------------------------------------------------------- path planning on the lattice graph
PATH_TRUNCATIONS = (1, 2, 4, 5, 6, 64, 511, 512, 513)   # around kNearK = 5 and kNearThreads = 512


def truncated_graph(g, m):
    """The GvdGraph of g's first m nodes: the edges with both ends below m, the label entries of those nodes."""
    ne = int(np.sum(g["node_label_counts"][:m]))
    keep = (g["edges"] < m).all(1)
    return {"nodes": g["nodes"][:m].copy(), "node_labels": g["node_labels"][:m].copy(),
            "node_cluster_indices": g["node_cluster_indices"][:m].copy(),
            "node_label_counts": g["node_label_counts"][:m].copy(),
            "node_label_clusters": g["node_label_clusters"][:ne].copy(),
            "node_label_types": g["node_label_types"][:ne].copy(),
            "edges": g["edges"][keep].copy(), "edge_lengths": g["edge_lengths"][keep].copy()}


def path_queries(g):
    """The planner states run on every graph: the first targets, the initial straight line to a point exactly on a
    node, exactly midway between two nodes and on the last node (across the skeleton's bars: trimmed), the robot on a
    lattice point (its nearest nodes tie exactly, k_nearest_k's (distance, index) order) and far outside the grid."""
    n = g["nodes"]
    mid = (n[0] + n[min(1, len(n) - 1)]) / 2
    sym = (LATTICE_X0 + 2 * LATTICE_PITCH, LATTICE_Y0 + LATTICE_PITCH)
    return [dict(target=0), dict(target=1, previous=0),
            dict(initial_waypoint_reached=False, initial_waypoint=(float(n[0, 0]), float(n[0, 1]))),
            dict(initial_waypoint_reached=False, initial_waypoint=(float(mid[0]), float(mid[1]))),
            dict(initial_waypoint_reached=False, initial_waypoint=(float(n[-1, 0]), float(n[-1, 1]))),
            dict(target=0, current=sym), dict(target=1, previous=0, current=sym),
            dict(target=1, current=(1.0e4, -3.0e3))]


def nearest_ties(g, p, k=NEAR_K):
    """Whether the k-th and (k + 1)-th nearest nodes of p are exactly as far (the index decides), or, with at most k
    nodes, any two are."""
    d = g["nodes"] - np.asarray(p, np.float64)
    d = np.sort(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
    return bool(d[k - 1] == d[k]) if len(d) > k else bool(len(d) > 1 and (d[1:] == d[:-1]).any())
