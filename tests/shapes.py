"""Non-orchard scenes for the parity tests (test infrastructure, imported like parity_util).

A binary raster is injected exactly through a point cloud: three points (z = 0, 0.01, 0.02) at the centre of
each set cell survive the default ROR (r = 0.2, minN = 2: the two others are 0.01 / 0.02 m away, the next cell's
0.25 m), the grid resolution is 0.25 and the polygon's lower-left corner is (256, 256), so every coordinate is
exact in float32 and far from the eleven exclusion discs. The grid is the polygon's box plus 2.5 m = 10 cells on
every side (origin 253.5), and points in that margin are rasterised too, so border cells can be set directly.
R = int(inflation_radius / 0.25): inflation_radius = 0.25 R + 0.01 selects R exactly.

The regime predictors restate the library's branch conditions on an oracle result, each constant named with its
source; tests/test_shapes_cpu.py checks every scene against them without a GPU.
"""
import functools
import math

import numpy as np

RES = 0.25
MARGIN = 10            # cells: getActiveBounds' 2.5 m margin (oracle_seedgen.cpp active_bounds) at RES
POLY_X0 = POLY_Y0 = 256.0
ORIGIN = POLY_X0 - MARGIN * RES   # 253.5

# the library's constants the predictors use
CCL_CHUNK = 2048       # csrc/cluster_seed.hip:111  kCclChunk
CCL_EDGE_LDS = 1024    # csrc/cluster_seed.hip:120  kCclEdgeLds
CCL_ECAP_MIN = 4096    # csrc/cluster_seed.hip:117  ccl_edge_cap: max(4096, nf / 4)
CL_COUNT_TB = 256      # csrc/cluster_seed.hip:294  kClTB (cells per k_cluster_count block)
STAT_LDS = 16384       # csrc/cluster_seed.hip:379  kStatLds
STAT_CAND = 2048       # csrc/cluster_seed.hip:386  cand[2048] (all-pairs branch beyond it, :475)
EXACT_SUM = 1 << 24    # csrc/cluster_seed.hip:491  exact_sums
ROW_CROSS_MAX = 256    # csrc/cluster_dev.h:19      kRowCrossMax
THIN_TH = 128          # csrc/grid_kernels.hip:216  AOS_THIN_TH (tile rows)
THIN_TW = 8 * 64       # csrc/grid_kernels.hip:218  TWW = 8 words (tile columns)
THIN_KIT = 8           # csrc/aos_internal.h:210    kThinItersPerLaunch
REPLAY_LDS_BYTES = 64 * 1024   # csrc/replay_gpu.hip:90 the GPU walk's box bitmap budget

_ORACLE_NAME = {"clipping_minz": "clip_minz", "clipping_maxz": "clip_maxz", "clipping_minx": "clip_minx",
                "clipping_maxx": "clip_maxx", "clipping_miny": "clip_miny", "clipping_maxy": "clip_maxy"}
_AOS_ONLY = ("thin_graph", "gvd_markers", "gvd_count_evals", "max_graph_publish_rate")


# ---------------------------------------------------------------- scene
def margin_cells(res=RES):
    """getActiveBounds' 2.5 m margin in cells of `res`, which must divide it (MARGIN at RES)."""
    m = 2.5 / res
    if m != int(m) or np.float32(res) != res:
        raise ValueError(f"res = {res}: a float32 binary fraction that divides the 2.5 m margin is needed")
    return int(m)


def rect_polygon(W, H, res=RES):
    m = margin_cells(res)
    x1, y1 = POLY_X0 + (W - 2 * m) * res, POLY_Y0 + (H - 2 * m) * res
    return np.array([[POLY_X0, POLY_Y0], [x1, POLY_Y0], [x1, y1], [POLY_X0, y1]], np.float64)


def scene(pattern, R, polygon=None, res=RES, **params):
    """(cloud, polygon, aos_kwargs, oracle_kwargs) of the frame whose raster is `pattern` (the whole H x W grid;
    the polygon spans cells [10, W - 10) x [10, H - 10)). polygon= overrides the rectangle with the same box.
    res= another grid resolution (0.15625, 0.3125, 0.5: the margin is then 2.5 / res cells instead of 10)."""
    pattern = np.asarray(pattern)
    H, W = pattern.shape
    margin = margin_cells(res)
    if W <= 2 * margin or H <= 2 * margin:
        raise ValueError(f"pattern {W} x {H}: the grid is the polygon's box plus {margin} cells on every side")
    rect = rect_polygon(W, H, res)
    if polygon is None:
        polygon = rect
    else:
        polygon = np.asarray(polygon, np.float64)
        if not (np.array_equal(polygon.min(0), rect.min(0)) and np.array_equal(polygon.max(0), rect.max(0))):
            raise ValueError("polygon= must keep the rectangle's bounding box")
    ys, xs = np.nonzero(pattern)
    pts = np.zeros((3 * len(xs), 4), np.float32)
    for k, z in enumerate((0.0, 0.01, 0.02)):
        pts[k::3, 0] = ORIGIN + (xs + 0.5) * res
        pts[k::3, 1] = ORIGIN + (ys + 0.5) * res
        pts[k::3, 2] = z
    cloud = pts.view(np.uint8).reshape(-1, 16)
    akw = dict(grid_resolution=res, inflation_radius=res * R + 0.01, **params)
    okw = {_ORACLE_NAME.get(k, k): v for k, v in akw.items() if k not in _AOS_ONLY}
    return cloud, polygon, akw, okw


# ---------------------------------------------------------------- pattern builders
def _empty(W, H):
    return np.zeros((H, W), np.uint8)


def disc_lattice(W, H, y0, y1, x0, x1, step):
    """Lattice points; inflated by R >= step / sqrt(2) they merge into one solid rectangle."""
    p = _empty(W, H)
    p[y0:y1:step, x0:x1:step] = 1
    return p


def dots(W, H, y0, y1, x0, x1, step):
    p = _empty(W, H)
    p[y0:y1:step, x0:x1:step] = 1
    return p


def comb(W, H, y0, y1, x0, x1, step):
    """Vertical teeth: columns x0, x0 + step, ... over rows [y0, y1)."""
    p = _empty(W, H)
    p[y0:y1, x0:x1:step] = 1
    return p


def lines(W, H, y0, y1, step, x0=None, x1=None):
    """Horizontal lines on rows y0, y0 + step, ... < y1 over columns [x0, x1) (default: the polygon's)."""
    p = _empty(W, H)
    p[y0:y1:step, (MARGIN if x0 is None else x0):(W - MARGIN if x1 is None else x1)] = 1
    return p


def random_sparse(W, H, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


def _plot(p, x, y):
    xi, yi = np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)
    ok = (xi >= 0) & (xi < p.shape[1]) & (yi >= 0) & (yi < p.shape[0])
    p[yi[ok], xi[ok]] = 1


def ring(W, H, cx, cy, r):
    t = np.linspace(0.0, 2 * np.pi, int(8 * 2 * np.pi * r) + 1)
    p = _empty(W, H)
    _plot(p, cx + r * np.cos(t), cy + r * np.sin(t))
    return p


def spiral(W, H, cx, cy, turns, pitch):
    """Archimedean spiral, radius pitch * turns at its outer end."""
    rmax = pitch * turns
    t = np.linspace(0.0, 2 * np.pi * turns, int(8 * 2 * np.pi * rmax * turns) + 1)
    rr = pitch * t / (2 * np.pi)
    p = _empty(W, H)
    _plot(p, cx + rr * np.cos(t), cy + rr * np.sin(t))
    return p


def star(W, H, cx, cy, arms, length, hub_r):
    """A hub ring of radius hub_r with `arms` straight arms of `length` cells leaving it."""
    p = ring(W, H, cx, cy, hub_r)
    rr = np.linspace(hub_r, hub_r + length, 4 * length + 1)
    for k in range(arms):
        a = 2 * np.pi * k / arms
        _plot(p, cx + rr * math.cos(a), cy + rr * math.sin(a))
    return p


def sawtooth_polygon(W, H, teeth, h0, h1, valley=3.0):
    """The scene's rectangle with `teeth` teeth cut into its top edge: apexes rising from h0 to h1 metres above the
    bottom edge, valleys at `valley` metres between them, the two top corners kept (so the bounding box stays):
    2 * teeth + 3 vertices."""
    rect = rect_polygon(W, H)
    x0, y0, x1, y1 = rect[0, 0], rect[0, 1], rect[2, 0], rect[2, 1]
    pitch = (x1 - x0) / (teeth + 1)
    top = [(x1, y1)]
    for k in range(teeth - 1, -1, -1):   # right to left
        top.append((x0 + (k + 1) * pitch, y0 + h0 + (h1 - h0) * k / max(teeth - 1, 1)))
        if k:
            top.append((x0 + (k + 0.5) * pitch, y0 + valley))
    top.append((x0, y1))
    return np.array([(x0, y0), (x1, y0)] + top, np.float64)


# ---------------------------------------------------------------- regime predictors (on an oracle result)
def _fg_rank(o):
    """H x W: a foreground cell's index in the raster-order list (k_fg_list), -1 elsewhere. The foreground is the
    union of the oracle's clusters (skeleton cells inside the polygon)."""
    H, W = o["height"], o["width"]
    fg = np.zeros((H, W), bool)
    cc = o["cluster_cells"]
    fg[cc[:, 1], cc[:, 0]] = True
    rank = np.full((H, W), -1, np.int64)
    rank[fg] = np.arange(int(fg.sum()))
    return rank


def ccl_links(o, chunk=CCL_CHUNK):
    """(nf, most cross-chunk links of one chunk, all cross-chunk links, the link list's capacity max(4096, nf // 4)):
    k_ccl_local's links of a cell to its three upper-row 8-neighbours whose list index lies below the cell's chunk."""
    rank = _fg_rank(o)
    nf = int(rank.max()) + 1
    per_chunk = np.zeros(max(1, -(-nf // chunk)), np.int64)
    up = np.full_like(rank, -1)
    up[1:] = rank[:-1]
    for dx in (-1, 0, 1):
        nb = np.full_like(rank, -1)
        if dx == -1:
            nb[:, 1:] = up[:, :-1]
        elif dx == 1:
            nb[:, :-1] = up[:, 1:]
        else:
            nb = up
        m = (rank >= 0) & (nb >= 0)
        i, j = rank[m], nb[m]
        cross = j < (i // chunk) * chunk
        np.add.at(per_chunk, i[cross] // chunk, 1)
    return nf, int(per_chunk.max()), int(per_chunk.sum()), max(CCL_ECAP_MIN, nf // 4)


def max_clusters_per_count_block(o):
    """The most distinct clusters among CL_COUNT_TB consecutive foreground cells (one k_cluster_count block)."""
    H, W = o["height"], o["width"]
    cid = np.full((H, W), -1, np.int64)
    cc, off = o["cluster_cells"], o["cluster_offsets"]
    cid[cc[:, 1], cc[:, 0]] = np.repeat(np.arange(len(off) - 1), np.diff(off))
    ids = cid[cid >= 0]   # raster order
    return max((len(np.unique(ids[b:b + CL_COUNT_TB])) for b in range(0, len(ids), CL_COUNT_TB)), default=0)


def stats_regime(o):
    """Per cluster (n, length candidates by k_cluster_stats' rule, sum x, sum y, box bits of the bordered bitmap, LB).
    The rule (cluster_seed.hip:438-465): LB = the larger squared distance between the cells of extreme x and of
    extreme y (ties: the smallest raster index); a cell is a candidate iff dxm^2 + dym^2 >= LB, dxm / dym its
    larger distance to the box's sides."""
    W = o["width"]
    cc, off = o["cluster_cells"].astype(np.int64), o["cluster_offsets"]
    out = []
    for c in range(len(off) - 1):
        x, y = cc[off[c]:off[c + 1], 0], cc[off[c]:off[c + 1], 1]
        p = y * W + x
        ix0, ix1 = np.lexsort((p, x))[0], np.lexsort((p, -x))[0]
        iy0, iy1 = np.lexsort((p, y))[0], np.lexsort((p, -y))[0]
        d2 = lambda a, b: (x[a] - x[b]) ** 2 + (y[a] - y[b]) ** 2   # noqa: E731
        LB = max(d2(ix0, ix1), d2(iy0, iy1))
        dxm = np.maximum(x - x.min(), x.max() - x)
        dym = np.maximum(y - y.min(), y.max() - y)
        ncand = int(np.count_nonzero(dxm * dxm + dym * dym >= LB))
        bw, bh = int(x.max() - x.min()) + 3, int(y.max() - y.min()) + 3   # a zero border of one cell
        out.append((len(x), ncand, int(x.sum()), int(y.sum()), (-(-bw // 32) * 32) * bh, int(LB)))
    return out


def quiet_solid_tiles(o):
    """Thinning tiles (r, c), r >= 1 and c >= 1, whose 3 x 3 tile block grown by THIN_KIT cells on every side is all
    ones in o["opened"]: nothing inside the block is deleted during the first launch, so the centre tile is copied
    through from the second launch on until the erosion front arrives."""
    op = np.asarray(o["opened"]) != 0
    H, W = op.shape
    out = []
    for r in range(1, -(-H // THIN_TH)):
        for c in range(1, -(-W // THIN_TW)):
            y0, y1 = (r - 1) * THIN_TH - THIN_KIT, (r + 2) * THIN_TH + THIN_KIT
            x0, x1 = (c - 1) * THIN_TW - THIN_KIT, (c + 2) * THIN_TW + THIN_KIT
            # (a negative start would silently give an empty slice, whose all() is true)
            if y0 < 0 or x0 < 0 or y1 > H or x1 > W:
                continue
            if op[y0:y1, x0:x1].all():
                out.append((r, c))
    return out


def row_crossings(polygon, o):
    """Per grid row, the polygon edges that straddle it (row_crossings, cluster_dev.h:28:
    fabs(dy) > 1e-9 && (piy > py) != (pjy > py)), py the row's cell_world (cluster_geom.h:53)."""
    poly = np.asarray(polygon, np.float64)
    res = np.float32(o["resolution"])
    py = (o["origin"][1] + (np.arange(o["height"], dtype=np.float32) * res).astype(np.float64)).astype(np.float32)
    py = py.astype(np.float64)[:, None]
    piy, pjy = poly[:, 1][None, :], np.roll(poly[:, 1], 1)[None, :]
    return np.count_nonzero((np.abs(pjy - piy) > 1e-9) & ((piy > py) != (pjy > py)), axis=1)


# ---------------------------------------------------------------- the grid scenes (test_gpu_shapes_grid.py)
# (W, H, R): every W mod 64 in {0, 1, 63}, W mod 16 != 0, WW mod 8 in {0, 1}, H mod 128 in {0, 1, 127}, H mod 4 != 0,
# R = 0 (identity), 1, 3, 15 and 63 (a disc wider than a word)
# (the issue's H = 5 cannot exist: the grid is the polygon's box plus 10 cells on every side, so the smallest grid of a
# polygon one cell high has H = 21; that size, H mod 4 = 1, takes its place)
H_MIN = 2 * MARGIN + 1
GRID_CASES = [
    (64, 127, 0), (64, 257, 15), (65, H_MIN, 1), (65, 128, 63), (65, 131, 3),
    (127, 127, 1), (127, 129, 63), (127, 257, 0), (193, 128, 15), (193, 131, 1), (193, H_MIN, 3),
    (512, 127, 3), (512, 129, 0), (512, 257, 15), (513, 128, 1), (513, 131, 15), (513, H_MIN, 0),
    (577, 127, 15), (577, 129, 3), (577, 257, 1),
]


def border_pattern(W, H, seed, density=0.004):
    """random_sparse plus set cells in the four corners and along the grid's border rows and columns."""
    p = random_sparse(W, H, density, seed)
    p[[0, 0, -1, -1], [0, -1, 0, -1]] = 1
    p[0, 3::7] = 1
    p[-1, 5::11] = 1
    p[2::9, 0] = 1
    p[4::5, -1] = 1
    return p


def grid_case_seed(W, H, R):
    return (W * 1000 + H) * 100 + R


BLOB = dict(W=2200, H=660, R=15)


def blob_pattern():
    return disc_lattice(BLOB["W"], BLOB["H"], 110, 540, 490, 2080, 20)


GRID_A, GRID_B = (577, 257), (193, 131)


def handle_frames():
    """The frames of the one-handle sequence: (name, (W, H), pattern), R = 3 throughout."""
    def blob(W, H):
        p = random_sparse(W, H, 0.004, W + H)
        p[H // 2 - 45:H // 2 + 45:4, W // 2 - 80:W // 2 + 80:4] = 1   # ~ 166 x 96 solid after inflation: T ~ 49
        return p
    return [("A sparse", GRID_A, random_sparse(*GRID_A, 0.004, 1)), ("A blob", GRID_A, blob(*GRID_A)),
            ("B sparse", GRID_B, random_sparse(*GRID_B, 0.004, 2)), ("A blob again", GRID_A, blob(*GRID_A)),
            ("A empty", GRID_A, _empty(*GRID_A)), ("B blob", GRID_B, blob(*GRID_B))]


HANDLE_R = 3


# ---------------------------------------------------------------- the cluster scenes (test_gpu_shapes_cluster.py)
def _comb_mixed():
    p = comb(4500, 200, 20, 34, 30, 4470, 4)
    return p | lines(4500, 200, 50, 181, 6)


def _spiral_with_dots():
    return spiral(1500, 700, 1100, 350, 22, 14) | dots(1500, 700, 20, 120, 20, 200, 6)


# name -> (pattern builder, R, polygon builder or None[, parameters]). The -length scenes: cluster_min_length between
# the length the pruning bound LB alone gives (200.001 / 159.5 m) and the farthest pair's (200.32 / 159.81 m), so the
# cluster is a tree row at all only if the all-pairs branch finds that pair (the length filter's edge; the other
# scenes see the branch's result in row_length).
CLUSTER_SCENES = {
    "ring": (lambda: ring(900, 900, 450, 450, 400), 2, None),
    "ring-length": (lambda: ring(900, 900, 450, 450, 400), 2, None, {"cluster_min_length": 200.16}),
    "star-length": (lambda: star(700, 700, 350, 350, 48, 280, 40), 1, None, {"cluster_min_length": 159.65}),
    "spiral": (_spiral_with_dots, 2, None),
    "star": (lambda: star(700, 700, 350, 350, 48, 280, 40), 1, None),
    "dots": (lambda: dots(1100, 300, 20, 280, 20, 1080, 6), 2, None),
    "comb-wide": (lambda: comb(8400, 60, 20, 40, 30, 8370, 4), 1, None),
    "comb-mixed": (_comb_mixed, 1, None),
    "sawtooth": (lambda: lines(4500, 200, 12, 190, 6), 1, lambda: sawtooth_polygon(4500, 200, 300, 8.0, 43.0)),
}


@functools.lru_cache(maxsize=None)
def cluster_scene(name):
    build, R, poly, *params = CLUSTER_SCENES[name]
    pattern = build()
    return (pattern,) + scene(pattern, R, polygon=None if poly is None else poly(), **(params[0] if params else {}))


def check_regime(name, o, polygon):
    """Asserts the scene's regime on the oracle result o; returns the figures (for the test's report)."""
    st = stats_regime(o)
    nf, lmax, ltot, cap = ccl_links(o)
    big = max(st) if st else (0, 0, 0, 0, 0, 0)
    fig = {"clusters": len(st), "nf": nf, "links_max": lmax, "links": ltot, "link_cap": cap, "largest": big}
    if name == "ring":
        # one closed loop: every cell a length candidate (the all-pairs branch), a box beyond the GPU walk's bitmap
        assert len(st) == 1 and big[1] == big[0] > STAT_CAND, fig
        assert big[4] > 8 * REPLAY_LDS_BYTES, fig
    elif name in ("ring-length", "star-length"):
        min_len = CLUSTER_SCENES[name][3]["cluster_min_length"]
        fig["length_from_LB"], fig["length"] = math.sqrt(big[5]) * RES, float(o["cluster_length"].max())
        assert len(st) == 1 and big[1] > STAT_CAND and fig["length_from_LB"] < min_len <= fig["length"], fig
        assert len(o["row_length"]) == 1, fig
    elif name == "spiral":
        # beyond the LDS copy, the all-pairs branch, inexact float sums (replayed), small clusters in the same launch
        assert big[0] > STAT_LDS and big[1] > STAT_CAND and big[2] > EXACT_SUM, fig
        assert sum(1 for s in st if s[0] <= 4) >= 100, fig
    elif name == "star":
        assert len(st) == 1 and big[0] > 10000, fig
    elif name == "dots":
        fig["ids_per_block"] = max_clusters_per_count_block(o)
        assert len(st) > 5000 and all(s[0] == 1 for s in st) and fig["ids_per_block"] >= 200, fig
        assert len(o["row_length"]) == 0, fig
    elif name == "comb-wide":
        # the LDS link list and the global list both overflow: k_ccl_cross' fallback on a real frame
        assert lmax > CCL_EDGE_LDS and ltot > cap, fig
        assert len(o["voronoi_seeds"]) > 10000, fig
    elif name == "comb-mixed":
        # the LDS link list overflows (direct global appends), the global list does not
        assert lmax > CCL_EDGE_LDS and ltot <= cap, fig
    elif name == "sawtooth":
        rc = row_crossings(polygon, o)
        fig["rows_over"] = int(np.count_nonzero(rc > ROW_CROSS_MAX))
        fig["rows_mid"] = int(np.count_nonzero((rc >= 3) & (rc <= ROW_CROSS_MAX)))
        fig["crossings_max"] = int(rc.max())
        assert fig["rows_over"] >= 50 and fig["rows_mid"] >= 20 and fig["crossings_max"] >= 2 * ROW_CROSS_MAX, fig
        assert len(st) > 2000, fig
    else:
        raise KeyError(name)
    return fig
