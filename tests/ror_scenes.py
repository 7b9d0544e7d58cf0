"""Designed clouds for the front of the frame: radius outlier removal, PassThrough, the exclusion discs and the raster
(csrc/ror.hip, ror_stage / ror_stage_append / ror_collect of csrc/ror_stage.hip). Test infrastructure, imported like
shapes.py.

The observability device: a *probe* is a clip candidate that is alone in its grid cell, so its raster bit (and its
unit of n_clipped) is its keep decision. Its decisive neighbours are *neighbour-only* points: inside the binned box
(the clip box grown by ror_margin) but outside the clip box, mostly with z in (clipping_maxz, clipping_maxz + r]. They
count as neighbours and never reach the raster or n_clipped. Coordinates are dyadic (shapes.py's origin 253.5 and
resolution 0.25) or stepped with np.nextafter, so ties are exact.

reference() is plain numpy written from the reference node's rules (PCL 1.12 RadiusOutlierRemoval over FLANN's
L2_Simple, PassThrough, processPointCloud's discs, generateOccupancyGrid); it reads neither ror.hip nor the oracle.
The predictors restate the library's branch conditions, each constant named with its source;
tests/test_ror_scenes_cpu.py checks every scene against both without a GPU.
"""
import functools
import math

import numpy as np

from shapes import MARGIN, ORIGIN, RES, rect_polygon

F = np.float32

# ---------------------------------------------------------------- the library's constants the predictors use
ROR_CAP = 2048            # csrc/ror.hip:362   kRorCap (records of a tile that fits LDS)
BUDGET1 = 12              # csrc/ror.hip:416   kRtBudgetLds (first pass, points per candidate)
BUDGET2 = 96              # csrc/ror.hip:416   kRtBudget2 (second pass)
Q1_CAP = 512              # csrc/ror.hip:416   kRtQCap
Q2_CAP = 128              # csrc/ror.hip:416   kRtQ2Cap
BUDGET_BIG = 64           # csrc/ror.hip:416   kRtBudgetBig
BIG_CHUNK = 4096          # csrc/ror.hip:447   kBigChunk
WIN_WORDS = 256           # csrc/ror.hip:421   kRtWinWords
PART_CHUNK = 4096         # csrc/ror.hip:136   kRtChunkQ
PART_G = 512              # csrc/ror.hip:135   kRtPartBlocks
COL_ROWS = 32             # csrc/ror.hip:269   kColRows
COL_TB = 256              # csrc/ror.hip:269   kColTB
MAX_TILES = 36000         # csrc/ror.h:60      kRtMaxTiles
BIN_CAP = 8192.0          # csrc/ror_stage.hip:56  kMaxBinsPerAxis, the bin grid's cap
PART_LDS_DEFAULT = 64 * 1024   # csrc/ror.hip:972   dynamic LDS beyond it needs hipFuncSetAttribute
TB16_PER32 = 1400.0       # csrc/ror.hip:922   kTilePointsMax: TB = 16 where tiles of 32 would average more records

# Exclusion discs of processPointCloud (reference src/aos_seed_gen_node.cpp:487-499): x, y, radius. Data.
DISCS = np.array([[0.646417, 3.83918, 1.0], [2.0405, 3.62485, 1.0], [65.3711, 2.09755, 1.0], [66.9094, 2.07515, 1.0],
                  [-1.61309, 5.69933, 1.0], [-1.97349, 4.77329, 1.0], [-2.11365, 3.74464, 1.0],
                  [-2.26381, 2.70848, 1.0], [-2.66426, 1.72738, 1.0], [68.0229, 2.31687, 1.0],
                  [65.4647, 2.18653, 1.0]], F)
# The default polygon of the reference's constructor (reference src/aos_seed_gen_node.cpp:196-199). Data.
DEFAULT_POLYGON = np.array([[-1.972916603088379, 7.9420671463012695], [-2.0726776123046875, 0.022441387176513672],
                            [70.22465515136719, 2.102720260620117], [69.48777770996094, 9.786612510681152]], np.float64)
# the fast-reject box of rt_candidate (csrc/ror.hip:84)
DISC_BOX = (F(-3.68), F(69.04), F(0.71), F(6.72))

_ORACLE_NAME = {"clipping_minz": "clip_minz", "clipping_maxz": "clip_maxz"}
ZTOP = F(0.5)             # clipping_maxz: the probes' plane (on the clip face)
MINZ = F(-0.4)


def aos_kwargs(r=0.2, min_n=2, res=RES, **kw):
    d = dict(grid_resolution=float(F(res)), ror_radius=float(r), ror_min_neighbors=int(min_n),
             inflation_radius=float(F(res)) + 0.01, clipping_minz=float(MINZ), clipping_maxz=float(ZTOP))
    d.update(kw)
    return d


def oracle_kwargs(akw):
    return {_ORACLE_NAME.get(k, k): v for k, v in akw.items()}


def as_cloud(xyz):
    """(n, 16) uint8 records: x, y, z, 0 as float32 (the common PointCloud2 layout)."""
    p = np.zeros((len(xyz), 4), F)
    p[:, :3] = xyz
    return p.view(np.uint8).reshape(-1, 16)


def relayout(xyz, step, offs):
    """(n, step) uint8 records with x, y, z at byte offsets offs, the other bytes a non-zero pattern."""
    xyz = np.ascontiguousarray(xyz, F)
    rec = np.full((len(xyz), step), 0xA5, np.uint8)
    for k in range(3):
        rec[:, offs[k]:offs[k] + 4] = xyz[:, k:k + 1].copy().view(np.uint8)
    return rec


# ---------------------------------------------------------------- frame geometry (generateOccupancyGrid)
def frame(polygon, res):
    """(minx, maxx, miny, maxy) float32, W, H: the polygon's box +- 2.5 m (getActiveBounds, seed_gen:874-890) and
    ceil(extent / res) cells in float (seed_gen:581-600)."""
    poly = DEFAULT_POLYGON if polygon is None else np.asarray(polygon, np.float64)
    minx, maxx = F(poly[:, 0].min() - 2.5), F(poly[:, 0].max() + 2.5)
    miny, maxy = F(poly[:, 1].min() - 2.5), F(poly[:, 1].max() + 2.5)
    res = F(res)
    W = max(1, int(math.ceil(F(max(F(0), F(maxx - minx)) / res))))
    H = max(1, int(math.ceil(F(max(F(0), F(maxy - miny)) / res))))
    return (minx, maxx, miny, maxy), W, H


# ---------------------------------------------------------------- the independent reference
def _sq_dist(p, q):
    """FLANN L2_Simple in float32: ((dx*dx) + dy*dy) + dz*dz, every step rounded."""
    d = (p - q).astype(F)
    s = (d[:, 0] * d[:, 0]).astype(F)
    s = (s + (d[:, 1] * d[:, 1]).astype(F)).astype(F)
    return (s + (d[:, 2] * d[:, 2]).astype(F)).astype(F)


def neighbour_counts(p, r, is_dense, block=20000):
    """Per point of p ((n, 3) float32, all finite), the points q of p (itself included) with
    double(d2) <= r * r (dense) or d2 < float32(r * r) (non-dense). Pairs come from a hash into cells of side
    1.0001 r in float64; the test itself is the exact float32 one."""
    n = len(p)
    if n == 0:
        return np.zeros(0, np.int64)
    if not r > 0:
        raise ValueError("the reference needs r > 0")
    h = r * 1.0001
    c = np.floor((p.astype(np.float64) - p.astype(np.float64).min(0)) / h).astype(np.int64) + 1
    NX, NY = int(c[:, 0].max()) + 2, int(c[:, 1].max()) + 2
    key = (c[:, 2] * NY + c[:, 1]) * NX + c[:, 0]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    r2, r2f = float(r) * float(r), F(float(r) * float(r))
    out = np.zeros(n, np.int64)
    for b0 in range(0, n, block):
        i = np.arange(b0, min(n, b0 + block))
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                k = key[i] + (dz * NY + dy) * NX
                lo, hi = np.searchsorted(skey, k - 1, "left"), np.searchsorted(skey, k + 1, "right")
                cnt = hi - lo
                tot = int(cnt.sum())
                if not tot:
                    continue
                ii = np.repeat(i, cnt)
                pos = np.repeat(lo, cnt) + (np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt))
                d2 = _sq_dist(p[ii], p[order[pos]])
                hit = (d2.astype(np.float64) <= r2) if is_dense else (d2 < r2f)
                out += np.bincount(ii[hit], minlength=n)
    return out


def in_disc(x, y):
    """processPointCloud's discs (seed_gen:487-525): float dx*dx + dy*dy <= radius*radius for any of the eleven."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    out = np.zeros(x.shape, bool)
    for ex, ey, er in DISCS:
        dx, dy = (x - ex).astype(F), (y - ey).astype(F)
        d = ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)
        out |= d <= F(er * er)
    return out


def reference(xyz, polygon, akw, is_dense):
    """keep (per point), raster (H x W bool), n_clipped, and what the reports use: counts (neighbours incl. self, -1 for
    non-finite points), cand (clip candidates before ROR), gx / gy (cells of every point, valid where cand)."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    r, need, res = akw["ror_radius"], akw["ror_min_neighbors"] + 1, F(akw["grid_resolution"])
    fin = np.isfinite(xyz).all(1)
    counts = np.full(n, -1, np.int64)
    counts[fin] = neighbour_counts(xyz[fin], r, is_dense)
    keep = counts >= need
    if is_dense and int(fin.sum()) < need:   # PCL's kNN finds fewer than k points: every point is removed
        keep[:] = False
    (minx, maxx, miny, maxy), W, H = frame(polygon, res)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(invalid="ignore"):
        cand = (fin & (z >= F(akw["clipping_minz"])) & (z <= F(akw["clipping_maxz"])) & (x >= minx) & (x <= maxx) &
                (y >= miny) & (y <= maxy))
        cand &= ~in_disc(np.where(fin, x, 0), np.where(fin, y, 0))
    gx, gy = np.zeros(n, np.int64), np.zeros(n, np.int64)
    gx[cand] = np.trunc((x[cand].astype(np.float64) - float(minx)) / float(res)).astype(np.int64)
    gy[cand] = np.trunc((y[cand].astype(np.float64) - float(miny)) / float(res)).astype(np.int64)
    counted = cand & keep
    ing = counted & (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)   # seed_gen:606-619
    raster = np.zeros((H, W), bool)
    raster[gy[ing], gx[ing]] = True
    return dict(keep=keep, raster=raster, n_clipped=int(counted.sum()), counts=counts, cand=cand, gx=gx, gy=gy,
                W=W, H=H)


# ---------------------------------------------------------------- regime predictors
class Geom:
    pass


def ror_margin(r):
    """csrc/ror_stage.hip:16 ror_margin: (float)(r * 1.01) + 1e-4f."""
    return F(F(r * 1.01) + F(1e-4))


def geometry(polygon, akw, n_read, est_binned=None, step=16, offs=(0, 4, 8), host=False):
    """ror_stage's launch geometry (launch_geometry and bin_grid, csrc/ror_stage.hip:33-69) and rt_configure's
    (csrc/ror.hip:923-949) for a frame whose partition passes read n_read records; est_binned None = a fresh handle
    (0.5 n, ror_stage.hip:147)."""
    g = Geom()
    r, res = akw["ror_radius"], F(akw["grid_resolution"])
    (cminx, cmaxx, cminy, cmaxy), g.W, g.H = frame(polygon, res)
    m = ror_margin(r)
    g.clip = (cminx, cmaxx, cminy, cmaxy, F(akw["clipping_minz"]), F(akw["clipping_maxz"]))
    g.box = (F(cminx - m), F(cmaxx + m), F(cminy - m), F(cmaxy + m), F(g.clip[4] - m), F(g.clip[5] + m))
    bminx, bmaxx, bminy, bmaxy = g.box[:4]
    cs = F(r * 1.001)
    ext = max(float(bmaxx) - float(bminx), float(bmaxy) - float(bminy))
    g.capped = ext / float(cs) > BIN_CAP
    if g.capped:
        cs = F(ext / BIN_CAP)
    g.coarsened = 0
    while True:
        g.inv_cs = F(F(1.0) / cs)
        g.nbx = max(1, int(F(F(bmaxx - bminx) * g.inv_cs)) + 1)
        g.nby = max(1, int(F(F(bmaxy - bminy) * g.inv_cs)) + 1)
        if ((g.nbx + 31) // 32) * ((g.nby + 31) // 32) <= MAX_TILES:
            break
        cs = F(cs * F(1.25))
        g.coarsened += 1
    g.cs = cs

    def tiles(tb):
        return ((g.nbx + tb - 1) // tb) * ((g.nby + tb - 1) // tb)
    est = 0.5 * n_read if est_binned is None else est_binned
    per32 = est * 1.15 / tiles(32)
    g.TB = 16 if (per32 > TB16_PER32 and tiles(16) <= MAX_TILES) else 32
    g.ntx, g.nty = (g.nbx + g.TB - 1) // g.TB, (g.nby + g.TB - 1) // g.TB
    g.ntiles = g.ntx * g.nty
    span = float(g.TB) / float(g.inv_cs) / float(res)
    cells = int(math.ceil(span)) + 6
    g.win_w = (cells + 63) // 64 + 1
    g.win_rows = cells if cells * g.win_w <= WIN_WORDS else 0
    gg = PART_G                                           # rt_part_blocks, csrc/ror.hip:951
    while gg > 64 and g.ntiles * gg > (16 << 20):
        gg //= 2
    g.G = max(1, min(gg, (n_read + PART_CHUNK - 1) // PART_CHUNK))
    g.chunk = ((n_read + g.G - 1) // g.G + PART_CHUNK - 1) // PART_CHUNK * PART_CHUNK   # rt_chunk
    g.row_groups = (g.G + COL_ROWS - 1) // COL_ROWS
    g.tile_blocks = (g.ntiles + COL_TB - 1) // COL_TB
    g.part_lds = 4 * g.ntiles
    # rt_layout (csrc/ror.hip:978); a host cloud is packed to float3 by the upload (LAY 2)
    g.lay = 2 if host else ((1 if step == 16 else 2 if step == 12 else 0) if tuple(offs) == (0, 4, 8) else 0)
    return g


def binned(xyz, g):
    """rt_binned (csrc/ror.hip:66): finite and inside the binned box, by the same float compares."""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(invalid="ignore"):
        return (np.isfinite(xyz).all(1) & (x >= g.box[0]) & (x <= g.box[1]) & (y >= g.box[2]) & (y <= g.box[3]) &
                (z >= g.box[4]) & (z <= g.box[5]))


def bins_of(xyz, g):
    """rt_bin (csrc/ror.hip:71) of binned points."""
    bx = np.clip(((xyz[:, 0] - g.box[0]).astype(F) * g.inv_cs).astype(F).astype(np.int64), 0, g.nbx - 1)
    by = np.clip(((xyz[:, 1] - g.box[2]).astype(F) * g.inv_cs).astype(F).astype(np.int64), 0, g.nby - 1)
    return bx, by


def staging(xyz, g):
    """What k_rt_part stages: per tile the records (own + halo copies, rt_tiles csrc/ror.hip:139), per point its own
    tile and the number of its copies, per bin the point count. Only the binned points of xyz are returned."""
    m = binned(xyz, g)
    p = xyz[m]
    bx, by = bins_of(p, g)
    tb = g.TB
    tx0, tx1 = np.maximum(bx - 1, 0) // tb, np.minimum(bx + 1, g.nbx - 1) // tb
    ty0, ty1 = np.maximum(by - 1, 0) // tb, np.minimum(by + 1, g.nby - 1) // tb
    staged = np.zeros(g.ntiles, np.int64)
    np.add.at(staged, ty0 * g.ntx + tx0, 1)
    hx, hy = tx1 > tx0, ty1 > ty0
    np.add.at(staged, (ty0 * g.ntx + tx1)[hx], 1)
    np.add.at(staged, (ty1 * g.ntx + tx0)[hy], 1)
    np.add.at(staged, (ty1 * g.ntx + tx1)[hx & hy], 1)
    bins = np.zeros((g.nby + 2, g.nbx + 2), np.int64)     # a zero ring, so 3 x 3 sums need no clamping
    np.add.at(bins, (by + 1, bx + 1), 1)
    reach = sum(bins[1 + dy:g.nby + 1 + dy, 1 + dx:g.nbx + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return dict(mask=m, bx=bx, by=by, tile=(by // tb) * g.ntx + bx // tb, copies=1 + hx + hy + (hx & hy),
                staged=staged, reach=reach[by, bx])


def cell_mismatch(v, origin, res):
    """Where rt_cell's fast path alone (csrc/ror.hip:101, trunc(a * (1 / res))) would give another cell than the
    division (int)(a / res) of generateOccupancyGrid: the points that need its exact branch."""
    a = np.asarray(v, F).astype(np.float64) - float(origin)
    r = float(F(res))
    return np.trunc(a * (1.0 / r)) != np.trunc(a / r)


def regimes(xyz, polygon, akw, is_dense, n_read=None, est_binned=None, ref=None, **layout):
    """The branches of ror.hip a frame takes, as a set of names, with the figures behind them. Budget and queue regimes
    are named only where no record order can change them: a candidate with need > 12 whose 3 x 3 bins hold more than
    12 records cannot be decided by the first pass (it examines at most 12 records), likewise 96 for the second."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    ref = ref or reference(xyz, polygon, akw, is_dense)
    g = geometry(polygon, akw, len(xyz) if n_read is None else n_read, est_binned, **layout)
    s = staging(xyz, g)
    need = akw["ror_min_neighbors"] + 1
    cand = ref["cand"][s["mask"]]
    below = ref["counts"][s["mask"]] < need
    big = s["staged"] > ROR_CAP
    fit_c = cand & ~big[s["tile"]]
    big_c = cand & big[s["tile"]]
    out = {f"TB{g.TB}", f"LAY{g.lay}", "win-on" if g.win_rows else "win-off"}
    fig = dict(TB=g.TB, ntiles=g.ntiles, nbx=g.nbx, nby=g.nby, cs=float(g.cs), G=g.G, row_groups=g.row_groups,
               tile_blocks=g.tile_blocks, part_lds=g.part_lds, win_rows=g.win_rows, staged_max=int(s["staged"].max(initial=0)),
               big_tiles=int(big.sum()), binned=int(s["mask"].sum()))
    per_tile = lambda m: np.bincount(s["tile"][m], minlength=g.ntiles)   # noqa: E731
    q1 = fit_c & (need > BUDGET1) & (s["reach"] > BUDGET1)
    q2 = fit_c & (need > BUDGET2) & (s["reach"] > BUDGET2)
    first = fit_c & (s["reach"] <= BUDGET1)
    fig.update(q1_max=int(per_tile(q1).max(initial=0)), q2_max=int(per_tile(q2).max(initial=0)))
    if first.any():
        out.add("first-pass")
    if q1.any():
        out.add("queue1")
    if fig["q1_max"] > Q1_CAP:
        out.add("queue1-full")
    if q2.any():
        out.update({"queue2", "wave-scan"})
    if fig["q2_max"] > Q2_CAP:
        out.add("queue2-full")
    if big.any():
        out.add("big-tile")
        chunks = -(-s["staged"][big] // BIG_CHUNK)
        fig["big_chunks"] = sorted(int(c) for c in chunks)
        if (chunks >= 2).any():
            out.add("big-chunks")
        # a below-need candidate with more than 64 records in reach stays undecided in the big path's first pass;
        # more than 512 of them per chunk on average fill some chunk's queue
        und = per_tile(big_c & below & (s["reach"] > BUDGET_BIG))[big]
        fig["big_undecided"] = [int(u) for u in und]
        if (und > 0).any():
            out.add("big-queue")
        if (und > Q1_CAP * chunks).any():
            out.add("big-queue-full")
    c = ref["cand"]
    if c.any():
        fig["cell_mismatch"] = int(cell_mismatch(xyz[c, 0], g.clip[0], akw["grid_resolution"]).sum() +
                                   cell_mismatch(xyz[c, 1], g.clip[2], akw["grid_resolution"]).sum())
        if fig["cell_mismatch"]:
            out.add("cell-exact")
    if g.capped:
        out.add("bin-cap")
    if g.coarsened:
        out.add("bin-coarsen")
    if g.part_lds > PART_LDS_DEFAULT:
        out.add("part-lds-64k")
    if g.row_groups >= 2:
        out.add("colscan-groups")
    if g.tile_blocks >= 2:
        out.add("colscan-blocks")
    return out, fig, g, s


# every branch the scenes must reach between them (tests/test_ror_scenes_cpu.py asserts the union)
ALL_REGIMES = {"TB16", "TB32", "first-pass", "queue1", "queue1-full", "queue2", "queue2-full", "wave-scan", "big-tile",
               "big-chunks", "big-queue", "big-queue-full", "win-on", "win-off", "bin-cap", "bin-coarsen",
               "part-lds-64k", "colscan-groups", "colscan-blocks", "LAY0", "LAY1", "LAY2", "cell-exact"}


# ---------------------------------------------------------------- building blocks
class Builder:
    """Collects points; probes are remembered by index."""

    def __init__(self, W, H, res=RES):
        self.W, self.H, self.res = W, H, F(res)
        self.pts, self.probes = [], []
        self.polygon = rect_polygon(W, H) if res == RES else None

    def centre(self, cx, cy):
        """The float32 centre of cell (cx, cy)."""
        return F(ORIGIN + (cx + 0.5) * float(self.res)), F(ORIGIN + (cy + 0.5) * float(self.res))

    def add(self, x, y, z, probe=False):
        if probe:
            self.probes.append(len(self.pts))
        self.pts.append((F(x), F(y), F(z)))
        return len(self.pts) - 1

    def stack(self, x, y, k, z0=None, step=2.0 ** -10):
        """k neighbour-only points above (x, y): z = clipping_maxz + step, + 2 step, ... (mutually near)."""
        for j in range(k):
            self.add(x, y, (float(ZTOP) if z0 is None else z0) + (j + 1) * step)

    def xyz(self):
        return np.array(self.pts, F).reshape(-1, 3)


def thresholds(r):
    """(r2df, r2f): the largest float whose double is <= r * r (dense), float(r * r) (non-dense, strict)."""
    r2 = float(r) * float(r)
    r2f = F(r2)
    r2df = r2f if float(r2f) <= r2 else np.nextafter(r2f, F(0))
    return r2df, r2f


def tie_heights(r, a=0.0, b=0.0, span=3):
    """Heights c (float32, exact as (clipping_maxz + c) - clipping_maxz) of a neighbour at horizontal offset (a, b)
    whose stepwise float d2 = (a*a + b*b) + c*c runs over the floats nearest the thresholds of r: 2 span + 1
    consecutive representable z around it. Returns [(z, d2)]."""
    r2df, _ = thresholds(r)
    base = math.sqrt(max(float(r2df) - a * a - b * b, 0.0))
    z = F(float(ZTOP) + base)
    for _ in range(span):
        z = np.nextafter(z, F(0))
    out = []
    for _ in range(2 * span + 1):
        q = np.array([[a, b, z]], F)
        out.append((z, float(_sq_dist(np.array([[0, 0, ZTOP]], F), q)[0])))
        z = np.nextafter(z, F(2))
    return out


def add_ties(B, cells, r, need, dirs=("z", "diag", "x", "y")):
    """Tie probes on the cells given (an iterator of (cx, cy), cells at least two apart): each probe has need - 2 sure
    neighbours, so with itself it stands at need - 1, and one neighbour at the threshold: d2 equal to it, a float or
    two below, a float or two above. z: straight above; diag: a 3-D diagonal; x / y: along the axis (stepped in the
    axis' own floats, with a height of 2^-6 that keeps the neighbour out of the clip box). Then two controls with
    need - 1 and need - 2 sure neighbours and no tie. Returns the d2 values used."""
    it = iter(cells)
    d2s = []
    h = 2.0 ** -6
    off = 0.125 if r >= 0.2 else (2.0 ** -5 if r >= 0.05 else 2.0 ** -7)
    for d in dirs:
        if d in ("z", "diag"):
            a = b = 0.0 if d == "z" else off
            for z, d2 in tie_heights(r, a, b):
                cx, cy = next(it)
                x, y = B.centre(cx, cy)
                B.add(x, y, ZTOP, probe=True)
                B.stack(x, y, need - 2, step=2.0 ** -12)
                B.add(F(x + F(a)), F(y + F(b)), z)
                d2s.append(d2)
        else:
            cx0, cy0 = next(it)
            x0, y0 = B.centre(cx0, cy0)
            base = F((x0 if d == "x" else y0) + F(math.sqrt(float(thresholds(r)[0]) - h * h)))
            for k in range(-3, 4):
                cx, cy = (cx0, cy0) if k == -3 else next(it)
                x, y = B.centre(cx, cy)
                t = base
                for _ in range(abs(k)):
                    t = np.nextafter(t, F(0) if k < 0 else F(1e9))
                dt = F(t - (x0 if d == "x" else y0))       # exact: the same binade
                B.add(x, y, ZTOP, probe=True)
                B.stack(x, y, need - 2, step=2.0 ** -12)
                q = (F(x + dt), y) if d == "x" else (x, F(y + dt))
                B.add(q[0], q[1], float(ZTOP) + h)
                d2s.append(float(_sq_dist(np.array([[x, y, ZTOP]], F), np.array([[q[0], q[1], F(float(ZTOP) + h)]], F))[0]))
    for sure in (need - 1, need - 2, need - 1, need - 2):
        cx, cy = next(it)
        x, y = B.centre(cx, cy)
        B.add(x, y, ZTOP, probe=True)
        B.stack(x, y, max(sure, 0), step=2.0 ** -12)
    return d2s


def spaced_cells(x0, y0, x1, y1, step=2):
    for cy in range(y0, y1, step):
        for cx in range(x0, x1, step):
            yield cx, cy


def ceiling(B, x0, x1, y0, y1, nx, ny, z):
    """A lattice of nx x ny neighbour-only points at height z over [x0, x1] x [y0, y1]."""
    xs, ys = np.linspace(x0, x1, nx).astype(F), np.linspace(y0, y1, ny).astype(F)
    for y in ys:
        for x in xs:
            B.add(x, y, z)


class Scene:
    """xyz (n, 3) float32, polygon (None: the default one), akw (aos parameter keywords), modes (is_dense values),
    probes (indices), expect (regimes the scene is named for), parts (index arrays of a streamed delivery)."""

    def __init__(self, name, xyz, polygon, akw, probes, expect=(), modes=(True, False), **extra):
        self.name, self.xyz, self.polygon, self.akw = name, np.ascontiguousarray(xyz, F), polygon, akw
        self.probes, self.expect, self.modes = np.asarray(probes, np.int64), set(expect), tuple(modes)
        self.est_binned = extra.pop("est_binned", None)
        self.extra = extra

    @property
    def cloud(self):
        return as_cloud(self.xyz)


# ---------------------------------------------------------------- the scenes
def radius_ties(r, min_n):
    W, H = 64, 44
    B = Builder(W, H)
    need = min_n + 1
    d2s = add_ties(B, spaced_cells(11, 11, W - 11, H - 11), r, need)
    if r == 0.25:   # candidates of adjacent cells, exactly r apart along x and along y (res == r)
        for cx, cy, dx, dy in ((12, 2, 1, 0), (16, 2, 0, 1), (20, 2, 1, 0), (24, 2, 0, 1)):
            for k in range(2):
                x, y = B.centre(cx + k * dx, cy + 2 * (cx % 8 == 4) + k * dy)
                B.add(x, y, ZTOP, probe=True)
                B.stack(x, y, need - 2, step=2.0 ** -12)
    return Scene(f"radius_ties-r{r}-n{min_n}", B.xyz(), B.polygon, aos_kwargs(r, min_n), B.probes,
                 {"first-pass", "TB32", "win-on"}, d2s=d2s)


def contraction_search(r, is_dense, want=32, seed=7):
    """Pairs (dx, dy, z) whose stepwise float d2 and whose FMA-contracted d2 (every way a compiler could fuse the two
    additions, evaluated in float64 and rounded once per fused step) fall on opposite sides of the keep threshold.
    dx, dy are multiples of 2^-15 (differences of floats near 260), z a float in (0.5, 0.75). Returns, per way of
    fusing (both additions with either product of the first fused, the first only likewise, the second only), two lists: stepwise in / contracted out, and stepwise
    out / contracted in."""
    r2df, r2f = thresholds(r)
    cmp_ = float(r2df) if is_dense else float(np.nextafter(r2f, F(0)))   # in iff d2 <= cmp_
    rng = np.random.default_rng(seed)
    n = 200000
    lim = int(0.6 * r * 2 ** 15)
    dx = (rng.integers(-lim, lim, n) * 2.0 ** -15).astype(F)
    dy = (rng.integers(-lim, lim, n) * 2.0 ** -15).astype(F)
    base = np.sqrt(np.maximum(cmp_ - dx.astype(np.float64) ** 2 - dy.astype(np.float64) ** 2, 0.0))
    z = (float(ZTOP) + base).astype(F)
    for _ in range(2):   # the nearest float and up to two floats either side
        z = np.where(rng.integers(0, 3, n) == 0, np.nextafter(z, F(0)), np.where(rng.integers(0, 2, n) == 0, z,
                                                                                  np.nextafter(z, F(2))))
    dz = (z - ZTOP).astype(F)
    ok = dz > F(0.03)
    dx, dy, dz, z = dx[ok], dy[ok], dz[ok], z[ok]
    xx = (dx * dx).astype(F)
    step = ((xx + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)).astype(F)
    d64 = lambda v: v.astype(np.float64)   # noqa: E731
    f1 = (d64(xx) + d64(dy) * d64(dy)).astype(F)                  # fma(dy, dy, dx*dx)
    both = (d64(f1) + d64(dz) * d64(dz)).astype(F)                # fma(dz, dz, fma(dy, dy, dx*dx))
    first = (f1 + (dz * dz).astype(F)).astype(F)                  # fma(dy, dy, dx*dx) + dz*dz
    second = (d64((xx + (dy * dy).astype(F)).astype(F)) + d64(dz) * d64(dz)).astype(F)   # fma(dz, dz, dx*dx + dy*dy)
    g1 = (d64(dx) * d64(dx) + d64((dy * dy).astype(F))).astype(F)   # fma(dx, dx, dy*dy): the other operand fused
    both_x = (d64(g1) + d64(dz) * d64(dz)).astype(F)              # fma(dz, dz, fma(dx, dx, dy*dy))
    first_x = (g1 + (dz * dz).astype(F)).astype(F)                # fma(dx, dx, dy*dy) + dz*dz
    s_in = step <= F(cmp_)
    out = {}
    for name, v in (("both", both), ("both-x", both_x), ("first", first), ("first-x", first_x), ("second", second)):
        c_in = v <= F(cmp_)
        out[name] = tuple([(dx[i], dy[i], z[i]) for i in np.flatnonzero(m)[:want]] for m in (s_in & ~c_in, ~s_in & c_in))
    return out


def contraction_pairs(is_dense, r=0.3):
    found = contraction_search(r, is_dense)
    W, H = 64, 44
    B = Builder(W, H)
    cells = spaced_cells(1, 1, W - 1, H - 1)
    for a, b in found.values():
        for dx, dy, z in a + b:
            x, y = B.centre(*next(cells))
            B.add(x, y, ZTOP, probe=True)
            B.add(F(x + dx), F(y + dy), z)
    return Scene(f"contraction_pairs-{'dense' if is_dense else 'sparse'}", B.xyz(), B.polygon, aos_kwargs(r, 1),
                 B.probes, {"first-pass"}, modes=(is_dense,), found={k: (len(a), len(b)) for k, (a, b) in found.items()})


def _junk(B, x, y, r, k):
    """k points in the probe's 3 x 3 bins but beyond r: 1.0005 r to the side (less than a bin of 1.001 r away)."""
    for j in range(k):
        B.add(F(x + F(r * 1.0005) * (1 if j % 2 else -1)), y, float(ZTOP) + (j // 2 + 1) * 2.0 ** -9)


def need_sweep(min_n):
    """Clumps of need - 1, need and need + 1 mutually-near points (the probe and a stack above it), each with junk in
    the bins beyond r. min_n 13 adds a block of more than 512 probes in one fitting tile (the first queue fills),
    min_n 100 a block of more than 128 (the second queue fills, the rest go to the wave scan) and a lone wave-scan
    probe whose deciding neighbour is alone in the last bin of its last bin row."""
    need = min_n + 1
    if min_n == 13:
        return _queue1_block()
    if min_n == 100:
        return _queue2_block()
    r = 0.2
    W, H = 64, 44
    B = Builder(W, H)
    cells = spaced_cells(11, 11, W - 11, H - 11)
    for rep in range(4):
        for sure in (need - 2, need - 1, need):
            if sure < 0:
                continue
            x, y = B.centre(*next(cells))
            B.add(x, y, ZTOP, probe=True)
            B.stack(x, y, sure, step=2.0 ** -11)
            _junk(B, x, y, r, (0, 6, 14, 110)[rep])
    exp = {"queue1"} if need > BUDGET1 else {"first-pass"}
    return Scene(f"need_sweep-n{min_n}", B.xyz(), B.polygon, aos_kwargs(r, min_n), B.probes, exp)


def _queue1_block():
    """need 14, r 0.3: a block of 24 x 24 probes, one per cell, each seeing its four edge neighbours (0.25 m) and one
    pool of 8 or 9 points over the block's even cell corners: 5 + 8 = 13 drops, 5 + 9 = 14 keeps. More than 512
    candidates of one fitting tile go to the first queue."""
    r, min_n, n = 0.3, 13, 24
    W = H = 48
    B = Builder(W, H)
    for j in range(n):
        for i in range(n):
            x, y = B.centre(2 + i, 2 + j)
            B.add(x, y, ZTOP, probe=True)
    for j in range(0, n + 1, 2):
        for i in range(0, n + 1, 2):
            B.stack(F(ORIGIN + (2 + i) * RES), F(ORIGIN + (2 + j) * RES), 8 + ((i // 2 + j // 2) % 2), step=2.0 ** -10)
    return Scene("need_sweep-n13", B.xyz(), B.polygon, aos_kwargs(r, min_n), B.probes, {"queue1", "queue1-full"})


def _queue2_block():
    """need 101, r 1.5 (six cells): a block of 16 x 16 probes that see each other, a disc of up to 113 cells, plus a
    sparse ceiling, so the inner probes keep and the outer ones drop; all have more than 96 records in reach, so all
    reach the second queue (128 slots) and the wave scan. Far away, two lone probes under stacks of 99: one has its
    101st point alone in the diagonal bin, the last of its last bin row, the other lacks it."""
    r, min_n = 1.5, 100
    W, H = 60, 200
    B = Builder(W, H)
    for j in range(16):
        for i in range(16):
            x, y = B.centre(12 + i, 12 + j)
            B.add(x, y, ZTOP, probe=True)
    for j in range(0, 16, 3):
        for i in range(0, 16, 3):
            x, y = B.centre(12 + i, 12 + j)
            B.add(x, y, float(ZTOP) + 0.25)
    g = geometry(B.polygon, aos_kwargs(r, min_n), 1000)
    for k, decisive in enumerate((True, False)):
        # a cell centre in the upper right ninth of its bin, the neighbour one bin up and right
        for cy in range(150 + 20 * k, 190):
            cx = next((c for c in range(20, 40) if _bin_frac(B.centre(c, cy), g)[0] > 0.7), None)
            if cx is not None and _bin_frac(B.centre(cx, cy), g)[1] > 0.7:
                break
        x, y = B.centre(cx, cy)
        B.add(x, y, ZTOP, probe=True)
        B.stack(x, y, 99, step=2.0 ** -10)
        if decisive:
            B.add(F(x + F(0.5)), F(y + F(0.5)), float(ZTOP) + 2.0 ** -6)
    return Scene("need_sweep-n100", B.xyz(), B.polygon, aos_kwargs(r, min_n), B.probes,
                 {"queue2", "queue2-full", "wave-scan"})


def _bin_frac(xy, g):
    fx = float(F(F(xy[0] - g.box[0]) * g.inv_cs))
    fy = float(F(F(xy[1] - g.box[2]) * g.inv_cs))
    return fx - math.floor(fx), fy - math.floor(fy)


def tile_edges(tb16):
    """A 4 x 4 tile grid (r 0.2, 90 x 90 cells), need 4. At every inner tile corner a probe and three neighbours, one
    per tile; along the tile edges probes whose deciding neighbour is across the edge in x only / y only; probes on
    the clip faces (the first and last bins that hold candidates) with neighbours in the margin band, on bmin / bmax
    and one float outside. tb16: a ceiling of 40 k far neighbour-only points, so a fresh handle picks TB = 16."""
    r, min_n = 0.2, 3
    W = H = 90
    B = Builder(W, H)
    akw = aos_kwargs(r, min_n)
    n_ceil = 210 * 210 if tb16 else 0
    g = geometry(B.polygon, akw, 3000 + n_ceil)
    assert g.TB == (16 if tb16 else 32), g.TB
    h = float(ZTOP) + 2.0 ** -6
    d = 0.05
    edge = lambda k, b0: float(b0) + k * g.TB * float(g.cs)   # noqa: E731  (tile boundary k, approximately)
    k = 0
    for ty in range(1, g.nty):
        for tx in range(1, g.ntx):
            ex, ey = edge(tx, g.box[0]), edge(ty, g.box[2])
            quad = [(-d, -d), (d, -d), (-d, d), (d, d)]
            keep = k % 3 != 2                 # every third corner lacks the diagonal neighbour: it drops
            own = quad[k % 4]
            diag = (-own[0], -own[1])
            B.add(ex + own[0], ey + own[1], ZTOP, probe=True)
            for q in quad:
                if q != own and (keep or q != diag):
                    B.add(ex + q[0], ey + q[1], h)
            # halfway along the edges that leave the corner: x only, y only
            my = ey + g.TB * float(g.cs) * (0.5 if ty < g.nty - 1 else -0.25)
            B.add(ex - d, my, ZTOP, probe=True)
            B.stack(ex - d, my, 1 + k % 2, step=2.0 ** -8)          # 2 or 3 with itself ...
            B.add(ex + d, my, h)                                    # ... + 1 across the edge in x
            mx = ex + g.TB * float(g.cs) * (0.5 if tx < g.ntx - 1 else -0.25)
            B.add(mx, ey + d, ZTOP, probe=True)
            B.stack(mx, ey + d, 2 - k % 2, step=2.0 ** -8)
            B.add(mx, ey - d, h)
            k += 1
    # clip faces: probes at x = cminx / cmaxx (and y), neighbours in the band; one on the box face, one a float outside
    cminx, cmaxx, cminy, cmaxy = g.clip[:4]
    for j, (px, py, ox, oy) in enumerate(((cminx, None, -1, 0), (cmaxx, None, 1, 0), (None, cminy, 0, -1),
                                          (None, cmaxy, 0, 1))):
        for v in range(4):
            t = F(ORIGIN + (20.5 + 6 * v + 2 * j) * RES)
            x, y = (px, t) if px is not None else (t, py)
            B.add(x, y, ZTOP, probe=True)
            for s in range(v):   # v near neighbours in the band (0.125 out): with itself v + 1, need 4
                B.add(F(x + F(ox * 0.125)), F(y + F(oy * 0.125)), float(ZTOP) - s * 2.0 ** -8)
            face = g.box[0] if ox < 0 else g.box[1] if ox > 0 else g.box[2] if oy < 0 else g.box[3]
            out = np.nextafter(face, F(-1e9) if ox + oy < 0 else F(1e9))
            for f in (face, out):
                B.add(f if ox else x, f if oy else y, ZTOP)
    if tb16:
        ceiling(B, float(g.box[0]) + 0.01, float(g.box[1]) - 0.01, float(g.box[2]) + 0.01, float(g.box[3]) - 0.01,
                210, 210, float(ZTOP) + 0.2016)   # 0.2016 > r above the probes' plane, inside bmaxz
    return Scene("tile_edges-tb16" if tb16 else "tile_edges", B.xyz(), B.polygon, akw, B.probes,
                 {"TB16" if tb16 else "TB32"})


BIG_TARGETS = (2048, 2049, 4096, 4097, 9000, 8192)


def big_tiles():
    """r 0.2 at resolution 0.05 (128 cells per tile side), need 7, a 6 x 3 tile grid (so the records average below
    1400 per tile and TB stays 32); six tiles are topped up with a never-neighbouring ceiling to exactly 2048 (fits),
    2049 (big), 4096 and 4097 (one and two chunks), 9000 and 8192 staged records. The first five carry tie probes and
    probes under stacks of six (they keep); the last a lattice of 39 x 39 probes 0.15 m apart (five points within r:
    they drop) under the ceiling: more than 64 records in reach each, more than 512 per chunk."""
    r, min_n, res = 0.2, 6, 0.05
    need = min_n + 1
    poly = np.array([[256.0, 256.0], [289.0, 256.0], [289.0, 269.5], [256.0, 269.5]], np.float64)
    akw = aos_kwargs(r, min_n, res)
    B = Builder(0, 0, res)
    B.polygon = poly
    g = geometry(poly, akw, 30000)
    assert (g.ntx, g.nty, g.TB) == (6, 3, 32), (g.ntx, g.nty, g.TB)
    side = g.TB * float(g.cs)
    cell0 = lambda v: int((v - ORIGIN) / res) + 2   # noqa: E731
    tiles = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (3, 1)]
    for (tx, ty), target in zip(tiles, BIG_TARGETS):
        x0, y0 = float(g.box[0]) + tx * side, float(g.box[2]) + ty * side
        cx0, cy0 = cell0(x0 + 0.3), cell0(y0 + 0.3)
        if target == 8192:
            for j in range(39):
                for i in range(39):
                    x, y = B.centre(cx0 + 3 * i, cy0 + 3 * j)
                    B.add(x, y, ZTOP, probe=True)
            continue
        add_ties(B, spaced_cells(cx0, cy0, cx0 + 90, cy0 + 30, 6), r, need, dirs=("z", "diag"))
        for k, (cx, cy) in enumerate(spaced_cells(cx0, cy0 + 36, cx0 + 112, cy0 + 112, 6)):
            if k < (target - 1400) // 12:
                x, y = B.centre(cx, cy)
                B.add(x, y, ZTOP, probe=True)
                B.stack(x, y, need - 1, step=2.0 ** -10)
    # the ceilings: interior lattices (no halo copies), sized by the predictor to the exact targets
    s = staging(B.xyz(), g)
    for (tx, ty), target in zip(tiles, BIG_TARGETS):
        have = int(s["staged"][ty * g.ntx + tx])
        x0, y0 = float(g.box[0]) + tx * side + 0.3, float(g.box[2]) + ty * side + 0.3
        k = target - have
        assert k > 0, (target, have)
        nx = int(math.ceil(math.sqrt(k)))
        xs = np.linspace(x0, x0 + side - 0.6, nx).astype(F)
        for q in range(k):
            B.add(xs[q % nx], F(y0 + (q // nx) * (side - 0.6) / nx), float(ZTOP) + 0.2016)
    return Scene("big_tiles", B.xyz(), poly, akw, B.probes,
                 {"big-tile", "big-chunks", "big-queue", "big-queue-full", "win-off"})


CHUNK_SIZES = (1, 2, 4095, 4096, 4097, 8193, 3 * 4096 + 5)


def chunk_edges(n, finite_only, extra=None, r=0.25, min_n=1):
    """n records, need 2. Across every boundary b = 4096 k of the partition passes' chunks: odd k, records b - 1 and b are
    lone probes (a doubled record would keep one); even k, record b - 1 is the only neighbour of probe b (a dropped
    record drops it). Record 0 is a probe whose only neighbour is record n - 1. A few pairs and lone probes sit inside
    the chunks; every other record lies outside the binned box: far off, high above, or (not finite_only) NaN / inf in
    one coordinate. extra: points placed from record 8 on (they must not touch the cells used here)."""
    W, H = 64, 44
    B = Builder(W, H)
    xyz = np.zeros((n, 3), F)
    k = np.arange(n)
    xyz[:, 0] = 300.0 + (k % 97)                      # far in x
    xyz[k % 3 == 1, 0] = 258.0
    xyz[k % 3 == 1, 2] = 3.0 + (k[k % 3 == 1] % 5)    # above the box
    xyz[:, 1] = 258.0
    if not finite_only:
        for c, v in enumerate((np.nan, np.inf, -np.inf)):
            m = k % 11 == 2 + c
            xyz[m, (k[m] // 11) % 3] = v
    probes = []
    cells = spaced_cells(11, 1, W - 1, 9)

    def probe(i):
        x, y = B.centre(*next(cells))
        xyz[i] = (x, y, ZTOP)
        probes.append(i)
        return x, y

    def pair(i, j):    # probe i, its neighbour j
        x, y = probe(i)
        xyz[j] = (x, y, float(ZTOP) + 0.125)

    if n >= 2:
        pair(0, n - 1)
    else:
        probe(0)
    for kb in range(1, (n - 1) // PART_CHUNK + 1):
        b = kb * PART_CHUNK
        if b >= n - 1:
            if b == n - 1:       # the boundary's second record is the last one (record 0's neighbour): probe b - 1 alone
                probe(b - 1)
            continue
        if kb % 2:
            probe(b - 1)
            probe(b)
        else:
            pair(b, b - 1)
    if n > 64:
        for i in range(4):
            pair(20 + 4 * i, 22 + 4 * i)
            probe(40 + 2 * i)
    if extra is not None and len(extra):
        assert n > 64 + len(extra)
        xyz[64:64 + len(extra)] = extra
    return B, xyz, probes


def chunk_edges_scene(n, finite_only=False):
    B, xyz, probes = chunk_edges(n, finite_only)
    return Scene(f"chunk_edges-{n}" + ("-finite" if finite_only else ""), xyz, B.polygon, aos_kwargs(0.25, 1), probes,
                 {"first-pass"}, modes=(True,) if finite_only else (False,))


def wide_scan():
    """r 0.05 on a 30 m square: 361 tiles (two tile-start blocks) and 136 900 ceiling points, none within r of
    another or of a probe, so the column scan has two row groups. The tie probes sit in the first records (first
    tile rows) and in the last (last tile rows)."""
    r, min_n = 0.05, 1
    W = H = 120 + 2 * MARGIN
    akw = aos_kwargs(r, min_n)
    A, Z = Builder(W, H), Builder(W, H)
    add_ties(A, spaced_cells(1, 1, W - 1, 5), r, 2)
    add_ties(Z, spaced_cells(1, H - 5, W - 1, H - 1), r, 2)
    g = geometry(A.polygon, akw, 140000)
    C = Builder(W, H)
    ceiling(C, float(g.box[0]) + 0.01, float(g.box[1]) - 0.01, float(g.box[2]) + 0.01, float(g.box[3]) - 0.01, 370, 370,
            float(ZTOP) + 0.0504)
    xyz = np.concatenate([A.xyz(), C.xyz(), Z.xyz()])
    probes = A.probes + [len(A.pts) + len(C.pts) + i for i in Z.probes]
    return Scene("wide_scan", xyz, A.polygon, akw, probes, {"colscan-groups", "colscan-blocks"})


def fine_radius():
    """r 0.02 on 165 x 95 m: ext / cs > 8192 (cs from the cap), 38 656 tiles of 32 bins (the coarsening loop runs
    once), then 24 805 tiles: 97 KB of LDS for the partition passes' histogram."""
    r, min_n = 0.02, 1
    W, H = 660 + 2 * MARGIN, 380 + 2 * MARGIN
    B = Builder(W, H)
    cells = [(cx, cy) for cy in (1, H // 2, H - 2) for cx in range(1, W - 1, 17)]
    add_ties(B, iter(cells), r, 2)
    return Scene("fine_radius", B.xyz(), B.polygon, aos_kwargs(r, min_n), B.probes,
                 {"bin-cap", "bin-coarsen", "part-lds-64k"})


CELL_RES = (0.25, float(F(0.1)), float(F(0.15)), 0.05)


def clip_faces_and_cells(res):
    """Every point but the third named below has a companion outside the clip box 2^-6 away (need 2), so ROR keeps it
    and the clip faces and the cell rule decide. Faces: a point on each of the six clip faces, one float inside, one
    float outside (a point on the x / y max face has cell W / H: counted, not rastered). Cells: the float nearest
    origin + k res and its two float neighbours, in x and in y, for k over the grid (rt_cell's near-integer test; the points
    where only its exact branch finds the cell are cell_exact's); every second k has no companions, so ROR drops its three points unless others' are near."""
    poly = np.array([[256.0, 256.0], [272.0, 256.0], [272.0, 268.0], [256.0, 268.0]], np.float64)
    akw = aos_kwargs(0.2, 1, res)
    (minx, maxx, miny, maxy), W, H = frame(poly, res)
    B = Builder(0, 0, res)
    B.polygon = poly
    h = 2.0 ** -6
    fres = float(F(res))
    taken = set()

    def lane(axis, k):
        """A free position along the other axis for a point whose cell along `axis` is k - 1, k or k + 1."""
        span = (H if axis == 0 else W) - 2
        cells = lambda j: [((k + d, j) if axis == 0 else (j, k + d)) for d in (-1, 0, 1)]   # noqa: E731
        start = (7 * len(taken) + 3) % span
        j = next(1 + (start + i) % span for i in range(span) if not any(c in taken for c in cells(1 + (start + i) % span)))
        taken.update(cells(j))
        return F(float(miny if axis == 0 else minx) + (j + 0.5) * fres)

    def pt(axis, v, k, companion=True):
        t = lane(axis, k)
        x, y = (v, t) if axis == 0 else (t, v)
        B.add(x, y, ZTOP, probe=True)
        if companion:
            B.add(x, y, F(float(ZTOP) + h))

    def around(v):
        return (np.nextafter(F(v), F(-1e9)), F(v), np.nextafter(F(v), F(1e9)))

    for face, axis, k in ((minx, 0, 0), (maxx, 0, W), (miny, 1, 0), (maxy, 1, H)):
        for v in around(face):
            pt(axis, v, k)
    for zf in (MINZ, ZTOP):
        for v in around(zf):
            t = lane(0, 7)
            B.add(F(float(minx) + 7.5 * fres), t, v, probe=True)
            B.add(F(float(minx) + 7.5 * fres), t, F(float(zf) + (h if zf > 0 else -h)))   # beyond the face
    n_face = len(B.probes)
    for axis in (0, 1):
        n_cells = W if axis == 0 else H
        for i, k in enumerate(sorted(set(int(v) for v in np.linspace(2, n_cells - 2, 16)))):
            for v in around(F(float(minx if axis == 0 else miny) + k * fres)):
                pt(axis, v, k, companion=i % 2 == 0)
    return Scene(f"clip_faces_and_cells-res{res:.2f}", B.xyz(), poly, akw, B.probes, n_face=n_face)


CELL_EXACT_RES = float(F(0.23))   # res * (1 / res) rounds below 1 in double: k res * (1 / res) < k for k a power of two


def cell_exact():
    """Resolution float32(0.23), the frame's origin at (0, 0): x = k res is exact in float32 for k = 1, 2, 4 .. 64, and
    there a * (1 / res) falls just below k while a / res is k, so only rt_cell's exact branch finds the cell. Those
    points and their float neighbours, along x (at y > 7.2, clear of the discs) and along y (at x > 69.5); every second
    one has a companion (need 2), the others drop."""
    res = CELL_EXACT_RES
    poly = np.array([[2.5, 2.5], [75.0, 2.5], [75.0, 15.0], [2.5, 15.0]], np.float64)
    akw = aos_kwargs(0.2, 1, res)
    (minx, _, miny, _), W, H = frame(poly, res)
    assert (float(minx), float(miny)) == (0.0, 0.0)
    B = Builder(0, 0, res)
    B.polygon = poly
    lane = 0
    for axis in (0, 1):
        for k in (1, 2, 4, 8, 16, 32, 64):
            e = F(k * res)
            for v in (np.nextafter(e, F(-1)), e, np.nextafter(e, F(1e9))):
                t = F(((33 if axis == 0 else 305) + lane % 30 + 0.5) * res)
                lane += 1
                x, y = (v, t) if axis == 0 else (t, v)
                B.add(x, y, ZTOP, probe=True)
                if lane % 2:
                    B.add(x, y, F(float(ZTOP) + 2.0 ** -6))
    return Scene("cell_exact", B.xyz(), poly, akw, B.probes, {"cell-exact"})


def disc_rims():
    """The default polygon at resolution 0.25. Per disc, the four axis points of the rim (exact where centre +- 1 is
    a float, or stepped one float out or in), 16 rim points (centre + (cos, sin), stepped -2 .. 2 floats in x), points in the strip between the discs' union and rt_candidate's fast-reject box and just outside the box, and
    probes outside a disc whose third point is a point the disc removes, and 64 points far from every disc. Every
    point has two companions above."""
    akw = aos_kwargs(0.2, 2)
    B = Builder(0, 0)
    B.polygon = None
    h = 2.0 ** -6
    taken = set()
    (minx, _, miny, _), W, H = frame(None, RES)

    def pt(x, y, companions=2):
        x, y = F(x), F(y)
        c = (int((float(x) - float(minx)) / RES), int((float(y) - float(miny)) / RES))
        if c in taken:
            return False
        taken.add(c)
        B.add(x, y, ZTOP, probe=True)
        for j in range(companions):
            B.add(x, y, float(ZTOP) + (j + 1) * h)
        return True

    for e, (ex, ey, er) in enumerate(DISCS):
        # the four axis points first: centre +- 1 is exact in float32 for most, so dist_sq == 1 exactly; then the same
        # a float further out (dist_sq just above 1) and a float further in, on the other axis points
        for a, (ux, uy) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):
            x, y = F(float(ex) + ux), F(float(ey) + uy)
            step = (0, 0, 1, -1)[(a + e) % 4]        # 0: on the rim, 1: outwards, -1: inwards
            for _ in range(abs(step)):
                if ux:
                    x = np.nextafter(x, F(1e9 * ux * step))
                else:
                    y = np.nextafter(y, F(1e9 * uy * step))
            pt(x, y)
        for a in range(16):
            t = 2 * math.pi * (a + 0.37 * (e % 3)) / 16
            x = F(float(ex) + math.cos(t))
            for _ in range(abs((a + e) % 5 - 2)):
                x = np.nextafter(x, F(-1e9) if (a + e) % 5 < 2 else F(1e9))
            pt(x, F(float(ey) + math.sin(t)))
    for x, y in ((-3.67, 1.8), (-3.67, 3.0), (69.03, 2.3), (69.03, 3.0), (30.0, 0.72), (10.0, 0.72), (30.0, 6.71),
                 (-1.0, 6.71), (-3.69, 1.8), (69.05, 2.3), (30.0, 0.70), (30.0, 6.73), (-3.68, 2.5), (69.04, 2.6),
                 (20.0, 0.71), (20.0, 6.72)):
        pt(x, y)
    for ex, ey, er in DISCS[[0, 2, 4, 8, 9]]:
        # a probe 0.05 outside the rim (straight below the centre) with one companion; its third point is a clip-plane
        # point 0.1 inside the rim, which the disc removes
        if pt(float(ex), float(ey) - 1.05, companions=1):
            B.add(F(float(ex)), F(float(ey) - 0.9), ZTOP, probe=True)
    for i in range(64):   # free points far from every disc
        pt(1.0 + i, 8.5 + 0.25 * (i % 3))
    return Scene("disc_rims", B.xyz(), None, akw, B.probes)


LAYOUTS = (("host", 16, (0, 4, 8)), ("device-16", 16, (0, 4, 8)), ("device-20", 20, (8, 0, 16)),
           ("device-32", 32, (12, 4, 20)))


def layouts():
    """radius_ties (r 0.25) inside chunk_edges' 8193 records; delivered in the four layouts of LAYOUTS."""
    ties = radius_ties(0.25, 1)
    B, xyz, probes = chunk_edges(8193, False, extra=ties.xyz)
    return Scene("layouts", xyz, B.polygon, aos_kwargs(0.25, 1), probes + [64 + int(i) for i in ties.probes],
                 modes=(False,))


@functools.lru_cache(maxsize=None)
def scene(name):
    return _BUILDERS[name]()


TIE_RADII = (0.25, 0.2, 0.12, 0.3)
_BUILDERS = {}
for _r in TIE_RADII:
    for _n in (1, 2):
        _BUILDERS[f"radius_ties-r{_r}-n{_n}"] = functools.partial(radius_ties, _r, _n)
_BUILDERS["contraction_pairs-dense"] = functools.partial(contraction_pairs, True)
_BUILDERS["contraction_pairs-sparse"] = functools.partial(contraction_pairs, False)
for _n in (0, 1, 2, 6, 13, 40, 100):
    _BUILDERS[f"need_sweep-n{_n}"] = functools.partial(need_sweep, _n)
_BUILDERS["tile_edges"] = functools.partial(tile_edges, False)
_BUILDERS["tile_edges-tb16"] = functools.partial(tile_edges, True)
_BUILDERS["big_tiles"] = big_tiles
for _n in CHUNK_SIZES:
    _BUILDERS[f"chunk_edges-{_n}"] = functools.partial(chunk_edges_scene, _n)
_BUILDERS["chunk_edges-8193-finite"] = functools.partial(chunk_edges_scene, 8193, True)
_BUILDERS["wide_scan"] = wide_scan
_BUILDERS["fine_radius"] = fine_radius
for _res in CELL_RES:
    _BUILDERS[f"clip_faces_and_cells-res{_res:.2f}"] = functools.partial(clip_faces_and_cells, _res)
_BUILDERS["cell_exact"] = cell_exact
_BUILDERS["disc_rims"] = disc_rims
_BUILDERS["layouts"] = layouts
SCENES = tuple(_BUILDERS)
# scenes whose probes are too few for the keep / drop thirds on their own (judged together, per family)
FAMILIES = {"chunk_edges": [n for n in SCENES if n.startswith("chunk_edges")]}

# handles through frames of changing size, density, polygon and is_dense: (scene, is_dense). A handle's parameters are
# fixed, so the scenes of one parameter set share a handle and the handles run interleaved. chunk_edges-2 -> radius_ties
# stages 35 times more (the staging guess overflows: the frame is redone); tile_edges -> tile_edges-tb16 -> tile_edges
# flips TB 32 -> 32 -> 16 -> 32 by the previous frame's binned count; big_tiles twice; the need_sweep blocks after others
HANDLE_ORDER = (("chunk_edges-2", False), ("radius_ties-r0.25-n1", False), ("wide_scan", True), ("tile_edges", True),
                ("tile_edges-tb16", True), ("tile_edges", False), ("tile_edges", True), ("big_tiles", True),
                ("chunk_edges-12293", False), ("disc_rims", True), ("need_sweep-n100", False), ("chunk_edges-1", False),
                ("fine_radius", True), ("big_tiles", False), ("radius_ties-r0.2-n2", True), ("disc_rims", False),
                ("wide_scan", False), ("chunk_edges-4097", False))


def handle_key(sc):
    return tuple(sorted(sc.akw.items()))


def stream_parts(sc, k=4, seed=3):
    """A scene's records in k deliveries: 40 % and 30 % at random (a probe's neighbours arrive later: it stays below
    need, then crosses it), then the western half of the rest (a scan that misses the other tiles), then the rest."""
    n = len(sc.xyz)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    a, b = perm[:int(0.4 * n)], perm[int(0.4 * n):int(0.7 * n)]
    rest = np.sort(perm[int(0.7 * n):])
    west = sc.xyz[rest, 0] < np.median(sc.xyz[:, 0])
    parts = [np.sort(a), np.sort(b), rest[west], rest[~west]]
    return parts[:k]


STREAM_SCENES = ("need_sweep-n6", "need_sweep-n13", "need_sweep-n100", "big_tiles")


def describe(sc, ref, is_dense, i):
    """A failing probe, for the tests' reports: index, coordinates, neighbour count, bin and tile."""
    _, _, g, s = regimes(sc.xyz, sc.polygon, sc.akw, is_dense, ref=ref)
    where = "not binned"
    j = np.flatnonzero(np.flatnonzero(s["mask"]) == i)
    if len(j):
        j = int(j[0])
        where = f"bin ({int(s['bx'][j])}, {int(s['by'][j])}) tile {int(s['tile'][j])} of {g.ntx} x {g.nty} (TB {g.TB})"
    return (f"point {i} at {tuple(float(v) for v in sc.xyz[i])}: cell ({int(ref['gx'][i])}, {int(ref['gy'][i])}), "
            f"{int(ref['counts'][i])} neighbours with itself, need {sc.akw['ror_min_neighbors'] + 1}, {where}")
