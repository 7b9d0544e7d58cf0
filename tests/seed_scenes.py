"""Designed skeletons for the stage between the clusters and the GVD (test infrastructure, imported like shapes.py):
the second half of run_cluster_seed_stage in csrc/cluster_seed.hip -- assemble_rows, k_virtual_candidates with
d_raycast, k_endpoint_rays, the three first-come 0.5 m de-duplications and k_concat3.

Three parts:
  * reference(): a plain numpy restatement of the reference node's rules for that stage (a10's k, a11, a12, the
    endpoint seeds, a13), from the oracle's rows, skeleton, grid info and the polygon. It classifies every candidate
    (base / hit / miss / exit, event step, clamped lookup, inside the polygon, kept or dropped by whom) and returns the
    three seed lists, which must equal the oracle's bit for bit (tests/test_seed_scenes_cpu.py).
  * predictors that restate the library's branch conditions, each constant named with its source line.
  * the scenes (SCENES) and check_regime(), which asserts on the reference's result alone that a scene reaches the
    regime it was designed for.
Scenes are built on shapes.scene: a raster injected through a cloud, R = 1, so a drawn line becomes a bar three cells
thick whose skeleton is the line (less a cell or so at each end).
"""
import functools
import math

import numpy as np

import shapes as S

# the library's constants the predictors use, each with the source line that sets it (tests/test_seed_scenes_cpu.py
# looks every one of these lines up in the source and compares the value, so a line that moves or changes fails there)
K_LOOK = 16            # cluster_seed.hip, above d_raycast:       constexpr int kLook = 16;  (samples per batch)
RAY_BATCH = 4          # cluster_seed.hip, k_endpoint_rays:       constexpr int kRayBatch = 4;  (groups of 64 per trip)
RAY_TRIP = RAY_BATCH * 64   #                                     base += 64 * kRayBatch
SMALL_MAX = 4096       # cluster_seed.h:                          constexpr int kSmallMax = 4096;  (k_dedup_small's limit)
SMALL_BUCKETS = 2048   # greedy.hip, above k_dedup_small:         kSmallBuckets = 2048;  (small_hash's cap)
LF_TB = 256            # greedy.hip, above k_lfmis:               constexpr int kLfTB = 256,  (candidates per block)
HASH_PAD = 50.0        # cluster_seed.hip, run_cluster_seed_stage: hx0 = g.minx - 50.0, ...  (the hash box's pad)

BASE, HIT, MISS, EXIT = 0, 1, 2, 3


# ---------------------------------------------------------------- the reference
def pip(px, py, poly):
    """isPointInPolygon seed_gen:1231-1255 (even-odd, double)."""
    inside = False
    n = len(poly)
    j = n - 1
    for i in range(n):
        xi, yi = poly[i]
        xj, yj = poly[j]
        dy = yj - yi
        if abs(dy) > 1e-9:
            if ((yi > py) != (yj > py)) and (px < (xj - xi) * (py - yi) / dy + xi):
                inside = not inside
        j = i
    return inside


class Grid:
    def __init__(self, o):
        self.W, self.H = int(o["width"]), int(o["height"])
        self.ox, self.oy = (float(v) for v in o["origin"])
        self.res32 = np.float32(o["resolution"])
        self.res = float(self.res32)
        self.skel = np.asarray(o["skeleton"]) == 100
        # castRayFromEndpoint's bounds: width * resolution is a float product (seed_gen:1809-1812)
        self.gw = float(np.float32(self.W) * self.res32)
        self.gh = float(np.float32(self.H) * self.res32)
        self.minx, self.maxx = self.ox, self.ox + self.gw
        self.miny, self.maxy = self.oy, self.oy + self.gh
        self.amax = math.sqrt(self.gw * self.gw + self.gh * self.gh) * 3.0
        t, cur = [], 1.0                      # current_dist = 1.0; current_dist += 0.1 (seed_gen:1833-1871)
        while cur <= self.amax:
            t.append(cur)
            cur += 0.1
        self.cur = np.array(t, np.float64)


def _world_to_grid(g, cx, cy):
    """worldToGrid seed_gen:760-769 on arrays: the float cast, the float quotient, floorf, the clamp.
    Returns (gx, gy, clamped)."""
    fx, fy = cx.astype(np.float32).astype(np.float64), cy.astype(np.float32).astype(np.float64)
    rx = np.floor(((fx - g.ox) / g.res).astype(np.float32)).astype(np.int64)
    ry = np.floor(((fy - g.oy) / g.res).astype(np.float32)).astype(np.int64)
    gx, gy = np.clip(rx, 0, g.W - 1), np.clip(ry, 0, g.H - 1)
    return gx, gy, (gx != rx) | (gy != ry)


def raycast(g, sx, sy, dx, dy, maxd=4.0, pad_to=1):
    """raycastToOccupiedCell seed_gen:1730-1771: f64 stepwise accumulation, min_distance 1.0.
    Returns a dict: hit, i (the hit's step index, -1), x, y, clamped (the hit's lookup), max_steps, dist (per step),
    occ (per step, the clamped lookup), and tail_occ: whether a step in [max_steps, max_steps rounded up to pad_to)
    finds skeleton at dist >= 1 (what a padded batch looks up and must mask)."""
    step = g.res * 0.5
    max_steps = int(maxd / step)
    n = -(-max_steps // pad_to) * pad_to
    incx, incy = dx * step, dy * step
    cx = np.add.accumulate(np.concatenate(([sx], np.full(n, incx))))[1:]     # cx += dir_x * step_size, in order
    cy = np.add.accumulate(np.concatenate(([sy], np.full(n, incy))))[1:]
    ddx, ddy = cx - sx, cy - sy
    dist = np.sqrt(ddx * ddx + ddy * ddy)
    gx, gy, clamped = _world_to_grid(g, cx, cy)
    occ = g.skel[gy, gx]
    ev = occ & ~(dist < 1.0)
    idx = np.nonzero(ev[:max_steps])[0]
    r = {"max_steps": max_steps, "dist": dist, "occ": occ, "tail_occ": bool(ev[max_steps:].any())}
    if len(idx):
        i = int(idx[0])
        same = (gx[:max_steps] == gx[i]) & (gy[:max_steps] == gy[i]) & ~(dist[:max_steps] < 1.0)
        skipped = occ[:i] & (dist[:i] < 1.0)
        r.update(hit=True, i=i, x=float(cx[i]), y=float(cy[i]), clamped=bool(clamped[i]), d=float(dist[i]),
                 alone=int(same.sum()) == 1, skip_d=float(dist[:i][skipped].max()) if skipped.any() else np.nan)
    else:
        skipped = occ[:max_steps] & (dist[:max_steps] < 1.0)
        r.update(hit=False, i=-1, x=sx + dx * maxd, y=sy + dy * maxd, clamped=False, d=np.nan, alone=False,
                 skip_d=float(dist[:max_steps][skipped].max()) if skipped.any() else np.nan)
    return r


def endpoint_ray(g, start, other, angle_deg):
    """castRayFromEndpoint seed_gen:1774-1891. Returns (class, event step, x, y, occ): occ the in-grid occupancy of
    every step of the distance table (for the regime checks)."""
    ex, ey = other[0] - start[0], other[1] - start[1]
    d = math.sqrt(ex * ex + ey * ey)
    if d < 1e-6:
        ex, ey = 1.0, 0.0
    else:
        z = ex * ex + ey * ey          # normalized(): v / sqrt(squaredNorm)
        if z > 0.0:
            q = math.sqrt(z)
            ex, ey = ex / q, ey / q
    ox_, oy_ = -ex, -ey
    px0, py0 = -ey, ex
    a = angle_deg * math.pi / 180.0
    if angle_deg > 0:
        c, s = math.cos(a), math.sin(a)
        rx, ry = c * ox_ + s * px0, c * oy_ + s * py0
    else:
        c, s = math.cos(-a), math.sin(-a)
        rx, ry = c * ox_ + s * (-px0), c * oy_ + s * (-py0)
    z = rx * rx + ry * ry
    if z > 0.0:
        q = math.sqrt(z)
        rx, ry = rx / q, ry / q
    px, py = start[0] + rx * g.cur, start[1] + ry * g.cur
    ins = (px >= g.minx) & (px <= g.maxx) & (py >= g.miny) & (py <= g.maxy)
    mx = ((px - g.ox) / g.res).astype(np.int64)      # static_cast<int>: towards zero (non-negative when inside)
    my = ((py - g.oy) / g.res).astype(np.int64)
    inr = ins & (mx >= 0) & (mx < g.W) & (my >= 0) & (my < g.H)
    occ = np.zeros(len(px), bool)
    occ[inr] = g.skel[my[inr], mx[inr]]
    ev = np.nonzero(~ins | occ)[0]
    if len(ev) == 0:                                   # the loop ran out (no real frame: amax is three diagonals)
        fx, fy = start[0] + rx * g.amax, start[1] + ry * g.amax
        fx, fy = max(g.minx, min(g.maxx, fx)), max(g.miny, min(g.maxy, fy))
        return MISS, len(px), fx, fy, occ
    i = int(ev[0])
    if not ins[i]:
        return EXIT, i, max(g.minx, min(g.maxx, float(px[i]))), max(g.miny, min(g.maxy, float(py[i]))), occ
    return HIT, i, float(px[i]), float(py[i]), occ


def first_come(cand, ok):
    """near_any's rule (seed_gen:2076-2085): a candidate joins the list unless an earlier kept one lies at
    sqrt(pow(dx, 2) + pow(dy, 2)) < 0.5. Returns (kept flags, by: the kept candidate that dropped it or -1)."""
    n = len(cand)
    kept = np.zeros(n, bool)
    by = np.full(n, -1, np.int64)
    kx, ky, ki = np.empty(n), np.empty(n), np.empty(n, np.int64)
    m = 0
    for c in range(n):
        if not ok[c]:
            continue
        dx, dy = kx[:m] - cand[c, 0], ky[:m] - cand[c, 1]
        near = np.nonzero(np.sqrt(dx * dx + dy * dy) < 0.5)[0]     # pow(x, 2) is x * x exactly
        if len(near):
            by[c] = ki[near[0]]
            continue
        kx[m], ky[m], ki[m] = cand[c, 0], cand[c, 1], c
        m += 1
        kept[c] = True
    return kept, by


def _listing(cand, ok, **meta):
    cand = np.array(cand, np.float64).reshape(-1, 2)
    ok = np.array(ok, bool)
    kept, by = first_come(cand, ok)
    d = {"cand": cand, "ok": ok, "kept": kept, "by": by, "seeds": cand[kept]}
    d.update({k: np.array(v) for k, v in meta.items()})
    return d


def row_k(start, end):
    """generateVirtualSeeds' seed count of a row (seed_gen:2020-2040): 0 below 1 m, else floor(distance)."""
    dx, dy = end[0] - start[0], end[1] - start[1]
    dist = math.sqrt(dx * dx + dy * dy)
    if dist < 1.0 or dist < 1e-6:
        return 0
    return int(math.floor(dist / 1.0))


def reference(o, polygon):
    """The stage's three candidate lists, classified, and its seed lists, from the oracle's rows, skeleton and grid.
    {"k": per row, "virtual" / "ray" / "endpoint": {cand, ok (outside the polygon and admissible), kept, by, seeds,
    cls, step, clamped, row ...}, "voronoi": the concatenation}."""
    g = Grid(o)
    poly = [(float(x), float(y)) for x, y in np.asarray(polygon, np.float64)]
    starts, ends, centers = o["row_start"], o["row_end"], o["row_center"]
    nr = len(starts)
    ks = [row_k(starts[r], ends[r]) for r in range(nr)]

    # a11 generateVirtualSeeds seed_gen:1987-2268
    vc, vok, vcls, vstep, vclamp, vrow, vtail, vd_nom, vmax = [], [], [], [], [], [], [], [], []
    vd, valone, vskip = [], [], []
    for r in range(nr):
        if not pip(centers[r][0], centers[r][1], poly) or ks[r] == 0:
            continue
        sx, sy, ex, ey = starts[r][0], starts[r][1], ends[r][0], ends[r][1]
        dx, dy = ex - sx, ey - sy
        nrm = math.sqrt(dx * dx + dy * dy)
        rdx, rdy = dx / nrm, dy / nrm
        for i in range(1, ks[r] + 1):
            t = float(i) / (ks[r] + 1)
            bx, by = sx + t * dx, sy + t * dy
            vc.append((bx, by)); vok.append(True); vcls.append(BASE); vstep.append(-1); vclamp.append(False)
            vrow.append(r); vtail.append(False); vd_nom.append(np.nan); vmax.append(0)
            vd.append(np.nan); valone.append(False); vskip.append(np.nan)
            for pdx, pdy in ((-rdy, rdx), (rdy, -rdx)):
                rc = raycast(g, bx, by, pdx, pdy, 4.0, pad_to=K_LOOK)
                vc.append((rc["x"], rc["y"]))
                vok.append(not pip(rc["x"], rc["y"], poly))
                vcls.append(HIT if rc["hit"] else MISS); vstep.append(rc["i"]); vclamp.append(rc["clamped"])
                vrow.append(r); vtail.append(rc["tail_occ"]); vmax.append(rc["max_steps"])
                nominal = int(round(1.0 / (g.res * 0.5))) - 1      # the step whose exact distance is 1.0
                vd_nom.append(rc["dist"][nominal])
                vd.append(rc["d"]); valone.append(rc["alone"]); vskip.append(rc["skip_d"])
    virtual = _listing(vc, vok, cls=vcls, step=vstep, clamped=vclamp, row=vrow, tail_occ=vtail, d_nominal=vd_nom,
                       max_steps=vmax, d=vd, alone=valone, skip_d=vskip)

    # a12 generateRayPointsFromEndpoints seed_gen:1894-1982
    rc_, rok, rcls, rstep, rrow, rlater = [], [], [], [], [], []
    for r in range(nr):
        e1, e2 = tuple(starts[r]), tuple(ends[r])
        for st, ot in ((e1, e2), (e2, e1)):
            for ang in (0.0, -90.0, 90.0):
                cls, i, x, y, occ = endpoint_ray(g, st, ot, ang)
                good = (math.isfinite(x) and math.isfinite(y) and g.minx <= x <= g.maxx and g.miny <= y <= g.maxy
                        and not pip(x, y, poly))
                rc_.append((x, y)); rok.append(good); rcls.append(cls); rstep.append(i); rrow.append(r)
                # an occupied step later in the same group of 64 steps: a second event lane in the one ballot that
                # decides the hit (an event at lane 63 has none)
                hi = min(len(occ), (i // 64 + 1) * 64)
                rlater.append(bool(occ[i + 1:hi].any()))
    ray = _listing(rc_, rok, cls=rcls, step=rstep, row=rrow, later_occ=rlater)

    # endpoint seeds seed_gen:1451-1496
    ec = [p for r in range(nr) for p in (tuple(starts[r]), tuple(ends[r]))]
    endpoint = _listing(ec, [True] * len(ec), row=[r for r in range(nr) for _ in (0, 1)])

    vor = np.concatenate([virtual["seeds"], ray["seeds"], endpoint["seeds"]])      # a13 seed_gen:1670-1710
    return {"k": np.array(ks, np.int64), "virtual": virtual, "ray": ray, "endpoint": endpoint, "voronoi": vor,
            "grid": g}


def assert_reference_equals_oracle(ref, o):
    for k, lst in (("virtual_seeds", ref["virtual"]["seeds"]), ("ray_seeds", ref["ray"]["seeds"]),
                   ("endpoint_seeds", ref["endpoint"]["seeds"]), ("voronoi_seeds", ref["voronoi"])):
        assert lst.shape == o[k].shape, (k, lst.shape, o[k].shape)
        assert np.array_equal(lst, o[k]), f"the reference's {k} differ from the oracle's"


# ---------------------------------------------------------------- predictors (the library's branch conditions)
def n_slots(ref):
    """assemble_rows (cluster_host.cpp): three candidate slots per virtual base seed."""
    return 3 * int(ref["k"].sum())


def uses_small_dedup(n_rows):
    """run_cluster_seed_stage (cluster_seed.hip), `if (6 * nr <= kSmallMax)`: the ray and endpoint lists go through
    k_dedup_small then, through k_lfmis otherwise."""
    return 6 * n_rows <= SMALL_MAX


def lfmis_blocks(n):
    """k_lfmis blocks for n candidates (greedy.hip: one block per kLfTB candidates)."""
    return -(-n // LF_TB)


def small_hash(g, cell=0.5):
    """small_hash = make_hash_cap over make_hash (all greedy.hip) on the grid's box padded by HASH_PAD: the
    cell grows by 1.25 until nx * ny <= kSmallBuckets. Returns (cell, nx, ny, x0, y0, inv)."""
    x0, x1, y0, y1 = g.minx - HASH_PAD, g.maxx + HASH_PAD, g.miny - HASH_PAD, g.maxy + HASH_PAD
    c = cell
    while True:
        inv = 1.0 / (c * (1.0 + 1e-9))
        nx, ny = max(1, int((x1 - x0) * inv + 2.0)), max(1, int((y1 - y0) * inv + 2.0))
        if nx * ny <= SMALL_BUCKETS:
            return c, nx, ny, x0, y0, inv
        c *= 1.25


def largest_small_bucket(g, pts):
    """The most points of `pts` in one bucket of small_hash."""
    c, nx, ny, x0, y0, inv = small_hash(g)
    bx = np.clip(((pts[:, 0] - x0) * inv).astype(np.int64), 0, nx - 1)
    by = np.clip(((pts[:, 1] - y0) * inv).astype(np.int64), 0, ny - 1)
    return int(np.bincount(by * nx + bx).max()) if len(pts) else 0


def cur_tab_len(g):
    """run_cluster_seed_stage's `for (double cur = 1.0;; cur += 0.1)` (cluster_seed.hip): the table holds every value
    <= amax and the first one above it."""
    return len(g.cur) + 1


def max_steps(res):
    """d_raycast (cluster_seed.hip): (int)(4.0 / (res * 0.5))."""
    return int(4.0 / (float(np.float32(res)) * 0.5))


# ---------------------------------------------------------------- scene building blocks
def bar(p, x, y, deg, L):
    """A line of L cells from (x, y) at `deg` degrees (R = 1 makes it a bar three cells thick)."""
    t = np.linspace(0.0, L, 8 * int(L) + 1)
    S._plot(p, x + t * math.cos(math.radians(deg)), y + t * math.sin(math.radians(deg)))


def cbar(p, cx, cy, deg, L):
    """bar() centred on (cx, cy)."""
    bar(p, cx - 0.5 * L * math.cos(math.radians(deg)), cy - 0.5 * L * math.sin(math.radians(deg)), deg, L)


def cell_polygon(cells, res=S.RES):
    """A polygon given in grid cell corners (cell 0 = the grid's origin)."""
    return np.array([(S.ORIGIN + x * res, S.ORIGIN + y * res) for x, y in cells], np.float64)


def l_polygon(W, H, cx, cy, res=S.RES):
    """The rectangle less its upper right part x > cx, y > cy (cells)."""
    m = S.margin_cells(res)
    return cell_polygon([(m, m), (W - m, m), (W - m, cy), (cx, cy), (cx, H - m), (m, H - m)], res)


def frame(pattern, polygon=None, res=S.RES, R=1, **params):
    cloud, poly, akw, okw = S.scene(pattern, R, polygon=polygon, res=res, **params)
    return {"pattern": pattern, "cloud": cloud, "polygon": poly, "akw": akw, "okw": okw}


OFF_AXIS = [q * 90 + off for off in (8, 21, 34, 47, 60, 73, 82) for q in (-2, -1, 0, 1)]   # none within 8 deg of an axis


def _fan(**params):
    """Slanted bars over an L-shaped polygon; a mesh of walls in the cut-out; bars along the cut-out's two edges, whose
    perpendicular rays cross the edge."""
    W = H = 340
    p = S._empty(W, H)
    for k in range(25):
        cbar(p, 32 + 28 * (k % 5), 32 + 28 * (k // 5), OFF_AXIS[k], 16)
    for j in range(6):
        cbar(p, 162, 188 + 24 * j, 90 + (12 + 5 * j) * (-1) ** j, 16)      # along the edge x = 170, y > 170
        cbar(p, 188 + 24 * j, 162, (12 + 5 * j) * (-1) ** j, 16)           # along the edge y = 170, x > 170
    p[173:326, 173:326:12] = 1
    p[173:326:12, 173:326] = 1
    return frame(p, l_polygon(W, H, 170, 170), **params)


def _cur_table(n):
    t, cur = [], 1.0
    for _ in range(n):
        t.append(cur)
        cur += 0.1
    return t


EVENT_TARGETS = [63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193, 254, 255, 256, 257, 258, 320, 321, 382, 383,
                 384, 385, 446, 447, 448, 449, 510, 511, 512, 513, 514, 574, 575, 576, 577]
EVENT_ROW_X1, EVENT_ROW_LEN, EVENT_PITCH = 272, 10, 8


def _event_walls(x_end):
    """For each wanted event step, the wall column whose cell the leftward ray from cell corner x_end first enters at
    that step (by the reference's distance table), where one exists."""
    cur = _cur_table(700)
    first = {}
    for i, c in enumerate(cur):
        col = math.floor(x_end - c / S.RES)
        first.setdefault(col, i)
    by_step = {i: col for col, i in first.items()}
    return [(i, by_step[i]) for i in EVENT_TARGETS if i in by_step]


def _event_lanes(x_end=EVENT_ROW_X1 - EVENT_ROW_LEN):
    """Short horizontal rows in a strip of the polygon on the right; each row's outward ray from its left end runs
    through the cut-out to a wall of its own, placed so that the ray's first occupied step is a chosen index."""
    walls = _event_walls(x_end)
    W, H = 300, 20 + 16 + EVENT_PITCH * len(walls) + 8
    p = S._empty(W, H)
    for j, (i, col) in enumerate(walls):
        y = 34 + EVENT_PITCH * j
        p[y, x_end - 1:EVENT_ROW_X1 + 1] = 1      # (the skeleton ends one cell inside the drawn line)
        p[y - 1:y + 2, col] = 1
    m = S.MARGIN
    sx = x_end - 2                          # the strip's left edge: two cells left of the rows' ends
    poly = cell_polygon([(m, m), (W - m, m), (W - m, H - m), (sx, H - m), (sx, m + 8), (m, m + 8)])
    return frame(p, poly, cluster_min_length=1.0)


def _min_distance():
    W, H = 220, 140
    p = S._empty(W, H)
    p[8, 14:206] = 1                       # a line in the margin four cells below the rows on cell row 12
    p[H - 8, 14:206] = 1                   # and one four cells above the rows on cell row H - 12
    for x in range(20, 190, 24):
        p[12, x:x + 14] = 1
        p[H - 12, x:x + 14] = 1
    for k in range(14):
        cbar(p, 24 + 13 * k, 50 + 30 * (k % 2), OFF_AXIS[2 * k], 16)
    return frame(p)


def _batch_tail(res):
    """Horizontal rows near the polygon's lower and upper edges and a line in each margin. Downwards, sample j lies at
    r - (j + 1) / 2 cells, so the line on cell row r - n_last holds the last valid sample alone (a hit in the last
    step); upwards, the line on cell row r + n_last is first reached by sample max_steps, which only a padded batch
    looks up (a miss: the 4 m point is the seed)."""
    m, ms = S.margin_cells(res), max_steps(res)
    n_last = (ms + 1) // 2
    L = {0.15625: 20, 0.3125: 12, 0.5: 8}[res]
    W, H = 2 * m + 6 * (L + 10), 2 * m + 90
    p = S._empty(W, H)
    lo, hi = n_last + 3, H - n_last - 4            # the rows' cell rows: the lines fall on rows 3 and H - 4
    assert m < lo and hi < H - m
    p[lo - n_last, 4:W - 4] = 1
    p[hi + n_last, 4:W - 4] = 1
    for k in range(6):
        x = m + 5 + k * (L + 10)
        p[lo, x:x + L] = 1
        p[hi, x:x + L] = 1
    return frame(p, res=res, cluster_min_length=1.0)


def _clamp():
    """Slanted rows close to the polygon's left edge; blocks of skeleton on grid column 0 with gaps. A perpendicular
    ray that crosses column 0 through a gap goes on outside the grid, where its samples' cell is clamped back onto
    column 0 and moves along it."""
    # A ray at t degrees from the x axis from a base bx cells from the border leaves the grid with 16 cos t - bx cells to
    # go, during which it moves 16 sin t - bx tan t cells along the border: at most ~1.2 cells for bx = 12 (two cells
    # inside the polygon), at t ~ 25 degrees. So the rows are steep (64 to 72 degrees), their lower bases lie 2 to 3 cells
    # inside the polygon, and the row pitch (23) walks them through every phase of the blocks' period (10: 8 cells of
    # skeleton, a gap of 2).
    W, H = 120, 40 + 23 * 22
    p = S._empty(W, H)
    for y in range(H):
        if y % 10 < 6:
            p[y, 0:2] = 1
    for j in range(22):
        cbar(p, 13.5, 30 + 23 * j, (64 + 2 * (j % 5)) * (-1) ** j, 12)
    return frame(p, cluster_min_length=1.0)


def _short_rows(kind, min_length=None):
    """Dots (zero-length rows), bars of two to five skeleton cells (k = 0) and long bars (k > 0) in raster order: short
    ones first, last, singly and in runs between long ones."""
    W, H = 200, 130
    p = S._empty(W, H)

    def dots(y, x0, n):
        p[y, x0:x0 + 6 * n:6] = 1

    def shorts(y, x0, lens):
        for k, L in enumerate(lens):
            p[y, x0 + 12 * k:x0 + 12 * k + L] = 1

    dots(14, 14, 8)
    shorts(20, 14, [4, 5, 6, 4, 5, 6])
    for band, y in enumerate(range(28, 100, 8)):
        x = 14
        for k in range(2):
            if kind != "noslots":
                p[y, x:x + 18] = 1                       # a long bar
            x += 24
            n = (2 * band + k) % 4                       # then 0 to 3 short bars (0.5 and 0.75 m) and as many dots
            shorts(y, x, [5, 6, 5][:n])
            x += 12 * n
            dots(y, x, n)
            x += 6 * n + 6
    shorts(106, 14, [6, 5, 4, 6])
    dots(114, 14, 8)
    return frame(p, cluster_min_length=min_length if min_length is not None else 0.5 if kind == "0.5" else 0.0)


# Slanted bars (cx, cy, degrees, cells) of the ties scene, found by a search over the oracle's result: hit and exit
# points and 4 m points of slanted rows are not on the 0.25 m lattice of the row ends, so they come as close to 0.5 m
# as one cares to search. The first two face each other across the polygon's slot: a 4 m point of the slanted one lies
# 0.49985 m from one of the level one's and is dropped by it. A ray of the third leaves through the left border
# 0.5 - 3.4e-13 m from the exit point of a ray of the staircase, which comes first.
TIES_NEAR_BARS = [(225.0, 124.0, 0.0, 12), (227.0, 157.0, -10.0, 12), (115.0, 176.0, 135.5, 8)]
# the largest distance at which each list of the ties scene must drop a candidate: row ends are cell corners, and on
# that lattice 0.25 sqrt(2) = 0.35355 is the largest distance below 0.5 (then comes 0.5 itself, along an axis)
TIES_DROPPED_AT_LEAST = {"virtual": 0.4998, "ray": 0.4999999, "endpoint": 0.3535}


def _ties(near_bars=None):
    W, H = 260, 200
    p = S._empty(W, H)
    for b in TIES_NEAR_BARS if near_bars is None else near_bars:
        cbar(p, *b)
    p[176, 230] = p[177, 231] = 1                        # a two-cell diagonal row: its ends are 0.35355 m apart
    for i in range(10):                                  # a staircase: exit points 0.25 m apart on both borders
        p[16 + i, 20 + 12 * i:20 + 12 * i + 8] = 1
    p[40, 180:231] = 1                                   # a wall that a one-cell notch of the polygon cuts at x = 205
    p[60:71, 204] = 1                                    # two teeth above it, on the columns beside and in the notch:
    p[80:91, 205] = 1                                    # the lower one's hit is inside the polygon and comes first
    for y in (60, 76, 92):                               # a stack 4 m apart: the 4 m point of one is the next one's base
        p[y, 60:74] = 1
    # rows 4 m below and 4 m above a slot of the polygon: their 4 m points meet in it, 0.5 m and 0.25 m apart
    p[124, 150:164] = 1
    p[158, 150:164] = 1
    p[124, 180:194] = 1
    p[157, 180:194] = 1
    p[100, 20:24] = 1                                    # a two-cell row: its ends are 0.25 m apart
    p[100, 40:44] = 1
    m = S.MARGIN
    poly = cell_polygon([(m, m), (204.5, m), (204.5, 45.5), (205.5, 45.5), (205.5, m), (W - m, m), (W - m, 138.5),
                         (140.5, 138.5), (140.5, 144.5), (W - m, 144.5), (W - m, H - m), (m, H - m)])
    return frame(p, poly, cluster_min_length=0.0)


def comb_teeth(n, per_line, W=None, tooth=7, pitch=4, line_pitch=None, stagger=0):
    """n vertical teeth of `tooth` cells (a skeleton of tooth - 2: 1.0 m for 7, so k = 1), per_line to a line; stagger:
    columns by which each line is shifted against the one below (with 1 and four lines no tooth stands in the way of
    another's vertical ray)."""
    line_pitch = line_pitch or tooth + 4
    lines = -(-n // per_line)
    W = W or 2 * S.MARGIN + 8 + pitch * per_line
    H = 2 * S.MARGIN + 8 + line_pitch * lines
    p = S._empty(W, H)
    for t in range(n):
        line = t // per_line
        x, y = S.MARGIN + 4 + pitch * (t % per_line) + stagger * line, S.MARGIN + 4 + line_pitch * line
        p[y:y + tooth, x] = 1
    return p


def _small_edge(kind):
    if kind == "wide":
        return frame(comb_teeth(682, 682), cluster_min_length=0.5)
    if kind == "dense":
        return frame(comb_teeth(682, 171, stagger=1), cluster_min_length=0.5)
    return frame(comb_teeth(int(kind), 62), cluster_min_length=0.5)


def _equal_centres():
    p = comb_teeth(96, 48, line_pitch=14)
    p[S.MARGIN + 4 + 14 + 7, S.MARGIN + 4:S.MARGIN + 4 + 4 * 48:8] = 1     # every other tooth of line 2 a cell longer
    return frame(p, cluster_min_length=0.5)


SCENES = {
    "fan": _fan,
    "event_lanes": _event_lanes,
    "min_distance": _min_distance,
    "batch_tail-0.15625": lambda: _batch_tail(0.15625),
    "batch_tail-0.3125": lambda: _batch_tail(0.3125),
    "batch_tail-0.5": lambda: _batch_tail(0.5),
    "clamp": _clamp,
    "short_rows-0": lambda: _short_rows("0"),
    "short_rows-0.5": lambda: _short_rows("0.5"),
    "short_rows-noslots": lambda: _short_rows("noslots"),
    "ties": _ties,
    "small_edge-682": lambda: _small_edge("682"),
    "small_edge-683": lambda: _small_edge("683"),
    "small_edge-wide": lambda: _small_edge("wide"),
    "small_edge-dense": lambda: _small_edge("dense"),
    "equal_centres": _equal_centres,
    # the one-handle sequence's frames share small_edge's parameters (cluster_min_length 0.5: no zero-length rows)
    "fan@0.5": lambda: _fan(cluster_min_length=0.5),
    "short_rows-noslots@0.5": lambda: _short_rows("noslots", 0.5),
}


def tie_pairs(lst):
    """Of a classified list: (pairs exactly 0.5 m apart with both kept, the largest distance below 0.5 m at which a
    candidate was dropped, or nan)."""
    c, ok, kept, by = lst["cand"], lst["ok"], lst["kept"], lst["by"]
    exact, below = 0, np.nan
    idx = np.nonzero(ok)[0]
    for b in idx:
        d = c[idx[idx < b]] - c[b]
        dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        if kept[b]:
            exact += int(np.count_nonzero((dist == 0.5) & kept[idx[idx < b]]))
        elif by[b] >= 0:
            db = c[by[b]] - c[b]
            below = np.nanmax([below, math.sqrt(db[0] * db[0] + db[1] * db[1])])
    return exact, float(below)


def longest_chain(lst):
    """The longest run c0 < c1 < ... of admissible candidates in which each one's only earlier admissible candidate
    within 0.5 m is its predecessor: alternate ones are kept, and a round-by-round resolution (k_dedup_small) needs as
    many rounds as the run is long."""
    c = lst["cand"]
    idx = np.nonzero(lst["ok"])[0]
    best, length = 0, {}
    for n, b in enumerate(idx):
        d = c[idx[:n]] - c[b]
        near = idx[:n][np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) < 0.5]
        length[b] = length[near[0]] + 1 if len(near) == 1 else 1
        best = max(best, length[b])
    return best


def blocked_then_kept(lst):
    """Candidates with ok = 0 that a later kept candidate follows within 0.5 m."""
    c, ok, kept = lst["cand"], lst["ok"], lst["kept"]
    n = 0
    for a in np.nonzero(~ok)[0]:
        later = np.nonzero(kept[a + 1:])[0] + a + 1
        d = c[later] - c[a]
        n += bool((np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) < 0.5).any())
    return n


def zero_runs(k):
    """(lengths of the runs of k = 0 rows that lie between rows with k > 0, k = 0 first, k = 0 last)."""
    nz = np.nonzero(k > 0)[0]
    if len(nz) == 0:
        return [], bool(len(k)), bool(len(k))
    gaps = np.diff(nz) - 1
    return [int(g) for g in gaps if g > 0], bool(k[0] == 0), bool(k[-1] == 0)


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


GVD_MAX_SEEDS = 3000   # the oracle's GVD is quadratic in the seeds
# one handle through these: the grid diagonal changes at every step (the distance table is rebuilt, shortened and
# rebuilt), the candidate buffers shrink and grow, the third frame has no slots
HANDLE_ORDER = ["small_edge-wide", "fan@0.5", "short_rows-noslots@0.5", "small_edge-wide"]
TILED_SCENES = ["fan", "short_rows-0"]


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    """(frame, oracle result, reference, regime figures, oracle GVD or None, oracle seconds) of a scene, computed once
    and shared (never modified). The regime is asserted here, so no test runs a scene that has drifted out of it."""
    import time

    import oracle_py as O
    f = scene(name)
    O.lib()                # builds and loads the oracle where it is missing or stale: not part of the frame's time
    t0 = time.perf_counter()
    o = O.seedgen(f["cloud"], f["polygon"], O.default_params(**f["okw"]))
    dt = time.perf_counter() - t0
    assert np.array_equal(o["raster"] != 0, f["pattern"] != 0), "the oracle's raster is not the pattern"
    ref = reference(o, f["polygon"])
    assert_reference_equals_oracle(ref, o)
    fig = check_regime(name, o, ref, f["polygon"])
    og = None
    if len(o["voronoi_seeds"]) < GVD_MAX_SEEDS:
        og = O.gvd(o["voronoi_seeds"], o["rows_info"], o, O.default_params(**f["okw"]))
    return f, o, ref, fig, og, dt


# ---------------------------------------------------------------- regimes
def row_angles(o):
    d = o["row_end"] - o["row_start"]
    return np.degrees(np.arctan2(d[:, 1], d[:, 0]))


def check_regime(name, o, ref, polygon):
    """Asserts, on the oracle's rows and the reference's classification alone, that the scene reaches its regime;
    returns the figures."""
    v, r, e = ref["virtual"], ref["ray"], ref["endpoint"]
    side = v["cls"] != BASE
    name, _, in_sequence = name.partition("@")
    fig = {"rows": len(o["row_length"]), "slots": n_slots(ref), "virtual": int(v["kept"].sum()),
           "ray": int(r["kept"].sum()), "endpoint": int(e["kept"].sum()),
           "ray_hits_kept": int(np.count_nonzero((r["cls"] == HIT) & r["kept"])),
           "side_hits_kept": int(np.count_nonzero((v["cls"] == HIT) & v["kept"]))}
    if name == "fan":
        a = row_angles(o)
        off = np.abs((a + 45.0) % 90.0 - 45.0)          # distance to the nearest axis
        fig["quadrants"] = [int(np.count_nonzero((a > q) & (a < q + 90))) for q in (-180, -90, 0, 90)]
        fig["min_off_axis"] = float(off.min())
        assert fig["rows"] >= 20 and min(fig["quadrants"]) >= 1 and fig["min_off_axis"] > 3.0, fig
        assert fig["ray_hits_kept"] >= 20 and fig["side_hits_kept"] >= 10, fig
    elif name == "event_lanes":
        hit = (r["cls"] == HIT) & r["kept"]
        i = r["step"][hit]
        fig["steps"] = sorted(int(x) for x in i)
        fig["thick"] = int(np.count_nonzero(r["later_occ"][hit]))
        assert {0, 1, 62, 63} <= {int(x) % 64 for x in i}, fig
        assert {0, 1, 2, 3} == {int(x) // 64 % 4 for x in i}, fig
        for edge in (RAY_TRIP, 2 * RAY_TRIP):
            # (in the last group of 64 before the trip's end and in the first one after it)
            assert ((i >= edge - 64) & (i < edge)).any() and ((i >= edge) & (i < edge + 64)).any(), fig
        assert fig["thick"] >= 1, fig
    elif name == "min_distance":
        hk = side & (v["cls"] == HIT) & v["kept"]
        fig["exact_alone"] = int(np.count_nonzero(hk & (v["d"] == 1.0) & v["alone"]))
        fig["exact_first_of_two"] = int(np.count_nonzero(hk & (v["d"] == 1.0) & ~v["alone"]))
        fig["skipped_0875"] = int(np.count_nonzero(side & (v["skip_d"] == 0.875)))
        a = row_angles(o)[v["row"]]
        slanted = side & (np.abs((a + 45.0) % 90.0 - 45.0) > 3.0)
        fig["nominal_below"] = int(np.count_nonzero(slanted & (v["d_nominal"] < 1.0)))
        fig["nominal_at_or_above"] = int(np.count_nonzero(slanted & (v["d_nominal"] >= 1.0)))
        assert fig["exact_alone"] >= 3 and fig["exact_first_of_two"] >= 3 and fig["skipped_0875"] >= 3, fig
        assert fig["nominal_below"] >= 5 and fig["nominal_at_or_above"] >= 5, fig
    elif name.startswith("batch_tail"):
        g = ref["grid"]
        ms = max_steps(g.res)
        fig["max_steps"] = ms
        fig["side_hits_last_step"] = int(np.count_nonzero(side & (v["cls"] == HIT) & (v["step"] == ms - 1) & v["kept"]))
        fig["tail_misses_kept"] = int(np.count_nonzero(side & (v["cls"] == MISS) & v["tail_occ"] & v["kept"]))
        assert set(v["max_steps"][side]) == {ms}, fig
        if name.endswith("-0.5"):
            assert ms == K_LOOK and fig["side_hits_kept"] >= 3, fig
        else:
            assert ms == {"0.15625": 51, "0.3125": 25}[name.split("-")[1]] and ms % K_LOOK != 0, fig
            assert fig["side_hits_last_step"] >= 3 and fig["tail_misses_kept"] >= 3, fig
    elif name == "clamp":
        fig["clamped_hits_kept"] = int(np.count_nonzero(side & (v["cls"] == HIT) & v["clamped"] & v["kept"]))
        g = ref["grid"]
        on_border = side & (v["cls"] == HIT) & ~v["clamped"] & v["kept"] & (v["cand"][:, 0] < g.minx + g.res)
        fig["border_column_hits_kept"] = int(np.count_nonzero(on_border))
        assert fig["clamped_hits_kept"] >= 3, fig
    elif name.startswith("short_rows"):
        k = ref["k"]
        runs, first, last = zero_runs(k)
        d = o["row_end"] - o["row_start"]
        fig.update(k0=int(np.count_nonzero(k == 0)), runs=sorted(set(runs)), first=first, last=last,
                   zero_length=int(np.count_nonzero((d == 0).all(axis=1))))
        if name.endswith("noslots"):
            assert fig["rows"] >= 20 and fig["slots"] == 0 and (fig["zero_length"] >= 10 or in_sequence), fig
        else:
            assert first and last and runs and max(runs) >= 3 and fig["slots"] > 0, fig
            assert fig["zero_length"] >= 10 or name.endswith("-0.5"), fig
    elif name == "ties":
        for key, lst in (("virtual", v), ("ray", r), ("endpoint", e)):
            fig[key + "_exact_pairs"], fig[key + "_dropped_below"] = tie_pairs(lst)
            assert fig[key + "_exact_pairs"] >= 1, fig
            assert TIES_DROPPED_AT_LEAST[key] <= fig[key + "_dropped_below"] < 0.5, fig
        fig["chain"] = max(longest_chain(lst) for lst in (v, r, e))
        fig["blocked_then_kept"] = [blocked_then_kept(lst) for lst in (v, r)]
        assert fig["chain"] >= 8 and sum(fig["blocked_then_kept"]) >= 3 and min(fig["blocked_then_kept"]) >= 1, fig
    elif name.startswith("small_edge"):
        nr = fig["rows"]
        g = ref["grid"]
        fig["small"] = uses_small_dedup(nr)
        fig["hash"] = small_hash(g)[:3]
        fig["largest_bucket"] = largest_small_bucket(g, r["cand"][r["ok"]])
        if name.endswith("683"):
            assert nr == 683 and not fig["small"] and lfmis_blocks(6 * nr) > 1 and lfmis_blocks(2 * nr) > 1, fig
        else:
            assert nr == 682 and fig["small"] and 6 * (nr + 1) > SMALL_MAX, fig
        # Hundreds of exit points in one bucket are not reached, 8 and 19 are. Nothing in k_dedup_small
        # depends on how full a bucket is (its walk over a bucket's items is one loop without a capacity, wholly in
        # LDS), so a fuller bucket takes no other branch, only more turns of that loop. The wide frame takes the
        # largest cell; the dense one (four staggered lines: every column of the upper and lower border an exit point
        # of these axis-parallel rays) the fullest bucket.
        if name.endswith("wide"):
            assert fig["hash"][0] > 7.0 and fig["largest_bucket"] >= 8, fig
        if name.endswith("dense"):
            assert fig["hash"][0] > 4.0 and fig["largest_bucket"] >= 16, fig
    elif name == "equal_centres":
        cy = o["row_center"][:, 1]
        vals, counts = np.unique(cy, return_counts=True)
        fig["most_equal"] = int(counts.max())
        fig["min_gap"] = float(np.diff(vals).min()) if len(vals) > 1 else 0.0
        assert fig["most_equal"] >= 40 and len(vals) >= 2 and fig["min_gap"] > 1e-6, fig
    else:
        raise KeyError(name)
    return fig
