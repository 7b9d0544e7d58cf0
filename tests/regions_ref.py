"""aos_gvd_regions restated with numpy, from the definitions in include/aos_gpu.h alone.

Occupied cell: the byte is 100. Sites: without caller labels the occupied cells of the 8-connected components with at
least min_component_cells cells, each labelled by its component's least linear index (a plain flood fill); with labels
the occupied cells whose label is >= 0. site[c] = the site with the least key d2 * 2^28 + index (d2 < 2^29 and
index < 2^28, so the key orders the pairs (d2, index) lexicographically). Two statements of it: brute force (every cell
against every site) for small grids and a separable one (per column the nearest site row, the smaller row at equal
distance; then every row's cells against every column) for mid-size grids; both are integer and have to agree word for
word. region = the site's label; the ridge by the pair rule, written as the header words it; ridge_d2 = clearance_ref's
field over the ridge cells.
"""
import numpy as np

import clearance_ref as C

SITE_NONE = 0xFFFFFFFF
REGION_NONE = -1
D2_NONE = C.D2_NONE
SHIFT = 28
BRUTE_MAX_PAIRS = 1 << 31   # cells x sites a test may ask of the brute force
BRUTE_PAIRS = 1 << 26       # ... up to which site_field() takes the brute force


def occupied(grid):
    return np.asarray(grid, np.int8) == 100


def components(grid):
    """(label image int64: the component's least linear index at occupied cells, -1 elsewhere; {label: cells})."""
    occ = occupied(grid)
    H, W = occ.shape
    lab = np.full((H, W), -1, np.int64)
    sizes = {}
    occl = occ.tolist()
    for y0, x0 in zip(*np.nonzero(occ)):   # raster order: the first cell met of a component is its least index
        if lab[y0, x0] >= 0:
            continue
        root = int(y0) * W + int(x0)
        stack, cells = [(int(y0), int(x0))], 0
        lab[y0, x0] = root
        while stack:
            y, x = stack.pop()
            cells += 1
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = y + dy, x + dx
                    if 0 <= ny < H and 0 <= nx < W and occl[ny][nx] and lab[ny, nx] < 0:
                        lab[ny, nx] = root
                        stack.append((ny, nx))
        sizes[root] = cells
    return lab, sizes


def sites_and_labels(grid, labels=None, min_component_cells=0):
    """(is_site bool, label int32 image valid at the site cells, counts)."""
    occ = occupied(grid)
    n = {"n_occupied": int(occ.sum())}
    if labels is not None:
        labels = np.asarray(labels, np.int32).reshape(occ.shape)
        is_site = occ & (labels >= 0)
        lab = np.where(is_site, labels, REGION_NONE).astype(np.int32)
        n.update(n_components=-1, n_regions=-1)
    else:
        comp, sizes = components(grid)
        kept = {r for r, k in sizes.items() if k >= min_component_cells}
        is_site = occ & np.isin(comp, sorted(kept)) if kept else np.zeros_like(occ)
        lab = np.where(is_site, comp, REGION_NONE).astype(np.int32)
        n.update(n_components=len(sizes), n_regions=len(kept))
    n["n_sites"] = int(is_site.sum())
    return is_site, lab, n


def _from_keys(key, any_site):
    if not any_site:
        return np.full(key.shape, SITE_NONE, np.uint32)
    return (key & ((1 << SHIFT) - 1)).astype(np.uint32)


def brute_site(is_site):
    H, W = is_site.shape
    out = np.full((H, W), SITE_NONE, np.uint32)
    cy, cx = np.nonzero(is_site)
    if len(cx) == 0 or W * H == 0:
        return out
    assert W * H * len(cx) <= BRUTE_MAX_PAIRS
    cx, cy = cx.astype(np.int64), cy.astype(np.int64)
    idx = cy * W + cx
    xs = np.arange(W, dtype=np.int64)
    rows = max(1, (1 << 24) // (W * len(cx)))
    for y0 in range(0, H, rows):
        ys = np.arange(y0, min(H, y0 + rows), dtype=np.int64)
        d = (xs[None, :, None] - cx[None, None, :]) ** 2 + (ys[:, None, None] - cy[None, None, :]) ** 2
        out[y0:y0 + len(ys)] = _from_keys(((d << SHIFT) + idx[None, None, :]).min(axis=2), True)
    return out


def nearest_row(is_site):
    """near[y, x] = the row of column x's site nearest to row y, the smaller row at equal distance (int64; -1: none)."""
    H, W = is_site.shape
    INF = 1 << 20
    ys = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(is_site, ys, -INF), axis=0)
    below = np.minimum.accumulate(np.where(is_site, ys, 2 * INF)[::-1], axis=0)[::-1]
    near = np.where(below - ys < ys - above, below, above)
    return np.where((above < 0) & (below >= INF), -1, near)


def separable_site(is_site):
    H, W = is_site.shape
    out = np.full((H, W), SITE_NONE, np.uint32)
    if W * H == 0 or not is_site.any():
        return out
    near = nearest_row(is_site)
    xs = np.arange(W, dtype=np.int64)
    ys = np.arange(H, dtype=np.int64)[:, None]
    BIG = np.int64(1) << 62
    colkey = np.where(near >= 0, ((ys - near) ** 2 << SHIFT) + near * W + xs[None, :], BIG)   # [y, x']
    dx2 = ((xs[:, None] - xs[None, :]) ** 2) << SHIFT                                          # [x, x']
    rows = max(1, (1 << 23) // (W * W))
    for y0 in range(0, H, rows):
        key = np.minimum(dx2[None, :, :] + colkey[y0:y0 + rows, None, :], BIG).min(axis=2)
        out[y0:y0 + rows] = _from_keys(key, True)
    return out


def site_field(is_site):
    """The brute force where it is affordable, else the separable statement."""
    return brute_site(is_site) if is_site.size * max(1, int(is_site.sum())) <= BRUTE_PAIRS else separable_site(is_site)


def d2_of_site(site):
    """d2[y, x] from site[y, x]: the squared centre distance, D2_NONE where there is no site."""
    H, W = site.shape
    out = np.full((H, W), D2_NONE, np.uint32)
    if W * H == 0:
        return out
    s = site.astype(np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    d = (xs - s % W) ** 2 + (ys - s // W) ** 2
    return np.where(site == SITE_NONE, D2_NONE, d).astype(np.uint32)


def region_of(site, lab):
    H, W = site.shape
    if W * H == 0:
        return np.zeros((H, W), np.int32)
    flat = lab.reshape(-1)
    s = np.where(site == SITE_NONE, 0, site).astype(np.int64)
    return np.where(site == SITE_NONE, REGION_NONE, flat[s]).astype(np.int32)


def ridge_of(region, is_site):
    """The pair rule: every pair (c, n) with n right of or below c whose regions are both not NONE and differ marks c
    if c is no site cell, otherwise n if n is no site cell, otherwise neither."""
    H, W = region.shape
    ridge = np.zeros((H, W), np.int8)
    for c, n in (((slice(None), slice(0, -1)), (slice(None), slice(1, None))),     # n = (x + 1, y)
                 ((slice(0, -1), slice(None)), (slice(1, None), slice(None)))):    # n = (x, y + 1)
        if region[c].size == 0:
            continue
        pair = (region[c] != REGION_NONE) & (region[n] != REGION_NONE) & (region[c] != region[n])
        marks_c = pair & ~is_site[c]
        marks_n = pair & is_site[c] & ~is_site[n]
        ridge[c][marks_c] = 100
        ridge[n][marks_n] = 100
    return ridge


def at_points(scene_or_shape, xy, origin, resolution, fields):
    """site, region, d2, ridge_d2 at points by the cell rule; fields: the four (H, W) images (ridge_d2 may be None)."""
    site, region, d2, rd2 = fields
    H, W = site.shape
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ok, mx, my = C.cells_of(xy[:, 0], xy[:, 1], origin, resolution, W, H)
    out = {"site": np.full(len(xy), SITE_NONE, np.uint32), "region": np.full(len(xy), REGION_NONE, np.int32),
           "d2": np.full(len(xy), D2_NONE, np.uint32), "ridge_d2": np.full(len(xy), D2_NONE, np.uint32)}
    if W * H:
        out["site"][ok] = site[my[ok], mx[ok]]
        out["region"][ok] = region[my[ok], mx[ok]]
        out["d2"][ok] = d2[my[ok], mx[ok]]
        if rd2 is not None:
            out["ridge_d2"][ok] = rd2[my[ok], mx[ok]]
    out["ridge_offset"] = C.metres(out["ridge_d2"], resolution)
    return out


def regions(scene, site=None):
    """Everything aos_gvd_regions returns for a scene (regions_scenes.scene), with the ridge distance."""
    grid = np.asarray(scene["grid"], np.int8)
    is_site, lab, n = sites_and_labels(grid, scene.get("labels"), scene.get("min_component_cells", 0))
    if site is None:
        site = site_field(is_site)
    d2 = d2_of_site(site)
    region = region_of(site, lab)
    ridge = ridge_of(region, is_site)
    ridge_d2 = C.field(ridge)
    r = dict(n)
    r.update(site=site, region=region, ridge=ridge, ridge_d2=ridge_d2, d2=d2, is_site=is_site,
             n_ridge=int((ridge == 100).sum()), max_d2=int(d2.max()) if n["n_sites"] else D2_NONE)
    nodes = at_points(None, scene["nodes"], scene["origin"], scene["resolution"], (site, region, d2, ridge_d2))
    r.update({"node_" + k: v for k, v in nodes.items()})
    return r
