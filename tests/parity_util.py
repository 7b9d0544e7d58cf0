"""Shared comparison helpers for GPU-vs-oracle parity (test infrastructure)."""
import numpy as np

SEED_TOL = 1e-6  # north_star: seeds within 1e-6; grids/skeleton/topology bit-exact


def grid_diff(a, b):
    return int(np.count_nonzero(np.asarray(a) != np.asarray(b)))


def assert_seedgen_parity(g: dict, o: dict, check_grids=True):
    assert (g["width"], g["height"]) == (o["width"], o["height"])
    assert g["origin"] == o["origin"] and np.float32(g["resolution"]) == np.float32(o["resolution"])
    if check_grids:
        assert grid_diff(g["occupancy"], o["occupancy"]) == 0, "occupancy grid differs"
        assert grid_diff(g["skeleton_framed"], o["skeleton_framed"]) == 0, "skeleton grid differs"
    assert g["thin_iters"] == o["thin_iters"], (g["thin_iters"], o["thin_iters"])
    assert g["n_clusters_all"] == len(o["cluster_length"])
    assert g["row_center"].shape == o["row_center"].shape, (g["row_center"].shape, o["row_center"].shape)
    for k in ("row_center", "row_start", "row_end", "row_length"):
        assert np.array_equal(g[k], o[k]), k
    for k in ("virtual_seeds", "ray_seeds", "endpoint_seeds", "voronoi_seeds", "rows_info", "cluster_info"):
        assert g[k].shape == o[k].shape, (k, g[k].shape, o[k].shape)
        if g[k].size:
            assert np.max(np.abs(g[k] - o[k])) <= SEED_TOL, k
    # the implementation is bit-exact by construction; report it as well
    return all(np.array_equal(g[k], o[k]) for k in ("voronoi_seeds", "rows_info", "cluster_info"))


def assert_seeds_exact(g: dict, o: dict):
    """DESIGN §2's claim for the row, ray and seed stage: the rows, the three seed lists and their concatenation, the
    sorted outputs and the three counts equal the oracle's bit for bit."""
    for k in ("row_center", "row_start", "row_end", "row_length", "virtual_seeds", "ray_seeds", "endpoint_seeds",
              "voronoi_seeds", "rows_info", "cluster_info"):
        assert g[k].shape == o[k].shape, (k, g[k].shape, o[k].shape)
        assert g[k].dtype == o[k].dtype == np.float64, (k, g[k].dtype, o[k].dtype)
        if not np.array_equal(g[k], o[k]):
            bad = np.nonzero((g[k] != o[k]).reshape(len(g[k]), -1).any(axis=1))[0]
            hexes = lambda a: [float(v).hex() for v in np.atleast_1d(a)]   # noqa: E731
            raise AssertionError(f"{k}: {len(bad)} of {len(g[k])} entries differ, first at {bad[0]}: "
                                 f"{hexes(g[k][bad[0]])} vs the oracle's {hexes(o[k][bad[0]])}")
    assert (g["n_virtual"], g["n_ray"], g["n_endpoint"]) == \
        (len(o["virtual_seeds"]), len(o["ray_seeds"]), len(o["endpoint_seeds"]))
    assert len(g["voronoi_seeds"]) == len(o["virtual_seeds"]) + len(o["ray_seeds"]) + len(o["endpoint_seeds"])


def assert_gvd_parity(g: dict, o: dict):
    assert g["published"] == o["published"]
    if not o["published"]:
        return
    assert g["n_merged"] == len(o["merged"]), (g["n_merged"], len(o["merged"]))
    assert g["n_vor_edges"] == len(o["vor_edges"]), (g["n_vor_edges"], len(o["vor_edges"]))
    assert g["n_boundary_raw"] == len(o["boundary_raw"]), (g["n_boundary_raw"], len(o["boundary_raw"]))
    assert g["nodes"].shape == o["nodes"].shape, (g["nodes"].shape, o["nodes"].shape)
    assert np.array_equal(g["nodes"], o["nodes"]), "node coordinates / order differ"
    assert g["edges"].shape == o["edges"].shape, (g["edges"].shape, o["edges"].shape)
    assert np.array_equal(g["edges"], o["edges"]), "edge topology differs"
    assert np.array_equal(g["edge_lengths"], o["edge_lengths"])
    assert np.array_equal(g["edge_clearances"], o["edge_clearances"])
    for k in ("node_labels", "node_cluster_indices", "node_label_counts", "node_label_clusters", "node_label_types"):
        assert np.array_equal(g[k], o[k]), k


def assert_gvd_full_parity(ctx, g: dict, o: dict):
    """assert_gvd_parity plus what it leaves out: the merged seeds, the rows' label points and the markers' cells
    of ctx's last GVD call (g its graph), bit for bit against the oracle result o (run with markers = 1)."""
    assert_gvd_parity(g, o)
    if not o["published"]:
        return
    assert g["n_merged"] == len(o["merged"]), (g["n_merged"], len(o["merged"]))
    m = ctx.gvd_markers()
    assert m["seeds"].shape == o["merged"].shape, (m["seeds"].shape, o["merged"].shape)
    assert np.array_equal(m["seeds"], o["merged"], equal_nan=True), "merged seeds differ"
    assert m["row_label_valid"].shape == o["row_label_valid"].shape, \
        (m["row_label_valid"].shape, o["row_label_valid"].shape)
    assert np.array_equal(m["row_label_valid"], o["row_label_valid"]), "row label validity differs"
    v = o["row_label_valid"].astype(bool)
    assert np.array_equal(m["row_label_pts"][v], o["row_label_pts"][v], equal_nan=True), "row label points differ"
    for k in ("cell_offsets", "cell_xy", "cell_center", "cell_rgba"):
        assert m[k].shape == o[k].shape, (k, m[k].shape, o[k].shape)
        assert np.array_equal(m[k], o[k], equal_nan=True), f"markers' {k} differ"


def binned_box(poly, ror_radius=0.2, minz=-0.4, maxz=0.5):
    """ror_stage.hip ror_binned_box / ror_stage: frame_geom's float bounds (polygon +- 2.5 m, double -> float)
    minus / plus ror_margin, in float32 as on the host."""
    f = np.float32
    m = f(f(ror_radius * 1.01) + f(1e-4))
    minx, maxx = f(poly[:, 0].min() - 2.5), f(poly[:, 0].max() + 2.5)
    miny, maxy = f(poly[:, 1].min() - 2.5), f(poly[:, 1].max() + 2.5)
    return [f(minx - m), f(maxx + m), f(miny - m), f(maxy + m), f(f(minz) - m), f(f(maxz) + m)]


def inside(cloud, box):
    import orchard
    p = orchard.xyz(cloud).astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero((x >= box[0]) & (x <= box[1]) & (y >= box[2]) & (y <= box[3]) &
                                    (z >= box[4]) & (z <= box[5])))


def sha_of(a, dt):
    """SHA-256 of an array as tools/make_golden.py hashes it (dtype, shape, bytes)."""
    import hashlib
    a = np.ascontiguousarray(np.asarray(a, dtype=dt))
    return hashlib.sha256(a.dtype.str.encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def assert_golden_hashes(g: dict, gg: dict, hs: dict, check_grids=True):
    """A GPU frame (seed-gen dict g, GVD dict gg) vs the oracle's SHA-256 fixture hs (make_golden.py)."""
    assert g["thin_iters"] == hs["meta"]["thin_iters"], (g["thin_iters"], hs["meta"]["thin_iters"])
    assert g["n_clipped"] == hs["meta"]["n_clipped"], (g["n_clipped"], hs["meta"]["n_clipped"])
    if check_grids:
        for k in ("occupancy", "skeleton_framed"):
            assert sha_of(g[k], np.int8) == hs["seedgen"][k], k
    for k in ("row_center", "row_start", "row_end", "row_length", "virtual_seeds", "ray_seeds", "endpoint_seeds",
              "voronoi_seeds", "rows_info", "cluster_info"):
        assert sha_of(g[k], np.float64) == hs["seedgen"][k], k
    for k, dt in (("nodes", np.float64), ("edges", np.int32), ("edge_lengths", np.float32),
                  ("edge_clearances", np.float32), ("node_labels", np.int32), ("node_cluster_indices", np.int32),
                  ("node_label_counts", np.int32), ("node_label_clusters", np.int32), ("node_label_types", np.int32)):
        assert sha_of(gg[k], dt) == hs["gvd"][k], k
