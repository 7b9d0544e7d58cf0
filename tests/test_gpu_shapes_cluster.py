"""Foreground, labelling, cluster-statistics and replay kernels vs the oracle on skeletons no orchard scene produces
(tests/shapes.py): a closed ring, a spiral, a many-armed star, thousands of one-cell clusters, combs whose
cross-chunk links overflow k_ccl_local's LDS list and k_ccl_cross' global list, and a polygon with hundreds of edges
per grid row. Every scene first asserts its regime on the oracle result (shapes.check_regime), so a scene that
drifts out of the branch it is meant for fails instead of passing vacuously."""
import numpy as np
import pytest

import aos_gpu
import aos_tiles as T
import oracle_py as O
import shapes as S
from parity_util import assert_gvd_parity, assert_seedgen_parity

pytestmark = pytest.mark.gpu

GVD_MAX_SEEDS = 3000   # the oracle's GVD is quadratic in the seeds: the large scenes stop at the seed-gen frame

_oracle = {}


def oracle_frame(name):
    """The scene, its oracle frame and regime figures, computed once and shared (never modified)."""
    if name not in _oracle:
        pattern, cloud, poly, akw, okw = S.cluster_scene(name)
        o = O.seedgen(cloud, poly, O.default_params(**okw))
        assert np.array_equal(o["raster"] != 0, pattern != 0)
        fig = S.check_regime(name, o, poly)
        og = None
        if len(o["voronoi_seeds"]) < GVD_MAX_SEEDS:
            og = O.gvd(o["voronoi_seeds"], o["rows_info"], o, O.default_params(**okw))
        _oracle[name] = (cloud, poly, akw, okw, o, og, fig)
    return _oracle[name]


def run_single(name):
    cloud, poly, akw, okw, o, og, fig = oracle_frame(name)
    c = aos_gpu.Ctx(aos_gpu.default_params(**akw))
    c.set_polygon(poly)
    g = c.seedgen(cloud)
    assert_seedgen_parity(g, o)
    assert g["n_clipped"] == o["n_clipped"]
    if og is not None:
        assert_gvd_parity(c.gvd_from_seedgen(), og)
    return c, g, o


@pytest.mark.parametrize("name", ["dots", "comb-wide", "comb-mixed", "sawtooth", "ring-length", "star-length"])
def test_scene_vs_oracle(name):
    c, g, o = run_single(name)
    c.close()


@pytest.mark.parametrize("where", ["host", "gpu"])
@pytest.mark.parametrize("name,replay_all", [("ring", False), ("ring", True), ("spiral", False), ("star", False),
                                             ("star", True)])
def test_replayed_scene_vs_oracle(name, replay_all, where):
    """The exact BFS replay on a loop, a spiral and a many-armed junction, on host threads and through the GPU walk
    (which hands a cluster whose box bitmap or queue it cannot hold to the host)."""
    try:
        aos_gpu.debug_replay(0 if where == "gpu" else 1 << 30, 0, replay_all=replay_all)
        c, g, o = run_single(name)
        rc = c.replay_counts()
        c.close()
    finally:
        aos_gpu.debug_replay()
    assert rc["all"] == g["n_bfs_replayed"], rc
    assert rc["gpu"] + rc["host_bits"] + rc["host_cells"] == rc["all"], rc
    if where == "host":
        assert rc["gpu"] == 0, rc
    if replay_all:
        assert rc["all"] == g["n_clusters_all"], rc
    if name == "spiral":   # sum x > 2^24: no certificate
        assert rc["all"] >= 1, rc
    if name == "ring" and replay_all and where == "gpu":   # a box beyond the GPU walk's bitmap goes to the host
        assert rc["gpu"] == 0 and rc["all"] == 1, rc


@pytest.mark.parametrize("tiles", [(2, 2), (3, 1)], ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("name", ["spiral", "ring", "sawtooth"])
def test_scene_tiled_vs_oracle(name, tiles):
    """The same frames through aos_group_* (ranks as the library's threads on one GPU): clusters that cross the tile
    borders many times and close loops over them (cluster_dist.hip's border union-find); the root's frame vs the
    oracle."""
    cloud, poly, akw, okw, o, og, fig = oracle_frame(name)
    world = tiles[0] * tiles[1]
    root = world - 1
    grp = aos_gpu.Group(aos_gpu.default_params(**akw), [0] * world, *tiles)
    try:
        grp.set_polygon(poly)
        parts = [T.shard(cloud, grp.plan(r)["points_box"]) for r in range(world)]
        g = grp.process(parts, root=root)
        assert_seedgen_parity(g, o)
        assert g["n_clipped"] == o["n_clipped"]
        if og is not None:
            assert_gvd_parity(grp.rank(root).gvd_from_seedgen(), og)
    finally:
        grp.close()
