"""Grid kernels (k_inflate, k_open, k_thin_block, the byte expansion) vs the oracle on rasters no orchard scene
produces: grid sizes at every word / tile remainder with set cells on the border rows and columns, R from 0 to 63,
a solid blob over 3 x 3 thinning tiles (the copy-through of a solid neighbourhood and its re-activation), and one
handle driven through frames whose T and geometry change (the captured first batch outgrown and re-captured).
The rasters are injected exactly through point clouds (tests/shapes.py)."""
import numpy as np
import pytest

import aos_gpu
import oracle_py as O
import shapes as S
from parity_util import assert_seedgen_parity, grid_diff

pytestmark = pytest.mark.gpu

STAGES = ("raster", "inflated", "opened", "skeleton_frameless")


def _oracle_stage(o, which):
    return {"raster": o["raster"], "inflated": o["inflated"], "opened": np.where(o["opened"] != 0, 100, 0),
            "skeleton_frameless": o["skeleton"]}[which]


def assert_grids(c, g, o, occ=None, skel=None):
    shape = (o["height"], o["width"])
    assert (g["height"], g["width"]) == shape
    for which in STAGES:
        got = c.debug_grid(which, shape)
        assert grid_diff(got, _oracle_stage(o, which)) == 0, which
    assert grid_diff(g["occupancy"] if occ is None else occ, o["occupancy"]) == 0, "occupancy"
    assert grid_diff(g["skeleton_framed"] if skel is None else skel, o["skeleton_framed"]) == 0, "skeleton_framed"
    assert g["thin_iters"] == o["thin_iters"], (g["thin_iters"], o["thin_iters"])


def assert_oracle_stages_chain(o, pattern, R):
    """The oracle frame equals its own stage functions chained by hand on the intended pattern."""
    raster = np.where(np.asarray(pattern) != 0, 100, 0).astype(np.int8)
    assert np.array_equal(o["raster"], raster)
    infl = O.inflate(raster, R)
    assert np.array_equal(infl, o["inflated"])
    opened = O.open_cross(infl == 100)
    assert np.array_equal(opened, o["opened"])
    sk, T = O.thin(opened)
    assert np.array_equal(np.where(sk != 0, 100, 0), o["skeleton"]) and T == o["thin_iters"]


def run_pattern(pattern, R, want_host=True, **params):
    cloud, poly, akw, okw = S.scene(pattern, R, **params)
    o = O.seedgen(cloud, poly, O.default_params(**okw))
    c = aos_gpu.Ctx(aos_gpu.default_params(**akw))
    c.set_polygon(poly)
    g = c.seedgen(cloud, want_host=want_host)
    return c, g, o


@pytest.mark.parametrize("W,H,R", S.GRID_CASES, ids=lambda v: str(v))
def test_geometry_sweep(W, H, R):
    pattern = S.border_pattern(W, H, S.grid_case_seed(W, H, R))
    c, g, o = run_pattern(pattern, R)
    assert_oracle_stages_chain(o, pattern, R)
    assert_grids(c, g, o)
    assert_seedgen_parity(g, o)
    c.close()


def test_geometry_frame_without_host_grids():
    """want_host = 0: the grids stay in HBM and come out through aos_seedgen_grids_copy."""
    W, H, R = 513, 131, 15
    pattern = S.border_pattern(W, H, 7)
    c, g, o = run_pattern(pattern, R, want_host=False)
    assert "occupancy" not in g
    occ, skel = c.grids_copy((H, W))
    assert_grids(c, g, o, occ, skel)
    assert_seedgen_parity(g, o, check_grids=False)
    c.close()


@pytest.mark.parametrize("fill", [0, 1])
def test_geometry_empty_and_full_pattern(fill):
    W, H, R = (127, 129, 3) if fill == 0 else (193, 131, 1)
    pattern = np.full((H, W), fill, np.uint8)
    c, g, o = run_pattern(pattern, R)
    assert_oracle_stages_chain(o, pattern, R)
    assert int(np.count_nonzero(o["opened"])) == fill * W * H
    assert_grids(c, g, o)
    assert_seedgen_parity(g, o)
    c.close()


@pytest.fixture(scope="module")
def blob_oracle():
    pattern = S.blob_pattern()
    cloud, poly, akw, okw = S.scene(pattern, S.BLOB["R"])
    return cloud, poly, akw, O.seedgen(cloud, poly, O.default_params(**okw))


@pytest.mark.parametrize("thin_graph", [1, 0])
def test_solid_blob_over_3x3_thinning_tiles(blob_oracle, thin_graph):
    """The centre tile of a solid 3 x 3 tile block goes quiet after the first launch, is copied through while the
    erosion front is more than a tile away and must wake up when it arrives: its skeleton cells are found last."""
    cloud, poly, akw, o = blob_oracle
    quiet = S.quiet_solid_tiles(o)
    assert quiet, "the blob no longer covers a solid 3 x 3 tile block"
    assert o["thin_iters"] > 64
    for r, c_ in quiet:   # the quiet tile holds part of the final skeleton: a tile left asleep would keep it solid
        tile = o["skeleton"][r * S.THIN_TH:(r + 1) * S.THIN_TH, c_ * S.THIN_TW:(c_ + 1) * S.THIN_TW]
        assert 0 < np.count_nonzero(tile) < tile.size // 8
    c = aos_gpu.Ctx(aos_gpu.default_params(**akw, thin_graph=thin_graph))
    c.set_polygon(poly)
    g = c.seedgen(cloud)
    assert (g["thin_graph"] != 0) == bool(thin_graph)
    assert_grids(c, g, o)
    assert_seedgen_parity(g, o)
    c.close()


def test_one_handle_through_changing_frames():
    """thin_graph = 1 on one handle: a small T, a T that outgrows the captured first batch, another grid size
    (re-capture), the first size again with the batch sized from the last T, an empty frame, a blob on the small
    grid; every frame against the oracle."""
    frames = S.handle_frames()
    _, _, akw, okw = S.scene(frames[0][2], S.HANDLE_R, thin_graph=1)
    c = aos_gpu.Ctx(aos_gpu.default_params(**akw))
    seen, graph, last_dims = [], {}, None
    for name, (W, H), pattern in frames:
        cloud, poly, _, _ = S.scene(pattern, S.HANDLE_R)
        if (W, H) != last_dims:
            c.set_polygon(poly)
        g = c.seedgen(cloud)
        o = O.seedgen(cloud, poly, O.default_params(**okw))
        assert np.array_equal(o["raster"] != 0, pattern != 0), name
        assert_grids(c, g, o)
        assert_seedgen_parity(g, o)
        seen.append((name, g["thin_iters"], g["thin_launches"]))
        graph[name] = g["thin_graph"]   # 2: the first batch's graph was captured in this frame, 1: replayed
        last_dims = (W, H)
    c.close()
    T = {n: t for n, t, _ in seen}
    launches = {n: k for n, _, k in seen}
    K = S.THIN_KIT
    assert T["A sparse"] <= 2 * K and launches["A sparse"] == 2, seen     # the first batch: two launches
    assert T["A blob"] > 2 * K and launches["A blob"] > 2, seen           # ... outgrown
    assert T["A blob again"] == T["A blob"] and T["B blob"] > 2 * K, seen
    # One graph is kept per batch size (thin_first_batch): grid A's two-launch graph is captured in the first frame,
    # replayed by "A blob", survives grid B's frame (whose batch, sized from T ~ 49, is another graph) and is replayed
    # again; "A empty" (a batch sized from T ~ 49 on grid A) and "B blob" (two launches on grid B) capture anew.
    assert graph == {"A sparse": 2, "A blob": 1, "B sparse": 2, "A blob again": 1, "A empty": 2, "B blob": 2}, graph
