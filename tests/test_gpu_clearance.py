"""aos_gvd_clearance on the GPU vs its numpy restatement (clearance_ref). Bar: the field, n_occupied, max_d2, node and
edge d2 and the float32 metres, bit for bit, on every designed scene (clearance_scenes); the NULL forms on the handle's
own graph and skeleton against the explicit forms; buffers that grow and are reused; the ABI's refusals."""
import ctypes

import numpy as np
import pytest

import aos_gpu
import clearance_ref as R
import clearance_scenes as S
import orchard
from test_clearance_cpu import assert_clearance_equal, invalid_scenes, scenes_and_refs

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4


def info_of(sc):
    H, W = sc["grid"].shape
    return {"origin": sc["origin"], "resolution": sc["resolution"], "width": W, "height": H}


def run_scene(c, sc):
    got = c.gvd_clearance(graph=sc, grid=sc["grid"], info=info_of(sc))
    got["field"] = c.clearance_field()
    return got


def check_scene(c, sc, ref, what):
    got = run_scene(c, sc)
    assert got["field"].shape == sc["grid"].shape, what
    assert_clearance_equal(got, ref, what)
    assert (got["d2_device"] is None) == (sc["grid"].size == 0), what
    d2, m = c.clearance_points(sc["nodes"])
    assert d2.tobytes() == ref["node_d2"].tobytes() and m.tobytes() == ref["node_clearances"].tobytes(), f"{what}: points"


@pytest.fixture(scope="module")
def ctx():
    c = aos_gpu.Ctx(aos_gpu.default_params())
    yield c
    c.close()


def test_every_scene(ctx):
    scenes, refs = scenes_and_refs()
    for name, sc in scenes.items():
        check_scene(ctx, sc, refs[name], name)


def test_c0_own_graph_and_forms():
    """aos_gvd_process on the C0 golden inputs, then the call with no arguments against the explicit graph + host
    skeleton form, the device-pointer form and the restatement; the GvdGraph's own edge_clearances stay zero."""
    import torch

    scenes, refs = scenes_and_refs()
    c0 = scenes["c0"]
    s = np.load(S.GOLDEN + "/c0_seedgen.npz")
    info = info_of(c0)
    c = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=c0["resolution"]))
    seeds = np.ascontiguousarray(s["voronoi_seeds"], np.float64).reshape(-1)
    rows = np.ascontiguousarray(s["rows_info"], np.float64).reshape(-1)
    sk = np.ascontiguousarray(c0["grid"]).reshape(-1)
    gi = aos_gpu.GridInfo(info["origin"][0], info["origin"][1], info["resolution"], info["width"], info["height"])
    gin = aos_gpu.GvdIn(seeds.ctypes.data_as(aos_gpu.P(aos_gpu.c_d)), seeds.size // 2,
                        rows.ctypes.data_as(aos_gpu.P(aos_gpu.c_d)), rows.size // 2, gi,
                        sk.ctypes.data_as(aos_gpu.P(ctypes.c_int8)))
    o = aos_gpu.GvdOut()
    aos_gpu._check(aos_gpu.lib().aos_gvd_process(c.h, ctypes.byref(gin), ctypes.byref(o)))
    gg = aos_gpu._gvd_dict(o)
    assert len(gg["edges"]) > 500 and not gg["edge_clearances"].any()
    ref = R.clearance(S.scene(c0["grid"], gg["nodes"], gg["edges"], c0["origin"], c0["resolution"]), refs["c0"]["field"])
    own = c.gvd_clearance()
    own["field"] = c.clearance_field()
    assert_clearance_equal(own, ref, "own graph, own skeleton")
    assert (own["width"], own["height"], own["resolution"], own["origin"]) == (512, 512, c0["resolution"], c0["origin"])
    explicit = c.gvd_clearance(graph=gg, grid=c0["grid"], info=info)
    explicit["field"] = c.clearance_field()
    assert_clearance_equal(explicit, ref, "explicit graph, host skeleton")
    d = torch.from_numpy(sk).cuda()
    torch.cuda.synchronize()
    dev = c.gvd_clearance(graph=gg, grid=d.data_ptr(), info=info, on_device=True)
    dev["field"] = c.clearance_field()
    assert_clearance_equal(dev, ref, "explicit graph, device skeleton")
    mixed = c.gvd_clearance(graph=gg)   # explicit graph, the handle's skeleton
    assert_clearance_equal(mixed, ref, "explicit graph, own skeleton", with_field=False)
    after = aos_gpu._gvd_dict(o)   # the same library-owned arrays, read again
    assert len(after["edge_clearances"]) == len(gg["edges"]) and not after["edge_clearances"].any()
    assert np.array_equal(after["nodes"], gg["nodes"]) and np.array_equal(after["edges"], gg["edges"])
    # /plan-like poses against the last field
    pts = np.array([c0["origin"], gg["nodes"][0], (1e9, 0.0), (np.nan, 0.0)], np.float64)
    d2, m = c.clearance_points(pts)
    assert d2.tolist() == R.at_points(ref["field"], pts, c0["origin"], c0["resolution"]).tolist()
    assert m.tobytes() == R.metres(d2, c0["resolution"]).tobytes() and d2[2] == d2[3] == R.D2_NONE
    del d
    c.close()


def test_buffers_grow_and_are_reused():
    """One handle through small, 700 x 500 and small scenes again; the last call's outputs stay right."""
    scenes, refs = scenes_and_refs()
    c = aos_gpu.Ctx(aos_gpu.default_params())
    for name in ("ties", "mid_700x500_0.05", "edges_257", "mid_700x500_0.001", "one_free", "no_cells_5x0", "on_cell_edges"):
        check_scene(c, scenes[name], refs[name], f"reuse {name}")
    c.close()


def test_state_errors():
    cfg = orchard.CONFIGS["C0"]
    cloud, poly = orchard.generate(cfg), orchard.polygon(cfg)
    c = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res))
    L = aos_gpu.lib()
    out = aos_gpu.ClearanceOut()
    buf = np.zeros(16, np.uint32)
    xy = np.zeros(2)
    assert L.aos_clearance_field_copy(c.h, buf.ctypes.data, 16) == E_STATE
    assert L.aos_clearance_points(c.h, xy.ctypes.data, 1, buf.ctypes.data, None) == E_STATE
    assert L.aos_gvd_clearance(c.h, None, None, 0, None, ctypes.byref(out)) == E_STATE   # no GVD call yet
    assert "no GVD graph" in L.aos_last_error().decode()
    sc = S.graph_scenes()["one_edge"]
    with pytest.raises(RuntimeError, match="no grid given and no GVD call"):
        c.gvd_clearance(graph=sc)
    assert L.aos_clearance_field_copy(c.h, buf.ctypes.data, 16) == E_STATE   # still no field
    c.set_polygon(poly)
    f = c.seedgen(cloud)
    gg = c.gvd_from_seedgen()
    own = c.gvd_clearance()
    own["field"] = c.clearance_field()
    info = {"origin": f["origin"], "resolution": f["resolution"], "width": f["width"], "height": f["height"]}
    explicit = c.gvd_clearance(graph=gg, grid=f["d_skeleton"], info=info, on_device=True)   # the frame's device skeleton
    explicit["field"] = c.clearance_field()
    ref = R.clearance(S.scene(f["skeleton_framed"], gg["nodes"], gg["edges"], f["origin"], f["resolution"]))
    assert_clearance_equal(own, ref, "own after gvd_from_seedgen")
    assert_clearance_equal(explicit, ref, "device skeleton of the frame")
    c.seedgen(cloud)
    with pytest.raises(RuntimeError, match="replaced by a later seed-gen frame"):
        c.gvd_clearance()
    assert L.aos_gvd_clearance(c.h, None, None, 0, None, ctypes.byref(out)) == E_STATE
    # a call refused before it touched anything leaves the last field in place
    assert c.clearance_field().tobytes() == ref["field"].tobytes()
    got = c.gvd_clearance(grid=f["skeleton_framed"], info=info)   # the handle's graph, the grid passed
    assert_clearance_equal(got, ref, "own graph, grid passed", with_field=False)
    c.close()


def test_refusals(ctx):
    L = aos_gpu.lib()
    scenes, refs = scenes_and_refs()
    ok = scenes["one_edge"]

    def call(sc, out="new", grid="host", info="own", counts=None, null_nodes=False, null_edges=False):
        o = aos_gpu.ClearanceOut() if out == "new" else out
        g = aos_gpu.PathGraph()
        g.num_nodes, g.num_edges = (len(sc["nodes"]), len(sc["edges"])) if counts is None else counts
        g.nodes_xy = None if null_nodes else sc["nodes"].ctypes.data_as(aos_gpu.P(aos_gpu.c_d))
        g.edges = None if null_edges else sc["edges"].ctypes.data_as(aos_gpu.P(aos_gpu.c_i))
        i = info_of(sc) if info == "own" else info
        gi = None if i is None else aos_gpu.GridInfo(i["origin"][0], i["origin"][1], i["resolution"], i["width"], i["height"])
        gp = sc["grid"].ctypes.data_as(ctypes.c_void_p) if grid == "host" else grid
        return L.aos_gvd_clearance(ctx.h, ctypes.byref(g), gp, 0,
                                   ctypes.byref(gi) if gi is not None else None,
                                   ctypes.byref(o) if o is not None else None)

    assert call(ok) == 0
    assert call(ok, out=None) == E_INVALID
    assert call(ok, counts=(-1, 1)) == E_INVALID and call(ok, counts=(2, -1)) == E_INVALID
    assert call(ok, null_nodes=True) == E_INVALID and call(ok, null_edges=True) == E_INVALID
    assert call(ok, info=None) == E_INVALID and "without grid info" in L.aos_last_error().decode()
    for w, h in ((16385, 1), (1, 16385), (1 << 20, 1 << 20)):
        assert call(ok, info={**info_of(ok), "width": w, "height": h}) == E_INVALID
        assert "16384" in L.aos_last_error().decode()
    for sc in invalid_scenes():
        assert call(sc) == E_INVALID, (sc["resolution"], sc["nodes"], sc["edges"])
    # the field and points calls
    assert call(ok) == 0
    buf = np.zeros(40 * 30, np.uint32)
    assert L.aos_clearance_field_copy(ctx.h, buf.ctypes.data, 40 * 30 - 1) == E_INVALID
    assert L.aos_clearance_field_copy(ctx.h, None, 40 * 30) == E_INVALID
    assert L.aos_clearance_field_copy(ctx.h, buf.ctypes.data, 40 * 30) == 0
    assert buf.reshape(30, 40).tobytes() == refs["one_edge"]["field"].tobytes()
    xy = np.ascontiguousarray(ok["nodes"])
    assert L.aos_clearance_points(ctx.h, xy.ctypes.data, -1, buf.ctypes.data, None) == E_INVALID
    assert L.aos_clearance_points(ctx.h, None, 2, buf.ctypes.data, None) == E_INVALID
    assert L.aos_clearance_points(ctx.h, None, 0, None, None) == 0
    m = np.zeros(2, np.float32)
    assert L.aos_clearance_points(ctx.h, xy.ctypes.data, 2, None, m.ctypes.data) == 0
    assert m.tobytes() == refs["one_edge"]["node_clearances"].tobytes()
    # the handle serves the next scene as before
    check_scene(ctx, scenes["zero_and_self"], refs["zero_and_self"], "after refusals")
