"""aos_gvd_regions on the GPU vs its numpy restatement (regions_ref). Bar: the four fields, the counts, the node arrays,
the float32 metres and the points, bit for bit, on every designed scene (regions_scenes); the NULL forms on the handle's
own graph and skeleton against the explicit forms; d2 from site against aos_gvd_clearance's field on the same handle,
which stays readable; buffers that grow and are reused; the ABI's refusals."""
import ctypes

import numpy as np
import pytest

import aos_gpu
import clearance_ref as C
import clearance_scenes as CS
import regions_ref as R
import regions_scenes as S
from test_regions_cpu import FIELDS, NODE_KEYS, assert_regions_equal, invalid_scenes, scenes_and_refs

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4


def info_of(sc):
    H, W = sc["grid"].shape
    return {"origin": sc["origin"], "resolution": sc["resolution"], "width": W, "height": H}


def run_scene(c, sc, want_ridge_distance=True, **kw):
    got = c.gvd_regions(graph=sc, grid=sc["grid"], info=info_of(sc), labels=sc.get("labels"),
                        min_component_cells=sc.get("min_component_cells", 0), want_ridge_distance=want_ridge_distance, **kw)
    for f in FIELDS[:3] + (("ridge_d2",) if want_ridge_distance else ()):
        got[f] = c.regions_field(f)
    return got


def check_scene(c, sc, ref, what):
    got = run_scene(c, sc)
    assert got["site"].shape == sc["grid"].shape, what
    assert_regions_equal(got, ref, what)
    for k in ("site_device", "region_device", "ridge_device", "ridge_d2_device"):
        assert (got[k] is None) == (sc["grid"].size == 0), (what, k)
    p = c.regions_points(sc["nodes"])
    for k in ("site", "region", "d2", "ridge_d2", "ridge_offset"):
        assert p[k].dtype == ref["node_" + k].dtype and p[k].tobytes() == ref["node_" + k].tobytes(), f"{what}: points {k}"


@pytest.fixture(scope="module")
def ctx():
    c = aos_gpu.Ctx(aos_gpu.default_params())
    yield c
    c.close()


def test_every_scene(ctx):
    scenes, refs = scenes_and_refs()
    for name, sc in scenes.items():
        check_scene(ctx, sc, refs[name], name)


def test_without_ridge_distance(ctx):
    """want_ridge_distance = 0: the same site, region and ridge; no ridge_d2 anywhere."""
    scenes, refs = scenes_and_refs()
    for name in ("walls_vertical", "labels_mixed", "sweep_257x129"):
        sc, ref = scenes[name], dict(refs[name])
        got = run_scene(ctx, sc, want_ridge_distance=False)
        ref["node_ridge_d2"] = np.full(len(sc["nodes"]), R.D2_NONE, np.uint32)
        ref["node_ridge_offset"] = np.full(len(sc["nodes"]), np.inf, np.float32)
        assert_regions_equal(got, ref, name, fields=FIELDS[:3])
        assert got["ridge_d2_device"] is None and got["site_device"] is not None
        buf = np.zeros(sc["grid"].size, np.uint32)
        assert aos_gpu.lib().aos_regions_field_copy(ctx.h, b"ridge_d2", buf.ctypes.data, buf.size) == E_INVALID
        assert "did not compute ridge_d2" in aos_gpu.lib().aos_last_error().decode()
        p = ctx.regions_points(sc["nodes"])
        assert (p["ridge_d2"] == R.D2_NONE).all() and np.isinf(p["ridge_offset"]).all()
        assert p["site"].tobytes() == ref["node_site"].tobytes() and p["d2"].tobytes() == ref["node_d2"].tobytes()
    # opts = NULL is {0, 0}
    sc, ref = scenes["filter_min_3"], refs["filter_min_3"]
    o, gi = aos_gpu.RegionsOut(), aos_gpu.GridInfo(*sc["origin"], sc["resolution"], 18, 12)
    g = aos_gpu.PathGraph()
    assert aos_gpu.lib().aos_gvd_regions(ctx.h, ctypes.byref(g), sc["grid"].ctypes.data, 0, ctypes.byref(gi), None, None,
                                         ctypes.byref(o)) == 0
    assert (o.n_sites, o.n_regions, o.n_ridge, o.ridge_d2_device) == (13, 2, ref["n_ridge"], None)
    site = np.zeros((12, 18), np.uint32)
    assert aos_gpu.lib().aos_regions_field_copy(ctx.h, b"site", site.ctypes.data, site.size) == 0
    assert site.tobytes() == ref["site"].tobytes()


def test_c0_own_graph_forms_and_clearance():
    """aos_gvd_process on the C0 golden inputs, then the call with no arguments against the explicit host-pointer and
    device-pointer forms and the restatement; d2 from site against aos_gvd_clearance's field on the same handle, which
    stays readable after aos_gvd_regions."""
    import torch

    scenes, refs = scenes_and_refs()
    c0 = scenes["c0"]
    s = np.load(CS.GOLDEN + "/c0_seedgen.npz")
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
    assert len(gg["nodes"]) > 500
    ref = R.regions(CS.scene(c0["grid"], gg["nodes"], gg["edges"], c0["origin"], c0["resolution"]), refs["c0"]["site"])
    clear = c.gvd_clearance()
    field = c.clearance_field()

    def fields(got):
        for f in FIELDS:
            got[f] = c.regions_field(f)
        return got

    own = fields(c.gvd_regions(want_ridge_distance=True))
    assert_regions_equal(own, ref, "own graph, own skeleton")
    assert (own["width"], own["height"], own["resolution"], own["origin"]) == (512, 512, c0["resolution"], c0["origin"])
    assert R.d2_of_site(own["site"]).tobytes() == field.tobytes() == C.field(c0["grid"]).tobytes()
    assert own["node_d2"].tobytes() == clear["node_d2"].tobytes() and own["max_d2"] == clear["max_d2"]
    # the clearance field of before the call is still the handle's
    assert c.clearance_field().tobytes() == field.tobytes()
    d2, m = c.clearance_points(gg["nodes"])
    assert d2.tobytes() == clear["node_d2"].tobytes() and m.tobytes() == clear["node_clearances"].tobytes()
    explicit = fields(c.gvd_regions(graph=gg, grid=c0["grid"], info=info, want_ridge_distance=True))
    assert_regions_equal(explicit, ref, "explicit graph, host skeleton")
    d = torch.from_numpy(sk).cuda()
    torch.cuda.synchronize()
    dev = fields(c.gvd_regions(graph=gg, grid=d.data_ptr(), info=info, on_device=True, want_ridge_distance=True))
    assert_regions_equal(dev, ref, "explicit graph, device skeleton")
    mixed = c.gvd_regions(graph=gg, want_ridge_distance=True)   # explicit graph, the handle's skeleton
    assert_regions_equal(mixed, ref, "explicit graph, own skeleton", fields=())
    # caller labels in device memory beside the device grid: two labels by the halves of the map
    lab = np.where(np.arange(512)[None, :] < 256, 11, 22).astype(np.int32) * np.ones((512, 1), np.int32)
    dl = torch.from_numpy(lab.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    lref = R.regions(S.with_opts(CS.scene(c0["grid"], gg["nodes"], gg["edges"], c0["origin"], c0["resolution"]), labels=lab))
    ldev = fields(c.gvd_regions(graph=gg, grid=d.data_ptr(), info=info, on_device=True, labels=dl.data_ptr(),
                                want_ridge_distance=True))
    assert_regions_equal(ldev, lref, "device skeleton, device labels")
    assert c.clearance_field().tobytes() == field.tobytes()
    # /plan-like poses against the last fields
    pts = np.array([c0["origin"], gg["nodes"][0], (1e9, 0.0), (np.nan, 0.0), (np.inf, -np.inf)], np.float64)
    p = c.regions_points(pts)
    want = R.at_points(None, pts, c0["origin"], c0["resolution"], (lref["site"], lref["region"], lref["d2"], lref["ridge_d2"]))
    for k, v in want.items():
        assert p[k].tobytes() == v.tobytes(), k
    assert (p["site"][2:] == R.SITE_NONE).all() and (p["region"][2:] == R.REGION_NONE).all() and np.isinf(p["ridge_offset"][2:]).all()
    del d, dl
    c.close()


def test_buffers_grow_and_are_reused():
    """One handle through large, small and large scenes; every call's outputs stay right."""
    scenes, refs = scenes_and_refs()
    c = aos_gpu.Ctx(aos_gpu.default_params())
    for name in ("mid_700x500_0.05", "tie_square", "lines_over_chunks", "one_free", "no_cells_5x0", "labels_random_130x67",
                 "mid_700x500_0.001", "graph_257_nodes", "mid_700x500_0.05"):
        check_scene(c, scenes[name], refs[name], f"reuse {name}")
    c.close()


def test_state_errors():
    import orchard

    cfg = orchard.CONFIGS["C0"]
    cloud, poly = orchard.generate(cfg), orchard.polygon(cfg)
    c = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res))
    L = aos_gpu.lib()
    out = aos_gpu.RegionsOut()
    buf = np.zeros(16, np.uint32)
    xy = np.zeros(2)
    assert L.aos_regions_field_copy(c.h, b"site", buf.ctypes.data, 16) == E_STATE
    assert L.aos_regions_points(c.h, xy.ctypes.data, 1, buf.ctypes.data, None, None, None, None) == E_STATE
    assert L.aos_gvd_regions(c.h, None, None, 0, None, None, None, ctypes.byref(out)) == E_STATE   # no GVD call yet
    assert "no GVD graph" in L.aos_last_error().decode()
    sc = S.graph_scenes()["graph_nodes"]
    with pytest.raises(RuntimeError, match="no grid given and no GVD call"):
        c.gvd_regions(graph=sc)
    assert L.aos_regions_field_copy(c.h, b"site", buf.ctypes.data, 16) == E_STATE   # still no field
    c.set_polygon(poly)
    f = c.seedgen(cloud)
    gg = c.gvd_from_seedgen()
    own = c.gvd_regions(want_ridge_distance=True)
    for k in FIELDS:
        own[k] = c.regions_field(k)
    ref = R.regions(CS.scene(f["skeleton_framed"], gg["nodes"], gg["edges"], f["origin"], f["resolution"]))
    assert_regions_equal(own, ref, "own after gvd_from_seedgen")
    info = {"origin": f["origin"], "resolution": f["resolution"], "width": f["width"], "height": f["height"]}
    explicit = c.gvd_regions(graph=gg, grid=f["d_skeleton"], info=info, on_device=True, want_ridge_distance=True)
    assert_regions_equal(explicit, ref, "device skeleton of the frame", fields=())
    c.seedgen(cloud)
    with pytest.raises(RuntimeError, match="replaced by a later seed-gen frame"):
        c.gvd_regions()
    assert L.aos_gvd_regions(c.h, None, None, 0, None, None, None, ctypes.byref(out)) == E_STATE
    # a call refused before it touched anything leaves the last fields in place
    assert c.regions_field("ridge").tobytes() == ref["ridge"].tobytes()
    got = c.gvd_regions(grid=f["skeleton_framed"], info=info, want_ridge_distance=True)   # the handle's graph, the grid passed
    assert_regions_equal(got, ref, "own graph, grid passed", fields=())
    c.close()


def test_refusals(ctx):
    L = aos_gpu.lib()
    scenes, refs = scenes_and_refs()
    ok = scenes["graph_nodes"]
    lab = np.zeros(ok["grid"].shape, np.int32)

    def call(sc, out="new", grid="host", info="own", count=None, null_nodes=False, labels=None, opts=None, graph=True):
        o = aos_gpu.RegionsOut() if out == "new" else out
        g = aos_gpu.PathGraph()
        g.num_nodes = len(sc["nodes"]) if count is None else count
        g.nodes_xy = None if null_nodes else sc["nodes"].ctypes.data_as(aos_gpu.P(aos_gpu.c_d))
        i = info_of(sc) if info == "own" else info
        gi = None if i is None else aos_gpu.GridInfo(i["origin"][0], i["origin"][1], i["resolution"], i["width"], i["height"])
        gp = sc["grid"].ctypes.data_as(ctypes.c_void_p) if grid == "host" else grid
        op = None if opts is None else aos_gpu.RegionsOpts(*opts)
        return L.aos_gvd_regions(ctx.h, ctypes.byref(g) if graph else None, gp, 0, ctypes.byref(gi) if gi is not None else None,
                                 None if labels is None else labels.ctypes.data, ctypes.byref(op) if op is not None else None,
                                 ctypes.byref(o) if o is not None else None)

    assert call(ok) == 0
    assert call(ok, out=None) == E_INVALID
    assert call(ok, count=-1) == E_INVALID and call(ok, null_nodes=True) == E_INVALID
    assert call(ok, info=None) == E_INVALID and "without grid info" in L.aos_last_error().decode()
    for w, h in ((16385, 1), (1, 16385), (1 << 20, 1 << 20)):
        assert call(ok, info={**info_of(ok), "width": w, "height": h}) == E_INVALID
        assert "16384" in L.aos_last_error().decode()
    for sc in invalid_scenes()[:-1]:
        assert call(sc) == E_INVALID, (sc["resolution"], sc["nodes"])
    # labels: fine alone and with min_component_cells <= 1; refused with a larger one, and without a grid
    assert call(ok, labels=lab) == 0 and call(ok, labels=lab, opts=(1, 1)) == 0 and call(ok, labels=lab, opts=(-4, 0)) == 0
    assert call(ok, labels=lab, opts=(2, 0)) == E_INVALID and "together with labels" in L.aos_last_error().decode()
    assert call(ok, labels=lab, grid=None, info=None) == E_INVALID and "labels without a grid" in L.aos_last_error().decode()
    assert call(ok, grid=None, info=None) == E_STATE          # the NULL grid form on a handle without a GVD call
    assert call(ok, graph=False) == E_STATE                   # ... and the NULL graph form
    # the field and points calls
    assert call(ok, opts=(0, 1)) == 0
    n = ok["grid"].size
    buf = np.zeros(n, np.uint32)
    assert L.aos_regions_field_copy(ctx.h, b"site", buf.ctypes.data, n - 1) == E_INVALID
    assert L.aos_regions_field_copy(ctx.h, b"site", None, n) == E_INVALID
    for which in (b"d2", b"", b"Site", b"ridge_d", None):
        assert L.aos_regions_field_copy(ctx.h, which, buf.ctypes.data, n) == E_INVALID, which
    assert L.aos_regions_field_copy(ctx.h, b"site", buf.ctypes.data, n) == 0
    assert buf.tobytes() == refs["graph_nodes"]["site"].tobytes()
    b8 = np.zeros(n, np.int8)
    assert L.aos_regions_field_copy(ctx.h, b"ridge", b8.ctypes.data, n) == 0 and b8.tobytes() == refs["graph_nodes"]["ridge"].tobytes()
    xy = np.ascontiguousarray(ok["nodes"])
    nn = len(xy)
    assert L.aos_regions_points(ctx.h, xy.ctypes.data, -1, buf.ctypes.data, None, None, None, None) == E_INVALID
    assert L.aos_regions_points(ctx.h, None, 2, buf.ctypes.data, None, None, None, None) == E_INVALID
    assert L.aos_regions_points(ctx.h, None, 0, None, None, None, None, None) == 0
    assert L.aos_regions_points(ctx.h, xy.ctypes.data, nn, None, None, None, None, None) == 0   # every output null
    m, reg = np.zeros(nn, np.float32), np.zeros(nn, np.int32)
    assert L.aos_regions_points(ctx.h, xy.ctypes.data, nn, None, reg.ctypes.data, None, None, m.ctypes.data) == 0
    assert m.tobytes() == refs["graph_nodes"]["node_ridge_offset"].tobytes()
    assert reg.tobytes() == refs["graph_nodes"]["node_region"].tobytes()
    # the handle serves the next scene as before
    check_scene(ctx, scenes["u_and_dot"], refs["u_and_dot"], "after refusals")
