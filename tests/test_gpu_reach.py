"""aos_gvd_reach on the GPU vs its restatement (reach_ref). Bar: the field, the counts, node_cost and the float32
node_metres, points, and the descents' indices and centres, bit for bit, on every designed scene (reach_scenes); the NULL
forms on the handle's own graph and skeleton against the explicit forms; the clearance and regions fields of the same
handle untouched; buffers that grow and are reused; the round limit; the ABI's refusals."""
import ctypes

import numpy as np
import pytest

import aos_gpu
import reach_ref as R
import reach_scenes as S
from test_reach_cpu import assert_reach_equal, invalid_scenes, scenes_and_refs

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4


def info_of(sc):
    H, W = sc["grid"].shape
    return {"origin": sc["origin"], "resolution": sc["resolution"], "width": W, "height": H}


def run_scene(c, sc, **kw):
    got = c.gvd_reach(sc["sources"], graph=sc, grid=sc["grid"], info=info_of(sc), min_d2=sc["min_d2"], **kw)
    got["field"] = c.reach_field()
    d = [c.reach_descend(s) for s in sc["starts"]]
    got["descents"], got["descent_xy"] = [v["cells"] for v in d], [v["xy"] for v in d]
    return got


def check_scene(c, sc, ref, what):
    got = run_scene(c, sc)
    assert got["field"].shape == sc["grid"].shape, what
    assert_reach_equal(got, ref, what)
    assert (got["cost_device"] is None) == (sc["grid"].size == 0), what
    cost, m = c.reach_points(sc["nodes"])
    assert cost.tobytes() == ref["node_cost"].tobytes() and m.tobytes() == ref["node_metres"].tobytes(), f"{what}: points"
    return got


@pytest.fixture(scope="module")
def ctx():
    c = aos_gpu.Ctx(aos_gpu.default_params())
    yield c
    c.close()


def test_every_scene(ctx):
    scenes, refs = scenes_and_refs()
    for name, sc in scenes.items():
        got = check_scene(ctx, sc, refs[name], name)
        if name == "serpentine":
            assert got["n_rounds"] > 3 * S.BATCH and got["n_tile_runs"] >= got["n_rounds"]
        if name in ("sources_none", "full_65x3"):
            assert got["n_tile_runs"] == 0 and got["n_rounds"] == 0


def test_descent_capacity(ctx):
    """A capacity below, equal to and above the length: the full length every time, the cells up to the capacity."""
    scenes, refs = scenes_and_refs()
    sc, ref = scenes["hand_17"], refs["hand_17"]
    run_scene(ctx, sc)
    want = ref["descents"][0]
    for cap in (0, 1, len(want) - 1, len(want), len(want) + 1, 4 * len(want)):
        d = ctx.reach_descend(sc["starts"][0], capacity=cap)
        k = min(cap, len(want))
        assert d["n_cells"] == len(want) and d["cells"].tolist() == want[:k].tolist(), cap
        assert d["xy"].tobytes() == ref["descent_xy"][0][:k].tobytes(), cap
    # the indices alone (xy NULL)
    n, cells = ctypes.c_uint64(0), np.zeros(len(want), np.uint32)
    s = np.ascontiguousarray(sc["starts"][0])
    assert aos_gpu.lib().aos_reach_descend(ctx.h, s.ctypes.data, cells.ctypes.data, None, len(want), ctypes.byref(n)) == 0
    assert n.value == len(want) and cells.tolist() == want.tolist()


def c0_handle(c0):
    """A handle after aos_gvd_process on the C0 golden inputs."""
    s = np.load(S.CS.GOLDEN + "/c0_seedgen.npz")
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
    return c, aos_gpu._gvd_dict(o), sk


def test_c0_own_graph_and_forms_and_other_fields():
    """The call with no graph and no grid against the explicit host and device forms and the restatement, at both
    radii; the clearance and regions fields computed before stay what they were."""
    import torch

    scenes, _ = scenes_and_refs()
    c0 = scenes["c0_min_d2_0"]
    info = info_of(c0)
    c, gg, sk = c0_handle(c0)
    clear = c.gvd_clearance()
    d2 = c.clearance_field()
    c.gvd_regions(want_ridge_distance=True)
    regions = {k: c.regions_field(k) for k in ("site", "region", "ridge", "ridge_d2")}
    for m in (0, S.C0_MIN_D2):
        sc = S.scene(c0["grid"], gg["nodes"], m, nodes=gg["nodes"], starts=c0["starts"], origin=c0["origin"],
                     resolution=c0["resolution"], cells=False)
        ref = R.reach(sc)
        assert ref["n_sources_used"] > 100
        own = c.gvd_reach(gg["nodes"], min_d2=m)
        own["field"] = c.reach_field()
        assert_reach_equal(own, ref, f"own graph, own skeleton, min_d2 {m}", with_descents=False)
        assert (own["width"], own["height"], own["resolution"], own["origin"]) == (512, 512, c0["resolution"], c0["origin"])
        explicit = run_scene(c, sc)
        assert_reach_equal(explicit, ref, f"explicit graph, host skeleton, min_d2 {m}")
        d = torch.from_numpy(sk).cuda()
        torch.cuda.synchronize()
        dev = c.gvd_reach(gg["nodes"], graph=gg, grid=d.data_ptr(), info=info, on_device=True, min_d2=m)
        dev["field"] = c.reach_field()
        assert_reach_equal(dev, ref, f"explicit graph, device skeleton, min_d2 {m}", with_descents=False)
        mixed = c.gvd_reach(gg["nodes"], graph=gg, min_d2=m)   # explicit graph, the handle's skeleton
        assert_reach_equal(mixed, ref, "explicit graph, own skeleton", with_field=False, with_descents=False)
        del d
    assert c.clearance_field().tobytes() == d2.tobytes()
    d2_again, _ = c.clearance_points(gg["nodes"])
    assert d2_again.tobytes() == clear["node_d2"].tobytes()
    for k, v in regions.items():
        assert c.regions_field(k).tobytes() == v.tobytes(), k
    c.close()


def test_buffers_grow_and_are_reused():
    """One handle through large, small and large scenes; every call's outputs are right."""
    scenes, refs = scenes_and_refs()
    c = aos_gpu.Ctx(aos_gpu.default_params())
    for name in ("wide_700x500", "tie_3", "no_cells_5x0", "one_free", "sources_mix", "wide_700x500", "hand_2x2"):
        check_scene(c, scenes[name], refs[name], f"reuse {name}")
    c.close()


def test_round_limit():
    scenes, refs = scenes_and_refs()
    sc = scenes["serpentine"]
    c = aos_gpu.Ctx(aos_gpu.default_params())
    L = aos_gpu.lib()
    buf = np.zeros(sc["grid"].size, np.uint32)
    check_scene(c, scenes["hand_3x3"], refs["hand_3x3"], "before the limit")
    with pytest.raises(RuntimeError, match="reach did not converge in 1 rounds") as e:
        run_scene(c, sc, max_rounds=1)
    assert f"error {E_STATE}:" in str(e.value)
    assert L.aos_reach_field_copy(c.h, buf.ctypes.data, buf.size) == E_STATE   # no field is left behind
    n = ctypes.c_uint64(7)
    assert L.aos_reach_descend(c.h, np.zeros(2).ctypes.data, buf.ctypes.data, None, 4, ctypes.byref(n)) == E_STATE
    assert L.aos_reach_points(c.h, np.zeros(2).ctypes.data, 1, buf.ctypes.data, None) == E_STATE
    with pytest.raises(RuntimeError, match=f"did not converge in {S.BATCH + 1} rounds"):
        run_scene(c, sc, max_rounds=S.BATCH + 1)   # a limit inside the second batch
    check_scene(c, sc, refs["serpentine"], "without the limit")
    got = run_scene(c, sc, max_rounds=1000)   # a limit the field settles under
    assert_reach_equal(got, refs["serpentine"], "under a generous limit")
    c.close()


def test_state_errors():
    c = aos_gpu.Ctx(aos_gpu.default_params())
    L = aos_gpu.lib()
    out = aos_gpu.ReachOut()
    buf, xy, n = np.zeros(16, np.uint32), np.zeros(2), ctypes.c_uint64(0)
    assert L.aos_reach_field_copy(c.h, buf.ctypes.data, 16) == E_STATE
    assert L.aos_reach_points(c.h, xy.ctypes.data, 1, buf.ctypes.data, None) == E_STATE
    assert L.aos_reach_descend(c.h, xy.ctypes.data, buf.ctypes.data, None, 16, ctypes.byref(n)) == E_STATE
    assert L.aos_gvd_reach(c.h, None, None, 0, None, xy.ctypes.data, 1, None, ctypes.byref(out)) == E_STATE   # no GVD call yet
    assert "no GVD graph" in L.aos_last_error().decode()
    sc = S.all_scenes()["hand_3x3"]
    with pytest.raises(RuntimeError, match="no grid given and no GVD call"):
        c.gvd_reach(sc["sources"], graph=sc)
    assert L.aos_reach_field_copy(c.h, buf.ctypes.data, 16) == E_STATE   # still no field
    c.close()


def test_refusals(ctx):
    L = aos_gpu.lib()
    scenes, refs = scenes_and_refs()
    ok = scenes["far_source_wins"]

    def call(sc, out="new", grid="host", info="own", n_nodes=None, null_nodes=False, n_sources=None, null_sources=False,
             opts=None):
        o = aos_gpu.ReachOut() if out == "new" else out
        g = aos_gpu.PathGraph()
        g.num_nodes = len(sc["nodes"]) if n_nodes is None else n_nodes
        g.nodes_xy = None if null_nodes else sc["nodes"].ctypes.data_as(aos_gpu.P(aos_gpu.c_d))
        i = info_of(sc) if info == "own" else info
        gi = None if i is None else aos_gpu.GridInfo(i["origin"][0], i["origin"][1], i["resolution"], i["width"], i["height"])
        gp = sc["grid"].ctypes.data_as(ctypes.c_void_p) if grid == "host" else grid
        return L.aos_gvd_reach(ctx.h, ctypes.byref(g), gp, 0, ctypes.byref(gi) if gi is not None else None,
                               None if null_sources else sc["sources"].ctypes.data,
                               len(sc["sources"]) if n_sources is None else n_sources,
                               ctypes.byref(opts) if opts is not None else None, ctypes.byref(o) if o is not None else None)

    assert call(ok) == 0
    assert call(ok, out=None) == E_INVALID
    assert call(ok, n_nodes=-1) == E_INVALID and call(ok, null_nodes=True) == E_INVALID
    assert call(ok, info=None) == E_INVALID and "without grid info" in L.aos_last_error().decode()
    for w, h in ((16385, 1), (1, 16385), (1 << 20, 1 << 20)):
        assert call(ok, info={**info_of(ok), "width": w, "height": h}) == E_INVALID
        assert "16384" in L.aos_last_error().decode()
    for sc in invalid_scenes():
        assert call(sc) == E_INVALID, (sc["resolution"], sc["nodes"])
    assert call(ok, n_sources=-1) == E_INVALID and "negative source count" in L.aos_last_error().decode()
    assert call(ok, n_sources=(1 << 20) + 1) == E_INVALID and "2^20" in L.aos_last_error().decode()   # refused unread
    assert call(ok, null_sources=True) == E_INVALID and "null sources" in L.aos_last_error().decode()
    assert call(ok, null_sources=True, n_sources=0) == 0
    # opts NULL is {0, 0}; a negative max_rounds is no limit
    o = aos_gpu.ReachOut()
    assert call(ok, out=o, opts=aos_gpu.ReachOpts(0, -5)) == 0 and o.n_reached == refs["far_source_wins"]["n_reached"]
    # the field, points and descent calls
    assert call(ok) == 0
    buf = np.zeros(30 * 20, np.uint32)
    assert L.aos_reach_field_copy(ctx.h, buf.ctypes.data, 30 * 20 - 1) == E_INVALID
    assert L.aos_reach_field_copy(ctx.h, None, 30 * 20) == E_INVALID
    assert L.aos_reach_field_copy(None, buf.ctypes.data, 30 * 20) == E_INVALID
    assert L.aos_reach_field_copy(ctx.h, buf.ctypes.data, 30 * 20) == 0
    assert buf.reshape(20, 30).tobytes() == refs["far_source_wins"]["field"].tobytes()
    xy = np.ascontiguousarray(ok["nodes"])
    assert L.aos_reach_points(ctx.h, xy.ctypes.data, -1, buf.ctypes.data, None) == E_INVALID
    assert L.aos_reach_points(ctx.h, None, 2, buf.ctypes.data, None) == E_INVALID
    assert L.aos_reach_points(ctx.h, None, 0, None, None) == 0
    m = np.zeros(len(xy), np.float32)
    assert L.aos_reach_points(ctx.h, xy.ctypes.data, len(xy), None, m.ctypes.data) == 0
    assert m.tobytes() == refs["far_source_wins"]["node_metres"].tobytes()
    n, s = ctypes.c_uint64(0), np.ascontiguousarray(ok["starts"][0])
    assert L.aos_reach_descend(ctx.h, None, buf.ctypes.data, None, 8, ctypes.byref(n)) == E_INVALID
    assert L.aos_reach_descend(ctx.h, s.ctypes.data, buf.ctypes.data, None, 8, None) == E_INVALID
    assert L.aos_reach_descend(ctx.h, s.ctypes.data, None, None, 8, ctypes.byref(n)) == E_INVALID
    assert L.aos_reach_descend(ctx.h, s.ctypes.data, None, None, 0, ctypes.byref(n)) == 0 and n.value == 19
    # the handle serves the next scene as before
    check_scene(ctx, scenes["notch"], refs["notch"], "after refusals")
