"""aos_gvd_soft on the GPU vs its restatement (soft_ref). Bar: the field, the counts with n_soft and max_weight,
node_cost, points, and the descents' indices, centres and plain_cost, bit for bit, on every designed scene
(soft_scenes); with gain 0 the field and descents of aos_gvd_reach on the same handle; the NULL forms on the handle's own
graph and skeleton against the explicit forms; the clearance, regions, reach and width fields of the same handle
untouched, and the soft field untouched by them; buffers that grow and are reused; the round limit; every refusal."""
import ctypes

import numpy as np
import pytest

import aos_gpu
import soft_ref as F
import soft_scenes as S
from test_gpu_reach import c0_handle, info_of
from test_soft_cpu import assert_soft_equal, invalid_scenes, scenes_and_refs

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4


def run_scene(c, sc, **kw):
    kw = {"min_d2": sc["min_d2"], "soft_cells": sc["soft_cells"], "gain": sc["gain"], **kw}
    got = c.gvd_soft(sc["sources"], graph=sc, grid=sc["grid"], info=info_of(sc), **kw)
    got["field"] = c.soft_field()
    d = [c.soft_descend(s) for s in sc["starts"]]
    got["descents"], got["descent_xy"] = [v["cells"] for v in d], [v["xy"] for v in d]
    got["plain_costs"] = [v["plain_cost"] for v in d]
    return got


def check_scene(c, sc, ref, what):
    got = run_scene(c, sc)
    assert got["field"].shape == sc["grid"].shape, what
    assert_soft_equal(got, ref, what)
    assert (got["cost_device"] is None) == (sc["grid"].size == 0), what
    assert c.soft_points(sc["nodes"]).tobytes() == ref["node_cost"].tobytes(), f"{what}: points"
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
        if name in ("serpentine", "serpentine_band"):
            assert got["n_rounds"] > 3 * S.BATCH and got["n_tile_runs"] >= got["n_rounds"]
        if name in ("sources_none", "full_65x3"):
            assert got["n_tile_runs"] == 0 and got["n_rounds"] == 0


def test_descent_capacity(ctx):
    """A capacity below, equal to and above the length: the full length and the whole descent's plain_cost every time,
    the cells up to the capacity."""
    scenes, refs = scenes_and_refs()
    sc, ref = scenes["corridor_7"], refs["corridor_7"]
    run_scene(ctx, sc)
    want = ref["descents"][0]
    for cap in (0, 1, len(want) - 1, len(want), len(want) + 1, 4 * len(want)):
        d = ctx.soft_descend(sc["starts"][0], capacity=cap)
        k = min(cap, len(want))
        assert d["n_cells"] == len(want) and d["cells"].tolist() == want[:k].tolist(), cap
        assert d["xy"].tobytes() == ref["descent_xy"][0][:k].tobytes() and d["plain_cost"] == ref["plain_costs"][0], cap
    # the indices alone (xy and plain_cost NULL)
    n, cells = ctypes.c_uint64(0), np.zeros(len(want), np.uint32)
    s = np.ascontiguousarray(sc["starts"][0])
    assert aos_gpu.lib().aos_soft_descend(ctx.h, s.ctypes.data, cells.ctypes.data, None, len(want), ctypes.byref(n), None) == 0
    assert n.value == len(want) and cells.tolist() == want.tolist()
    # a start without a cell and one on an occupied cell: no cells, plain_cost 0
    for start in (S.centre(-4, 3), S.centre(0, 5)):
        d = ctx.soft_descend(start, capacity=4)
        assert (d["n_cells"], d["plain_cost"], len(d["cells"])) == (0, 0, 0)


def test_gain_zero_is_reach(ctx):
    """Without weights the field and the descents are aos_gvd_reach's and aos_reach_descend's on the same handle."""
    scenes, _ = scenes_and_refs()
    for name in ("wide_700x500", "sources_mix", "band_x29", "corridor_min_d2_16", "two_ways_gain_50", "serpentine", "c0_min_d2_16"):
        sc = scenes[name]
        for soft_cells, gain in ((sc["soft_cells"], 0), (0, sc["gain"])):
            soft = run_scene(ctx, sc, soft_cells=soft_cells, gain=gain)
            reach = ctx.gvd_reach(sc["sources"], graph=sc, grid=sc["grid"], info=info_of(sc), min_d2=sc["min_d2"])
            assert ctx.reach_field().tobytes() == soft["field"].tobytes(), name
            assert soft["n_soft"] == 0 and soft["max_weight"] == (1 if soft["n_passable"] else 0), name
            for k in ("n_passable", "n_reached", "n_sources_used", "max_cost"):
                assert soft[k] == reach[k], (name, k)
            assert soft["node_cost"].tobytes() == reach["node_cost"].tobytes(), name
            for s, cells, plain in zip(sc["starts"], soft["descents"], soft["plain_costs"]):
                d = ctx.reach_descend(s)
                assert d["cells"].tolist() == cells.tolist(), name
                assert plain == (int(ctx.reach_points([s])[0][0]) if len(cells) else 0), name


def test_c0_own_graph_and_forms_and_other_fields():
    """The call with no graph and no grid against the explicit host and device forms and the restatement; the
    clearance, regions, reach and width fields computed before stay what they were, and the soft field stays what it
    was across each of those calls."""
    import torch

    scenes, _ = scenes_and_refs()
    c0 = scenes["c0_min_d2_16"]
    info = info_of(c0)
    c, gg, sk = c0_handle(c0)
    clear = c.gvd_clearance()
    d2 = c.clearance_field()
    c.gvd_regions(want_ridge_distance=True)
    regions = {k: c.regions_field(k) for k in ("site", "region", "ridge", "ridge_d2")}
    c.gvd_reach(gg["nodes"], min_d2=9)
    reach, reach_path = c.reach_field(), c.reach_descend(c0["starts"][2])["cells"]
    c.gvd_width(gg["nodes"])
    width = c.width_field()
    sc = S.soften(S.RS.scene(c0["grid"], gg["nodes"], 16, nodes=gg["nodes"], starts=c0["starts"], origin=c0["origin"],
                             resolution=c0["resolution"], cells=False), 10, 2)
    ref = F.soft(sc)
    assert ref["n_sources_used"] > 100 and ref["n_soft"] > 1000
    opts = {"min_d2": 16, "soft_cells": 10, "gain": 2}
    own = c.gvd_soft(gg["nodes"], **opts)
    own["field"] = c.soft_field()
    assert_soft_equal(own, ref, "own graph, own skeleton", with_descents=False)
    assert (own["width"], own["height"], own["resolution"], own["origin"]) == (512, 512, c0["resolution"], c0["origin"])
    explicit = run_scene(c, sc)
    assert_soft_equal(explicit, ref, "explicit graph, host skeleton")
    d = torch.from_numpy(sk).cuda()
    torch.cuda.synchronize()
    dev = c.gvd_soft(gg["nodes"], graph=gg, grid=d.data_ptr(), info=info, on_device=True, **opts)
    dev["field"] = c.soft_field()
    assert_soft_equal(dev, ref, "explicit graph, device skeleton", with_descents=False)
    mixed = c.gvd_soft(gg["nodes"], graph=gg, **opts)   # explicit graph, the handle's skeleton
    assert_soft_equal(mixed, ref, "explicit graph, own skeleton", with_field=False, with_descents=False)
    del d
    # the other calls' fields after the soft calls
    assert c.clearance_field().tobytes() == d2.tobytes()
    assert c.clearance_points(gg["nodes"])[0].tobytes() == clear["node_d2"].tobytes()
    for k, v in regions.items():
        assert c.regions_field(k).tobytes() == v.tobytes(), k
    assert c.reach_field().tobytes() == reach.tobytes()
    assert c.reach_descend(c0["starts"][2])["cells"].tolist() == reach_path.tolist()
    assert c.width_field().tobytes() == width.tobytes()
    # the soft field after each of the other calls
    soft = c.soft_field()
    path = c.soft_descend(c0["starts"][2])
    for again in (lambda: c.gvd_clearance(), lambda: c.gvd_regions(want_ridge_distance=True),
                  lambda: c.gvd_reach(gg["nodes"], min_d2=25), lambda: c.reach_pull(c0["starts"][2]),
                  lambda: c.gvd_width(gg["nodes"])):
        again()
        assert c.soft_field().tobytes() == soft.tobytes()
        p = c.soft_descend(c0["starts"][2])
        assert p["cells"].tolist() == path["cells"].tolist() and p["plain_cost"] == path["plain_cost"]
        assert c.soft_points(gg["nodes"]).tobytes() == ref["node_cost"].tobytes()
    c.close()


def test_buffers_grow_and_are_reused():
    """One handle through large, small and large scenes; every call's outputs are right."""
    scenes, refs = scenes_and_refs()
    c = aos_gpu.Ctx(aos_gpu.default_params())
    for name in ("wide_700x500", "tie_3", "no_cells_5x0", "one_free", "sources_mix", "wide_700x500", "corridor_3"):
        check_scene(c, scenes[name], refs[name], f"reuse {name}")
    c.close()


def test_round_limit():
    scenes, refs = scenes_and_refs()
    sc = scenes["serpentine"]
    c = aos_gpu.Ctx(aos_gpu.default_params())
    L = aos_gpu.lib()
    buf = np.zeros(sc["grid"].size, np.uint32)
    check_scene(c, scenes["corridor_3"], refs["corridor_3"], "before the limit")
    with pytest.raises(RuntimeError, match="soft did not converge in 1 rounds") as e:
        run_scene(c, sc, max_rounds=1)
    assert f"error {E_STATE}:" in str(e.value)
    assert L.aos_soft_field_copy(c.h, buf.ctypes.data, buf.size) == E_STATE   # no field is left behind
    n = ctypes.c_uint64(7)
    assert L.aos_soft_descend(c.h, np.zeros(2).ctypes.data, buf.ctypes.data, None, 4, ctypes.byref(n), None) == E_STATE
    assert L.aos_soft_points(c.h, np.zeros(2).ctypes.data, 1, buf.ctypes.data) == E_STATE
    with pytest.raises(RuntimeError, match=f"did not converge in {S.BATCH + 1} rounds"):
        run_scene(c, sc, max_rounds=S.BATCH + 1)   # a limit inside the second batch
    check_scene(c, sc, refs["serpentine"], "without the limit")
    got = run_scene(c, sc, max_rounds=1000)   # a limit the field settles under
    assert_soft_equal(got, refs["serpentine"], "under a generous limit")
    c.close()


def test_state_errors():
    c = aos_gpu.Ctx(aos_gpu.default_params())
    L = aos_gpu.lib()
    out = aos_gpu.SoftOut()
    buf, xy, n = np.zeros(16, np.uint32), np.zeros(2), ctypes.c_uint64(0)
    assert L.aos_soft_field_copy(c.h, buf.ctypes.data, 16) == E_STATE
    assert L.aos_soft_points(c.h, xy.ctypes.data, 1, buf.ctypes.data) == E_STATE
    assert L.aos_soft_descend(c.h, xy.ctypes.data, buf.ctypes.data, None, 16, ctypes.byref(n), None) == E_STATE
    assert L.aos_gvd_soft(c.h, None, None, 0, None, xy.ctypes.data, 1, None, ctypes.byref(out)) == E_STATE   # no GVD call yet
    assert "no GVD graph" in L.aos_last_error().decode()
    sc = S.all_scenes()["corridor_3"]
    with pytest.raises(RuntimeError, match="no grid given and no GVD call"):
        c.gvd_soft(sc["sources"], graph=sc)
    assert L.aos_soft_field_copy(c.h, buf.ctypes.data, 16) == E_STATE   # still no field
    c.close()


def test_refusals(ctx):
    L = aos_gpu.lib()
    scenes, refs = scenes_and_refs()
    ok = scenes["far_source_wins"]

    def call(sc, out="new", grid="host", info="own", n_nodes=None, null_nodes=False, n_sources=None, null_sources=False,
             opts="own"):
        o = aos_gpu.SoftOut() if out == "new" else out
        g = aos_gpu.PathGraph()
        g.num_nodes = len(sc["nodes"]) if n_nodes is None else n_nodes
        g.nodes_xy = None if null_nodes else sc["nodes"].ctypes.data_as(aos_gpu.P(aos_gpu.c_d))
        i = info_of(sc) if info == "own" else info
        gi = None if i is None else aos_gpu.GridInfo(i["origin"][0], i["origin"][1], i["resolution"], i["width"], i["height"])
        gp = sc["grid"].ctypes.data_as(ctypes.c_void_p) if grid == "host" else grid
        if opts == "own":
            opts = aos_gpu.SoftOpts(sc["min_d2"], sc["soft_cells"], sc["gain"], 0)
        return L.aos_gvd_soft(ctx.h, ctypes.byref(g), gp, 0, ctypes.byref(gi) if gi is not None else None,
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
    assert len(invalid_scenes()) == 7 + len(S.refused_scenes())
    for sc in invalid_scenes()[:7]:
        assert call(sc) == E_INVALID, (sc["resolution"], sc["nodes"])
    assert call(ok, n_sources=-1) == E_INVALID and "negative source count" in L.aos_last_error().decode()
    assert call(ok, n_sources=(1 << 20) + 1) == E_INVALID and "2^20" in L.aos_last_error().decode()   # refused unread
    assert call(ok, null_sources=True) == E_INVALID and "null sources" in L.aos_last_error().decode()
    assert call(ok, null_sources=True, n_sources=0) == 0
    # the options and the bound; a refused call leaves no field behind
    buf = np.zeros(30 * 20, np.uint32)
    for name, (sc, word) in S.refused_scenes().items():
        assert call(ok) == 0 and L.aos_soft_field_copy(ctx.h, buf.ctypes.data, buf.size) == 0
        assert call(sc) == E_INVALID and word in L.aos_last_error().decode(), (name, L.aos_last_error().decode())
        if name == "bound_first":
            assert "max_weight 255" in L.aos_last_error().decode()
            assert L.aos_soft_field_copy(ctx.h, buf.ctypes.data, buf.size) == E_STATE
    # opts NULL is {0, 0, 0, 0}: reach's field; a negative max_rounds is no limit
    o = aos_gpu.SoftOut()
    assert call(ok, out=o, opts=None) == 0 and (o.n_soft, o.max_weight) == (0, 1)
    assert call(ok, out=o, opts=aos_gpu.SoftOpts(0, 4, 3, -5)) == 0 and o.n_reached == refs["far_source_wins"]["n_reached"]
    # the field, points and descent calls
    assert L.aos_soft_field_copy(ctx.h, buf.ctypes.data, 30 * 20 - 1) == E_INVALID
    assert L.aos_soft_field_copy(ctx.h, None, 30 * 20) == E_INVALID
    assert L.aos_soft_field_copy(None, buf.ctypes.data, 30 * 20) == E_INVALID
    assert L.aos_soft_field_copy(ctx.h, buf.ctypes.data, 30 * 20) == 0
    assert buf.reshape(20, 30).tobytes() == refs["far_source_wins"]["field"].tobytes()
    xy = np.ascontiguousarray(ok["nodes"])
    assert L.aos_soft_points(ctx.h, xy.ctypes.data, -1, buf.ctypes.data) == E_INVALID
    assert L.aos_soft_points(ctx.h, None, 2, buf.ctypes.data) == E_INVALID
    assert L.aos_soft_points(ctx.h, None, 0, None) == 0
    assert L.aos_soft_points(None, xy.ctypes.data, 1, buf.ctypes.data) == E_INVALID
    n, s, plain = ctypes.c_uint64(0), np.ascontiguousarray(ok["starts"][0]), ctypes.c_uint32(9)
    assert L.aos_soft_descend(ctx.h, None, buf.ctypes.data, None, 8, ctypes.byref(n), None) == E_INVALID
    assert L.aos_soft_descend(ctx.h, s.ctypes.data, buf.ctypes.data, None, 8, None, None) == E_INVALID
    assert L.aos_soft_descend(ctx.h, s.ctypes.data, None, None, 8, ctypes.byref(n), None) == E_INVALID
    assert L.aos_soft_descend(None, s.ctypes.data, buf.ctypes.data, None, 8, ctypes.byref(n), None) == E_INVALID
    assert L.aos_soft_descend(ctx.h, s.ctypes.data, None, None, 0, ctypes.byref(n), ctypes.byref(plain)) == 0
    assert n.value == len(refs["far_source_wins"]["descents"][0]) and plain.value == refs["far_source_wins"]["plain_costs"][0]
    # the handle serves the next scene as before
    check_scene(ctx, scenes["notch"], refs["notch"], "after refusals")
