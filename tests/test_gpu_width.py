"""aos_gvd_width on the GPU vs its restatement (width_ref). Bar: the field, the counts, node_width and the float32
node_radius_m, and points, bit for bit, on every designed scene (width_scenes); the NULL forms on the handle's own graph
and skeleton against the explicit forms; the cross-check against aos_gvd_reach on the same handle (min_d2 = width
reaches the cell, width + 1 does not); the reach, clearance and regions fields of the same handle untouched; buffers
that grow and are reused; the round limit; the ABI's refusals."""
import ctypes

import numpy as np
import pytest

import aos_gpu
import reach_ref as R
import width_ref as WR
import width_scenes as S
from test_gpu_reach import c0_handle, info_of
from test_width_cpu import assert_width_equal, invalid_scenes, scenes_and_refs, seeded_cells

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4
NONE = WR.D2_NONE


def run_scene(c, sc, **kw):
    got = c.gvd_width(sc["sources"], graph=sc, grid=sc["grid"], info=info_of(sc), **kw)
    got["field"] = c.width_field()
    got["point_width"], got["point_radius_m"] = c.width_points(sc["points"])
    return got


def check_scene(c, sc, ref, what):
    got = run_scene(c, sc)
    assert got["field"].shape == sc["grid"].shape, what
    assert_width_equal(got, ref, what)
    assert (got["width_device"] is None) == (sc["grid"].size == 0), what
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
        if name == "wide_serpentine":
            assert got["n_rounds"] > 3 * S.BATCH and got["n_tile_runs"] >= got["n_rounds"]
        if name in ("sources_none", "full_65x3"):
            assert got["n_tile_runs"] == 0 and got["n_rounds"] == 0


def cross_check(c, name, sc, ref, reach_args):
    """At most 8 seeded reached cells: aos_gvd_reach with min_d2 = the cell's width reaches it, with width + 1 it does
    not; the width field of the handle is still the reference afterwards."""
    cells = seeded_cells(name, ref, 8, reached_only=True)
    xy = np.array([S.centre(x, y, sc["origin"], sc["resolution"]) for x, y in cells]).reshape(-1, 2)
    for (x, y), p in zip(cells, xy):
        w = int(ref["field"][y, x])
        c.gvd_reach(sc["sources"], min_d2=w, **reach_args)
        assert c.reach_points(p)[0][0] != R.COST_NONE, (name, x, y, w)
        if w != NONE:
            c.gvd_reach(sc["sources"], min_d2=w + 1, **reach_args)
            assert c.reach_points(p)[0][0] == R.COST_NONE, (name, x, y, w + 1)
    assert c.width_field().tobytes() == ref["field"].tobytes(), name
    return len(cells)


def test_cross_check_against_reach(ctx):
    scenes, refs = scenes_and_refs()
    n = 0
    for name, sc in scenes.items():
        H, W = sc["grid"].shape
        if W * H == 0 or W > S.SMALL or H > S.SMALL:
            continue
        check_scene(ctx, sc, refs[name], name)
        n += cross_check(ctx, name, sc, refs[name], {"graph": sc, "grid": sc["grid"], "info": info_of(sc)})
    assert n > 100


def test_c0_forms_cross_check_and_other_fields():
    """The call with no graph and no grid against the explicit host and device forms and the restatement; the
    cross-check against aos_gvd_reach on the handle's own skeleton; the reach, clearance and regions fields computed
    before stay what they were across aos_gvd_width, and its field across them."""
    import torch

    scenes, refs = scenes_and_refs()
    c0, ref = scenes["c0"], refs["c0"]
    info = info_of(c0)
    c, gg, sk = c0_handle(c0)
    if not np.array_equal(gg["nodes"], c0["nodes"]):   # the handle's own graph decides, should it differ from the golden one
        c0 = S.scene(c0["grid"], gg["nodes"], nodes=gg["nodes"], origin=c0["origin"], resolution=c0["resolution"], cells=False,
                     points=c0["points"])
        ref = WR.width(c0)
    clear = c.gvd_clearance()
    d2 = c.clearance_field()
    c.gvd_regions(want_ridge_distance=True)
    regions = {k: c.regions_field(k) for k in ("site", "region", "ridge", "ridge_d2")}
    c.gvd_reach(gg["nodes"], min_d2=9)
    cost = c.reach_field()
    start = S.centre(256, 256, c0["origin"], c0["resolution"])
    descent = c.reach_descend(start)["cells"]
    own = c.gvd_width(gg["nodes"])
    own["field"] = c.width_field()
    assert_width_equal(own, ref, "own graph, own skeleton", with_points=False)
    assert (own["width"], own["height"], own["resolution"], own["origin"]) == (512, 512, c0["resolution"], c0["origin"])
    # what was there before is unchanged
    assert c.reach_field().tobytes() == cost.tobytes() and c.reach_descend(start)["cells"].tobytes() == descent.tobytes()
    assert c.clearance_field().tobytes() == d2.tobytes()
    assert c.clearance_points(gg["nodes"])[0].tobytes() == clear["node_d2"].tobytes()
    for k, v in regions.items():
        assert c.regions_field(k).tobytes() == v.tobytes(), k
    # the source cells' width is their clearance: the two calls check each other
    assert own["node_width"].tobytes() == clear["node_d2"].tobytes()
    assert cross_check(c, "c0", c0, ref, {}) == 8
    c.reach_pull(start)
    assert c.width_field().tobytes() == ref["field"].tobytes()
    explicit = run_scene(c, c0)
    assert_width_equal(explicit, ref, "explicit graph, host skeleton")
    d = torch.from_numpy(sk).cuda()
    torch.cuda.synchronize()
    dev = c.gvd_width(gg["nodes"], graph=gg, grid=d.data_ptr(), info=info, on_device=True)
    dev["field"] = c.width_field()
    assert_width_equal(dev, ref, "explicit graph, device skeleton", with_points=False)
    mixed = c.gvd_width(gg["nodes"], graph=gg)   # explicit graph, the handle's skeleton
    assert_width_equal(mixed, ref, "explicit graph, own skeleton", with_field=False, with_points=False)
    del d
    c.close()


def test_buffers_grow_and_are_reused():
    """One handle through large, small and large scenes; every call's outputs are right."""
    scenes, refs = scenes_and_refs()
    c = aos_gpu.Ctx(aos_gpu.default_params())
    for name in ("wide_700x500", "corner_3", "no_cells_5x0", "one_free", "sources_mix", "wide_700x500", "staircase"):
        check_scene(c, scenes[name], refs[name], f"reuse {name}")
    c.close()


def test_round_limit():
    scenes, refs = scenes_and_refs()
    sc = scenes["wide_serpentine"]
    c = aos_gpu.Ctx(aos_gpu.default_params())
    L = aos_gpu.lib()
    buf = np.zeros(sc["grid"].size, np.uint32)
    check_scene(c, scenes["staircase"], refs["staircase"], "before the limit")
    for limit in (1, S.BATCH + 1):   # inside the first batch, inside the second
        with pytest.raises(RuntimeError, match=f"width did not converge in {limit} rounds") as e:
            run_scene(c, sc, max_rounds=limit)
        assert f"error {E_STATE}:" in str(e.value)
        assert L.aos_width_field_copy(c.h, buf.ctypes.data, buf.size) == E_STATE   # no field is left behind
        assert L.aos_width_points(c.h, np.zeros(2).ctypes.data, 1, buf.ctypes.data, None) == E_STATE
    check_scene(c, sc, refs["wide_serpentine"], "without the limit")
    got = run_scene(c, sc, max_rounds=1000)   # a limit the field settles under
    assert_width_equal(got, refs["wide_serpentine"], "under a generous limit")
    c.close()


def test_state_errors():
    c = aos_gpu.Ctx(aos_gpu.default_params())
    L = aos_gpu.lib()
    out = aos_gpu.WidthOut()
    buf, xy = np.zeros(16, np.uint32), np.zeros(2)
    assert L.aos_width_field_copy(c.h, buf.ctypes.data, 16) == E_STATE
    assert L.aos_width_points(c.h, xy.ctypes.data, 1, buf.ctypes.data, None) == E_STATE
    assert L.aos_gvd_width(c.h, None, None, 0, None, xy.ctypes.data, 1, None, ctypes.byref(out)) == E_STATE   # no GVD call yet
    assert "no GVD graph" in L.aos_last_error().decode()
    sc = S.all_scenes()["staircase"]
    with pytest.raises(RuntimeError, match="no grid given and no GVD call"):
        c.gvd_width(sc["sources"], graph=sc)
    assert L.aos_width_field_copy(c.h, buf.ctypes.data, 16) == E_STATE   # still no field
    # a field of aos_gvd_reach is no field of aos_gvd_width
    c.gvd_reach(sc["sources"], graph=sc, grid=sc["grid"], info=info_of(sc))
    assert L.aos_width_field_copy(c.h, buf.ctypes.data, 16) == E_STATE
    c.close()


def test_refusals(ctx):
    L = aos_gpu.lib()
    scenes, refs = scenes_and_refs()
    ok = scenes["two_components"]
    H, W = ok["grid"].shape

    def call(sc, out="new", grid="host", info="own", n_nodes=None, null_nodes=False, n_sources=None, null_sources=False,
             opts=None, handle=ctx.h):
        o = aos_gpu.WidthOut() if out == "new" else out
        g = aos_gpu.PathGraph()
        g.num_nodes = len(sc["nodes"]) if n_nodes is None else n_nodes
        g.nodes_xy = None if null_nodes else sc["nodes"].ctypes.data_as(aos_gpu.P(aos_gpu.c_d))
        i = info_of(sc) if info == "own" else info
        gi = None if i is None else aos_gpu.GridInfo(i["origin"][0], i["origin"][1], i["resolution"], i["width"], i["height"])
        gp = sc["grid"].ctypes.data_as(ctypes.c_void_p) if grid == "host" else grid
        return L.aos_gvd_width(handle, ctypes.byref(g), gp, 0, ctypes.byref(gi) if gi is not None else None,
                               None if null_sources else sc["sources"].ctypes.data,
                               len(sc["sources"]) if n_sources is None else n_sources,
                               ctypes.byref(opts) if opts is not None else None, ctypes.byref(o) if o is not None else None)

    assert call(ok) == 0
    assert call(ok, out=None) == E_INVALID and call(ok, handle=None) == E_INVALID
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
    # opts NULL is {0}; a negative max_rounds is no limit
    o = aos_gpu.WidthOut()
    assert call(ok, out=o, opts=aos_gpu.WidthOpts(-5)) == 0 and o.n_reached == refs["two_components"]["n_reached"]
    # the field and points calls
    assert call(ok) == 0
    buf = np.zeros(W * H, np.uint32)
    assert L.aos_width_field_copy(ctx.h, buf.ctypes.data, W * H - 1) == E_INVALID
    assert L.aos_width_field_copy(ctx.h, None, W * H) == E_INVALID
    assert L.aos_width_field_copy(None, buf.ctypes.data, W * H) == E_INVALID
    assert L.aos_width_field_copy(ctx.h, buf.ctypes.data, W * H) == 0
    assert buf.reshape(H, W).tobytes() == refs["two_components"]["field"].tobytes()
    xy = np.ascontiguousarray(ok["nodes"])
    assert L.aos_width_points(ctx.h, xy.ctypes.data, -1, buf.ctypes.data, None) == E_INVALID
    assert L.aos_width_points(ctx.h, None, 2, buf.ctypes.data, None) == E_INVALID
    assert L.aos_width_points(None, xy.ctypes.data, 1, buf.ctypes.data, None) == E_INVALID
    assert L.aos_width_points(ctx.h, None, 0, None, None) == 0
    # either output of aos_width_points may be null
    r = np.zeros(len(xy), np.float32)
    assert L.aos_width_points(ctx.h, xy.ctypes.data, len(xy), None, r.ctypes.data) == 0
    assert r.tobytes() == refs["two_components"]["node_radius_m"].tobytes()
    w = np.full(len(xy), 7, np.uint32)
    assert L.aos_width_points(ctx.h, xy.ctypes.data, len(xy), w.ctypes.data, None) == 0
    assert w.tobytes() == refs["two_components"]["node_width"].tobytes()
    assert L.aos_width_points(ctx.h, xy.ctypes.data, len(xy), None, None) == 0
    # the handle serves the next scene as before
    check_scene(ctx, scenes["ties"], refs["ties"], "after refusals")
