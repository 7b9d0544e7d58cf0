"""aos_reach_sight / aos_reach_pull on the GPU vs their restatement (sight_ref). Bar: n_touched, n_blocked, n_cells,
start_cost, the waypoints' steps, cells and centres, length_m and descent_m, bit for bit, on every designed scene
(sight_scenes); segment counts around a workgroup's; the state errors and the refusals; null outputs; buffers that grow
and are reused; the field, the points and a descent of the same handle unchanged afterwards; the NULL-graph and
NULL-grid form on the C0 handle."""
import ctypes

import numpy as np
import pytest

import aos_gpu
import reach_ref as R
import sight_ref as G
import sight_scenes as S
from test_gpu_reach import c0_handle, info_of
from test_sight_cpu import assert_pull_equal, everything

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4


def reach(c, sc, **kw):
    return c.gvd_reach(sc["sources"], graph=sc, grid=sc["grid"], info=info_of(sc), min_d2=sc["min_d2"], **kw)


def check_sight(c, name, what=None):
    sc, refs, q, qa, p, pa = everything()
    if name not in q:
        return 0
    a, b = q[name]
    t, bl = c.reach_sight(a, b)
    assert t.dtype == bl.dtype == np.uint32
    assert t.tolist() == qa[name][0].tolist(), f"{what or name}: n_touched"
    assert bl.tolist() == qa[name][1].tolist(), f"{what or name}: n_blocked"
    return len(a)


def check_pulls(c, name, what=None):
    sc, refs, q, qa, p, pa = everything()
    n = 0
    for (k, s, span), ref in zip(p, pa):
        if k != name:
            continue
        got = c.reach_pull(s, max_span=span)
        assert_pull_equal(got, ref, f"{what or name} start {s} max_span {span}")
        steps = len(ref["steps"]) - 1
        assert steps <= got["n_steps_launched"] <= max(0, -(-steps // S.PULL_BATCH) * S.PULL_BATCH), (name, s, span)
        n += 1
    return n


def check_scene(c, name, what=None):
    sc = everything()[0]
    reach(c, sc[name])
    return check_sight(c, name, what), check_pulls(c, name, what)


@pytest.fixture(scope="module")
def ctx():
    c = aos_gpu.Ctx(aos_gpu.default_params())
    yield c
    c.close()


def test_state_errors_then_success():
    """AOS_E_STATE before any reach and after a reach stopped by max_rounds, then success on the same handle."""
    sc = everything()[0]
    c = aos_gpu.Ctx(aos_gpu.default_params())
    L = aos_gpu.lib()
    xy, buf, out = np.zeros(2), np.zeros(4, np.uint32), aos_gpu.PullOut()
    for _ in range(2):
        assert L.aos_reach_sight(c.h, xy.ctypes.data, xy.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data) == E_STATE
        assert "no aos_gvd_reach" in L.aos_last_error().decode()
        assert L.aos_reach_sight(c.h, None, None, 0, None, None) == E_STATE
        assert L.aos_reach_pull(c.h, xy.ctypes.data, None, ctypes.byref(out)) == E_STATE
        with pytest.raises(RuntimeError, match="did not converge in 1 rounds"):
            reach(c, sc["serpentine"], max_rounds=1)
    assert check_scene(c, "pillar") == (len(everything()[2]["pillar"][0]), 4)
    with pytest.raises(RuntimeError, match="did not converge in 1 rounds"):
        reach(c, sc["serpentine"], max_rounds=1)
    assert L.aos_reach_pull(c.h, xy.ctypes.data, None, ctypes.byref(out)) == E_STATE
    assert check_scene(c, "serpentine")[1] == 2
    c.close()


def test_every_scene(ctx):
    sc = everything()[0]
    n_seg = n_pull = 0
    for name in sc:
        a, b = check_scene(ctx, name)
        n_seg, n_pull = n_seg + a, n_pull + b
    assert n_seg == sum(len(a) for a, _ in everything()[2].values()) > 4000 and n_pull == len(everything()[4]) > 250


def test_segment_counts_around_a_workgroup(ctx):
    sc, refs, q, qa, p, pa = everything()
    reach(ctx, sc["seeded_15"])
    a, b = q["seeded_15"]
    for n in S.batch_sizes():
        for off in (0, 37):
            t, bl = ctx.reach_sight(a[off:off + n], b[off:off + n])
            assert t.tolist() == qa["seeded_15"][0][off:off + n].tolist(), n
            assert bl.tolist() == qa["seeded_15"][1][off:off + n].tolist(), n


def test_refusals_and_null_outputs(ctx):
    sc, refs, q, qa, p, pa = everything()
    L = aos_gpu.lib()
    reach(ctx, sc["pillar"])
    a, b = (np.ascontiguousarray(v) for v in q["pillar"])
    n = len(a)
    t, bl = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    assert L.aos_reach_sight(ctx.h, a.ctypes.data, b.ctypes.data, -1, t.ctypes.data, bl.ctypes.data) == E_INVALID
    assert "negative segment count" in L.aos_last_error().decode()
    assert L.aos_reach_sight(ctx.h, None, b.ctypes.data, n, t.ctypes.data, bl.ctypes.data) == E_INVALID
    assert L.aos_reach_sight(ctx.h, a.ctypes.data, None, n, t.ctypes.data, bl.ctypes.data) == E_INVALID
    assert "null ends" in L.aos_last_error().decode()
    assert L.aos_reach_sight(None, a.ctypes.data, b.ctypes.data, n, t.ctypes.data, bl.ctypes.data) == E_INVALID
    assert L.aos_reach_sight(ctx.h, None, None, 0, None, None) == 0
    # either output may be null
    assert L.aos_reach_sight(ctx.h, a.ctypes.data, b.ctypes.data, n, t.ctypes.data, None) == 0
    assert L.aos_reach_sight(ctx.h, a.ctypes.data, b.ctypes.data, n, None, bl.ctypes.data) == 0
    assert L.aos_reach_sight(ctx.h, a.ctypes.data, b.ctypes.data, n, None, None) == 0
    assert t.tolist() == qa["pillar"][0].tolist() and bl.tolist() == qa["pillar"][1].tolist()
    s, out = np.ascontiguousarray(sc["pillar"]["starts"][0]), aos_gpu.PullOut()
    assert L.aos_reach_pull(ctx.h, None, None, ctypes.byref(out)) == E_INVALID
    assert L.aos_reach_pull(ctx.h, s.ctypes.data, None, None) == E_INVALID
    assert L.aos_reach_pull(None, s.ctypes.data, None, ctypes.byref(out)) == E_INVALID
    # opts NULL is {0}; a negative max_span is no limit
    assert L.aos_reach_pull(ctx.h, s.ctypes.data, None, ctypes.byref(out)) == 0
    assert (out.n_cells, out.n_waypoints, out.waypoint_steps[1]) == (24, 2, 23)
    o = aos_gpu.PullOpts(-3)
    assert L.aos_reach_pull(ctx.h, s.ctypes.data, ctypes.byref(o), ctypes.byref(out)) == 0 and out.n_waypoints == 2
    # a start without a cell, and one that is not finite
    for bad in ((1e9, 0.0), (np.nan, 0.0)):
        r = ctx.reach_pull(bad)
        assert (r["n_cells"], r["start_cost"], len(r["steps"]), r["length_m"], r["descent_m"]) == (0, R.COST_NONE, 0, 0.0, np.inf)
    # the handle serves the next scene as before
    assert check_scene(ctx, "notch")[1] == 3


def test_buffers_grow_and_are_reused():
    """One handle through large, small and large scenes; every call's outputs are right."""
    c = aos_gpu.Ctx(aos_gpu.default_params())
    for name in ("wide_700x500", "tie_3", "no_cells_5x0", "free_15", "serpentine", "wide_700x500", "hand_2x2"):
        check_scene(c, name, f"reuse {name}")
    c.close()


def test_other_outputs_unchanged(ctx):
    """The reach field, reach_points and a reach_descend of the same handle read again afterwards are what they were, and
    a pull's arrays stay valid across sight, points and descend calls."""
    sc, refs, q, qa, p, pa = everything()
    s = sc["serpentine"]
    reach(ctx, s)
    fld = ctx.reach_field()
    pts = ctx.reach_points(s["nodes"])
    d = ctx.reach_descend(s["starts"][0])
    out, st = aos_gpu.PullOut(), np.ascontiguousarray(s["starts"][1])
    assert aos_gpu.lib().aos_reach_pull(ctx.h, st.ctypes.data, None, ctypes.byref(out)) == 0
    check_sight(ctx, "serpentine")
    again = ctx.reach_descend(s["starts"][0])
    assert ctx.reach_field().tobytes() == fld.tobytes() == refs["serpentine"]["field"].tobytes()
    assert [v.tobytes() for v in ctx.reach_points(s["nodes"])] == [v.tobytes() for v in pts]
    assert again["cells"].tobytes() == d["cells"].tobytes() and again["xy"].tobytes() == d["xy"].tobytes()
    ref = G.pull(refs["serpentine"]["field"], refs["serpentine"]["mask"], s["starts"][1], s["origin"], s["resolution"])
    assert np.ctypeslib.as_array(out.waypoint_steps, (out.n_waypoints,)).tolist() == ref["steps"].tolist()
    assert np.ctypeslib.as_array(out.waypoint_cells, (out.n_waypoints,)).tolist() == ref["cells"].tolist()
    assert check_pulls(ctx, "serpentine") == 2


def test_c0_own_graph_and_grid():
    """After a frame, the call with no graph and no grid: sight and pull on the handle's own skeleton."""
    sc, refs, q, qa, p, pa = everything()
    c0 = sc["c0_min_d2_0"]
    c, gg, sk = c0_handle(c0)
    for m in (0, S.RS.C0_MIN_D2):
        name = f"c0_min_d2_{m}"
        scm = S.RS.scene(c0["grid"], gg["nodes"], m, nodes=gg["nodes"], starts=c0["starts"], origin=c0["origin"],
                         resolution=c0["resolution"], cells=False)
        ref = R.reach(scm)
        c.gvd_reach(gg["nodes"], min_d2=m)
        a, b = q[name]
        t, bl = c.reach_sight(a, b)
        wt, wb = G.sight(ref["mask"], a, b, c0["origin"], c0["resolution"])
        assert t.tolist() == wt.tolist() and bl.tolist() == wb.tolist(), name
        for s in c0["starts"]:
            assert_pull_equal(c.reach_pull(s), G.pull(ref["field"], ref["mask"], s, c0["origin"], c0["resolution"]), f"{name} {s}")
    c.close()
