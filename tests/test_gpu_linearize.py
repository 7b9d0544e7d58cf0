"""aos_path_linearize (the /aos/path -> /plan step) on the GPU vs the restatement of
aos_path_linearization_node (linearize_ref). Bar: published, long_distance, breakpoints, /plan poses (x, y, qz, qw)
and the number of split searches, bit for bit, on every designed scene (linearize_scenes), in the fused form after
aos_path_plan, and across calls that grow and reuse the handle's buffers; the ABI's refusals."""
import ctypes

import numpy as np
import pytest

import aos_gpu
import linearize_ref as R
import linearize_scenes as S
from test_gpu_path import assert_path_equal, c0_fixture, queries
from test_linearize_cpu import invalid_paths

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = -1, -4


def assert_linear_equal(got, ref, what):
    for k in ("published", "long_distance", "n_split_searches"):
        assert got[k] == ref[k], f"{what}: {k} {got[k]} != {ref[k]}"
    assert np.array_equal(got["breakpoints"], ref["breakpoints"]), \
        f"{what}: breakpoints {got['breakpoints'].tolist()} vs {ref['breakpoints'].tolist()}"
    a, b = got["poses"], ref["poses"]
    assert a.shape == b.shape, f"{what}: poses {a.shape} vs {b.shape}"
    if a.tobytes() != b.tobytes():
        bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
        raise AssertionError(f"{what}: poses differ at {bad[:4].tolist()}: " +
                             ", ".join(f"{a[tuple(i)]!r} vs {b[tuple(i)]!r}" for i in bad[:4]))


@pytest.fixture(scope="module")
def ctx():
    c = aos_gpu.Ctx(aos_gpu.default_params())
    yield c
    c.close()


def test_every_scene(ctx):
    scenes = S.all_scenes()
    searched = 0
    for name, p in scenes.items():
        ref = R.linearize(p)
        assert_linear_equal(ctx.path_linearize(p), ref, name)
        searched += ref["n_split_searches"]
    assert searched > 150


def test_fused_after_path_plan():
    """path_plan then path_linearize() on the C0 fixture, every query of test_gpu_path: the plan's poses linearized,
    the plan's own arrays untouched; a failed plan publishes nothing."""
    g, grid = c0_fixture()
    c = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=grid["resolution"]))
    first = c.path_plan(aos_gpu.path_query(target=0), graph=g, skeleton=grid["skeleton_framed"], info=grid)
    n_wp = len(first["waypoints"])
    gs, keep = aos_gpu.path_graph(g)
    sk = np.ascontiguousarray(grid["skeleton_framed"], np.int8).reshape(-1)
    gi = aos_gpu.GridInfo(grid["origin"][0], grid["origin"][1], grid["resolution"], grid["width"], grid["height"])
    failed = regressed = 0
    for kw in queries(n_wp):
        q = aos_gpu.path_query(**kw)
        o = aos_gpu.PathOut()
        aos_gpu._check(aos_gpu.lib().aos_path_plan(c.h, ctypes.byref(gs), sk.ctypes.data_as(ctypes.c_void_p), 0,
                                                   ctypes.byref(gi), ctypes.byref(q), ctypes.byref(o)))
        before = aos_gpu._path_dict(o)   # copies of the library-owned arrays
        got = c.path_linearize()
        after = aos_gpu._path_dict(o)    # the same pointers, read again after the linearize call
        assert_path_equal(after, before, f"plan arrays after linearize {kw}")
        ref = R.linearize(before["poses"])
        assert_linear_equal(got, ref, f"fused {kw}")
        assert_linear_equal(c.path_linearize(before["poses"]), ref, f"explicit {kw}")
        if before["status"] == 0:
            assert len(before["poses"]) == 0 and got["published"] == 0 and len(got["poses"]) == 0
            failed += 1
        regressed += ref["n_split_searches"] > 0
    assert regressed >= 5
    if not failed:   # the fixture's queries all plan: a graph without nodes fails
        empty = {k: np.zeros((0, 2) if k in ("nodes", "edges") else 0, np.float64 if k == "nodes" else np.int32)
                 for k in ("nodes", "node_labels", "node_cluster_indices", "node_label_counts", "node_label_clusters",
                           "node_label_types", "edges")}
        empty["edge_lengths"] = np.zeros(0, np.float32)
        r = c.path_plan(aos_gpu.path_query(target=0), graph=empty, skeleton=grid["skeleton_framed"], info=grid)
        assert r["status"] == 0
        got = c.path_linearize()
        assert got["published"] == 0 and len(got["poses"]) == 0 and len(got["breakpoints"]) == 0
    del keep
    c.close()


def test_buffers_grow_and_are_reused():
    """One handle through 300, 5, 0 and 600 poses."""
    c = aos_gpu.Ctx(aos_gpu.default_params())
    for legs, per in ((10, 30), (1, 5), (0, 0), (20, 30)):
        p = S.zigzag(legs, per) if legs else np.zeros((0, 4))
        if legs == 1:
            p = S.five()
        assert len(p) == legs * per
        assert_linear_equal(c.path_linearize(p), R.linearize(p), f"n = {len(p)}")
    c.close()


def test_refusals(ctx):
    L = aos_gpu.lib()
    out = aos_gpu.LinearPathOut()
    ok = np.ascontiguousarray(S.five())

    def call(h, arr, n, o=out):
        return L.aos_path_linearize(h, arr.ctypes.data if arr is not None else None, n,
                                    ctypes.byref(o) if o is not None else None)

    fresh = aos_gpu.Ctx(aos_gpu.default_params())
    assert call(fresh.h, None, 0) == E_STATE and "no aos_path_plan" in aos_gpu.lib().aos_last_error().decode()
    fresh.close()
    assert call(ctx.h, ok, 5, None) == E_INVALID
    assert call(None, ok, 5) == E_INVALID
    assert call(ctx.h, ok, -1) == E_INVALID
    assert call(ctx.h, None, 5) == E_INVALID
    big = np.zeros((R.MAX_POSES_IN + 1, 4))
    assert call(ctx.h, big, len(big)) == E_INVALID and "65536" in aos_gpu.lib().aos_last_error().decode()
    for p in invalid_paths():
        with pytest.raises(ValueError):
            R.linearize(p)
        p = np.ascontiguousarray(p, np.float64)
        assert call(ctx.h, p, len(p)) == E_INVALID, p
    # the handle serves the next path as before
    assert call(ctx.h, ok, 5) == 0 and out.published == 1 and out.n_split_searches == 3
    assert_linear_equal(ctx.path_linearize(ok), R.linearize(ok), "after refusals")
