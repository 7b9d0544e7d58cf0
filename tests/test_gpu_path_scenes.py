"""aos_path_plan (csrc/path.hip: k_trim_check, k_nearest_k and the host planner) on the designed scenes of
tests/path_scenes.py, bit for bit against the oracle on every key of test_gpu_path.assert_path_equal; no tolerance
anywhere. tests/test_path_scenes_cpu.py asserts, without a GPU, that each scene is in the regime it was built for."""
import functools

import numpy as np
import pytest

import aos_gpu
import gvd_scenes as GS
import oracle_py as O
import path_scenes as PS
from test_gpu_path import assert_path_equal

pytestmark = pytest.mark.gpu

SCENES = PS.all_scenes()
BY_NAME = {s.name: s for s in SCENES}


@functools.lru_cache(maxsize=None)
def ref(name):
    s = BY_NAME[name]
    return O.path_plan(s.graph, s.grid, **s.query)


def new_ctx():
    return aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=0.25))


def run(c, s, what, device_grid=None):
    q = aos_gpu.path_query(**s.query)
    if device_grid is None:
        got = c.path_plan(q, graph=s.graph, skeleton=s.grid["skeleton_framed"], info=s.grid)
    else:
        got = c.path_plan(q, graph=s.graph, skeleton=device_grid.data_ptr(), info=s.grid, on_device=True)
    assert_path_equal(got, ref(s.name), f"{what} {s.name}")


@pytest.mark.parametrize("family", PS.FAMILIES)
def test_family_on_a_fresh_handle(family):
    c = new_ctx()
    for s in SCENES:
        if s.family == family:
            run(c, s, "fresh handle")
    c.close()


def test_trim_with_the_skeleton_on_the_device():
    import torch

    c = new_ctx()
    for s in SCENES:
        if s.family == "trim":
            d = torch.from_numpy(np.ascontiguousarray(s.grid["skeleton_framed"])).cuda()
            torch.cuda.synchronize()
            run(c, s, "device skeleton", d)
    c.close()


def test_one_handle_through_all_scenes():
    """The node, pose and grid buffers and the result words carried from plan to plan, small and large in turn."""
    c = new_ctx()
    order = PS.handle_order(SCENES)
    for k, s in enumerate(order):
        try:
            run(c, s, "one handle")
        except AssertionError as e:
            raise AssertionError(f"plan {k} after {[x.name for x in order[max(0, k - 3):k]]}: {e}") from e
    c.close()


def test_own_graph_is_never_stale():
    """The planner keeps the handle's own graph by (address, generation): a second GVD result on the same handle must
    replace it, and an external graph in between must not stick."""
    def own_queries(c, name, what):
        gr = GS.scene(name)[2]
        og = gvd_oracle(name)
        statuses = set()
        for kw in GS.path_queries(og):
            want = O.path_plan(og, gr, **kw)
            assert_path_equal(c.path_plan(aos_gpu.path_query(**kw)), want, f"{what} {kw}")
            statuses.add(want["status"])
        return statuses

    c = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=GS.RES))
    first, second = "lattice", "labels-sparse"
    assert len(gvd_oracle(first)["nodes"]) != len(gvd_oracle(second)["nodes"])
    c.gvd(*GS.scene(first))
    assert own_queries(c, first, "first own graph") == {1}
    c.gvd(*GS.scene(second))
    assert 1 in own_queries(c, second, "second own graph")
    ext = BY_NAME["host-grid6x6-1"]
    run(c, ext, "external graph between")
    assert 1 in own_queries(c, second, "own graph after an external one")
    c.gvd(*GS.scene(first))
    assert own_queries(c, first, "first graph again") == {1}
    c.close()


@functools.lru_cache(maxsize=None)
def gvd_oracle(name):
    seeds, rows, gr = GS.scene(name)
    return O.gvd(seeds, rows, gr, O.default_params(grid_resolution=GS.RES, markers=1))
