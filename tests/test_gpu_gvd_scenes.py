"""The GVD stage (gvd.hip, greedy.hip's de-duplication, path.hip) on the non-orchard scenes of tests/gvd_scenes.py, bit
for bit against the oracle: graph, merged seeds, row label points and markers' cells. Each scene forces a branch that
orchard seeds steer round; tests/test_gvd_scenes_cpu.py asserts, without a GPU, that it does."""
import functools

import numpy as np
import pytest

import aos_gpu
import gvd_scenes as GS
import oracle_py as O
from parity_util import assert_gvd_full_parity, assert_gvd_parity
from test_gpu_path import assert_path_equal

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def oracle(name, rect_mode=0):
    seeds, rows, gr = GS.scene(name)
    return O.gvd(seeds, rows, gr, O.default_params(grid_resolution=GS.RES, markers=1, subdiv_rect_mode=rect_mode))


def new_ctx(rect_mode=0, **kw):
    return aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=GS.RES, subdiv_rect_mode=rect_mode, **kw))


def run_scene(c, name, rect_mode=0):
    seeds, rows, gr = GS.scene(name)
    gg = c.gvd(seeds, rows, gr)
    assert_gvd_full_parity(c, gg, oracle(name, rect_mode))
    return gg


@pytest.mark.parametrize("name,rect_mode", [(n, 0) for n in GS.SCENES] + [(n, 1) for n in GS.RECT_MODE_SCENES])
def test_scene_on_a_fresh_handle(name, rect_mode):
    c = new_ctx(rect_mode)
    run_scene(c, name, rect_mode)
    c.close()


def test_one_handle_through_all_scenes():
    """Scratch carried between frames: the pair lists' capacity (both pairs-big frames rerun, test_gvd_scenes_cpu),
    the group counts a rerun leaves, the cell indices' counts, the de-duplication's epochs, the label index of a frame
    without rows."""
    c = new_ctx()
    for k, name in enumerate(GS.HANDLE_ORDER):
        try:
            run_scene(c, name)
        except AssertionError as e:
            raise AssertionError(f"frame {k} ({name}) after {GS.HANDLE_ORDER[:k]}: {e}") from e
    c.close()


def test_counted_evaluations_on_labels_sparse():
    """A label job whose nearest candidate is two index cells away or farther, or that has none (castRay), must reach
    pass 2, which tests every node once; counting changes nothing in the graph."""
    name = "labels-sparse"
    seeds, rows, gr = GS.scene(name)
    og = oracle(name)
    cls, _, _ = GS.label_regime(rows, gr, og)
    full_scans = int(np.count_nonzero(cls >= 2))
    assert full_scans >= 16
    c = new_ctx()
    plain = run_scene(c, name)
    c.gvd_set_count_evals(True)
    counted = run_scene(c, name)
    e = c.gvd_evals()
    print(e, "jobs by class", [int(np.count_nonzero(cls == k)) for k in range(4)])
    assert e["counted"] == 1 and e["filtered_nodes"] == len(og["nodes"]) and e["n_label_jobs"] == len(cls)
    assert e["edge_ends"] == 2 * len(og["vor_edges"]) and e["boundary_points"] == len(og["boundary_raw"])
    assert e["gpu_labels"] >= full_scans * e["filtered_nodes"], (e["gpu_labels"], full_scans, e["filtered_nodes"])
    # no pass tests a node twice, and there are three passes
    assert e["gpu_labels"] <= 3 * len(cls) * e["filtered_nodes"]
    for k in ("nodes", "edges", "edge_lengths", "node_labels", "node_cluster_indices", "node_label_counts",
              "node_label_clusters", "node_label_types"):
        assert np.array_equal(plain[k], counted[k]), k
    c.gvd_set_count_evals(False)
    assert_gvd_parity(c.gvd(seeds, rows, gr), og)
    c.close()


# ---------------------------------------------------------------- path planning on the lattice graph
@pytest.fixture(scope="module")
def path_handle():
    """One handle for all path tests (external graphs are reloaded on every call)."""
    c = new_ctx()
    yield c
    c.close()


def check_queries(c, graph, ref_graph, gr, what, external):
    statuses = set()
    for kw in GS.path_queries(ref_graph):
        ref = O.path_plan(ref_graph, gr, **kw)
        if external:
            got = c.path_plan(aos_gpu.path_query(**kw), graph=graph, skeleton=gr["skeleton_framed"], info=gr)
        else:
            got = c.path_plan(aos_gpu.path_query(**kw))
        assert_path_equal(got, ref, f"{what} {kw}")
        statuses.add(ref["status"])
    return statuses


def test_path_on_the_handles_own_lattice_graph(path_handle):
    c = path_handle
    gr = GS.scene("lattice")[2]
    og = oracle("lattice")
    run_scene(c, "lattice")
    assert len(og["nodes"]) > GS.NEAR_THREADS
    assert check_queries(c, None, og, gr, "own graph", external=False) == {1}
    # the same graph given from outside, and the handle's own again after it
    assert check_queries(c, og, og, gr, "external graph", external=True) == {1}
    assert check_queries(c, None, og, gr, "own graph again", external=False) == {1}


@pytest.mark.parametrize("m", GS.PATH_TRUNCATIONS)
def test_path_on_truncated_lattice_graphs(path_handle, m):
    """The first m nodes as an external graph: fewer nodes than k_nearest_k's k, node counts around its 512 threads."""
    c = path_handle
    gr = GS.scene("lattice")[2]
    g = GS.truncated_graph(oracle("lattice"), m)
    assert len(g["nodes"]) == m
    st = check_queries(c, g, g, gr, f"first {m} nodes", external=True)
    assert st == ({0, 1} if m <= 4 else {1}), st
