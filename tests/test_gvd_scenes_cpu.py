"""The scenes of tests/gvd_scenes.py against the oracle, without a GPU: each scene is in the regime its GPU test is
meant for (the predictors use the library's constants: a constant that moves shows here), the one-handle sequence reruns
its pair lists where the GPU test needs it to, and the oracle call is quick enough for the suite.

The figures when the scenes were chosen (test_scene_regime prints them; seeds -> merged, nodes / edges, the regime):
  chain-clump           1524 -> 716, 726 / 1383; 47 earlier conflicts, chain 1428, owners in rows -1, 0, +1
  chain-clump-shuffled  1524 -> 628, 1123 / 1681; 47 earlier conflicts, another merged set than the 716
  circle                64 seeds, 1 / 0; 352 earlier conflicting ends, 50 ends on the `over` branch, 55 distinct ends
                        within 5 cm of the centre
  circle-centre         65 seeds, 64 / 64; 64 distinct ends on the inner circle, a facet of 65 corners, no conflicts
  circle-jitter         96 seeds, 12 / 66; 407 earlier conflicting ends, 77 on `over`, decided from rows -1, 0, +1
  lattice               784 seeds, 729 / 1004; 408 of 560 label jobs tie exactly
  collinear             40 seeds, 0 / 0; y extent 0; near-collinear: 0.0019
  tiny-1 / -2 / -3      3 / 7 / 11 Voronoi edges, no nodes; identical-50: 50 -> 1, 3 edges
  far-seeds             123 seeds, 109 / 196; 3 seeds beyond g1's index, 110 edge ends beyond g5's
  labels-sparse         60 seeds, 94 / 88; label jobs by class (pass 0, pass 1, pass 2, castRay) 31 / 66 / 45 / 30
  labels-dup-rows       7 nodes with more than 16 label entries, at most 23; no-rows: 94 nodes, no entries
  wide-grid             30 seeds, 42 / 55; node index 6375 cells > 4096: cells of 7.83 m (label 6.94 m, g5 7.28 m)
  pairs-small           150 -> 147; P = 36, first capacity 3456, leaves 1024
  pairs-big             4000 -> 2111, 3861 / 6248; P = 2550 (a fresh handle's capacity: 50524), leaves 3187
The oracle takes at most 0.05 s on a scene, 0.49 s on pairs-big."""
import functools
import re
import time
from pathlib import Path

import numpy as np
import pytest

import gvd_scenes as GS
import oracle_py as O

pytest.importorskip("scipy.spatial")

ORACLE_SECONDS = 3.0   # generous: the slowest scene (pairs-big, 4000 seeds) took 0.43 s when the scenes were chosen

CSRC = Path(__file__).resolve().parent.parent / "active-orchard-slam_amd" / "csrc"


@functools.lru_cache(maxsize=None)
def timed_oracle(name, rect_mode=0):
    seeds, rows, gr = GS.scene(name)
    t0 = time.perf_counter()
    og = O.gvd(seeds, rows, gr, O.default_params(grid_resolution=GS.RES, markers=1, subdiv_rect_mode=rect_mode))
    return og, time.perf_counter() - t0


def oracle_of(name):
    return timed_oracle(name)[0]


@pytest.mark.parametrize("text,path,value", [
    (r"constexpr int kLfTB = (\d+), kLfList = \d+;", "greedy.hip", GS.LF_TB),
    (r"constexpr int kLfTB = \d+, kLfList = (\d+);", "greedy.hip", GS.LF_LIST),
    (r"constexpr int kNodeMatch = (\d+);", "gvd.hip", GS.NODE_MATCH),
    (r"constexpr int kNearThreads = (\d+), kNearK = \d+;", "path.hip", GS.NEAR_THREADS),
    (r"constexpr int kNearThreads = \d+, kNearK = (\d+);", "path.hip", GS.NEAR_K),
    # the stage's named constants, at their definitions at the top of gvd.hip
    (r"constexpr double kMergeRadius = ([\d.]+);", "gvd.hip", GS.MERGE_R),
    (r"constexpr double kMergeRange = ([\d.]+);", "gvd.hip", GS.MERGE_RANGE),
    (r"constexpr double kBpCell = ([\d.]+);", "gvd.hip", GS.BP_CELL),
    (r"constexpr double kBpRange = ([\d.]+);", "gvd.hip", GS.BP_RANGE),
    (r"constexpr double kBpThr = ([\d.]+);", "gvd.hip", GS.BP_THR_SQ ** 0.5),
    (r"constexpr double kNodeCell = ([\d.]+);", "gvd.hip", GS.NODE_CELL),
    (r"constexpr double kNodeRange = ([\d.]+);", "gvd.hip", GS.NODE_RANGE),
    (r"constexpr double kLabelCell = ([\d.]+);", "gvd.hip", GS.LABEL_CELL),
    (r"constexpr double kLabelRange = ([\d.]+);", "gvd.hip", GS.LABEL_RANGE),
    (r"long long n, double cells_per_item = ([\d.]+)\);", "dev_prims.h", GS.CELLS_PER_ITEM),
    (r"std::max\(([\d.]+), cells_per_item \* \(double\)std::max\(n, 1LL\)\)", "greedy.hip", GS.HASH_MIN_CELLS),
    (r"c \*= ([\d.]+);", "greedy.hip", GS.HASH_GROW),
    # the pair capacity's floor, and that both the first capacity and the one a frame leaves take it
    (r"constexpr int kPairCapMin = (\d+);(?s:.*)\? G\.pairs_cap : std::max\(kPairCapMin, 2 \* F\.no\);", "gvd.hip",
     GS.PAIR_CAP_MIN),
    (r"constexpr int kPairCapMin = (\d+);(?s:.*)G\.pairs_cap = std::max\(kPairCapMin, z\.P \+ z\.P / 4\);", "gvd.hip",
     GS.PAIR_CAP_MIN),
    (r"constexpr double kPairMin = [\de.-]+, kPairMax = ([\d.]+);", "gvd.hip", GS.PAIR_MAX),
    (r"constexpr double kPairMin = ([\de.-]+), kPairMax = [\d.]+;", "gvd.hip", GS.PAIR_MIN),
    (r"if \(pass == 0 && !\(z <= ([\d.]+) \* \(1\.0 \+ 1e-12\)\)\) return;", "gvd.hip", 25.0),
    (r"const double two_cells = ([\d.]+) / cn\.h\.inv \* \(1\.0 - 1e-9\);", "gvd.hip", 2.0),
])
def test_predictor_constants_match_the_library(text, path, value):
    m = re.search(text, (CSRC / path).read_text())
    assert m, f"{path}: {text} not found (the code moved: update tests/gvd_scenes.py)"
    assert float(m.group(1)) == value


def test_rerun_rule_matches_the_library():
    """The rerun rule the pattern predictor restates: rerun iff P > cap, once."""
    src = (CSRC / "gvd.hip").read_text()
    assert re.search(r"if \(z\.P <= cap\) break;", src) and re.search(r"if \(attempt\) throw", src)
    assert re.search(r"F\.no = 2 \* F\.ne;", src)


@pytest.mark.parametrize("name", GS.SCENES)
def test_scene_regime(name):
    og, dt = timed_oracle(name)
    fig = GS.check_regime(name, og, oracle_of)
    print(name, f"{dt:.3f} s", fig)
    assert dt < ORACLE_SECONDS, f"oracle call took {dt:.1f} s"


@pytest.mark.parametrize("name", GS.RECT_MODE_SCENES)
def test_scene_regime_rect_mode_1(name):
    """The scenes that also run with subdiv_rect_mode = 1 stay in their regime there."""
    og, dt = timed_oracle(name, 1)
    print(name, f"{dt:.3f} s", GS.check_regime(name, og, oracle_of))
    assert dt < ORACLE_SECONDS, f"oracle call took {dt:.1f} s"


def test_scenes_are_deterministic_and_read_only():
    for name in ("chain-clump-shuffled", "labels-sparse", "pairs-big"):
        a = GS.scene(name)
        GS.scene.cache_clear()
        b = GS.scene(name)
        assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2]))
        assert np.array_equal(a[2]["skeleton_framed"], b[2]["skeleton_framed"])
        assert not a[0].flags.writeable and not a[2]["skeleton_framed"].flags.writeable


def test_handle_sequence_reruns_its_pair_lists():
    """Both pairs-big frames of the one-handle sequence overflow the capacity the frame before left: the first follows a
    fresh handle's pairs-small (cap 1024), the second whatever the second pairs-small left."""
    order = GS.HANDLE_ORDER
    assert set(order) <= set(GS.SCENES)
    pat = GS.rerun_pattern([oracle_of(n) for n in order])
    print(list(zip(order, pat)))
    big = [k for k, n in enumerate(order) if n == "pairs-big"]
    assert len(big) == 2
    for k in big:
        P, cap, rerun = pat[k]
        assert order[k - 1] == "pairs-small" and cap == GS.PAIR_CAP_MIN and rerun and P > cap, pat[k]
    assert pat[0] == (GS.pair_count(oracle_of("pairs-small")), GS.pair_cap_first(oracle_of("pairs-small")), False)
    # a fresh handle has room for pairs-big: only the carried capacity makes it rerun
    assert not GS.rerun_pattern([oracle_of("pairs-big")])[0][2]
    # frames that shrink after a large one (the scratch a large frame leaves is larger than they need)
    assert sum(1 for k in range(1, len(order)) if len(GS.scene(order[k])[0]) < len(GS.scene(order[k - 1])[0]) // 4) >= 3


def test_path_cases_on_the_lattice_graph():
    """What the GPU path tests rely on: the oracle plans on the lattice graph and its truncations with both statuses,
    some path is trimmed at the skeleton's bars, and the robot's lattice-symmetric position ties k_nearest_k's
    distances exactly (at the k-th place too)."""
    og, gr = oracle_of("lattice"), GS.scene("lattice")[2]
    assert np.count_nonzero(gr["skeleton_framed"] == 100) > 0
    statuses, trims, ties = set(), 0, 0
    for m in (None,) + GS.PATH_TRUNCATIONS:
        g = og if m is None else GS.truncated_graph(og, m)
        assert m is None or (len(g["nodes"]) == m and (g["edges"] < m).all()
                             and len(g["node_label_clusters"]) == g["node_label_counts"].sum())
        for kw in GS.path_queries(g):
            r = O.path_plan(g, gr, **kw)
            statuses.add(r["status"])
            trims += r["trimmed_from"] >= 0
            if r["status"] == 1 and kw.get("initial_waypoint_reached", True) and "current" in kw:
                ties += GS.nearest_ties(g, kw["current"])
    assert statuses == {0, 1}, statuses
    assert trims >= 3 and ties >= 8, (trims, ties)
    assert {m for m in GS.PATH_TRUNCATIONS if m < GS.NEAR_K} and \
        {GS.NEAR_THREADS - 1, GS.NEAR_THREADS, GS.NEAR_THREADS + 1} <= set(GS.PATH_TRUNCATIONS)


def test_label_regime_restates_the_oracle():
    """label_regime asserts, per job, that its arg-min is the oracle's label point; here: on every scene with nodes."""
    n = 0
    for name in ("labels-sparse", "lattice", "wide-grid", "pairs-small", "far-seeds"):
        seeds, rows, gr = GS.scene(name)
        cls, _, _ = GS.label_regime(rows, gr, oracle_of(name))
        n += int(np.count_nonzero(cls >= 0))
    assert n > 500
