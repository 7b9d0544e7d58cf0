"""The scenes of tests/path_scenes.py, without a GPU: on every scene the oracle's planner (oracle/oracle_path.cpp) must
agree with the plain restatement of the two device-side operations (tests/path_ref.py), every scene must be in the
regime it was built for, and every mistake path_ref can make (its variant= switches) must change the answer of at
least one scene, or be shown to be no mistake at all on a float32 resolution."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import oracle_py as O
import path_ref as R
import path_scenes as PS
from test_path_oracle import graph

SCENES = PS.all_scenes()
BY_NAME = {s.name: s for s in SCENES}
OF = {f: [s for s in SCENES if s.family == f] for f in PS.FAMILIES}


@functools.lru_cache(maxsize=None)
def plan(name, zero_grid=False):
    s = BY_NAME[name]
    gr = s.grid
    if zero_grid:
        gr = dict(gr, skeleton_framed=np.zeros_like(gr["skeleton_framed"]))
    return O.path_plan(s.graph, gr, **s.query)


def start_of(s, r):
    """planAndPublishPath's start point of a query (:1060-1090)."""
    q = s.query
    if q.get("current") is not None:
        return tuple(q["current"])
    p = q.get("previous", -1)
    if 0 <= p < len(r["waypoints"]):
        return tuple(r["waypoints"][p].tolist())
    return tuple(q.get("initial_waypoint", (8.0, 0.0)))


def test_the_scene_set_is_whole():
    assert {s.family for s in SCENES} == set(PS.FAMILIES)
    assert all(OF[f] for f in PS.FAMILIES)
    assert max(len(s.graph["nodes"]) for s in SCENES) == 5121
    assert max(s.grid["width"] * s.grid["height"] for s in SCENES) == 513 * 257
    assert {(s.grid["width"], s.grid["height"]) for s in SCENES} >= {(1, 1), (1, 300), (300, 1), (513, 257)}
    order = PS.handle_order(SCENES)
    assert sorted(s.name for s in order) == sorted(BY_NAME)
    sizes = [PS.size(s) for s in order]
    ups = sum(b > a for a, b in zip(sizes, sizes[1:]))
    downs = sum(b < a for a, b in zip(sizes, sizes[1:]))
    assert ups > len(order) // 3 and downs > len(order) // 3


# ---------------------------------------------------------------------------------------------------- trim
@pytest.mark.parametrize("name", [s.name for s in SCENES])
def test_oracle_trim_is_path_ref_trim(name):
    """The oracle's cut index equals path_ref's, recomputed from the oracle's own untrimmed poses (the same query on
    an all-zero grid)."""
    s = BY_NAME[name]
    r, free = plan(name), plan(name, True)
    assert free["trimmed_from"] == -1
    cut = R.trim_first(free["poses"][:, :2], s.grid["skeleton_framed"], s.grid) if len(free["poses"]) else None
    if cut is None:
        assert r["trimmed_from"] == -1 and np.array_equal(r["poses"], free["poses"])
    else:
        assert r["trimmed_from"] == len(free["poses"]) and np.array_equal(r["poses"], free["poses"][:cut])
    if "cut" in s.regime:
        assert cut == s.regime["cut"], (cut, s.regime["cut"])
        assert r["status"] == 1
        assert free["poses"][:, :2].tolist() == [list(p) for p in s.regime["poses"]], "the poses are not the designed ones"
    else:
        assert cut is None, "a scene of another family is trimmed"


def test_trim_offset_regimes():
    ext = {r: PS.offset_extremes(r) for r in PS.RESOLUTIONS}
    assert ext[0.05][:2] == ((3, 2), (4, 0)) and ext[0.04][0] == (5, 0) and ext[0.04][2] == (6, 0)
    assert ext[0.0625][:2] == ((3, 1), (3, 2)) and ext[0.1][:2] == ((1, 1), (2, 0))
    assert ext[0.2][:2] == ((0, 0), (1, 0)) and ext[0.25][:2] == ((0, 0), (1, 0))
    assert ext[0.025][:2] == ((6, 5), (8, 0))
    res = float(np.float32(0.05))
    assert R.radius_cells(res) == 4 and 4 * res > 0.2          # 0.200000003 m: skipped
    res = float(np.float32(0.04))
    assert R.radius_cells(res) == 6 and 5 * res < 0.2 and (5, 0) in R.offsets(res) and (6, 0) not in R.offsets(res)
    for s in OF["trim"]:
        if "offset" not in s.regime:
            continue
        x, y = s.regime["poses"][1]
        c = R.sample_cell(x, y, *s.regime["offset"], s.grid)
        assert c is not None and s.grid["skeleton_framed"].reshape(s.grid["height"], -1)[c[1], c[0]] == 100
        assert (s.regime["offset"] in R.offsets(s.regime["res"])) == (s.regime["cut"] == 1)
        # the sample is well inside its cell: these scenes are about the offsets alone
        res = s.regime["res"]
        fx = (x + s.regime["offset"][0] * res - s.grid["origin"][0]) / res
        assert 0.4 < fx - math.floor(fx) < 0.6


def test_trim_edge_regimes():
    for s in OF["trim"]:
        if "f" not in s.regime:
            continue
        x, y = s.regime["poses"][1]
        res = R.grid_res(s.grid)
        assert R.offsets(res) == [(0, 0)]
        got = ((x - s.grid["origin"][0]) / res, (y - s.grid["origin"][1]) / res)
        for g, want in zip(got, s.regime["f"]):
            assert want is None or g == want
    W = 8.0
    assert np.nextafter(W, 0) < W and float(np.nextafter(np.nextafter(W, 0), 9)) == W      # one ulp
    # the border scenes' quotients lie in (-1, 0) when they cut and below -1 when they do not
    for name, lo in (("border-left-in", True), ("border-left-out", False)):
        fx = (BY_NAME[name].regime["poses"][1][0] - 10.0) / 0.25
        assert (-1.0 < fx < 0.0) == lo and fx < 0.0
    for name, lo in (("border-below-in", True), ("border-below-out", False)):
        fy = (BY_NAME[name].regime["poses"][1][1] - 10.0) / 0.25
        assert (-1.0 < fy < 0.0) == lo and fy < 0.0
    # the range scenes: every far pose has a quotient outside the int range
    s = BY_NAME["range-far-then-inside"]
    for x, y in s.regime["poses"][1:-1]:
        assert not (R.INT_LO < x / 0.25 < R.INT_HI and R.INT_LO < y / 0.25 < R.INT_HI)
    assert np.all(s.grid["skeleton_framed"] == 100)
    assert len(plan("range-far-then-inside")["poses"]) == len(s.regime["poses"]) - 1
    assert len(plan("offset-0.1-kept")["poses"]) == 1              # pose 1 cut: one pose is left
    assert plan("pose0-only")["trimmed_from"] == -1
    # block scenes: later poses are occupied too, in other 128-thread blocks
    for f in PS.FIRST_CUTS:
        for name in (f"block-chain-{f}", f"block-straight-x-{f}"):
            s = BY_NAME[name]
            poses = s.regime["poses"]
            assert len(poses) >= 300
            hits = [i for i in range(1, len(poses))
                    if R.trim_first([poses[0], poses[i]], s.grid["skeleton_framed"], s.grid) == 1]
            assert hits[0] == f and len(hits) >= 3 and hits[-1] > f, (name, hits)
            assert f >= 2 * PS.TRIM_BLOCK or hits[-1] // PS.TRIM_BLOCK > f // PS.TRIM_BLOCK, (name, hits)


def test_trim_variants_change_a_scene():
    """floor, any non-zero value and pose 0 are caught by a scene; `>=`, the fused sample and rc = round(...) cannot
    differ from the reference's arithmetic on a float32 resolution (shown below)."""
    caught = {v: [] for v in R.TRIM_VARIANTS}
    for s in OF["trim"]:
        poses = s.regime["poses"]
        if len(poses) > 16:
            continue
        for v in R.TRIM_VARIANTS:
            if R.trim_first(poses, s.grid["skeleton_framed"], s.grid, v) != s.regime["cut"]:
                caught[v].append(s.name)
    assert "border-left-in" in caught["floor"] and "border-below-in" in caught["floor"]
    assert any(n.startswith("value-") for n in caught["nonzero"]) and "pose0-only" in caught["pose0"]
    assert not caught["ge"] and not caught["fma"] and not caught["round"]


def test_trim_variants_that_are_no_mistakes():
    """Why no grid tells `>=`, a fused x + dx * res or rc = round(0.2 / res) from the reference:
      * res is a float32 (24 significant bits) and |dx| < 2^29, so dx * res is exact in double: fusing rounds once
        where the plain form also rounds once;
      * sqrt(dx^2 + dy^2) * res == 0.2 needs a float32 within 2^-53 of 0.2 / sqrt(...): none for any offset within
        64 cells (searched here; the nearest float32s on both sides of every quotient);
      * an offset within 0.2 m has |dx| * res <= 0.2, so |dx| <= floor(0.2 / res): rounding the radius up or to the
        nearest never adds or removes a kept offset."""
    rng = np.random.default_rng(7)
    rs = [np.float32(r) for r in PS.RESOLUTIONS] + list(rng.uniform(0.001, 0.5, 200).astype(np.float32))
    for r32 in rs:
        res = float(r32)
        for dx in (1, 3, 7, 200, 2 ** 28 + 1):
            assert Fraction(dx) * Fraction(res) == Fraction(dx * res)
        assert R.offsets(res) == R.offsets(res, "round") == R.offsets(res, "ge")
    for d2 in range(1, 2 * 64 * 64 + 1):
        root = math.sqrt(d2)
        near = np.float32(0.2 / root)
        for r32 in (np.nextafter(near, np.float32(0)), near, np.nextafter(near, np.float32(1))):
            assert root * float(r32) != 0.2, (d2, r32)
    # the fused sample itself, on the scenes' poses
    for s in OF["trim"][:40]:
        x, y = s.regime["poses"][1]
        res = R.grid_res(s.grid)
        for dx, dy in R.offsets(res):
            assert R.fma(dx, res, x) == x + dx * res and R.fma(dy, res, y) == y + dy * res
    assert R.fma(3.0, 1.0 / 3.0, -1.0) != 3.0 * (1.0 / 3.0) - 1.0       # (the emulation does fuse)


# ---------------------------------------------------------------------------------------------------- nearest
@functools.lru_cache(maxsize=None)
def _oracle_candidates(key):
    nodes, p = _CAND_ARGS[key]
    want = R.k_nearest(nodes, p, PS.NEAR_K + 3)
    n = len(nodes)
    d = R.distances(nodes, p)
    probes = [k for k in want if math.isfinite(d[k])]
    away = 2.0 * max(d[k] for k in probes) + 1.0e6                       # the goal, node n: farther than every probe
    all_nodes = np.vstack([nodes, [[p[0] + away, p[1]]]])
    got = []
    free = PS.grid(2, 2, 0.25, (p[0], p[1] + 1.0e7))
    while True:
        e = [v for k in probes if k not in got for v in (k, n)]
        g = graph(all_nodes, e, [0.0] * (len(e) // 2), [(n, 0, 3)])
        r = O.path_plan(g, free, target=0, current=p)
        if r["status"] == 0:
            return got
        assert len(r["node_path"]) == 2 and r["node_path"][1] == n
        got.append(int(r["node_path"][0]))
        assert len(got) <= PS.NEAR_K


_CAND_ARGS = {}


def oracle_candidates(nodes, p):
    """The oracle's findKNearestNodes(p, 5), finite distances only, read off its plans: every probed node gets an edge
    of length 0 to a far goal, so the candidate at the smallest distance, first in the list among equals, carries the
    path; its edge is removed and the next one shows, until no candidate has an edge (the probes past the fifth)."""
    nodes = np.ascontiguousarray(nodes, np.float64)
    key = (hash(nodes.tobytes()), tuple(p))
    _CAND_ARGS[key] = (nodes, tuple(p))
    return _oracle_candidates(key)


@pytest.mark.parametrize("name", [s.name for s in SCENES])
def test_oracle_candidates_are_path_ref_candidates(name):
    s = BY_NAME[name]
    if s.query.get("initial_waypoint_reached", True) is False:
        return   # (the straight line asks for no candidates)
    nodes = s.graph["nodes"]
    p = start_of(s, plan(name))
    d = R.distances(nodes, p)
    want = R.k_nearest(nodes, p, PS.NEAR_K)
    if "cands" in s.regime:
        assert want == s.regime["cands"] and tuple(p) == tuple(s.regime["p"])
    assert oracle_candidates(nodes, p) == [k for k in want if math.isfinite(d[k])]


def test_nearest_regimes():
    seen = set()
    for s in OF["nearest"]:
        r = plan(s.name)
        reg = s.regime
        assert r["status"] == reg.get("status", 1), s.name
        if "node_path" in reg:
            assert r["node_path"].tolist() == reg["node_path"], s.name
        if "n_poses" in reg:
            assert len(r["poses"]) == reg["n_poses"]
        if "pattern" not in reg:
            continue
        nodes, rank, pat, n = s.graph["nodes"], reg["rank"], reg["pattern"], reg["n"]
        seen.add((n, pat))
        d = R.distances(nodes, reg["p"])
        others = np.delete(d, list(reg["near"]))
        assert others.min() >= 1000.0 and len(rank) >= PS.NEAR_K + 1
        th = [k % PS.NEAR_THREADS for k in rank]
        if pat == "stride-descending":
            assert [d[k] for k in rank] == [5.0, 6.0, 7.0, 8.0, 9.0, 10.0] and set(th) == {7} and rank == sorted(rank)[::-1]
            continue
        if pat == "tail":
            assert rank[0] == n - 1 and d[n - 1] == 3.0
            rank = rank[1:]
        tied = [k for k in reg["near"] if d[k] == 5.0]
        assert len(tied) == (6 if pat == "last-stride" else 12) and rank[:len(tied)] == sorted(tied)
        if pat.startswith("apart-"):
            assert PS.merge_level(rank[0], rank[3]) == int(pat[6:]) and rank[3] in reg["cands"]
        if pat.startswith("straddle-"):
            assert PS.merge_level(rank[4], rank[5]) == int(pat[9:])
        if pat == "stride-six":
            assert set(th[:6]) == {7}
        if pat == "last-stride":
            assert all(k >= (n - 1) // PS.NEAR_THREADS * PS.NEAR_THREADS for k in rank[:6]) and n % PS.NEAR_THREADS == 6
    for n in PS.NEAR_N:
        for pat in ("apart-256", "apart-128", "apart-1", "straddle-256", "straddle-128", "straddle-1", "tail"):
            assert (n, pat) in seen
    assert (5121, "stride-six") in seen and (5121, "stride-descending") in seen
    assert {n for n, pat in seen if pat == "last-stride"} == set(PS.LAST_STRIDE_N)
    # same position: every pair of distances ties; the fused pair is ordered the other way round when fused
    for n in range(1, 7):
        s = BY_NAME[f"near-same-position-{n}"]
        assert set(R.distances(s.graph["nodes"], s.regime["p"]).tolist()) == {5.0}
    s = BY_NAME["near-fma-pair"]
    a, b = s.regime["fma_pair"]
    plain, fused = R.distances(s.graph["nodes"], PS.FMA_P), R.distances(s.graph["nodes"], PS.FMA_P, "fma")
    assert plain[a] < plain[b] and fused[a] > fused[b] and a > b
    for s in OF["nearest"]:
        if s.regime.get("overflow"):
            d = R.distances(s.graph["nodes"], s.regime["p"])
            assert 1 < np.count_nonzero(np.isfinite(d)) < PS.NEAR_K and np.all(d[~np.isfinite(d)] == np.inf)
            inf_part = [k for k in s.regime["cands"] if not math.isfinite(d[k])]
            assert inf_part == sorted(inf_part) and inf_part[0] == min(np.flatnonzero(~np.isfinite(d)))


def test_nearest_variants_change_a_scene():
    caught = {v: [] for v in R.NEAREST_VARIANTS}
    for s in OF["nearest"]:
        if s.regime.get("n", 0) > 600 and not s.name.endswith("-all"):
            continue   # (the same nodes as the -all scene)
        for v in R.NEAREST_VARIANTS:
            if v == "fma" and len(s.graph["nodes"]) > 600:
                continue
            if R.k_nearest(s.graph["nodes"], s.regime["p"], PS.NEAR_K, v) != s.regime["cands"]:
                caught[v].append(s.name)
    assert "near-fma-pair" in caught["fma"]
    assert any("straddle-256" in n for n in caught["larger-index"]) and "near-same-position-6" in caught["larger-index"]


# ---------------------------------------------------------------------------------------------------- origin, host
def test_origin_regimes_and_variant():
    changed = []
    for s in OF["origin"]:
        r = plan(s.name)
        nodes, reg = s.graph["nodes"], s.regime
        goal = R.nearest(nodes, (0.0, 0.0))
        assert goal == reg["goal"], s.name
        assert r["status"] == reg.get("status", 1) and r["target"] == reg.get("target", 1)
        assert r["waypoint_nodes"][r["target"]] == -1            # the origin return
        if goal >= 0:
            assert r["node_path"].tolist() == reg["node_path"] and r["node_path"][-1] == goal
            assert r["poses"][-1, :2].tolist() == [0.0, 0.0]
        if "tied" in reg:
            d = R.distances(nodes, (0.0, 0.0))
            assert {d[k] for k in reg["tied"]} == {5.0} and d.min() == 5.0
        if "n_waypoints" in reg:
            assert len(r["waypoints"]) == reg["n_waypoints"]
        if R.nearest(nodes, (0.0, 0.0), "accept-inf") != goal:
            changed.append(s.name)
    assert changed == ["origin-all-overflow"]
    s = BY_NAME["origin-all-overflow"]
    assert np.all(np.isinf(R.distances(s.graph["nodes"], (0.0, 0.0))))
    assert R.nearest(s.graph["nodes"], (0.0, 0.0), "accept-inf") == 0
    # the tie goes to three different positions in the three tie scenes
    assert len({tuple(x.graph["nodes"][x.regime["goal"]].tolist()) for x in OF["origin"] if "tied" in x.regime}) == 3


def test_host_regimes():
    for s in OF["host"]:
        r, reg = plan(s.name), s.regime
        for a, b in reg.get("eq", ()):
            assert a == b, s.name
        for a, b in reg.get("gt", ()):
            assert a > b and a == float(np.nextafter(b, np.inf)), s.name
        if "node_path" in reg:
            assert r["status"] == 1 and r["node_path"].tolist() == reg["node_path"], (s.name, r["node_path"])
        if "n_poses" in reg:
            assert len(r["poses"]) == reg["n_poses"], (s.name, r["poses"])
        if "n_waypoints" in reg:
            assert len(r["waypoints"]) == reg["n_waypoints"], (s.name, r["waypoint_nodes"])
        if "target" in reg:
            assert r["target"] == reg["target"], (s.name, r["target"])
        if "status" in reg:
            assert r["status"] == reg["status"], s.name
        if reg.get("counts_past_end"):
            assert int(s.graph["node_label_counts"].sum()) > len(s.graph["node_label_clusters"])
        if reg.get("fallback"):
            assert len(s.graph["node_label_clusters"]) == 0 and len(r["cluster_ids"]) == 3
            assert any(bin(int(m)).count("1") > 1 for m in s.graph["node_labels"] if m > 0)
    assert plan("host-dup-long-first")["node_path"].tolist() != plan("host-dup-short-first")["node_path"].tolist()
    assert plan("host-repeat-1e-300")["poses"].shape == plan("host-repeat-same")["poses"].shape
    statuses = {plan(s.name)["status"] for s in OF["host"]}
    assert statuses == {0, 1}
    assert plan("host-ids-0-2-7-t0")["cluster_ids"].tolist() == [0, 2, 7]
    assert plan("host-ids-odd-only-t0")["cluster_ids"].tolist() == [1, 3]
    assert (plan("host-ids-missing-corners-t0")["cluster_nodes"] == -1).sum() >= 10
    assert plan("host-bitmask-t0")["cluster_nodes"].tolist() == [[9, 1, 0, 0], [-1, 2, 2, 5], [-1, 10, 7, -1]]
    assert plan("host-saved-completed-out")["waypoint_nodes"][-1] == -1
