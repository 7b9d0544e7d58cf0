"""aos_reach_sight / aos_reach_pull without a GPU: the three statements of "touched cells" (sight_ref) against each
other, the touched counts and hand answers of the definition, "move allowed" against "nothing blocked", the regime each
designed scene (sight_scenes) was built for, the clearance guarantee of every leg, the length bound, the ABI
declaration, and the product's host code (csrc/sight_host.cpp + csrc/sight.h) as a stand-alone program under ASan +
UBSan, bit for bit against the restatement on every scene.

The length bound. A leg is no longer than the part of the staircase it spans (the triangle inequality), so the
polyline is at most res * (a + sqrt(2) * d) long for a descent of a axis and d diagonal moves, while descent_m =
res * (5 a + 7 d) / 5. The ratio is largest for a = 0: length_m <= descent_m * 5 sqrt(2) / 7 (about 1.0102), asserted
with a relative slack of 1e-12 for the double sums.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import aos_gpu
import reach_ref as R
import sight_ref as G
import sight_scenes as S
from test_reach_cpu import scenes_and_refs

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "active-orchard-slam_amd", "csrc")
ENTRY_POINTS = ("aos_reach_sight", "aos_reach_pull")
LENGTH_BOUND = 5.0 * np.sqrt(2.0) / 7.0 * (1.0 + 1e-12)

_CACHE = {}


def everything():
    """(scenes, reach refs, {scene: (from, to)}, {scene: (n_touched, n_blocked)}, [(scene, start, span)], [pull ref]),
    computed once per process (test_gpu_sight shares it)."""
    if not _CACHE:
        rs, rr = scenes_and_refs()
        sc = S.all_scenes(rs)
        # (a lane scene has no source: its mask is all of its reference that is read)
        bare = lambda v: {"mask": R.passable(v["grid"]), "field": np.full(v["grid"].shape, R.COST_NONE, np.uint32)}  # noqa: E731
        refs = {k: rr[k] if k in rr else bare(v) if k.startswith("lane_") else R.reach(v) for k, v in sc.items()}
        q = S.queries(sc)
        qa = {k: G.sight(refs[k]["mask"], a, b, sc[k]["origin"], sc[k]["resolution"]) for k, (a, b) in q.items()}
        p = S.pulls(sc)
        pa = [G.pull(refs[k]["field"], refs[k]["mask"], s, sc[k]["origin"], sc[k]["resolution"], span) for k, s, span in p]
        _CACHE["all"] = (sc, refs, q, qa, p, pa)
    return _CACHE["all"]


def pull_of(name, start_index=0, span=0):
    sc, _, _, _, p, pa = everything()
    s = sc[name]["starts"][start_index]
    return pa[p.index((name, (float(s[0]), float(s[1])), span))]


def test_three_statements_agree():
    for dx in range(-7, 8):
        for dy in range(-7, 8):
            a, b = (9, 8), (9 + dx, 8 + dy)
            box = G.touched_bbox(a, b)
            assert box == G.touched_exact(a, b) == G.touched_columns(a, b), (dx, dy)
            assert a in box and b in box and box == G.touched_bbox(b, a)
    rng = np.random.default_rng(3)
    ends = rng.integers(0, 120, (24, 4))
    ends[:6] = [(299, 0, 0, 1), (5, 0, 5, 299), (0, 7, 299, 7), (3, 299, 4, 0), (0, 0, 119, 119), (0, 0, 119, 118)]
    k, x, y = G.columns(*ends.T)
    for i, (ax, ay, bx, by) in enumerate(ends.tolist()):
        got = set(zip(x[k == i].tolist(), y[k == i].tolist()))
        assert int((k == i).sum()) == len(got) and got == G.touched_bbox((ax, ay), (bx, by)), i
    for ax, ay, bx, by in ends[:4].tolist():   # the exact clip on the long thin ones (it is the slow form)
        assert G.touched_exact((ax, ay), (bx, by)) == G.touched_bbox((ax, ay), (bx, by))


def test_touched_counts():
    n = lambda a, b: len(G.touched_bbox(a, b))  # noqa: E731
    assert G.touched_bbox((4, 4), (4, 4)) == {(4, 4)}
    for s in (1, 2, 7, 64):
        assert n((3, 3), (3 + s, 3)) == s + 1 == n((3, 3), (3, 3 + s)) == n((3 + s, 3), (3, 3))
        for sx, sy in S.SIGNS:
            assert n((70, 70), (70 + sx * s, 70 + sy * s)) == 3 * s + 1
    assert n((0, 0), (2, 1)) == 4 and n((0, 0), (6, 3)) == 10
    assert G.touched_bbox((0, 0), (1, 1)) == {(0, 0), (1, 0), (0, 1), (1, 1)}
    t, b = G.sight_cells(np.ones((8, 8), bool), [0, 0, 3], [0, 0, 3], [2, 6, 3], [1, 3, 3])
    assert t.tolist() == [4, 10, 1] and b.tolist() == [0, 0, 0]


def test_move_allowed_iff_nothing_blocked():
    mask = R.passable(S.RS.seeded(40, 30, 0.3, 21))
    ys, xs = np.nonzero(mask)
    n = 0
    for dx, dy in R.MOVES:
        ok = (xs + dx >= 0) & (xs + dx < 40) & (ys + dy >= 0) & (ys + dy < 30)
        _, blocked = G.sight_cells(mask, xs[ok], ys[ok], xs[ok] + dx, ys[ok] + dy)
        want = [R.allowed(mask, int(x), int(y), dx, dy) for x, y in zip(xs[ok], ys[ok])]
        assert (blocked == 0).tolist() == want, (dx, dy)
        n += len(want) - sum(want)
        for x, y in zip(xs[~ok][:3], ys[~ok][:3]):
            assert not R.allowed(mask, int(x), int(y), dx, dy)
    assert n > 500   # refused moves were among them


def test_hand_answers():
    sc, refs, q, qa, p, pa = everything()
    r = refs["pillar"]
    d = r["descents"][0].astype(np.int64)
    assert len(d) == 24 and d[0] == 6 * 24 + 23 and d[-1] == 0
    _, b = G.sight_cells(r["mask"], np.full(24, 23), np.full(24, 6), d % 24, d // 24)
    assert (b == 0).tolist() == [True] * 18 + [False] * 3 + [True] * 3   # visibility is not monotone
    assert pull_of("pillar")["steps"].tolist() == [0, 23]
    assert pull_of("pillar", span=19)["steps"].tolist() == [0, 17, 23]
    assert pull_of("pillar", span=3)["steps"].tolist() == list(range(0, 22, 3)) + [23]
    assert pull_of("pillar", span=1)["steps"].tolist() == list(range(24))
    h = pull_of("hand_17")
    assert h["n_cells"] == 161 and len(h["steps"]) == 18 and h["steps"][:5].tolist() == [0, 16, 18, 34, 36]
    assert [v.tolist() for v in G.sight_cells(refs["diag_touch_inside"]["mask"], [10], [11], [11], [10])] == [[4], [2]]
    assert pull_of("diag_touch_inside")["steps"].tolist() == [0, 1, 3, 5, 6]
    assert [(pull_of("serpentine", i)["n_cells"], len(pull_of("serpentine", i)["steps"])) for i in (0, 1)] == [(2131, 61), (2200, 62)]
    assert (pull_of("spiral")["n_cells"], len(pull_of("spiral")["steps"])) == (881, 42)
    assert [len(pull_of("reenter", i)["steps"]) for i in (0, 1)] == [32, 31]
    assert pull_of("c0_min_d2_0", 3)["steps"].tolist() == [0, 230, 238, 240]
    assert [len(pull_of("c0_min_d2_0", i)["steps"]) for i in (0, 1, 2, 4)] == [2, 2, 2, 2]


def test_scene_regimes():
    sc, refs, q, qa, p, pa = everything()
    assert (S.SEGS_PER_WG, S.CANDS_PER_WG, S.PULL_BATCH, S.LANES) == (4, 4, 16, 64)
    src = open(os.path.join(CSRC, "sight.h")).read()
    for text in ("kSightTB = 256", "kSegsPerWG = kSightTB / 64", "kCandsPerWG = kSightTB / 64", "kPullBatch = 16"):
        assert text in src, text
    # more than three batches of anchor steps
    assert len(pull_of("serpentine")["steps"]) - 1 > 3 * S.PULL_BATCH
    # the lane scenes: each of the four segments (and its swap) meets exactly its own occupied cell
    for L in S.LENGTHS:
        for o in "xy":
            for block in S.BLOCKS:
                t, b = qa[f"lane_{o}{L}_{block}"]
                assert len(t) == 8 and (b == 1).all() and t[:4].tolist() == t[4:].tolist(), (L, o, block)
                assert L + 1 < t[0] <= L + 1 + 2 * S.LANE_MINOR
    assert set(S.LENGTHS) == {63, 64, 65, 127, 128, 129}
    # all 15 x 15 offsets, both ways round
    for name in ("free_15", "seeded_15"):
        a, b = q[name]
        t, bl = qa[name]
        assert len(a) >= 450 and t[-450:-225].tolist() == t[-225:].tolist() and bl[-450:-225].tolist() == bl[-225:].tolist()
    for k, (a, b) in q.items():   # and every query of every scene
        t, bl = G.sight(refs[k]["mask"], b, a, sc[k]["origin"], sc[k]["resolution"])
        assert t.tolist() == qa[k][0].tolist() and bl.tolist() == qa[k][1].tolist(), k
    assert (qa["free_15"][1] == 0).all() and 0 < (qa["seeded_15"][1] == 0).sum() < len(qa["seeded_15"][1])
    # corner to corner: a diagonal of the 700 x 500 grid touches more than 700 cells, a shallow one 701 or 702
    t, b = qa["wide_700x500"]
    assert t.max() > 1100 and 700 in (t - 2).tolist() and (b > 0).any()
    # ends without a cell, not finite, equal, on an occupied cell
    t, b = qa["far_source_wins"]
    none = (t == 0)
    assert (b[none] == G.COST_NONE).all() and (b[~none] != G.COST_NONE).all() and 0.3 < none.mean() < 0.8
    assert (t == 1).sum() >= 6 and ((t == 1) & (b == 1)).sum() >= 1   # equal ends; the one on the wall
    # the corridor (the last six segments: three and their swaps)
    assert [v.tolist()[-6:-3] for v in qa["corridor_min_d2_16"]] == [[40, 42, 40], [0, 21, 40]]
    assert qa["corridor_min_d2_17"][1][-6:-3].tolist() == [40, 42, 40]
    assert qa["corridor_min_d2_15"][1][-6] == 0
    # pulls: no cell, unreached, cost 0, two cells, and lengths around the sizes
    by_len = {}
    for (name, s, span), r in zip(p, pa):
        by_len.setdefault(r["n_cells"], []).append((name, len(r["steps"])))
    assert {0, 1, 2} <= set(by_len) and all(n == 0 for _, n in by_len[0]) and all(n == 1 for _, n in by_len[1])
    assert all(n == 2 for _, n in by_len[2])
    rows = [r for (name, s, span), r in zip(p, pa) if name == "row_40"]
    assert sorted(set(r["n_cells"] for r in rows)) == sorted(S.PULL_LENGTHS)
    assert {len(r["steps"]) - 1 for r in rows} >= {1, S.PULL_BATCH - 1, S.PULL_BATCH, S.PULL_BATCH + 1, 2 * S.PULL_BATCH + 1}
    assert any(r["n_sight_tests"] > 10000 for r in pa)


def test_every_leg_keeps_the_clearance_and_the_length_bound():
    sc, refs, q, qa, p, pa = everything()
    d2 = {}
    n_legs = 0
    for (name, s, span), r in zip(p, pa):
        mask = refs[name]["mask"]
        x, y = G.leg_cells(mask, r["cells"])
        assert mask[y, x].all() if len(x) else True, (name, span)
        m = sc[name]["min_d2"]
        if m >= 2 and len(x):
            if name not in d2:
                d2[name] = R.C.field(sc[name]["grid"]).astype(np.uint64)
            assert (d2[name][y, x] >= m).all(), name
        if r["n_cells"]:
            assert r["length_m"] <= r["descent_m"] * LENGTH_BOUND, (name, r["length_m"], r["descent_m"])
            assert r["steps"][0] == 0 and r["steps"][-1] == r["n_cells"] - 1 and (np.diff(r["steps"].astype(int)) > 0).all()
            if span > 0:
                assert (np.diff(r["steps"].astype(int)) <= span).all()
        n_legs += max(len(r["steps"]) - 1, 0)
    assert n_legs > 500 and len(d2) >= 3


def test_declared_and_exported():
    if not os.path.exists(aos_gpu.LIB_PATH):
        aos_gpu.build()
    lib = ctypes.CDLL(aos_gpu.LIB_PATH)
    for f in ENTRY_POINTS:
        assert f in aos_gpu.header_functions() and hasattr(lib, f), f
    hdr = open(aos_gpu.HEADER).read()
    for field in ("n_cells", "start_cost", "n_waypoints", "waypoint_steps", "waypoint_cells", "waypoints_xy", "length_m",
                  "descent_m", "n_steps_launched", "n_sight_tests", "ms_descend", "ms_pull", "max_span"):
        assert field in hdr, field
    # the header's layout: 8 + 4 + 4 + 3 pointers + 2 doubles + 4 (+ 4) + 8 + 2 floats
    assert ctypes.sizeof(aos_gpu.PullOut) == 80 and ctypes.sizeof(aos_gpu.PullOpts) == 4
    assert ctypes.sizeof(aos_gpu.ReachOut) == 120
    for m in ("reach_sight", "reach_pull"):
        assert callable(getattr(aos_gpu.Ctx, m))
    assert os.path.exists(os.path.join(CSRC, "sight_host.cpp")) and os.path.exists(os.path.join(CSRC, "sight.hip"))


def blob(names, sc, q, p):
    b = np.int32(len(names)).tobytes()
    for k in names:
        s = sc[k]
        H, W = s["grid"].shape
        a, e = q.get(k, (np.zeros((0, 2)), np.zeros((0, 2))))
        pl = [(st, span) for name, st, span in p if name == k]
        b += np.array([W, H, len(s["sources"]), len(a), len(pl)], np.int32).tobytes()
        b += np.uint32(s["min_d2"]).tobytes() + np.array(s["origin"], np.float64).tobytes()
        b += np.float32(s["resolution"]).tobytes()
        b += s["grid"].tobytes() + s["sources"].tobytes() + np.ascontiguousarray(a).tobytes() + np.ascontiguousarray(e).tobytes()
        for st, span in pl:
            b += np.array(st, np.float64).tobytes() + np.int32(span).tobytes()
    return b


def parse_host_output(raw, names, q, p):
    out, off = {}, 0
    for k in names:
        status = int(np.frombuffer(raw, np.int32, 1, off)[0]); off += 4
        if status:
            out[k] = {"status": status}
            continue
        n = len(q.get(k, ((), ()))[0])
        t = np.frombuffer(raw, np.uint32, n, off).copy(); off += 4 * n
        b = np.frombuffer(raw, np.uint32, n, off).copy(); off += 4 * n
        pulls = []
        for _ in [1 for name, _, _ in p if name == k]:
            m = int(np.frombuffer(raw, np.uint64, 1, off)[0]); off += 8
            cost, nw = (int(v) for v in np.frombuffer(raw, np.uint32, 2, off)); off += 8
            steps = np.frombuffer(raw, np.uint32, nw, off).copy(); off += 4 * nw
            cells = np.frombuffer(raw, np.uint32, nw, off).copy(); off += 4 * nw
            xy = np.frombuffer(raw, np.float64, 2 * nw, off).copy().reshape(-1, 2); off += 16 * nw
            length, descent = (float(v) for v in np.frombuffer(raw, np.float64, 2, off)); off += 16
            tests = int(np.frombuffer(raw, np.uint64, 1, off)[0]); off += 8
            pulls.append({"n_cells": m, "start_cost": cost, "steps": steps, "cells": cells, "xy": xy, "length_m": length,
                          "descent_m": descent, "n_sight_tests": tests})
        out[k] = {"status": 0, "sight": (t, b), "pulls": pulls}
    assert off == len(raw)
    return out


def assert_pull_equal(got, ref, what):
    for k in ("n_cells", "start_cost", "n_sight_tests"):
        assert got[k] == ref[k], f"{what}: {k} {got[k]} vs {ref[k]}"
    for k in ("steps", "cells"):
        assert got[k].dtype == np.uint32 and got[k].tolist() == ref[k].tolist(), f"{what}: {k}"
    assert got["xy"].shape == ref["xy"].shape and got["xy"].tobytes() == ref["xy"].tobytes(), f"{what}: centres"
    for k in ("length_m", "descent_m"):
        assert np.float64(got[k]).tobytes() == np.float64(ref[k]).tobytes(), f"{what}: {k} {got[k]!r} vs {ref[k]!r}"


def test_host_code_under_asan_ubsan(tmp_path):
    """csrc/sight_host.cpp as tests/sight_host/sight_host_main.cpp (its own main, the sanitizer runtimes linked
    statically, nothing preloaded): every scene bit for bit, the refused inputs refused, the 65536-cell limit through
    the check function, no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    sc, refs, q, qa, p, pa = everything()
    exe = str(tmp_path / "sight_host_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall",
                    "-I", CSRC, os.path.join(HERE, "sight_host", "sight_host_main.cpp"), os.path.join(CSRC, "sight_host.cpp"),
                    os.path.join(CSRC, "reach_host.cpp"), os.path.join(CSRC, "clearance_host.cpp"), "-o", exe], check=True)
    names = list(sc)
    bad = {f"bad_{i}": S.RS.scene(np.zeros((3, 4), np.int8), [(0, 0)], resolution=r)
           for i, r in enumerate((0.0, -0.05, np.nan, np.inf))}
    fi, fo = tmp_path / "in.bin", tmp_path / "out.bin"
    fi.write_bytes(blob(names + list(bad), {**sc, **bad}, q, p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(fi), str(fo)], capture_output=True, text=True, env=env, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and f"sight_host_main ok {len(names) + len(bad)} scenes" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert "sight_host_main checks ok" in r.stdout
    got = parse_host_output(fo.read_bytes(), names + list(bad), q, p)
    assert all(got[k]["status"] == -1 for k in bad)
    for k in names:
        assert got[k]["status"] == 0, k
        if k in q:
            assert got[k]["sight"][0].tolist() == qa[k][0].tolist() and got[k]["sight"][1].tolist() == qa[k][1].tolist(), k
        want = [r for (name, _, _), r in zip(p, pa) if name == k]
        assert len(got[k]["pulls"]) == len(want)
        for i, (a, b) in enumerate(zip(got[k]["pulls"], want)):
            assert_pull_equal(a, b, f"{k} pull {i}")
