"""aos_gvd_reach without a GPU: the restatement (reach_ref) against scipy's Dijkstra on a graph built independently from
the move rule, the hand answers, the regime each designed scene (reach_scenes) was built for, the C0 answers, the ABI
declaration, and the product's host code (csrc/reach_host.cpp + csrc/reach.h) as a stand-alone program under ASan +
UBSan, bit for bit against the restatement on every scene."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import aos_gpu
import reach_ref as R
import reach_scenes as S

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "active-orchard-slam_amd", "csrc")
ENTRY_POINTS = ("aos_gvd_reach", "aos_reach_field_copy", "aos_reach_points", "aos_reach_descend")
COUNTS = ("n_passable", "n_reached", "n_sources_used", "max_cost")


@pytest.fixture(scope="module", autouse=True)
def declared():
    """What this file checks is the library's call: nothing here passes against a header without it."""
    fns = aos_gpu.header_functions()
    assert all(f in fns for f in ENTRY_POINTS)
    assert os.path.exists(os.path.join(CSRC, "reach_host.cpp")) and os.path.exists(os.path.join(CSRC, "reach.h"))


_CACHE = {}


def scenes_and_refs():
    """Every scene with its reference, computed once per process (test_gpu_reach shares it)."""
    if not _CACHE:
        sc = S.all_scenes()
        _CACHE["scenes"] = sc
        _CACHE["refs"] = {k: R.reach(v) for k, v in sc.items()}
    return _CACHE["scenes"], _CACHE["refs"]


@pytest.fixture(scope="module")
def scenes():
    return scenes_and_refs()[0]


@pytest.fixture(scope="module")
def refs():
    return scenes_and_refs()[1]


def move_graph(mask):
    """The move relation as a sparse matrix, built with whole-array shifts (no per-cell walk as in reach_ref)."""
    from scipy.sparse import coo_matrix
    H, W = mask.shape
    idx = np.arange(H * W).reshape(H, W)
    rows, cols, w = [], [], []
    for dx, dy in ((1, 0), (0, 1), (1, 1), (-1, 1)):   # one of each pair; the matrix is made symmetric below
        ys, yd = slice(0, H - dy), slice(dy, H)
        xs, xd = (slice(0, W - 1), slice(1, W)) if dx == 1 else (slice(1, W), slice(0, W - 1)) if dx == -1 else (slice(0, W),) * 2
        ok = mask[ys, xs] & mask[yd, xd]
        if dx and dy:
            ok = ok & mask[ys, xd] & mask[yd, xs]
        rows.append(idx[ys, xs][ok]); cols.append(idx[yd, xd][ok]); w.append(np.full(int(ok.sum()), 5 if not (dx and dy) else 7))
    r, c, w = np.concatenate(rows), np.concatenate(cols), np.concatenate(w).astype(np.float64)
    return coo_matrix((np.concatenate([w, w]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(H * W, H * W)).tocsr()


def test_restatement_against_scipy(scenes, refs):
    from scipy.sparse.csgraph import dijkstra
    n = 0
    for k, sc in scenes.items():
        mask = refs[k]["mask"]
        H, W = mask.shape
        kept, cells = R.source_cells(sc["sources"], sc["origin"], sc["resolution"], mask)
        want = np.full(H * W, R.COST_NONE, np.uint32)
        if kept.any():
            d = dijkstra(move_graph(mask), directed=False, indices=np.unique(cells[kept]), min_only=True)
            want = np.where(np.isinf(d), R.COST_NONE, d).astype(np.uint32)
            n += 1
        assert np.array_equal(refs[k]["field"].ravel(), want), k
        assert refs[k]["n_reached"] == int((want != R.COST_NONE).sum()), k
    assert n >= len(scenes) - 8


def test_hand_answers(refs):
    N = R.COST_NONE
    assert refs["hand_3x3"]["field"].tolist() == [[0, 5, 10], [5, 7, 12], [10, 12, 14]]
    assert refs["hand_2x2"]["field"].tolist() == [[0, N], [5, 10]]   # the diagonal is refused: 10, not 7
    r = refs["hand_17"]
    assert r["field"][16, 16] == 800 == r["max_cost"] and r["n_reached"] == r["n_passable"] == 9 * 17 + 8
    assert len(r["descents"][0]) == 161 == 800 // 5 + 1 and r["descents"][1].tolist() == [0]
    assert R.metres(np.array([0, 5, 7, N], np.uint32), 0.25).tolist() == [0.0, 0.25, np.float32(7 * 0.25 / 5.0), np.inf]
    assert R.metres(np.array([12], np.uint32), 0.05)[0] == np.float32(12.0 * float(np.float32(0.05)) / 5.0)


def tile_rounds(mask, fld0, limit=1000):
    """Rounds of a plain tile simulation: every flagged tile is brought to its fixed point against the halo as the round
    found it, and flags the tiles behind the border cells that fell. Returns (rounds in which a tile ran, the field)."""
    H, W = mask.shape
    T = S.TILE
    nty, ntx = -(-H // T), -(-W // T)
    cost = np.where(fld0 == R.COST_NONE, 1 << 40, fld0.astype(np.int64))
    flags = np.zeros((nty, ntx), bool)
    for y, x in np.argwhere(cost == 0):
        flags[max(y // T - 1, 0):y // T + 2, max(x // T - 1, 0):x // T + 2] = True
    rounds = 0
    while flags.any() and rounds < limit:
        rounds += 1
        snap, nxt = cost.copy(), np.zeros_like(flags)
        for ty, tx in np.argwhere(flags):
            y0, y1, x0, x1 = max(ty * T - 1, 0), min(ty * T + T + 1, H), max(tx * T - 1, 0), min(tx * T + T + 1, W)
            win, m = snap[y0:y1, x0:x1].copy(), mask[y0:y1, x0:x1]
            own = np.zeros_like(m)
            own[ty * T - y0:ty * T + T - y0, tx * T - x0:tx * T + T - x0] = True
            while True:   # Jacobi passes inside the window; only the tile's own cells take new values
                best = win.copy()
                h, w = win.shape
                for dx, dy in R.MOVES:
                    ys, yd = (slice(0, h - 1), slice(1, h)) if dy == 1 else (slice(1, h), slice(0, h - 1)) if dy == -1 else (slice(0, h),) * 2
                    xs, xd = (slice(0, w - 1), slice(1, w)) if dx == 1 else (slice(1, w), slice(0, w - 1)) if dx == -1 else (slice(0, w),) * 2
                    ok = m[ys, xs] & m[yd, xd]
                    if dx and dy:
                        ok = ok & m[ys, xd] & m[yd, xs]
                    cand = np.where(ok, win[yd, xd] + (7 if dx and dy else 5), 1 << 41)
                    best[ys, xs] = np.minimum(best[ys, xs], cand)
                best = np.where(own, best, win)
                if np.array_equal(best, win):
                    break
                win = best
            fell = own & (win < snap[y0:y1, x0:x1])
            cost[y0:y1, x0:x1] = np.where(own, win, cost[y0:y1, x0:x1])
            for y, x in np.argwhere(fell):
                gy, gx = y + y0 - ty * T, x + x0 - tx * T   # inside the tile
                for dy in {0, -1 if gy == 0 else 0, 1 if gy == T - 1 else 0}:
                    for dx in {0, -1 if gx == 0 else 0, 1 if gx == T - 1 else 0}:
                        if (dx or dy) and 0 <= ty + dy < nty and 0 <= tx + dx < ntx:
                            nxt[ty + dy, tx + dx] = True
        flags = nxt
    return rounds, np.where(cost >= 1 << 40, R.COST_NONE, cost).astype(np.uint32)


def test_scene_regimes(scenes, refs):
    N = R.COST_NONE
    assert refs["one_free"]["field"].tolist() == [[0]] and refs["one_free"]["max_cost"] == 0
    r = refs["one_occupied"]
    assert r["field"].tolist() == [[N]] and (r["n_passable"], r["n_reached"], r["n_sources_used"], r["max_cost"]) == (0, 0, 0, N)
    assert refs["w70_h1"]["field"][0].tolist() == [5 * abs(x - 3) for x in range(70)]
    assert refs["w1_h70"]["field"][:, 0].tolist() == [5 * abs(y - 66) for y in range(70)]
    for n in S.SWEEP:
        assert scenes[f"sweep_{n}x5"]["grid"].shape == (5, n) and scenes[f"sweep_5x{n}"]["grid"].shape == (n, 5)
        assert refs[f"sweep_{n}x5"]["n_sources_used"] == 1 == refs[f"sweep_5x{n}"]["n_sources_used"]
    assert set(S.SWEEP) == {S.TILE - 1, S.TILE, S.TILE + 1, 2 * S.TILE - 1, 2 * S.TILE, 2 * S.TILE + 1}
    H, W = scenes["wide_700x500"]["grid"].shape
    assert W % S.TILE and H % S.TILE and -(-W // S.TILE) * -(-H // S.TILE) > 256
    r = refs["wide_700x500"]
    assert r["n_sources_used"] == 3 and 0.5 * r["n_passable"] < r["n_reached"] < r["n_passable"]
    assert refs["empty_70x5"]["n_reached"] == 350 and refs["empty_70x5"]["max_cost"] == 4 * 7 + 65 * 5
    r = refs["full_65x3"]
    assert r["n_passable"] == 0 and r["n_sources_used"] == 0 and (r["field"] == N).all()
    r = refs["values"]   # only 100 blocks: 20 of the 21 cells are passable and reached
    assert r["n_passable"] == 20 == r["n_reached"] and r["field"][1, 6] == N
    assert set(scenes["values"]["grid"].ravel().tolist()) >= {-128, -1, 0, 1, 99, 100, 101, 127}
    # the corner rule: between two obstacles that touch diagonally no diagonal passes: six axis moves around one, not 7
    for k, (x, y) in (("diag_touch_inside", (11, 10)), ("diag_touch_tile_corner", (S.TILE, S.TILE - 1))):
        assert refs[k]["field"][y, x] == 6 * 5 and len(refs[k]["descents"][0]) == 7, k
    r = refs["checkerboard"]
    assert r["n_reached"] == 2 == r["n_sources_used"] and r["max_cost"] == 0 and r["n_passable"] == 41
    r = refs["notch"]
    assert r["field"][5, 6] != N and r["field"][6, 7] == N and r["n_reached"] == 61 and r["n_passable"] == 122
    assert [len(p) for p in r["descents"]] == [6, 0, 0]
    # thresholds
    for m in (15, 16):
        r = refs[f"corridor_min_d2_{m}"]
        assert r["n_passable"] == 40 == r["n_reached"] and r["n_sources_used"] == 1 and r["max_cost"] == 195
        assert (r["mask"][4]).all() and not r["mask"][3].any()
    r = refs["corridor_min_d2_17"]
    assert r["n_passable"] == 0 and r["n_sources_used"] == 0 and r["max_cost"] == N
    assert np.array_equal(refs["min_d2_0"]["field"], refs["min_d2_1"]["field"])
    assert refs["min_d2_2"]["n_passable"] < refs["min_d2_1"]["n_passable"] == 1200 - int((scenes["min_d2_1"]["grid"] == 100).sum())
    # long wavefronts under the tile simulation (the serpentine takes more than three batches of rounds)
    for k, least in (("serpentine", 3 * S.BATCH + 1), ("reenter", 2), ("spiral", 2), ("diag_touch_tile_corner", 2)):
        sc, r = scenes[k], refs[k]
        f0 = np.where(r["field"] == 0, 0, N).astype(np.uint32)
        rounds, fld = tile_rounds(r["mask"], f0)
        assert np.array_equal(fld, r["field"]) and rounds >= least, (k, rounds)
    # the reenter scene's descent crosses the line between the tile columns once per lane
    p = refs["reenter"]["descents"][0] % 40
    assert int((np.diff((p >= S.TILE).astype(int)) != 0).sum()) >= 12
    r = refs["spiral"]
    assert r["n_reached"] == r["n_passable"] == len(r["descents"][0]) == 881 and r["max_cost"] == 880 * 5
    # a far source wins where the near one is walled off
    r = refs["far_source_wins"]
    assert r["field"][10, 11] == 18 * 5 and r["field"][10, 9] == 0 and r["descents"][0][-1] == 10 * 30 + 29
    r = refs["one_room_of_two"]
    assert r["n_reached"] == 19 * 20 and r["n_passable"] == 29 * 20 and [len(p) for p in r["descents"]] == [19, 0, 0]
    r = refs["diagonals_20"]
    assert r["field"][19, 19] == 19 * 7 and r["field"][7, 19] == 7 * 7 + 12 * 5 == r["field"][19, 7]
    # (19, 7): the first admissible neighbour is (-1, 0) as long as an axis move remains, so the 5s come first
    p = r["descents"][1]
    assert (np.diff(p.astype(np.int64))[:12] == -1).all() and (np.diff(p.astype(np.int64))[12:] == -21).all()
    # sources
    r = refs["sources_mix"]
    assert len(scenes["sources_mix"]["sources"]) == 11 and r["n_sources_used"] == 5 and r["n_reached"] < r["n_passable"]
    assert int((r["field"] == 0).sum()) == 3 and r["field"][50, 51] == N and scenes["sources_mix"]["grid"][50, 51] == 0
    for k in ("sources_none", "sources_all_dropped"):
        assert refs[k]["n_sources_used"] == 0 == refs[k]["n_reached"] and refs[k]["max_cost"] == N and refs[k]["n_passable"] > 0
    # descent ties: neighbour k and every later one of its kind are admissible, k is taken
    for k in range(8):
        r, (dx, dy) = refs[f"tie_{k}"], R.MOVES[k]
        f = r["field"].astype(np.int64)
        w = lambda j: 5 if j < 4 else 7  # noqa: E731
        adm = [j for j, (ax, ay) in enumerate(R.MOVES) if f[2 + ay, 2 + ax] + w(j) == f[2, 2]]
        assert adm == list(range(k, 4 if k < 4 else 8)) and r["descents"][0].tolist() == [12, (2 + dy) * 5 + 2 + dx], k
    # nodes
    ok = R.C.cells_of(*scenes["nodes_border_nodes"]["nodes"].T, scenes["nodes_border_nodes"]["origin"], S.RES, 40, 30)[0]
    r = refs["nodes_border_nodes"]
    assert ok.tolist() == [True, False, False, True, True, False, False, True, True, True]
    assert (r["node_cost"][~ok] == N).all() and np.isinf(r["node_metres"][~ok]).all() and (r["node_cost"][ok] != N).sum() >= 4
    assert [len(p) for p, o in zip(r["descents"], ok) if not o] == [0] * 4
    for k in ("no_cells_0x0", "no_cells_5x0"):
        r = refs[k]
        assert (r["n_passable"], r["n_reached"], r["n_sources_used"], r["max_cost"]) == (0, 0, 0, N) and r["field"].size == 0
        assert (r["node_cost"] == N).all() and np.isinf(r["node_metres"]).all() and len(r["descents"][0]) == 0


def test_c0_known_answers(scenes, refs):
    """The C0 golden skeleton with its graph's nodes as the sources (the restatement and scipy gave these words when the
    test was written)."""
    sc = scenes["c0_min_d2_0"]
    assert sc["grid"].shape == (512, 512) and len(sc["nodes"]) == 878 == len(sc["sources"])
    r = refs["c0_min_d2_0"]
    assert (r["n_passable"], r["n_reached"], r["n_sources_used"], r["max_cost"]) == (257835, 257835, 878, 1242)
    assert not r["node_cost"].any()
    assert [len(p) for p in r["descents"]] == C0_DESCENTS[0]
    r = refs[f"c0_min_d2_{S.C0_MIN_D2}"]
    assert (r["n_passable"], r["n_reached"], r["n_sources_used"], r["max_cost"]) == (203908, 203803, 304, 1282)
    unreached = r["node_cost"] == R.COST_NONE
    assert int(unreached.sum()) == 574 and not r["node_cost"][~unreached].any()
    assert [int(r["node_cost"][i]) for i in (0, 100, 877)] == C0_NODE_COSTS
    assert [len(p) for p in r["descents"]] == C0_DESCENTS[1]


C0_DESCENTS = ([7, 205, 90, 241, 92], [0, 0, 90, 236, 92])   # cells per descent from reach_scenes.C0_STARTS
C0_NODE_COSTS = [0, R.COST_NONE, 0]                          # nodes 0, 100 and 877 at min_d2 81: node 100 is dropped


def test_declared_and_exported():
    if not os.path.exists(aos_gpu.LIB_PATH):
        aos_gpu.build()
    lib = ctypes.CDLL(aos_gpu.LIB_PATH)
    for f in ENTRY_POINTS:
        assert f in aos_gpu.header_functions() and hasattr(lib, f), f
    assert ctypes.sizeof(aos_gpu.ReachOut) == 120 and ctypes.sizeof(aos_gpu.ReachOpts) == 8
    assert aos_gpu.COST_NONE == R.COST_NONE
    for m in ("gvd_reach", "reach_field", "reach_points", "reach_descend"):
        assert callable(getattr(aos_gpu.Ctx, m))


def invalid_scenes():
    """Inputs the library must refuse with AOS_E_INVALID."""
    g = np.zeros((3, 4), np.int8)
    bad = [S.scene(g, [(0, 0)], resolution=r) for r in (0.0, -0.05, np.nan, np.inf)]
    for v in (np.nan, np.inf, -np.inf):
        bad.append(S.scene(g, [(0, 0)], nodes=[(0.0, 0.0), (0.1, v)]))
    return bad


def blob(scene_list):
    b = np.int32(len(scene_list)).tobytes()
    for sc in scene_list:
        H, W = sc["grid"].shape
        b += np.array([W, H, len(sc["nodes"]), len(sc["sources"]), len(sc["starts"])], np.int32).tobytes()
        b += np.uint32(sc["min_d2"]).tobytes() + np.array(sc["origin"], np.float64).tobytes()
        b += np.float32(sc["resolution"]).tobytes()
        b += sc["grid"].tobytes() + sc["nodes"].tobytes() + sc["sources"].tobytes() + sc["starts"].tobytes()
    return b


def parse_host_output(raw, scene_list):
    out, off = [], 0
    for sc in scene_list:
        H, W = sc["grid"].shape
        N = len(sc["nodes"])
        status = int(np.frombuffer(raw, np.int32, 1, off)[0])
        off += 4
        if status:
            out.append({"status": status})
            continue
        n_pass, n_reached = (int(v) for v in np.frombuffer(raw, np.uint64, 2, off))
        used = int(np.frombuffer(raw, np.int32, 1, off + 16)[0])
        max_cost = int(np.frombuffer(raw, np.uint32, 1, off + 20)[0])
        off += 24
        take = lambda n, dt: np.frombuffer(raw, dt, n, off).copy()  # noqa: E731
        fld = take(W * H, np.uint32).reshape(H, W); off += 4 * W * H
        nc = take(N, np.uint32); off += 4 * N
        nm = take(N, np.float32); off += 4 * N
        paths, xys = [], []
        for _ in range(len(sc["starts"])):
            n = int(np.frombuffer(raw, np.uint64, 1, off)[0]); off += 8
            paths.append(take(n, np.uint32)); off += 4 * n
            xys.append(take(2 * n, np.float64).reshape(-1, 2)); off += 16 * n
        out.append({"status": 0, "n_passable": n_pass, "n_reached": n_reached, "n_sources_used": used, "max_cost": max_cost,
                    "field": fld, "node_cost": nc, "node_metres": nm, "descents": paths, "descent_xy": xys})
    assert off == len(raw)
    return out


def assert_reach_equal(got, ref, what, with_field=True, with_descents=True):
    for k in COUNTS:
        assert got[k] == ref[k], f"{what}: {k} {got[k]} vs {ref[k]}"
    for k in ("field",) * with_field + ("node_cost", "node_metres"):
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k} {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            raise AssertionError(f"{what}: {k} differs in {len(bad)} places, first {bad[:4].tolist()}: " +
                                 ", ".join(f"{a[tuple(i)]!r} vs {b[tuple(i)]!r}" for i in bad[:4]))
    if with_descents:
        assert len(got["descents"]) == len(ref["descents"]), what
        for i, (a, b, ax, bx) in enumerate(zip(got["descents"], ref["descents"], got["descent_xy"], ref["descent_xy"])):
            assert a.dtype == b.dtype == np.uint32 and a.tolist() == b.tolist(), f"{what}: descent {i}"
            assert ax.shape == bx.shape and ax.tobytes() == bx.tobytes(), f"{what}: descent {i} centres"


def test_host_code_under_asan_ubsan(scenes, refs, tmp_path):
    """csrc/reach_host.cpp as tests/reach_host/reach_host_main.cpp (its own main, the sanitizer runtimes linked
    statically, nothing preloaded): every scene bit for bit, the refused inputs refused, no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "reach_host_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall",
                    "-I", CSRC, os.path.join(HERE, "reach_host", "reach_host_main.cpp"),
                    os.path.join(CSRC, "reach_host.cpp"), os.path.join(CSRC, "clearance_host.cpp"), "-o", exe], check=True)
    names = list(scenes)
    bad = invalid_scenes()
    everything = [scenes[k] for k in names] + bad
    fi, fo = tmp_path / "in.bin", tmp_path / "out.bin"
    fi.write_bytes(blob(everything))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(fi), str(fo)], capture_output=True, text=True, env=env, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and f"reach_host_main ok {len(everything)} scenes" in r.stdout, (r.stdout, r.stderr[-2000:])
    got = parse_host_output(fo.read_bytes(), everything)
    for k, g in zip(names, got):
        assert g["status"] == 0, k
        assert_reach_equal(g, refs[k], k)
    assert all(g["status"] == -1 for g in got[len(names):])
