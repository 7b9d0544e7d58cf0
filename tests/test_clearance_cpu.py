"""aos_gvd_clearance without a GPU: the two statements of the field (clearance_ref) against each other, the regime each
designed scene (clearance_scenes) was built for, the C0 answers, the ABI declaration, and the product's host code
(csrc/clearance_host.cpp + csrc/clearance.h) as a stand-alone program under ASan + UBSan, bit for bit against the
restatement on every scene."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import aos_gpu
import clearance_ref as R
import clearance_scenes as S

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "active-orchard-slam_amd", "csrc")
ENTRY_POINTS = ("aos_gvd_clearance", "aos_clearance_field_copy", "aos_clearance_points")
BRUTE_PAIRS = 1 << 28   # cells x occupied cells up to which a test runs the brute force


@pytest.fixture(scope="module", autouse=True)
def declared():
    """What this file checks is the library's call: nothing here passes against a header without it."""
    fns = aos_gpu.header_functions()
    assert all(f in fns for f in ENTRY_POINTS)
    assert os.path.exists(os.path.join(CSRC, "clearance_host.cpp")) and os.path.exists(os.path.join(CSRC, "clearance.h"))


_CACHE = {}


def scenes_and_refs():
    """Every scene with its reference, computed once per process (test_gpu_clearance shares it)."""
    if not _CACHE:
        sc = S.all_scenes()
        _CACHE["scenes"] = sc
        _CACHE["refs"] = {k: R.clearance(v) for k, v in sc.items()}
    return _CACHE["scenes"], _CACHE["refs"]


@pytest.fixture(scope="module")
def scenes():
    return scenes_and_refs()[0]


@pytest.fixture(scope="module")
def refs():
    return scenes_and_refs()[1]


def test_brute_and_separable_fields_agree(scenes):
    n = 0
    for k, sc in scenes.items():
        occ = R.occupied(sc["grid"])
        if occ.size * max(1, int(occ.sum())) > BRUTE_PAIRS:
            continue
        a, b = R.brute_field(sc["grid"]), R.separable_field(sc["grid"])
        assert a.dtype == b.dtype == np.uint32 and np.array_equal(a, b), k
        n += 1
    assert n == len(scenes) - 3   # all but the two denser 700 x 500 grids and C0


def test_hand_answers():
    f = R.brute_field(np.array([[0, 0, 0], [0, 0, 100]], np.int8))
    assert f.tolist() == [[5, 2, 1], [4, 1, 0]]
    assert R.brute_field(np.zeros((2, 3), np.int8)).tolist() == [[R.D2_NONE] * 3] * 2
    assert R.metres(np.array([0, 25, R.D2_NONE], np.uint32), 0.25).tolist() == [0.0, 1.25, np.inf]
    assert R.metres(np.array([2], np.uint32), 0.05)[0] == np.float32(np.sqrt(2.0) * float(np.float32(0.05)))
    # the cell rule: -1 < fx < 0 is column 0, fx = -1 and fx = W are outside
    ok, mx, my = R.cells_of([-0.125, -0.25, 1.0, 0.99], [0.0, 0.0, 0.0, 0.1], (0.0, 0.0), 0.25, 4, 1)
    assert ok.tolist() == [True, False, False, True] and mx[0] == 0 and mx[3] == 3 and my[3] == 0
    # len 1, res 0.25: step 0.125, num = 8 + 1, samples t = 0, 1/9 .. 8/9, 1
    px, py = R.edge_samples((0.0, 0.0), (1.0, 0.0), 0.25)
    assert len(px) == 10 and px[0] == 0.0 and px[9] == 1.0 and px[3] == (3 / 9 * 1.0) * 1.0 and not py.any()
    assert R.edge_num(1e9, 0.05) == -(1 << 31) + 1 and R.edge_num(1.0, 0.25) == 9
    assert len(R.edge_samples((1.0, 2.0), (1.0, 2.0 + 5e-7), 0.25)[0]) == 1


def test_scene_regimes(scenes, refs):
    r = refs["one_occupied"]
    assert r["field"].tolist() == [[0]] and r["n_occupied"] == 1 and r["max_d2"] == 0
    assert refs["one_free"]["field"].tolist() == [[R.D2_NONE]] and refs["one_free"]["max_d2"] == R.D2_NONE
    assert np.isinf(refs["one_free"]["node_clearances"]).all() and np.isinf(refs["one_free"]["edge_clearances"]).all()
    assert refs["w1_h130"]["field"][:, 0].tolist() == [min(y * y, (y - 77) ** 2) for y in range(130)]
    assert refs["w130_h1"]["field"][0].tolist() == [min((x - 3) ** 2, (x - 129) ** 2) for x in range(130)]
    assert (refs["empty_70x5"]["field"] == R.D2_NONE).all() and refs["empty_70x5"]["n_occupied"] == 0
    assert not refs["full_65x3"]["field"].any() and refs["full_65x3"]["n_occupied"] == 65 * 3
    assert refs["values"]["n_occupied"] == 1 and refs["values"]["field"][0, 0] == 36 + 1
    assert set(scenes["values"]["grid"].ravel().tolist()) >= {-128, -1, 0, 1, 99, 100, 101, 127}
    for k, far in (("corner_300x200", (199, 299)), ("far_corner_300x200", (0, 0))):   # the longest search
        assert refs[k]["max_d2"] == 299 ** 2 + 199 ** 2 == refs[k]["field"][far] and refs[k]["n_occupied"] == 1
    cols = np.nonzero(R.occupied(scenes["block_edges_130"]["grid"]))[1]
    assert sorted(cols.tolist()) == [S.BLOCK - 1, S.BLOCK, 2 * S.BLOCK - 1, 2 * S.BLOCK, 2 * S.BLOCK + 1]
    f, g = refs["diagonal_wins"]["field"], R.column_distance(scenes["diagonal_wins"]["grid"])
    assert g[4, 4] == 6 and f[4, 4] == 13 and not R.occupied(scenes["diagonal_wins"]["grid"])[4].any()
    assert refs["ties"]["field"][4, 4] == 16
    for n in S.SWEEP:
        for k, shape in ((f"sweep_{n}x5", (5, n)), (f"sweep_5x{n}", (n, 5))):
            assert scenes[k]["grid"].shape == shape and refs[k]["field"][shape[0] - 1, shape[1] - 1] == 0
    assert all(v in S.SWEEP for b in (S.BAND, S.WORKGROUP, S.BLOCK) for v in (b - 1, b, b + 1))
    for share in (0.001, 0.05, 0.6):
        occ = refs[f"mid_700x500_{share}"]["n_occupied"] / 350000.0
        assert 0.7 * share < occ < 1.3 * share
    # graph scenes
    sc = scenes["on_cell_edges"]
    res = sc["resolution"]
    px, py = R.edge_samples(sc["nodes"][0], sc["nodes"][1], res)
    fx = (px - sc["origin"][0]) / res
    assert len(px) > 30 and (fx == 7.0).all()
    px, py = R.edge_samples(sc["nodes"][2], sc["nodes"][3], res)
    assert ((py - sc["origin"][1]) / res == 5.0).all()
    sc, r = scenes["border_nodes"], refs["border_nodes"]
    ok, mx, my = R.cells_of(sc["nodes"][:, 0], sc["nodes"][:, 1], sc["origin"], res, 40, 30)
    assert ok.tolist() == [True, False, False, True, True, False, False, True, True, True]
    assert (mx[0], mx[3], my[4], my[7], mx[8], my[8], mx[9], my[9]) == (0, 39, 0, 29, 0, 0, 39, 29)
    assert (r["node_d2"][~ok] == R.D2_NONE).all() and (r["node_d2"][ok] != R.D2_NONE).all()
    r = refs["outside_and_partly"]
    assert r["edge_d2"][0] == R.D2_NONE and np.isinf(r["edge_clearances"][0]) and (r["edge_d2"][1:] != R.D2_NONE).all()
    assert r["node_d2"][2] == R.D2_NONE and r["node_d2"][3] != R.D2_NONE
    sc, r = scenes["long_1e4m"], refs["long_1e4m"]
    assert R.edge_num(float(np.hypot(*(sc["nodes"][1] - sc["nodes"][0]))), res) > 80000
    assert (r["edge_d2"][:2] != R.D2_NONE).all() and (r["node_d2"] == R.D2_NONE).all()
    assert r["edge_d2"][2] == R.D2_NONE   # as long, and past the grid
    sc, r = scenes["overflow_1e9m"], refs["overflow_1e9m"]
    assert R.edge_num(1e9, sc["resolution"]) < 0 and R.edge_num(5e8, sc["resolution"]) < 0
    assert r["edge_d2"].tolist()[0] == R.D2_NONE == r["edge_d2"].tolist()[2] and r["edge_d2"][1] != R.D2_NONE
    r = refs["zero_and_self"]
    assert r["edge_d2"][0] == r["node_d2"][0] == r["edge_d2"][3] and r["edge_d2"][1] == r["node_d2"][2]
    assert r["edge_d2"][2] == R.D2_NONE == r["node_d2"][3]
    assert len(refs["no_graph"]["node_d2"]) == 0 and len(refs["no_graph"]["edge_d2"]) == 0
    assert [len(scenes[f"edges_{n}"]["edges"]) for n in (255, 256, 257)] == [255, 256, 257]
    sc = scenes["short_255_long_1"]
    lens = np.hypot(*(sc["nodes"][sc["edges"][:, 1]] - sc["nodes"][sc["edges"][:, 0]]).T)
    assert len(lens) == S.WORKGROUP and (np.sort(lens)[:255] < 0.15).all() and lens.max() > 300
    assert 2 * 1200 > S.ROUND and (refs["short_255_long_1"]["edge_d2"] != R.D2_NONE).all()
    for k in ("no_cells_0x0", "no_cells_5x0"):
        assert refs[k]["n_occupied"] == 0 and refs[k]["max_d2"] == R.D2_NONE and refs[k]["field"].size == 0
        assert (refs[k]["node_d2"] == R.D2_NONE).all() and np.isinf(refs[k]["edge_clearances"]).all()


def test_c0_known_answers(scenes, refs):
    """The C0 golden skeleton and graph (both statements of the field gave these words when the test was written)."""
    sc, r = scenes["c0"], refs["c0"]
    assert sc["grid"].shape == (512, 512) and len(sc["nodes"]) == 878 and len(sc["edges"]) == 883
    assert r["n_occupied"] == 4309 and r["max_d2"] == 43681
    assert (r["node_d2"] != R.D2_NONE).all() and (r["edge_d2"] != R.D2_NONE).all()
    assert np.isfinite(r["edge_clearances"]).all()
    assert int(r["edge_d2"].min()) == 49 and int(r["edge_d2"].max()) == 32400
    assert r["edge_clearances"].min() == np.float32(7 * float(np.float32(0.2)))     # 1.4 m
    assert r["edge_clearances"].max() == np.float32(180 * float(np.float32(0.2)))   # 36.0 m


def test_declared_and_exported():
    if not os.path.exists(aos_gpu.LIB_PATH):
        aos_gpu.build()
    lib = ctypes.CDLL(aos_gpu.LIB_PATH)
    for f in ENTRY_POINTS:
        assert f in aos_gpu.header_functions() and hasattr(lib, f), f
    assert ctypes.sizeof(aos_gpu.ClearanceOut) == 104 and aos_gpu.D2_NONE == R.D2_NONE
    for m in ("gvd_clearance", "clearance_field", "clearance_points"):
        assert callable(getattr(aos_gpu.Ctx, m))


def invalid_scenes():
    """Inputs the library must refuse with AOS_E_INVALID."""
    g = np.zeros((3, 4), np.int8)
    ok_nodes, ok_edges = [(0.0, 0.0), (0.1, 0.1)], [(0, 1)]
    bad = [S.scene(g, ok_nodes, ok_edges, resolution=r) for r in (0.0, -0.05, np.nan, np.inf)]
    for v in (np.nan, np.inf, -np.inf):
        bad.append(S.scene(g, [(0.0, 0.0), (0.1, v)], ok_edges))
    bad += [S.scene(g, ok_nodes, [(0, 2)]), S.scene(g, ok_nodes, [(-1, 1)]), S.scene(g, np.zeros((0, 2)), [(0, 0)])]
    return bad


def blob(scene_list):
    b = np.int32(len(scene_list)).tobytes()
    for sc in scene_list:
        H, W = sc["grid"].shape
        b += np.array([W, H, len(sc["nodes"]), len(sc["edges"])], np.int32).tobytes()
        b += np.array(sc["origin"], np.float64).tobytes() + np.float32(sc["resolution"]).tobytes()
        b += sc["grid"].tobytes() + sc["nodes"].tobytes() + sc["edges"].tobytes()
    return b


def parse_host_output(raw, scene_list):
    out, off = [], 0
    for sc in scene_list:
        H, W = sc["grid"].shape
        N, E = len(sc["nodes"]), len(sc["edges"])
        status = int(np.frombuffer(raw, np.int32, 1, off)[0])
        off += 4
        if status:
            out.append({"status": status})
            continue
        n_occ = int(np.frombuffer(raw, np.uint64, 1, off)[0])
        max_d2 = int(np.frombuffer(raw, np.uint32, 1, off + 8)[0])
        off += 12
        take = lambda n, dt: np.frombuffer(raw, dt, n, off).copy()  # noqa: E731
        fld = take(W * H, np.uint32).reshape(H, W); off += 4 * W * H
        nd = take(N, np.uint32); off += 4 * N
        ed = take(E, np.uint32); off += 4 * E
        nm = take(N, np.float32); off += 4 * N
        em = take(E, np.float32); off += 4 * E
        out.append({"status": 0, "n_occupied": n_occ, "max_d2": max_d2, "field": fld, "node_d2": nd, "edge_d2": ed,
                    "node_clearances": nm, "edge_clearances": em})
    assert off == len(raw)
    return out


def assert_clearance_equal(got, ref, what, with_field=True):
    assert got["n_occupied"] == ref["n_occupied"] and got["max_d2"] == ref["max_d2"], \
        f"{what}: n_occupied {got['n_occupied']} vs {ref['n_occupied']}, max_d2 {got['max_d2']} vs {ref['max_d2']}"
    keys = ("field",) * with_field + ("node_d2", "edge_d2", "node_clearances", "edge_clearances")
    for k in keys:
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k} {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            raise AssertionError(f"{what}: {k} differs in {len(bad)} places, first {bad[:4].tolist()}: " +
                                 ", ".join(f"{a[tuple(i)]!r} vs {b[tuple(i)]!r}" for i in bad[:4]))


def test_host_code_under_asan_ubsan(scenes, refs, tmp_path):
    """csrc/clearance_host.cpp as tests/clearance_host/clear_host_main.cpp (its own main, the sanitizer runtimes linked
    statically, nothing preloaded): every scene bit for bit, the refused inputs refused, no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "clear_host_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall",
                    "-I", CSRC, os.path.join(HERE, "clearance_host", "clear_host_main.cpp"),
                    os.path.join(CSRC, "clearance_host.cpp"), "-o", exe], check=True)
    names = list(scenes)
    bad = invalid_scenes()
    everything = [scenes[k] for k in names] + bad
    fi, fo = tmp_path / "in.bin", tmp_path / "out.bin"
    fi.write_bytes(blob(everything))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(fi), str(fo)], capture_output=True, text=True, env=env, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and f"clear_host_main ok {len(everything)} scenes" in r.stdout, (r.stdout, r.stderr[-2000:])
    got = parse_host_output(fo.read_bytes(), everything)
    for k, g in zip(names, got):
        assert g["status"] == 0, k
        assert_clearance_equal(g, refs[k], k)
    assert all(g["status"] == -1 for g in got[len(names):])
