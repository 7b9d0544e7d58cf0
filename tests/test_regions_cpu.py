"""aos_gvd_regions without a GPU: the two statements of the site field (regions_ref) against each other, the components
against scipy's, the regime each designed scene (regions_scenes) was built for, d2 against clearance_ref's field, the C0
answers, the ABI declaration, and the product's host code (csrc/regions_host.cpp + csrc/regions.h) as a stand-alone
program under ASan + UBSan, word for word against the restatement on every scene."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import aos_gpu
import clearance_ref as C
import regions_ref as R
import regions_scenes as S

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "active-orchard-slam_amd", "csrc")
ENTRY_POINTS = ("aos_gvd_regions", "aos_regions_field_copy", "aos_regions_points")
BRUTE_PAIRS = 1 << 28   # cells x sites up to which a test runs the brute force
FIELDS = ("site", "region", "ridge", "ridge_d2")
COUNTS = ("n_occupied", "n_components", "n_sites", "n_regions", "n_ridge", "max_d2")
NODE_KEYS = ("node_site", "node_region", "node_d2", "node_ridge_d2", "node_ridge_offset")

_CACHE = {}


def scenes_and_refs():
    """Every scene with its reference, computed once per process (test_gpu_regions shares it)."""
    if not _CACHE:
        sc = S.all_scenes()
        _CACHE["scenes"] = sc
        _CACHE["refs"] = {k: R.regions(v) for k, v in sc.items()}
    return _CACHE["scenes"], _CACHE["refs"]


@pytest.fixture(scope="module")
def scenes():
    return scenes_and_refs()[0]


@pytest.fixture(scope="module")
def refs():
    return scenes_and_refs()[1]


def test_brute_and_separable_sites_agree(scenes, refs):
    n = 0
    for k, r in refs.items():
        s = r["is_site"]
        if s.size * max(1, int(s.sum())) > BRUTE_PAIRS:
            continue
        a, b = R.brute_site(s), R.separable_site(s)
        assert a.dtype == b.dtype == np.uint32 and np.array_equal(a, b), k
        assert np.array_equal(a, r["site"]), k
        n += 1
    assert n == len(scenes) - 2   # all but the denser 700 x 500 grid and C0


def test_hand_answers():
    sc = S.scene(S.grid_of(5, 2, [(0, 0), (4, 1)]))
    r = R.regions(sc)
    assert r["site"].tolist() == [[0, 0, 0, 9, 9], [0, 0, 9, 9, 9]]      # (2, 0): d2 4 against 5; (2, 1): 5 against 4
    assert r["region"].tolist() == r["site"].tolist() and r["d2"].tolist() == [[0, 1, 4, 2, 1], [1, 2, 4, 1, 0]]
    assert r["ridge"].tolist() == [[0, 0, 100, 0, 0], [0, 100, 0, 0, 0]]   # the pairs mark their first cell
    assert r["ridge_d2"].tolist() == [[2, 1, 0, 1, 4], [1, 0, 1, 2, 5]]   # to (2, 0) and (1, 1)
    assert (r["n_occupied"], r["n_components"], r["n_sites"], r["n_regions"], r["n_ridge"], r["max_d2"]) == (2, 2, 2, 2, 2, 4)
    # two sites side by side with different labels: both cells of the pair are site cells, nothing is marked; the
    # cells above them are split between the regions and the first cell of that pair is marked
    sc = S.with_opts(S.scene(S.grid_of(2, 2, [(0, 1), (1, 1)])), labels=[[9, 9], [4, 5]])
    r = R.regions(sc)
    assert r["region"].tolist() == [[4, 5], [4, 5]] and r["ridge"].tolist() == [[100, 0], [0, 0]]
    # a pair whose first cell is a site cell marks its second cell
    sc = S.scene(S.grid_of(3, 1, [(0, 0), (2, 0)]))
    assert R.regions(sc)["site"].tolist() == [[0, 0, 2]] and R.regions(sc)["ridge"].tolist() == [[0, 100, 0]]
    sc = S.with_opts(S.scene(S.grid_of(3, 1, [(0, 0), (1, 0)])), labels=[[1, 2, 0]])
    assert R.regions(sc)["region"].tolist() == [[1, 2, 2]] and not R.regions(sc)["ridge"].any()


def test_components_against_scipy(scenes):
    """The flood fill's partition on every scene with components, against scipy.ndimage.label (8-connectivity)."""
    from scipy import ndimage

    for k, sc in scenes.items():
        if "labels" in sc or sc["grid"].size == 0:
            continue
        lab, sizes = R.components(sc["grid"])
        ref, n = ndimage.label(R.occupied(sc["grid"]), structure=np.ones((3, 3), int))
        assert n == len(sizes), k
        occ = R.occupied(sc["grid"])
        pairs = set(zip(lab[occ].tolist(), ref[occ].tolist()))
        assert len(pairs) == n, k                                   # one flood-fill label per scipy label and back
        for root, cells in sizes.items():
            assert lab.reshape(-1)[root] == root and cells == int((lab == root).sum()), k
            assert root == int(np.flatnonzero(lab.reshape(-1) == root)[0]), k   # the label is the least index


def cell(r, key, x, y):
    return int(r[key][y, x])


def test_scene_regimes(scenes, refs):
    r = refs["one_occupied"]
    assert r["site"].tolist() == [[0]] and r["region"].tolist() == [[0]] and not r["ridge"].any()
    assert (r["ridge_d2"] == R.D2_NONE).all() and r["max_d2"] == 0
    for k in ("one_free", "empty_70x5", "no_sites_after_filter", "labels_all_negative"):
        r = refs[k]
        assert (r["site"] == R.SITE_NONE).all() and (r["region"] == R.REGION_NONE).all() and not r["ridge"].any(), k
        assert r["n_sites"] == 0 and r["max_d2"] == R.D2_NONE and np.isinf(r["node_ridge_offset"]).all(), k
    assert refs["no_sites_after_filter"]["n_occupied"] == 6 and refs["no_sites_after_filter"]["n_components"] == 3
    assert refs["w1_h130"]["n_components"] == 3 and refs["w130_h1"]["n_ridge"] == 2
    for k in ("full_65x3", "one_component"):
        assert refs[k]["n_regions"] == 1 and refs[k]["n_ridge"] == 0 and (refs[k]["ridge_d2"] == R.D2_NONE).all(), k
    for k in ("no_cells_0x0", "no_cells_5x0", "labels_no_cells_0x0"):
        assert refs[k]["site"].size == 0 and refs[k]["n_sites"] == 0 and (refs[k]["node_site"] == R.SITE_NONE).all(), k
    for n in S.SWEEP:
        for k, shape in ((f"sweep_{n}x5", (5, n)), (f"sweep_5x{n}", (n, 5))):
            assert scenes[k]["grid"].shape == shape and refs[k]["site"][-1, -1] == shape[0] * shape[1] - 1
            assert refs[k]["n_ridge"] > 0
    assert all(v in S.SWEEP for b in (S.BAND, S.WORKGROUP, S.BLOCK) for v in (b - 1, b, b + 1))
    assert max(sc["grid"].size for sc in scenes.values()) == 700 * 500
    # the tie scenes hold their ties: at least two sites at the least d2, and the least index among them wins
    for k, ((x, y), (wx, wy), d2) in S.TIES.items():
        sy, sx = np.nonzero(refs[k]["is_site"])
        d = (sx - x) ** 2 + (sy - y) ** 2
        W = scenes[k]["grid"].shape[1]
        assert d.min() == d2 and (d == d2).sum() >= 2, k
        assert cell(refs[k], "site", x, y) == wy * W + wx == int((sy * W + sx)[d == d2].min()), k
    assert S.TIES["tie_col_band"][0][1] == S.BAND and S.TIES["tie_row_blocks"][0][0] == S.BLOCK
    r = refs["tie_up_down_beside_nearer"]
    assert R.nearest_row(r["is_site"])[4, 4] == 0 and cell(r, "site", 4, 4) == 4 * 9 + 6 and cell(r, "d2", 4, 4) == 4
    for k, far_block in (("tie_strict_prune_wins", True), ("tie_strict_prune_loses", False)):
        (x, y), (wx, wy), d2 = S.TIES[k]
        bx = [c for c in np.nonzero(refs[k]["is_site"])[1].tolist() if c // S.BLOCK != x // S.BLOCK][0]
        gap = x - (bx // S.BLOCK * S.BLOCK + S.BLOCK - 1)
        col = abs(int(np.nonzero(refs[k]["is_site"][:, bx])[0][0]) - y)
        assert bx == S.BLOCK - 1 and gap * gap + col * col == d2      # the block's bound equals the best: not greater
        assert (wx == bx) == far_block
    for k in ("tie_strict_walk_end", "tie_strict_walk_end_right"):
        (x, y), (wx, wy), d2 = S.TIES[k]
        assert wx // S.BLOCK != x // S.BLOCK and (wx - x) ** 2 == d2   # the winner's block lies exactly sqrt(d2) away
    # components
    r = refs["diagonal_only"]
    assert (r["n_components"], sorted(np.unique(r["region"]).tolist())) == (2, [1 * 14 + 1, 1 * 14 + 12])
    r = refs["u_and_dot"]
    assert r["n_components"] == 2 and cell(r, "region", 2, 3) == 1 * 16 + 8 == cell(r, "region", 2, 8)
    r = refs["spiral_and_dot"]
    inner = np.argwhere(R.occupied(scenes["spiral_and_dot"]["grid"])[5:12, 5:12])
    assert r["n_components"] == 2 and len(inner) and cell(r, "region", 8, 8) == 1 * 24 + 1 == cell(r, "region", 7, 7)
    r = refs["lines_over_chunks"]
    assert r["n_occupied"] > 3 * S.CHUNK and r["n_components"] == 2 and cell(r, "region", 20, 3) == 1 * 2600 + 20
    assert int((r["region"][r["is_site"]] == 2620).sum()) == 5001 > 2 * S.CHUNK
    assert [refs[f"filter_min_{m}"]["n_regions"] for m in (3, 4, 5)] == [2, 2, 1]
    assert [refs[f"filter_min_{m}"]["n_sites"] for m in (3, 4, 5)] == [13, 13, 9]
    assert refs["filter_min_5"]["n_occupied"] == 13 and refs["filter_min_5"]["n_components"] == 2
    for k in ("filter_min_1", "filter_negative"):
        assert refs[k]["site"].tobytes() == refs["filter_min_3"]["site"].tobytes()
    # labels
    sc, r = scenes["labels_mixed"], refs["labels_mixed"]
    assert (r["n_occupied"], r["n_sites"], r["n_components"], r["n_regions"]) == (11, 9, -1, -1)
    assert sorted(np.unique(r["region"]).tolist()) == [3, 7, S.INT32_MAX]
    assert not r["is_site"][2, 15] and not r["is_site"][3, 16] and cell(r, "site", 15, 2) != 2 * 26 + 15
    assert not r["ridge"][5:7, 10:12].any() and r["ridge"][4, 10] == 100        # 4-adjacent sites mark nothing
    assert cell(r, "region", 0, 0) == 7 == cell(r, "region", 25, 12)               # one region in two pieces
    assert (sc["labels"][~R.occupied(sc["grid"])] >= 0).any() and (sc["labels"][~R.occupied(sc["grid"])] < 0).any()
    assert refs["labels_zero_everywhere"]["n_ridge"] == 0 and refs["labels_zero_everywhere"]["n_sites"] == 11
    # walls: the single free column between the walls two cells apart is marked; even and odd gaps
    r = refs["walls_vertical"]
    assert (r["ridge"][:, 14] == 100).all() and (r["ridge"][:, [4, 10]] == 100).all() and r["n_ridge"] == 3 * 12
    assert not r["ridge"][:, [3, 5, 6, 8, 9, 11, 12]].any()
    assert refs["walls_horizontal"]["ridge"].tobytes() == np.ascontiguousarray(r["ridge"].T).tobytes()
    # graphs
    sc, r = scenes["graph_nodes"], refs["graph_nodes"]
    ok, mx, my = C.cells_of(sc["nodes"][:, 0], sc["nodes"][:, 1], sc["origin"], sc["resolution"], 19, 12)
    # (the point one ulp under the grid's far corner has fx = 19.0 after the subtraction's rounding: no cell)
    assert ok.tolist() == [True] * 5 + [False] * 7 + [True] * 8
    assert (r["node_site"][~ok] == R.SITE_NONE).all() and (r["node_region"][~ok] == R.REGION_NONE).all()
    # (the even gap's pair (4, 5) marks column 4: the node in column 5 lies one cell off the ridge)
    assert r["node_ridge_d2"][12:18].tolist() == [0, 0, 0, 0, 1, 0]
    assert r["node_ridge_offset"][12:18].tolist() == [0.0, 0.0, 0.0, 0.0, S.RES, 0.0]
    assert (r["node_d2"][18:] == 0).all() and (r["node_ridge_d2"][18:] > 0).all()
    assert (mx[0], my[0], mx[3], my[3]) == (7, 2, 13, 0) and r["node_d2"][0] == 0
    assert len(refs["graph_none"]["node_site"]) == 0
    assert [len(scenes[f"graph_{n}_nodes"]["nodes"]) for n in (255, 256, 257)] == [255, 256, 257]


def test_d2_equals_the_clearance_field(scenes, refs):
    """d2 derived from site is clearance_ref's field wherever every occupied cell is a site."""
    n = 0
    for k, r in refs.items():
        if r["n_sites"] != r["n_occupied"]:
            continue
        assert r["d2"].tobytes() == C.field(scenes[k]["grid"]).tobytes(), k
        n += 1
    assert n >= len(scenes) - 8


def test_c0_known_answers(scenes, refs):
    """The C0 golden skeleton and graph (the brute force and the separable statement gave these when the test was
    written)."""
    sc, r = scenes["c0"], refs["c0"]
    assert sc["grid"].shape == (512, 512) and len(sc["nodes"]) == 878
    assert (r["n_occupied"], r["n_components"], r["n_sites"], r["n_regions"]) == (4309, 7, 4309, 7)
    assert r["n_ridge"] == 3323 and r["max_d2"] == 43681
    assert (r["node_site"] != R.SITE_NONE).all() and np.isfinite(r["node_ridge_offset"]).all()


def test_declared_and_exported():
    if not os.path.exists(aos_gpu.LIB_PATH):
        aos_gpu.build()
    lib = ctypes.CDLL(aos_gpu.LIB_PATH)
    for f in ENTRY_POINTS:
        assert f in aos_gpu.header_functions() and hasattr(lib, f), f
    assert ctypes.sizeof(aos_gpu.RegionsOut) == 176 and ctypes.sizeof(aos_gpu.RegionsOpts) == 8
    assert aos_gpu.SITE_NONE == R.SITE_NONE == 0xFFFFFFFF and aos_gpu.REGION_NONE == R.REGION_NONE == -1
    hdr = open(aos_gpu.HEADER).read()
    assert "#define AOS_SITE_NONE 0xFFFFFFFFu" in hdr and "#define AOS_REGION_NONE (-1)" in hdr
    for m in ("gvd_regions", "regions_field", "regions_points"):
        assert callable(getattr(aos_gpu.Ctx, m))


def invalid_scenes():
    """Inputs the library must refuse with AOS_E_INVALID."""
    g = np.zeros((3, 4), np.int8)
    bad = [S.scene(g, [(0.0, 0.0)], np.zeros((0, 2), np.int32), resolution=r) for r in (0.0, -0.05, np.nan, np.inf)]
    for v in (np.nan, np.inf, -np.inf):
        bad.append(S.scene(g, [(0.0, 0.0), (0.1, v)], np.zeros((0, 2), np.int32)))
    bad.append(S.with_opts(S.scene(g), labels=np.zeros((3, 4)), min_component_cells=2))
    return bad


def blob(scene_list):
    """The scenes as regions_host_main reads them (the ridge distance always wanted)."""
    b = np.int32(len(scene_list)).tobytes()
    for sc in scene_list:
        H, W = sc["grid"].shape
        has = "labels" in sc
        b += np.array([W, H, len(sc["nodes"]), int(has), sc.get("min_component_cells", 0), 1], np.int32).tobytes()
        b += np.array(sc["origin"], np.float64).tobytes() + np.float32(sc["resolution"]).tobytes()
        b += sc["grid"].tobytes() + (sc["labels"].tobytes() if has else b"") + sc["nodes"].tobytes()
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
        g = {"status": 0}
        for k, dt in (("n_occupied", np.uint64), ("n_sites", np.uint64), ("n_ridge", np.uint64), ("n_components", np.int64),
                      ("n_regions", np.int64), ("max_d2", np.uint32)):
            g[k] = int(np.frombuffer(raw, dt, 1, off)[0])
            off += np.dtype(dt).itemsize
        for k, dt in (("site", np.uint32), ("region", np.int32), ("ridge", np.int8), ("ridge_d2", np.uint32)):
            g[k] = np.frombuffer(raw, dt, W * H, off).copy().reshape(H, W)
            off += np.dtype(dt).itemsize * W * H
        for k, dt in zip(NODE_KEYS, (np.uint32, np.int32, np.uint32, np.uint32, np.float32)):
            g[k] = np.frombuffer(raw, dt, N, off).copy()
            off += 4 * N
        out.append(g)
    assert off == len(raw)
    return out


def assert_regions_equal(got, ref, what, fields=FIELDS, node_keys=NODE_KEYS):
    for k in COUNTS:
        assert got[k] == ref[k], f"{what}: {k} {got[k]} vs {ref[k]}"
    for k in tuple(fields) + tuple(node_keys):
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k} {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)
            raise AssertionError(f"{what}: {k} differs in {len(bad)} places, first {bad[:4].tolist()}: " +
                                 ", ".join(f"{a[tuple(i)]!r} vs {b[tuple(i)]!r}" for i in bad[:4]))


def test_host_code_under_asan_ubsan(scenes, refs, tmp_path):
    """csrc/regions_host.cpp as tests/regions_host/regions_host_main.cpp (its own main, the sanitizer runtimes linked
    statically, nothing preloaded): every scene word for word, the refused inputs refused, no sanitizer report."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "regions_host_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall",
                    "-I", CSRC, os.path.join(HERE, "regions_host", "regions_host_main.cpp"),
                    os.path.join(CSRC, "regions_host.cpp"), os.path.join(CSRC, "clearance_host.cpp"), "-o", exe], check=True)
    names = list(scenes)
    bad = invalid_scenes()
    everything = [scenes[k] for k in names] + bad
    fi, fo = tmp_path / "in.bin", tmp_path / "out.bin"
    fi.write_bytes(blob(everything))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(fi), str(fo)], capture_output=True, text=True, env=env, timeout=300)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and f"regions_host_main ok {len(everything)} scenes" in r.stdout, (r.stdout, r.stderr[-2000:])
    got = parse_host_output(fo.read_bytes(), everything)
    for k, g in zip(names, got):
        assert g["status"] == 0, k
        assert_regions_equal(g, refs[k], k)
    assert all(g["status"] == -1 for g in got[len(names):])
