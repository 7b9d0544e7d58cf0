"""The scenes of tests/shapes.py against the oracle, without a GPU: the injected raster is the intended pattern
exactly, each scene is in the regime its GPU test is meant for (the predictors use the library's constants: a
constant that moves shows here), and the oracle frame is quick enough for the suite."""
import re
import time
from pathlib import Path

import numpy as np
import pytest

import oracle_py as O
import shapes as S

ORACLE_SECONDS = 6.0   # generous: the slowest frame (the solid blob) took ~4 s when the scenes were chosen

CSRC = Path(__file__).resolve().parent.parent / "active-orchard-slam_amd" / "csrc"


def timed_oracle(pattern, R, polygon=None, scene=None):
    cloud, poly, _, okw = scene or S.scene(pattern, R, polygon=polygon)
    t0 = time.perf_counter()
    o = O.seedgen(cloud, poly, O.default_params(**okw))
    dt = time.perf_counter() - t0
    assert (o["width"], o["height"]) == pattern.shape[::-1]
    assert o["origin"] == (S.ORIGIN, S.ORIGIN)
    assert np.array_equal(o["raster"] != 0, pattern != 0), "the oracle's raster is not the pattern"
    assert o["n_clipped"] == 3 * np.count_nonzero(pattern)
    assert dt < ORACLE_SECONDS, f"oracle frame took {dt:.1f} s"
    return o, poly


@pytest.mark.parametrize("text,path,value", [
    (r"static const int kCclChunk = (\d+);", "cluster_seed.hip", S.CCL_CHUNK),
    (r"constexpr int kCclEdgeLds = (\d+);", "cluster_seed.hip", S.CCL_EDGE_LDS),
    (r"std::max\((\d+), nf / 4\)", "cluster_seed.hip", S.CCL_ECAP_MIN),
    (r"constexpr int kClTB = (\d+),", "cluster_seed.hip", S.CL_COUNT_TB),
    (r"kStatLds = (\d+);", "cluster_seed.hip", S.STAT_LDS),
    (r"__shared__ int cand\[(\d+)\];", "cluster_seed.hip", S.STAT_CAND),
    (r"constexpr int kRowCrossMax = (\d+);", "cluster_dev.h", S.ROW_CROSS_MAX),
    (r"#define AOS_THIN_TH (\d+)", "grid_kernels.hip", S.THIN_TH),
    (r"TWW = (\d+),", "grid_kernels.hip", S.THIN_TW // 64),
    (r"constexpr int kThinItersPerLaunch = (\d+);", "aos_internal.h", S.THIN_KIT),
])
def test_predictor_constants_match_the_library(text, path, value):
    m = re.search(text, (CSRC / path).read_text())
    assert m, f"{path}: {text} not found (the constant moved: update tests/shapes.py)"
    assert int(m.group(1)) == value


@pytest.mark.parametrize("W,H,R", S.GRID_CASES, ids=lambda v: str(v))
def test_geometry_sweep_scene(W, H, R):
    pattern = S.border_pattern(W, H, S.grid_case_seed(W, H, R))
    assert pattern[0].any() and pattern[-1].any() and pattern[:, 0].any() and pattern[:, -1].any()
    assert pattern[0, 0] and pattern[0, -1] and pattern[-1, 0] and pattern[-1, -1]
    o, _ = timed_oracle(pattern, R)
    if R == 0:
        assert np.array_equal(o["inflated"], o["raster"])


def test_geometry_sweep_covers_the_remainders():
    Ws, Hs, Rs = ({c[i] for c in S.GRID_CASES} for i in range(3))
    assert {w % 64 for w in Ws} >= {0, 1, 63} and any(w % 16 for w in Ws)
    assert {-(-w // 64) % 8 for w in Ws} >= {0, 1}
    assert {h % 128 for h in Hs} >= {0, 1, 127} and any(h % 4 for h in Hs)
    assert Rs == {0, 1, 3, 15, 63}
    assert Ws == {64, 65, 127, 193, 512, 513, 577} and Hs == {S.H_MIN, 127, 128, 129, 131, 257}


def test_blob_scene():
    o, _ = timed_oracle(S.blob_pattern(), S.BLOB["R"])
    assert S.quiet_solid_tiles(o) == [(2, 2)]
    assert o["thin_iters"] > 64
    tile = o["skeleton"][2 * S.THIN_TH:3 * S.THIN_TH, 2 * S.THIN_TW:3 * S.THIN_TW]
    assert np.count_nonzero(tile) > 0


def test_quiet_solid_tiles_guards_its_slices():
    """A grid too small for a grown 3 x 3 tile block has no such tile, solid or not."""
    assert S.quiet_solid_tiles({"opened": np.ones((3 * S.THIN_TH, 3 * S.THIN_TW), np.uint8)}) == []
    full = np.ones((3 * S.THIN_TH + 16, 3 * S.THIN_TW + 16), np.uint8)
    assert S.quiet_solid_tiles({"opened": full}) == []            # (the block would have to start at tile 0)
    full = np.ones((4 * S.THIN_TH + 8, 4 * S.THIN_TW + 8), np.uint8)
    assert S.quiet_solid_tiles({"opened": full}) == [(2, 2)]
    full[S.THIN_TH - 8, 2 * S.THIN_TW] = 0
    assert S.quiet_solid_tiles({"opened": full}) == []


def test_handle_sequence_scenes():
    K = S.THIN_KIT
    T = {}
    for name, (W, H), pattern in S.handle_frames():
        o, _ = timed_oracle(pattern, S.HANDLE_R)
        T[name] = o["thin_iters"]
    assert T["A sparse"] <= 2 * K and T["B sparse"] <= 2 * K, T
    assert T["A blob"] > 2 * K and T["B blob"] > 2 * K, T       # the two-launch first batch is outgrown


@pytest.mark.parametrize("name", list(S.CLUSTER_SCENES))
def test_cluster_scene(name):
    pattern, cloud, poly, akw, okw = S.cluster_scene(name)
    o, poly = timed_oracle(pattern, None, scene=(cloud, poly, akw, okw))
    fig = S.check_regime(name, o, poly)
    print(name, fig)
