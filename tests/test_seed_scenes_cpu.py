"""The designed skeletons of tests/seed_scenes.py without a GPU: the numpy reference of the row, ray and seed stage equals
the oracle bit for bit on every scene, every scene reaches the regime it is named for (asserted on the oracle's rows
and the reference's classification alone, with the library's constants: one that moves shows here), and the oracle
frames are quick enough for the suite."""
import re
from pathlib import Path

import numpy as np
import pytest

import seed_scenes as SS

ORACLE_SECONDS = 5.0   # generous: the slowest frame took ~0.05 s when the scenes were chosen
MAX_CELLS = 1 << 20
MAX_CLUSTER = 400      # cells: the oracle's length loop is quadratic

CSRC = Path(__file__).resolve().parent.parent / "active-orchard-slam_amd" / "csrc"


@pytest.mark.parametrize("text,path,value", [
    (r"constexpr int kLook = (\d+);", "cluster_seed.hip", SS.K_LOOK),
    (r"constexpr int kRayBatch = (\d+);", "cluster_seed.hip", SS.RAY_BATCH),
    (r"base \+= (\d+) \* kRayBatch\)", "cluster_seed.hip", SS.RAY_TRIP // SS.RAY_BATCH),
    (r"constexpr int kSmallMax = (\d+);", "cluster_seed.h", SS.SMALL_MAX),
    (r"kSmallBuckets = (\d+);", "greedy.hip", SS.SMALL_BUCKETS),
    (r"constexpr int kLfTB = (\d+),", "greedy.hip", SS.LF_TB),
    (r"hx0 = g\.minx - (\d+)\.0, hx1 = g\.maxx \+ \1\.0, hy0 = g\.miny - \1\.0, hy1 = g\.maxy \+ \1\.0;",
     "cluster_seed.hip", int(SS.HASH_PAD)),
    (r"if \((\d+) \* nr <= kSmallMax\)", "cluster_seed.hip", 6),
    (r"const int max_steps = \(int\)\(maxd / step\);\s+double cx = sx, cy = sy;\s+for \(int i0 = (\d+); i0 < max_steps; "
     r"i0 \+= kLook\)", "cluster_seed.hip", 0),
    (r"for \(double cur = (\d+)\.0;; cur \+= 0\.1\) \{ t\.push_back\(cur\); if \(!\(cur <= g\.amax\)\) break; \}",
     "cluster_seed.hip", 1),
    (r"c \*= (\d+)\.25;", "greedy.hip", 1),
])
def test_predictor_constants_match_the_library(text, path, value):
    m = re.search(text, (CSRC / path).read_text())
    assert m, f"{path}: {text} not found (the rule moved: update tests/seed_scenes.py)"
    assert int(m.group(1)) == value


def test_first_come_rule_on_a_line_of_points():
    """0.25 m apart: each conflicts with its neighbours only (0.5 is not below 0.5), alternate ones are kept."""
    c = np.array([(0.25 * i, 0.0) for i in range(9)])
    lst = SS._listing(c, [True] * 9)
    assert lst["kept"].tolist() == [True, False] * 4 + [True]
    assert lst["by"].tolist() == [-1, 0, -1, 2, -1, 4, -1, 6, -1]
    assert SS.longest_chain(lst) == 9
    assert SS.tie_pairs(lst) == (4, 0.25)
    # a candidate that is not admissible neither joins the list nor drops anything
    lst = SS._listing(c, [False] + [True] * 8)
    assert lst["kept"].tolist() == [False, True, False] + [True, False] * 3
    assert SS.blocked_then_kept(lst) == 1
    # one double below 0.5 m is dropped, 0.5 m is kept
    lst = SS._listing([(0.0, 0.0), (np.nextafter(0.5, 0.0), 0.0), (0.0, 0.5)], [True] * 3)
    assert lst["kept"].tolist() == [True, False, True]


def test_zero_runs():
    assert SS.zero_runs(np.array([0, 0, 2, 0, 1, 0, 0, 0, 3, 0])) == ([1, 3], True, True)
    assert SS.zero_runs(np.array([1, 0, 1])) == ([1], False, False)
    assert SS.zero_runs(np.array([0, 0])) == ([], True, True)


def test_resolutions_against_the_batch():
    assert [SS.max_steps(r) for r in (0.15625, 0.25, 0.3125, 0.5)] == [51, 32, 25, 16]


@pytest.mark.parametrize("name", list(SS.SCENES))
def test_scene(name):
    """The reference equals the oracle and the regime holds (both asserted in oracle_frame); the frame is small."""
    f, o, ref, fig, og, dt = SS.oracle_frame(name)
    print(name, f"{o['width']} x {o['height']}, oracle {dt:.2f} s", fig)
    assert dt < ORACLE_SECONDS, f"oracle frame took {dt:.1f} s"
    assert o["width"] * o["height"] < MAX_CELLS
    assert np.diff(o["cluster_offsets"]).max() <= MAX_CLUSTER
    # the reference's own bookkeeping: whoever dropped a candidate is an earlier kept one within 0.5 m
    for lst in (ref["virtual"], ref["ray"], ref["endpoint"]):
        dropped = np.nonzero(lst["by"] >= 0)[0]
        by = lst["by"][dropped]
        assert (by < dropped).all() and lst["kept"][by].all() and lst["ok"][dropped].all()
        d = lst["cand"][by] - lst["cand"][dropped]
        assert (np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) < 0.5).all()
        assert not (lst["kept"] & ~lst["ok"]).any()
    assert len(ref["ray"]["cand"]) == 6 * len(o["row_length"]) and len(ref["endpoint"]["cand"]) == 2 * len(o["row_length"])
    assert len(ref["virtual"]["cand"]) == SS.n_slots(ref)
    assert not (ref["ray"]["cls"] == SS.MISS).any()      # amax is three grid diagonals: every ray leaves the grid first
    g = ref["grid"]                                      # the distance table stops at the first value above amax
    assert g.cur[0] == 1.0 and g.cur[-1] <= g.amax < g.cur[-1] + 0.1


def test_the_sequence_rebuilds_and_shortens_the_distance_table():
    """The one-handle sequence of test_gpu_seed_scenes.py: the grid diagonal (cur_tab's key) changes at every step, the
    table grows, shrinks and grows again, and so do the candidate buffers."""
    lens = [SS.cur_tab_len(SS.oracle_frame(n)[2]["grid"]) for n in SS.HANDLE_ORDER]
    amax = [SS.oracle_frame(n)[2]["grid"].amax for n in SS.HANDLE_ORDER]
    cands = [SS.n_slots(SS.oracle_frame(n)[2]) + 8 * len(SS.oracle_frame(n)[1]["row_length"]) for n in SS.HANDLE_ORDER]
    print(lens, cands)
    assert lens == [20664, 3598, 1781, 20664] and cands == [7502, 593, 256, 7502]      # the figures DESIGN.md names
    assert all(a != b for a, b in zip(amax, amax[1:]))
    assert lens[0] > lens[1] > lens[2] < lens[3] and lens[3] == lens[0]
    assert cands[0] == cands[3] > 10 * max(cands[1], cands[2])
    assert SS.n_slots(SS.oracle_frame(SS.HANDLE_ORDER[2])[2]) == 0


def test_shapes_scene_res_keyword_keeps_the_default():
    import shapes as S
    p = S.border_pattern(65, 41, 7)
    a, b = S.scene(p, 1), S.scene(p, 1, res=S.RES)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    for res, m in ((0.15625, 16), (0.3125, 8), (0.5, 5)):
        assert S.margin_cells(res) == m
    with pytest.raises(ValueError):
        S.margin_cells(0.3)
