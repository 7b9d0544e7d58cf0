"""The designed ROR / clip / raster scenes of tests/ror_scenes.py without a GPU: the oracle equals the independent numpy
reference on every scene (every prefix of the streamed ones), the probes observe what they should, and the predictors
show that the scenes reach the branches of csrc/ror.hip they are named for."""
import functools

import numpy as np
import pytest

import oracle_py as O
import ror_scenes as RS


@functools.lru_cache(maxsize=None)
def frames(name):
    """Per mode of the scene: (is_dense, reference, regimes, figures)."""
    sc = RS.scene(name)
    out = []
    for dense in sc.modes:
        ref = RS.reference(sc.xyz, sc.polygon, sc.akw, dense)
        reg, fig, _, _ = RS.regimes(sc.xyz, sc.polygon, sc.akw, dense, ref=ref, host=True)
        out.append((dense, ref, reg, fig))
    return out


def oracle_frame(xyz, polygon, akw, dense):
    return O.seedgen(RS.as_cloud(xyz), polygon, O.default_params(**RS.oracle_kwargs(akw)), is_dense=dense)


def assert_oracle_equals_reference(o, ref, what):
    assert (o["width"], o["height"]) == (ref["W"], ref["H"]), what
    assert np.array_equal(o["ror_keep"] != 0, ref["keep"]), what
    assert np.array_equal(o["raster"] != 0, ref["raster"]), what
    assert int(o["n_clipped"]) == ref["n_clipped"], what


def counted(sc, ref):
    return (ref["cand"] & ref["keep"])[sc.probes]


@pytest.mark.parametrize("name", RS.SCENES)
def test_oracle_equals_reference_and_probes_observe(name):
    sc = RS.scene(name)
    for dense, ref, reg, fig in frames(name):
        what = f"{name} dense={dense}"
        assert_oracle_equals_reference(oracle_frame(sc.xyz, sc.polygon, sc.akw, dense), ref, what)
        # every candidate is alone in its cell, and the candidates are probes
        c = np.flatnonzero(ref["cand"])
        cells = ref["gy"][c] * (ref["W"] + 2) + ref["gx"][c]
        assert len(np.unique(cells)) == len(cells), what
        assert set(c) <= set(int(i) for i in sc.probes), what
        if not name.startswith(("clip_faces", "disc_rims")):   # (there the clip and the discs decide: some are none)
            assert ref["cand"][sc.probes].all(), what
        assert sc.expect <= reg, (what, sorted(sc.expect - reg), fig)


@pytest.mark.parametrize("name", [n for n in RS.SCENES if not n.startswith("chunk_edges")] + list(RS.FAMILIES))
def test_a_third_kept_and_a_third_dropped(name):
    """Neither "keep all" nor "drop all" passes a scene. (need_sweep-n0 has need 1: every point keeps itself, so
    nothing can drop; the chunk_edges clouds are judged together.)"""
    for dense in (True, False):
        k = n = 0
        for member in RS.FAMILIES.get(name, [name]):
            sc = RS.scene(member)
            for d, ref, _, _ in frames(member):
                if d == dense:
                    k += int(counted(sc, ref).sum())
                    n += len(sc.probes)
        if n == 0:
            continue
        assert 3 * k >= n, (name, dense, k, n)
        if name != "need_sweep-n0":
            assert 3 * (n - k) >= n, (name, dense, k, n)


def test_radius_ties_straddle_the_thresholds():
    for r in RS.TIE_RADII:
        r2df, r2f = RS.thresholds(r)
        d2 = np.array(RS.scene(f"radius_ties-r{r}-n1").extra["d2s"], np.float32)
        assert (d2 <= r2df).any() and (d2 > r2df).any() and (d2 < r2f).any() and (d2 >= r2f).any(), r
    # r = 0.25: r2df == r2f == 0.0625 exactly, and a neighbour sits exactly there: dense keeps, non-dense drops
    d2 = np.array(RS.scene("radius_ties-r0.25-n1").extra["d2s"], np.float32)
    assert RS.thresholds(0.25) == (0.0625, 0.0625) and (d2 == np.float32(0.0625)).any()
    (_, a, _, _), (_, b, _, _) = frames("radius_ties-r0.25-n1")
    assert (a["keep"] & ~b["keep"]).any()


def test_contraction_pairs_found_both_ways():
    for name in ("contraction_pairs-dense", "contraction_pairs-sparse"):
        found = RS.scene(name).extra["found"]
        for order in ("both", "both-x", "second"):
            assert found[order] == (32, 32), (name, found)


def test_tile_edges_outside_points_are_never_neighbours():
    """ror_margin > r: a point one float outside the binned box is farther than r from every candidate."""
    for name in ("tile_edges", "tile_edges-tb16"):
        sc = RS.scene(name)
        g = RS.geometry(sc.polygon, sc.akw, len(sc.xyz))
        assert float(RS.ror_margin(sc.akw["ror_radius"])) > sc.akw["ror_radius"]
        out = ~RS.binned(sc.xyz, g)
        assert out.sum() >= 4
        ref = RS.reference(sc.xyz, sc.polygon, sc.akw, True)
        inside = RS.reference(sc.xyz[~out], sc.polygon, sc.akw, True)
        assert np.array_equal(ref["keep"][~out][inside["cand"]], inside["keep"][inside["cand"]])   # (the candidates' decisions)
        on = (sc.xyz[:, 0] == g.box[0]) | (sc.xyz[:, 0] == g.box[1]) | (sc.xyz[:, 1] == g.box[2]) | (sc.xyz[:, 1] == g.box[3])
        assert (on & ~out).sum() >= 4


def test_big_tiles_hit_their_record_counts():
    sc = RS.scene("big_tiles")
    g = RS.geometry(sc.polygon, sc.akw, len(sc.xyz))
    staged = RS.staging(sc.xyz, g)["staged"]
    assert sorted(int(v) for v in staged[staged > 1000]) == sorted(RS.BIG_TARGETS), staged
    # the same handle's second frame sizes its tiles from the binned count: the same cloud through TB 16
    assert g.TB == 32 and RS.geometry(sc.polygon, sc.akw, len(sc.xyz), est_binned=len(sc.xyz)).TB == 16


def test_fine_radius_and_wide_scan_figures():
    _, _, reg, fig = frames("fine_radius")[0]
    assert {"bin-cap", "bin-coarsen", "part-lds-64k"} <= reg and fig["ntiles"] > 16384, fig
    _, _, reg, fig = frames("wide_scan")[0]
    assert fig["row_groups"] >= 2 and fig["tile_blocks"] >= 2 and fig["binned"] > 32 * 4096, fig


def test_clip_scene_windows_on_and_off():
    wins = {("win-on" in frames(f"clip_faces_and_cells-res{res:.2f}")[0][2]) for res in RS.CELL_RES}
    assert wins == {True, False}


def test_layout_predictor():
    sc = RS.scene("layouts")
    lays = {RS.geometry(sc.polygon, sc.akw, len(sc.xyz), step=step, offs=offs, host=(what == "host")).lay
            for what, step, offs in RS.LAYOUTS}
    assert lays == {0, 1, 2}


@pytest.mark.parametrize("name", RS.STREAM_SCENES)
def test_stream_prefixes(name):
    """Every prefix of the streamed delivery: oracle == reference; a kept probe stays kept; some probe is below need in
    one prefix and kept in a later one; in the scenes of many tiles some delivery leaves a tile that holds records
    untouched. big_tiles: a tile
    fits LDS after one delivery and is big after the next, and a probe that crosses need later was below it in a tile
    that was already big (the big path carries its count)."""
    sc = RS.scene(name)
    parts = RS.stream_parts(sc)
    assert sorted(np.concatenate(parts).tolist()) == list(range(len(sc.xyz)))
    dense = True
    need = sc.akw["ror_min_neighbors"] + 1
    g = RS.geometry(sc.polygon, sc.akw, len(parts[0]))   # the store keeps the first frame's tile size
    all_s = RS.staging(sc.xyz, g)
    tile_of = np.full(len(sc.xyz), -1)
    tile_of[all_s["mask"]] = all_s["tile"]
    prev = None
    crossed = crossed_big = turned_big = missed = 0
    for k in range(len(parts)):
        idx = np.concatenate(parts[:k + 1])
        xyz = sc.xyz[idx]
        ref = RS.reference(xyz, sc.polygon, sc.akw, dense)
        assert_oracle_equals_reference(oracle_frame(xyz, sc.polygon, sc.akw, dense), ref, f"{name} prefix {k}")
        keep = np.zeros(len(sc.xyz), bool)
        keep[idx] = ref["keep"]
        below = np.zeros(len(sc.xyz), bool)
        below[idx] = ref["cand"] & (ref["counts"] < need)
        staged = RS.staging(xyz, g)["staged"]
        if prev is not None:
            assert not (prev["keep"] & ~keep).any()
            x = prev["below"] & keep
            crossed += int(x.sum())
            crossed_big += int((prev["staged"][tile_of[x]] > RS.ROR_CAP).sum())
            turned_big += int(((prev["staged"] <= RS.ROR_CAP) & (prev["staged"] > 0) & (staged > RS.ROR_CAP)).sum())
            missed += int(((prev["staged"] > 0) & (RS.staging(sc.xyz[parts[k]], g)["staged"] == 0)).sum())
        prev = dict(keep=keep, below=below, staged=staged)
    assert crossed > 0, name
    if name in ("big_tiles", "need_sweep-n6"):   # (the need_sweep blocks fill one tile or two: every delivery reaches them)
        assert missed > 0, name
    if name == "big_tiles":
        assert turned_big > 0 and crossed_big > 0, (turned_big, crossed_big)


def test_disc_rims_touch_every_disc():
    """Per disc: a scene point with dist_sq == 1 exactly, one just inside and one just outside, by the float rule."""
    sc = RS.scene("disc_rims")
    p = sc.xyz[sc.probes]
    for ex, ey, er in RS.DISCS:
        dx, dy = (p[:, 0] - ex).astype(np.float32), (p[:, 1] - ey).astype(np.float32)
        d = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
        assert (d == 1).any() and ((d < 1) & (d > 1 - 1e-4)).any() and ((d > 1) & (d < 1 + 1e-4)).any(), (ex, ey)


def test_every_regime_is_reached():
    union = set()
    for name in RS.SCENES:
        for _, _, reg, _ in frames(name):
            union |= reg
    sc = RS.scene("layouts")
    for what, step, offs in RS.LAYOUTS:
        union.add(f"LAY{RS.geometry(sc.polygon, sc.akw, len(sc.xyz), step=step, offs=offs, host=(what == 'host')).lay}")
    assert union >= RS.ALL_REGIMES, sorted(RS.ALL_REGIMES - union)


def test_handle_order_changes_tile_size_and_overflows_the_guess():
    """The one-handle sequence: the tile size follows the previous frame's binned count (32 -> 16 -> 32), and a frame
    far larger than its predecessor stages more than the earlier capacity."""
    est, last, tbs, grew = {}, {}, {}, False
    for name, dense in RS.HANDLE_ORDER:
        sc = RS.scene(name)
        key = RS.handle_key(sc)
        g = RS.geometry(sc.polygon, sc.akw, len(sc.xyz), est_binned=est.get(key), host=True)
        s = RS.staging(sc.xyz, g)
        tbs.setdefault(key, []).append(g.TB)
        total = int(s["staged"].sum())
        grew |= key in last and total > 20 * max(last[key], 1)
        last[key] = max(last.get(key, 0), total)
        est[key] = float(s["mask"].sum())
    assert any(t[:4] == [32, 32, 16, 32] for t in tbs.values()), tbs
    assert grew
