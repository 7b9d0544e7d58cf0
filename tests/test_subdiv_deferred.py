"""Subdiv2D's deferred star (a hand-over insert leaves its star pending in the ring arrays and the next insert
retires it, subdiv2d.h) against the swap loop: two instances get the same points, one on the default path and one
forced onto OpenCV's swap loop, and their complete state (rings, end points, firstEdge, recentEdge, free lists) must
be equal, compared after every insert (same_state looks through a flushed view and leaves the star pending) and, in
a second run, only after the last insert, so that pending stars follow each other with no call in between.
Every case runs on a normal build and on a -DAOS_SD_POISON build, where each pending field holds INT_MIN and a
record read that returns it is counted: the count must stay 0.
CPU-only: subdiv2d.cpp is compiled here into throw-away libraries, as in test_subdiv_handover.py."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "active-orchard-slam_amd", "csrc", "subdiv2d.cpp")

SHIM = r"""
#include "subdiv2d.h"
#include <cstring>
#include <vector>
using aos::Subdiv2D;
static long poison() {
#ifdef AOS_SD_POISON
    return aos::sd_poison_reads;
#else
    return 0;
#endif
}
// st: inserts that returned true, n_handover, n_cavity, n_loop, n_ho_bail, n_deferred, n_ho_pocket, poison reads,
// inserts after which the star was pending
static void count(const Subdiv2D& a, bool ok, long* st) {
    st[0] += ok;
    st[1] = a.n_handover; st[2] = a.n_cavity; st[3] = a.n_loop; st[4] = a.n_ho_bail; st[5] = a.n_deferred;
    st[6] = a.n_ho_pocket; st[7] = poison(); st[8] += a.star_pending();
}
static bool feed(Subdiv2D& a, Subdiv2D& r, const double* s, int i, bool compare, long* st) {
    const float x = (float)s[2 * i], y = (float)s[2 * i + 1];
    const bool ka = a.insert(x, y), kr = r.insert(x, y);
    if (ka != kr || (compare && !a.same_state(r))) return false;
    count(a, ka, st);
    return true;
}
// -1: equal at every comparison (after every insert, or with every = 0 after the last one only); else the insert's index
extern "C" int df_check(const double* s, int n, float rx, float ry, float rw, float rh, int deferred, int every, long* st) {
    Subdiv2D a, r;
    a.set_deferred(deferred != 0);
    r.set_swap_loop(true);
    a.init_delaunay(rx, ry, rw, rh, 0); r.init_delaunay(rx, ry, rw, rh, 0);
    for (int i = 0; i < 16; ++i) st[i] = 0;
    for (int i = 0; i < n; ++i)
        if (!feed(a, r, s, i, every || i + 1 == n, st)) return i;
    return -1;
}
// the exports straight after the last insert, with no call in between. 0: equal; 1: the star was not pending (the
// case does not test what it should); 2: raw_into bytes differ; 3: voronoi_edges differ; 4: state differs afterwards
extern "C" int df_export(const double* s, int n, float rx, float ry, float rw, float rh, long* st) {
    Subdiv2D a, r;
    r.set_swap_loop(true);
    a.init_delaunay(rx, ry, rw, rh, 0); r.init_delaunay(rx, ry, rw, rh, 0);
    for (int i = 0; i < 16; ++i) st[i] = 0;
    for (int i = 0; i < n; ++i)
        if (!feed(a, r, s, i, false, st)) return 4;
    if (!a.star_pending()) return 1;
    const Subdiv2D& ca = a;
    std::vector<char> ba(ca.raw_bytes()), br(r.raw_bytes());
    ca.raw_into(ba.data()); r.raw_into(br.data());
    if (ba.size() != br.size() || memcmp(ba.data(), br.data(), ba.size())) return 2;
    Subdiv2D a2, r2;   // (voronoi_edges creates the virtual vertices: a fresh pair)
    r2.set_swap_loop(true);
    a2.init_delaunay(rx, ry, rw, rh, 0); r2.init_delaunay(rx, ry, rw, rh, 0);
    for (int i = 0; i < n; ++i)
        if (!feed(a2, r2, s, i, false, st + 16)) return 4;
    if (!a2.star_pending()) return 1;
    std::vector<float> ea, er;
    a2.voronoi_edges(ea); r2.voronoi_edges(er);
    if (ea.size() != er.size() || memcmp(ea.data(), er.data(), 4 * ea.size())) return 3;
    st[7] = poison();
    return a.same_state(r) && a2.same_state(r2) ? 0 : 4;
}
// init_delaunay on an instance whose star is pending, then a second point set. -1 equal; -2 the star was not pending
extern "C" int df_reinit(const double* s1, int n1, const double* s2, int n2, float rx, float ry, float rw, float rh, long* st) {
    Subdiv2D a, r;
    r.set_swap_loop(true);
    a.init_delaunay(rx, ry, rw, rh, 0);
    for (int i = 0; i < 16; ++i) st[i] = 0;
    for (int i = 0; i < n1; ++i) a.insert((float)s1[2 * i], (float)s1[2 * i + 1]);
    if (!a.star_pending()) return -2;
    a.init_delaunay(rx, ry, rw, rh, 0); r.init_delaunay(rx, ry, rw, rh, 0);
    if (a.star_pending() || !a.same_state(r)) return 0;
    for (int i = 0; i < n2; ++i)
        if (!feed(a, r, s2, i, true, st)) return i;
    return -1;
}
// a copy of an instance with a pending star, continued with its own points beside the original. -1 equal; -2 the
// star was not pending at the copy; else 2 * index + (0 original, 1 copy)
extern "C" int df_copy(const double* s, int n, int split, const double* sb, int nb, float rx, float ry, float rw, float rh,
                       int every, long* st) {
    Subdiv2D a, r;
    r.set_swap_loop(true);
    a.init_delaunay(rx, ry, rw, rh, 0); r.init_delaunay(rx, ry, rw, rh, 0);
    for (int i = 0; i < 32; ++i) st[i] = 0;
    for (int i = 0; i < split; ++i)
        if (!feed(a, r, s, i, false, st)) return 2 * i;
    if (!a.star_pending()) return -2;
    Subdiv2D b(a), rb(r);
    if (!b.star_pending()) return -2;
    for (int i = 0; split + i < n || i < nb; ++i) {
        if (split + i < n && !feed(a, r, s, split + i, every || split + i + 1 == n, st)) return 2 * (split + i);
        if (i < nb && !feed(b, rb, sb, i, every || i + 1 == nb, st + 16)) return 2 * i + 1;
    }
    return -1;
}
// two instances fed alternately (set 1, set 2, set 1, ...), each against a swap-loop instance of its own
extern "C" int df_check2(const double* s1, int n1, const double* s2, int n2, float rx, float ry, float rw, float rh, int every,
                         long* st) {
    Subdiv2D a[2], r[2];
    const double* s[2] = {s1, s2};
    const int n[2] = {n1, n2};
    for (int k = 0; k < 2; ++k) {
        r[k].set_swap_loop(true);
        a[k].init_delaunay(rx, ry, rw, rh, 0); r[k].init_delaunay(rx, ry, rw, rh, 0);
    }
    for (int i = 0; i < 32; ++i) st[i] = 0;
    for (int i = 0; i < n1 || i < n2; ++i)
        for (int k = 0; k < 2; ++k)
            if (i < n[k] && !feed(a[k], r[k], s[k], i, every || i + 1 == n[k], st + 16 * k)) return 2 * i + k;
    return -1;
}
extern "C" int df_available() { return Subdiv2D::simd_ok() ? 1 : 0; }
"""

_libs = {}
F4 = [ctypes.c_float] * 4
P, I = ctypes.c_void_p, ctypes.c_int


def shim(mode):
    if mode not in _libs:
        d = tempfile.mkdtemp(prefix=f"subdiv_df_shim_{mode}_")
        src = os.path.join(d, "shim.cpp")
        open(src, "w").write(SHIM)
        so = os.path.join(d, "libshim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared"]
                              + (["-DAOS_SD_POISON"] if mode == "poison" else [])
                              + ["-I", os.path.dirname(SRC), "-o", so, src, SRC])
        lib = ctypes.CDLL(so)
        for name, args in (("df_check", [P, I] + F4 + [I, I, P]), ("df_export", [P, I] + F4 + [P]),
                           ("df_reinit", [P, I, P, I] + F4 + [P]), ("df_copy", [P, I, I, P, I] + F4 + [I, P]),
                           ("df_check2", [P, I, P, I] + F4 + [I, P])):
            getattr(lib, name).restype = I
            getattr(lib, name).argtypes = args
        assert lib.df_available() == 1, "the deferred star needs the hand-over, which needs AVX2 (every supported host has it)"
        _libs[mode] = lib
    return _libs[mode]


MODES = ["normal", "poison"]
RECT = (-5.0, -5.0, 60.0, 40.0)   # x, y, w, h: every point set below lies inside it, but for the ones meant not to

STAT = ("inserted", "n_handover", "n_cavity", "n_loop", "n_ho_bail", "n_deferred", "n_ho_pocket", "poison_reads",
        "pending_after")


def flat(pts):
    return np.ascontiguousarray(pts, np.float64).reshape(-1)


def stats(st, at=0):
    return dict(zip(STAT, (int(v) for v in st[at:at + len(STAT)])))


def check(mode, pts, deferred=1):
    """pts through a default-path instance and a swap-loop instance, compared after every insert and then, in a
    fresh pair, after the last insert only; returns the second run's counters."""
    s = flat(pts)
    st = np.zeros(16, np.int64)
    for every in (1, 0):
        bad = shim(mode).df_check(s.ctypes.data, s.size // 2, *RECT, deferred, every, st.ctypes.data)
        assert bad == -1, f"state differs from the swap loop's after insert {bad} of {s.size // 2} (every={every})"
        assert st[7] == 0, f"{st[7]} record reads returned a pending field (every={every})"
    return stats(st)


def rows(n_rows, n, order, seed=0, jitter=0.02, dx=1.1, dy=2.3):
    """n_rows tree lines of n points, inserted row by row: order 0 left to right, 1 right to left, 2 alternating."""
    rng = np.random.default_rng(1000 * seed + 10 * n_rows + n)
    out = []
    for r in range(n_rows):
        x = np.arange(n) * dx + rng.uniform(-jitter, jitter, n)
        y = r * dy + rng.uniform(-jitter, jitter, n)
        row = np.stack([x, y], -1)
        if order == 1 or (order == 2 and r % 2 == 1):
            row = row[::-1]
        out.append(row)
    return np.concatenate(out)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("n_rows", [2, 3, 5])
@pytest.mark.parametrize("n", [3, 4, 5, 7, 13, 40])
def test_rows_equal_swap_loop(n, n_rows, order, mode):
    """Jittered rows have no duplicate and no point on an edge, so every insert is a cavity insert, and every cavity
    insert that does not bail out leaves its star pending: most row inserts, and with the switch off none."""
    pts = rows(n_rows, n, order)
    st = check(mode, pts)
    assert st["inserted"] == n_rows * n
    assert st["n_deferred"] > 0.8 * st["inserted"], st
    assert st["pending_after"] == st["n_deferred"]
    off = check(mode, pts, deferred=0)
    assert off["n_deferred"] == 0 and off["pending_after"] == 0 and off["inserted"] == n_rows * n
    assert off["n_handover"] > 0


@pytest.mark.parametrize("mode", MODES)
def test_duplicate_between_fan_inserts(mode):
    pts = rows(3, 20, 2)
    rep = []
    for i, p in enumerate(pts):
        rep.append(p)
        if i % 5 == 2:
            rep.extend([p, p])          # located as an existing vertex (loc = 1): the star is flushed, nothing is inserted
    st = check(mode, np.array(rep))
    assert st["inserted"] == len(rep)   # insert() returns true for an existing vertex
    assert st["n_cavity"] + st["n_loop"] == len(pts)
    assert st["n_deferred"] > 0.8 * len(pts) and st["n_handover"] > 0.5 * len(pts)


@pytest.mark.parametrize("mode", MODES)
def test_point_on_a_spoke_between_fan_inserts(mode):
    """Exactly collinear rows in the order 0, 2, 1, 4, 3, ...: point i - 1 falls on the spoke from i - 2 to the just
    inserted i (loc = 2: flush, delete the edge, swap loop), and the next point is a fan insert again."""
    out = []
    for r in range(3):
        idx = [0]
        for i in range(2, 24, 2):
            idx += [i, i - 1]
        out.append(np.stack([np.array(idx) * 0.5, np.full(len(idx), r * 2.0)], -1))
    pts = np.concatenate(out)
    st = check(mode, pts)
    assert st["inserted"] == len(pts)
    assert st["n_loop"] >= 20 and st["n_handover"] > 0 and st["n_deferred"] > 0


@pytest.mark.parametrize("mode", MODES)
def test_point_outside_the_rectangle_between_fan_inserts(mode):
    pts = rows(3, 20, 0)
    pts = np.insert(pts, [25, 26, 47], [[500.0, 3.0], [-100.0, -100.0], [7.0, 1000.0]], axis=0)
    st = check(mode, pts)
    assert st["inserted"] == len(pts) - 3
    assert st["n_deferred"] > 0.8 * len(pts)
    assert st["pending_after"] >= st["n_deferred"] + 3   # the rejected points leave the star pending


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [7, 61, 120])
def test_export_straight_after_a_deferred_insert(n, mode):
    s = flat(rows(3, 40, 2)[:n])
    st = np.zeros(32, np.int64)
    rc = shim(mode).df_export(s.ctypes.data, n, *RECT, st.ctypes.data)
    assert rc == 0, {1: "the star was not pending before the export", 2: "raw_into bytes differ",
                     3: "voronoi_edges differ", 4: "state differs"}[rc]
    assert st[7] == 0


@pytest.mark.parametrize("mode", MODES)
def test_init_delaunay_drops_a_pending_star(mode):
    s1, s2 = flat(rows(3, 20, 2)), flat(rows(4, 13, 1, seed=3, dx=0.8, dy=1.7) + np.array([2.0, 1.0]))
    st = np.zeros(16, np.int64)
    bad = shim(mode).df_reinit(s1.ctypes.data, s1.size // 2, s2.ctypes.data, s2.size // 2, *RECT, st.ctypes.data)
    assert bad != -2, "the star was not pending at init_delaunay"
    assert bad == -1, f"state differs after insert {bad} of the second set"
    st = stats(st)
    assert st["inserted"] == s2.size // 2 and st["poison_reads"] == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("every", [1, 0])
def test_copy_of_a_pending_instance(every, mode):
    a = rows(4, 20, 2, seed=1)
    b = rows(3, 13, 0, seed=2, dx=0.9, dy=1.3) + np.array([25.0, 10.0])   # the copy goes on elsewhere
    sa, sb = flat(a), flat(b)
    st = np.zeros(32, np.int64)
    bad = shim(mode).df_copy(sa.ctypes.data, len(a), 31, sb.ctypes.data, len(b), *RECT, every, st.ctypes.data)
    assert bad != -2, "the star was not pending at the copy"
    assert bad == -1, f"state differs after insert {bad // 2} of {'the copy' if bad % 2 else 'the original'}"
    assert stats(st)["inserted"] == len(a) and stats(st, 16)["inserted"] == len(b)
    assert stats(st, 16)["poison_reads"] == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("every", [1, 0])
def test_two_instances_fed_alternately(every, mode):
    a, b = rows(3, 40, 2, seed=1), rows(5, 13, 1, seed=2, dx=0.7, dy=1.9) + np.array([3.0, 1.0])
    s1, s2 = flat(a), flat(b)
    st = np.zeros(32, np.int64)
    bad = shim(mode).df_check2(s1.ctypes.data, len(a), s2.ctypes.data, len(b), *RECT, every, st.ctypes.data)
    assert bad == -1, f"state differs after alternating insert {bad}"
    s0, s1_ = stats(st), stats(st, 16)
    assert s0["inserted"] == len(a) and s1_["inserted"] == len(b)
    assert s0["n_deferred"] > 0.8 * len(a) and s1_["n_deferred"] > 0.8 * len(b)
    assert s1_["poison_reads"] == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mirror", [False, True])
def test_pocket_of_a_non_convex_star(mirror, mode):
    """X lies inside the triangle A, B, c, so after c's insert it has degree 3 and is a reflex vertex of c's star:
    the triangle right of the link edge between X and A has the ring vertex B as apex. c is outside the circle
    through A, X, B (centre (5, -5.25), radius 7.25), so the star is Delaunay; p lies in the fan triangle X, A, c
    and inside that circle, so its root link edge swaps onto B while c's star is pending."""
    A, X, B, c, p = (0.0, 0.0), (5.0, 2.0), (10.0, 0.0), (5.0, 6.0), (4.5, 1.9)
    pts = np.array([A, X, B, c, p])
    if mirror:
        pts[:, 0] = 10.0 - pts[:, 0]
    pts = np.concatenate([pts, rows(2, 6, 0) + np.array([20.0, 12.0])])   # and on with ordinary fan inserts
    st = check(mode, pts)
    assert st["inserted"] == len(pts)
    assert st["n_ho_pocket"] >= 1, st
