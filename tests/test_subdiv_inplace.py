"""Subdiv2D's in-place hand-over (a hand-over insert builds its ring in the window of the previous ring and copies only
the ends, subdiv2d.h) against the swap loop and against the copying walk: three instances get the same points, one on
the default path, one with set_inplace(false) and one forced onto OpenCV's swap loop, and the complete state (rings,
end points, firstEdge, recentEdge, free lists) of the first two must equal the third's, compared after every insert
and, in a second run, only after the last insert.
Every case runs on a normal build and on a -DAOS_SD_POISON build, where each pending field holds INT_MIN and a record
read that returns it is counted: the count must stay 0.
CPU-only: subdiv2d.cpp is compiled here into throw-away libraries, as in test_subdiv_deferred.py."""
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
// st: inserts that returned true, n_handover, n_inplace, n_ip_fallback, n_rebase, n_ip_seam, n_ip_unwrap, n_ho_pocket,
// poison reads, n_loop, n_cavity, in-place inserts of the instance with the switch off, n_ho_bail
static void count(const Subdiv2D& a, const Subdiv2D& b, bool ok, long* st) {
    st[0] += ok;
    st[1] = a.n_handover; st[2] = a.n_inplace; st[3] = a.n_ip_fallback; st[4] = a.n_rebase; st[5] = a.n_ip_seam;
    st[6] = a.n_ip_unwrap; st[7] = a.n_ho_pocket; st[8] = poison(); st[9] = a.n_loop; st[10] = a.n_cavity;
    st[11] = b.n_inplace; st[12] = a.n_ho_bail;
}
// a: in place, b: the copying walk, r: the swap loop
struct Trio {
    Subdiv2D a, b, r;
    Trio(float rx, float ry, float rw, float rh, int slack = 0, int seam_copy = 1) {
        b.set_inplace(false);
        r.set_swap_loop(true);
        if (slack > 0) { a.set_ring_slack(slack); b.set_ring_slack(slack); }
        a.set_seam_copy(seam_copy != 0);
        a.init_delaunay(rx, ry, rw, rh, 0); b.init_delaunay(rx, ry, rw, rh, 0); r.init_delaunay(rx, ry, rw, rh, 0);
    }
    bool feed(const double* s, int i, bool compare, long* st) {
        const float x = (float)s[2 * i], y = (float)s[2 * i + 1];
        const bool ka = a.insert(x, y), kb = b.insert(x, y), kr = r.insert(x, y);
        if (ka != kr || kb != kr || (compare && !(a.same_state(r) && b.same_state(r)))) return false;
        count(a, b, ka, st);
        return true;
    }
};
// -1: equal at every comparison (after every insert, or with every = 0 after the last one only); else the insert's index
extern "C" int ip_check(const double* s, int n, float rx, float ry, float rw, float rh, int every, int slack, int seam_copy,
                        long* st) {
    Trio t(rx, ry, rw, rh, slack, seam_copy);
    for (int i = 0; i < 16; ++i) st[i] = 0;
    for (int i = 0; i < n; ++i)
        if (!t.feed(s, i, every || i + 1 == n, st)) return i;
    return -1;
}
// the exports straight after the last insert, with no call in between. 0: equal; 1: the last insert was not in place
// (the case does not test what it should); 2: raw_into bytes differ; 3: voronoi_edges differ; 4: state differs
extern "C" int ip_export(const double* s, int n, float rx, float ry, float rw, float rh, long* st) {
    for (int i = 0; i < 16; ++i) st[i] = 0;
    for (int form = 0; form < 2; ++form) {   // (voronoi_edges creates the virtual vertices: a fresh trio)
        Trio t(rx, ry, rw, rh);
        long before = 0;
        for (int i = 0; i < n; ++i) {
            before = t.a.n_inplace;
            if (!t.feed(s, i, false, st)) return 4;
        }
        if (t.a.n_inplace != before + 1 || !t.a.star_pending()) return 1;
        if (form == 0) {
            const Subdiv2D& ca = t.a;
            std::vector<char> ba(ca.raw_bytes()), br(t.r.raw_bytes());
            ca.raw_into(ba.data()); t.r.raw_into(br.data());
            if (ba.size() != br.size() || memcmp(ba.data(), br.data(), ba.size())) return 2;
        } else {
            std::vector<float> ea, er;
            t.a.voronoi_edges(ea); t.r.voronoi_edges(er);
            if (ea.size() != er.size() || memcmp(ea.data(), er.data(), 4 * ea.size())) return 3;
        }
        if (!t.a.same_state(t.r)) return 4;
    }
    st[8] = poison();
    return 0;
}
// init_delaunay straight after an in-place insert, then a second point set. -1 equal; -2 the last insert was not in place
extern "C" int ip_reinit(const double* s1, int n1, const double* s2, int n2, float rx, float ry, float rw, float rh, long* st) {
    Trio t(rx, ry, rw, rh);
    for (int i = 0; i < 16; ++i) st[i] = 0;
    long before = 0;
    for (int i = 0; i < n1; ++i) { before = t.a.n_inplace; t.a.insert((float)s1[2 * i], (float)s1[2 * i + 1]); }
    if (t.a.n_inplace != before + 1) return -2;
    t.a.init_delaunay(rx, ry, rw, rh, 0);
    if (t.a.star_pending() || !t.a.same_state(t.r)) return 0;
    for (int i = 0; i < n2; ++i)
        if (!t.feed(s2, i, true, st)) return i;
    return -1;
}
// a copy of an instance straight after an in-place insert, continued with its own points beside the original. -1 equal;
// -2 the insert before the copy was not in place; else 2 * index + (0 original, 1 copy)
extern "C" int ip_copy(const double* s, int n, int split, const double* sb, int nb, float rx, float ry, float rw, float rh,
                       int every, long* st) {
    Trio t(rx, ry, rw, rh);
    for (int i = 0; i < 32; ++i) st[i] = 0;
    long before = 0;
    for (int i = 0; i < split; ++i) {
        before = t.a.n_inplace;
        if (!t.feed(s, i, false, st)) return 2 * i;
    }
    if (t.a.n_inplace != before + 1) return -2;
    Trio u(t);
    for (int i = 0; split + i < n || i < nb; ++i) {
        if (split + i < n && !t.feed(s, split + i, every || split + i + 1 == n, st)) return 2 * (split + i);
        if (i < nb && !u.feed(sb, i, every || i + 1 == nb, st + 16)) return 2 * i + 1;
    }
    return -1;
}
// two trios fed alternately (set 1, set 2, set 1, ...)
extern "C" int ip_check2(const double* s1, int n1, const double* s2, int n2, float rx, float ry, float rw, float rh, int every,
                         long* st) {
    Trio t[2] = {Trio(rx, ry, rw, rh), Trio(rx, ry, rw, rh)};
    const double* s[2] = {s1, s2};
    const int n[2] = {n1, n2};
    for (int i = 0; i < 32; ++i) st[i] = 0;
    for (int i = 0; i < n1 || i < n2; ++i)
        for (int k = 0; k < 2; ++k)
            if (i < n[k] && !t[k].feed(s[k], i, every || i + 1 == n[k], st + 16 * k)) return 2 * i + k;
    return -1;
}
extern "C" int ip_available() { return Subdiv2D::simd_ok() ? 1 : 0; }
"""

_libs = {}
F4 = [ctypes.c_float] * 4
P, I = ctypes.c_void_p, ctypes.c_int


def shim(mode):
    if mode not in _libs:
        d = tempfile.mkdtemp(prefix=f"subdiv_ip_shim_{mode}_")
        src = os.path.join(d, "shim.cpp")
        open(src, "w").write(SHIM)
        so = os.path.join(d, "libshim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared"]
                              + (["-DAOS_SD_POISON"] if mode == "poison" else [])
                              + ["-I", os.path.dirname(SRC), "-o", so, src, SRC])
        lib = ctypes.CDLL(so)
        for name, args in (("ip_check", [P, I] + F4 + [I, I, I, P]), ("ip_export", [P, I] + F4 + [P]),
                           ("ip_reinit", [P, I, P, I] + F4 + [P]), ("ip_copy", [P, I, I, P, I] + F4 + [I, P]),
                           ("ip_check2", [P, I, P, I] + F4 + [I, P])):
            getattr(lib, name).restype = I
            getattr(lib, name).argtypes = args
        assert lib.ip_available() == 1, "the in-place hand-over needs the hand-over, which needs AVX2 (every supported host has it)"
        _libs[mode] = lib
    return _libs[mode]


MODES = ["normal", "poison"]
RECT = (-5.0, -5.0, 60.0, 40.0)   # x, y, w, h: every point set below lies inside it, but for the ones meant not to

STAT = ("inserted", "n_handover", "n_inplace", "n_ip_fallback", "n_rebase", "n_ip_seam", "n_ip_unwrap", "n_ho_pocket",
        "poison_reads", "n_loop", "n_cavity", "inplace_with_switch_off", "n_ho_bail")


def flat(pts):
    return np.ascontiguousarray(pts, np.float64).reshape(-1)


def stats(st, at=0):
    d = dict(zip(STAT, (int(v) for v in st[at:at + len(STAT)])))
    d["interior"] = d["n_ip_fallback"] - d["n_rebase"] - d["n_ip_seam"]   # redone because of where the swapped links lay
    return d


def check(mode, pts, slack=0, seam_copy=1):
    """pts through the three instances, compared after every insert and then, in a fresh trio, after the last insert
    only; returns the second run's counters."""
    s = flat(pts)
    st = np.zeros(16, np.int64)
    for every in (1, 0):
        bad = shim(mode).ip_check(s.ctypes.data, s.size // 2, *RECT, every, slack, seam_copy, st.ctypes.data)
        assert bad == -1, f"state differs from the swap loop's after insert {bad} of {s.size // 2} (every={every})"
        assert st[8] == 0, f"{st[8]} record reads returned a pending field (every={every})"
        assert st[11] == 0, "inserts ran in place with set_inplace(false)"
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
    """Jittered rows: every insert is a cavity insert, and from the second row on nearly every one is a hand-over
    insert, which runs in place unless it has to be redone by the copying walk."""
    st = check(mode, rows(n_rows, n, order))
    assert st["inserted"] == n_rows * n
    # every hand-over insert was tried in place; one redone by the copying walk may still bail out there
    assert st["n_handover"] <= st["n_inplace"] + st["n_ip_fallback"] <= st["n_handover"] + st["n_ho_bail"] + st["n_ho_pocket"]
    if n >= 7:
        assert st["n_inplace"] > 0.8 * st["n_handover"] > 0, st


@pytest.mark.parametrize("mode", MODES)
def test_seam_inside_the_kept_run(mode):
    """A ring the copying walk left starts at whichever root the walk began with, so the next insert's chains often
    cross the window's seam. By default such an insert copies the slots beyond the seam to the window's other end and
    runs in place; with that switched off it is redone by the copying walk."""
    unwrap = seam = 0
    for order in (0, 1, 2):
        for seed in range(3):
            pts = rows(3, 40, order, seed=seed)
            st = check(mode, pts)
            unwrap += st["n_ip_unwrap"]
            assert st["n_ip_seam"] <= st["n_ip_fallback"]
            off = check(mode, pts, seam_copy=0)
            assert off["n_ip_unwrap"] == 0
            seam += off["n_ip_seam"]
    assert unwrap > 0 and seam > 0, (unwrap, seam)


def interior_link_points(mirror):
    """c at the centre of a jittered 24-gon of radius 10, so that the 24-gon is c's ring; w just outside the link edge
    that crosses the positive x axis (its end points at +-7.5 degrees), outside the circle through that edge and c.
    p = (7, 0.05) lies in the fan triangle of that edge, inside the circumcircles of the seven fan triangles within 46
    degrees of the axis (both chains run three slots) and inside the circle through the edge and w (centre (8.4, 0),
    radius 2): the link in the middle of the kept run swaps."""
    rng = np.random.default_rng(7)
    ang = np.deg2rad(np.arange(24) * 15.0 + 7.5)
    rad = 10.0 + rng.uniform(-1e-3, 1e-3, 24)
    ring = np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1)
    pts = np.concatenate([ring, [[10.4, 0.0]], [[0.0, 0.0]], [[7.0, 0.05]]])
    if mirror:
        pts[:, 1] = -pts[:, 1]
    return pts + np.array([25.0, 14.0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mirror", [False, True])
def test_interior_swapped_link(mirror, mode):
    pts = np.concatenate([interior_link_points(mirror), rows(2, 6, 0) + np.array([40.0, 26.0])])
    st = check(mode, pts)
    assert st["inserted"] == len(pts)
    assert st["interior"] >= 1, st


@pytest.mark.parametrize("mode", MODES)
def test_duplicate_between_inplace_inserts(mode):
    pts = rows(3, 20, 2)
    rep = []
    for i, p in enumerate(pts):
        rep.append(p)
        if i % 5 == 2:
            rep.extend([p, p])          # located as an existing vertex (loc = 1): the star is flushed, nothing is inserted
    st = check(mode, np.array(rep))
    assert st["inserted"] == len(rep)   # insert() returns true for an existing vertex
    assert st["n_cavity"] + st["n_loop"] == len(pts)
    assert st["n_inplace"] > 0.5 * len(pts)


@pytest.mark.parametrize("mode", MODES)
def test_point_on_a_spoke_between_inplace_inserts(mode):
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
    assert st["n_loop"] >= 20 and st["n_inplace"] > 0


@pytest.mark.parametrize("mode", MODES)
def test_point_outside_the_rectangle_between_inplace_inserts(mode):
    pts = rows(3, 20, 0)
    pts = np.insert(pts, [25, 26, 47], [[500.0, 3.0], [-100.0, -100.0], [7.0, 1000.0]], axis=0)
    st = check(mode, pts)
    assert st["inserted"] == len(pts) - 3
    assert st["n_inplace"] > 0.5 * len(pts)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [61, 97, 120])
def test_export_straight_after_an_inplace_insert(n, mode):
    s = flat(rows(3, 40, 2)[:n])
    st = np.zeros(32, np.int64)
    rc = shim(mode).ip_export(s.ctypes.data, n, *RECT, st.ctypes.data)
    assert rc == 0, {1: "the last insert before the export was not in place", 2: "raw_into bytes differ",
                     3: "voronoi_edges differ", 4: "state differs"}[rc]
    assert st[8] == 0


@pytest.mark.parametrize("mode", MODES)
def test_init_delaunay_straight_after_an_inplace_insert(mode):
    s1, s2 = flat(rows(3, 20, 2)), flat(rows(4, 13, 1, seed=3, dx=0.8, dy=1.7) + np.array([2.0, 1.0]))
    st = np.zeros(16, np.int64)
    bad = shim(mode).ip_reinit(s1.ctypes.data, s1.size // 2, s2.ctypes.data, s2.size // 2, *RECT, st.ctypes.data)
    assert bad != -2, "the last insert before init_delaunay was not in place"
    assert bad == -1, f"state differs after insert {bad} of the second set"
    st = stats(st)
    assert st["inserted"] == s2.size // 2 and st["poison_reads"] == 0 and st["n_inplace"] > 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("every", [1, 0])
def test_copy_straight_after_an_inplace_insert(every, mode):
    a = rows(4, 20, 2, seed=1)
    b = rows(3, 13, 0, seed=2, dx=0.9, dy=1.3) + np.array([25.0, 10.0])   # the copy goes on elsewhere
    sa, sb = flat(a), flat(b)
    st = np.zeros(32, np.int64)
    bad = shim(mode).ip_copy(sa.ctypes.data, len(a), 31, sb.ctypes.data, len(b), *RECT, every, st.ctypes.data)
    assert bad != -2, "the insert before the copy was not in place"
    assert bad == -1, f"state differs after insert {bad // 2} of {'the copy' if bad % 2 else 'the original'}"
    assert stats(st)["inserted"] == len(a) and stats(st, 16)["inserted"] == len(b)
    assert stats(st, 16)["poison_reads"] == 0 and stats(st, 16)["n_inplace"] > stats(st)["n_inplace"] // 4


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("every", [1, 0])
def test_two_instances_fed_alternately(every, mode):
    a, b = rows(3, 40, 2, seed=1), rows(5, 13, 1, seed=2, dx=0.7, dy=1.9) + np.array([3.0, 1.0])
    s1, s2 = flat(a), flat(b)
    st = np.zeros(32, np.int64)
    bad = shim(mode).ip_check2(s1.ctypes.data, len(a), s2.ctypes.data, len(b), *RECT, every, st.ctypes.data)
    assert bad == -1, f"state differs after alternating insert {bad}"
    s0, s1_ = stats(st), stats(st, 16)
    assert s0["inserted"] == len(a) and s1_["inserted"] == len(b)
    assert s0["n_inplace"] > 0.5 * len(a) and s1_["n_inplace"] > 0.4 * len(b)
    assert s1_["poison_reads"] == 0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order,slack", [(0, 2), (1, 16)])
def test_rebase_when_the_window_reaches_the_end_of_its_slack(order, slack, mode):
    """Rows inserted in one direction slide the window one way, by the two or three slots an insert drops at one end
    and adds at the other: left to right upward, where a buffer has at least its window's length again as room, right
    to left downward, where it has the slack alone. With little slack the window reaches an end of its buffer every
    few inserts and the copying walk puts it back."""
    pts = rows(4, 40, order)
    st = check(mode, pts, slack=slack)
    assert st["inserted"] == len(pts)
    assert st["n_rebase"] >= 2 and st["n_inplace"] > 0.5 * len(pts), st
    assert check(mode, pts)["n_rebase"] == 0   # and none with the default slack


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mirror", [False, True])
def test_pocket_of_a_non_convex_star(mirror, mode):
    """X lies inside the triangle A, B, c, so after c's insert it has degree 3 and is a reflex vertex of c's star:
    the triangle right of the link edge between X and A has the ring vertex B as apex. c is outside the circle
    through A, X, B (centre (5, -5.25), radius 7.25), so the star is Delaunay; p lies in the fan triangle X, A, c
    and inside that circle, so its root link edge swaps onto B while c's star is pending: the in-place walk bails
    out as the copying walk does, having changed nothing."""
    A, X, B, c, p = (0.0, 0.0), (5.0, 2.0), (10.0, 0.0), (5.0, 6.0), (4.5, 1.9)
    pts = np.array([A, X, B, c, p])
    if mirror:
        pts[:, 0] = 10.0 - pts[:, 0]
    pts = np.concatenate([pts, rows(2, 6, 0) + np.array([20.0, 12.0])])   # and on with ordinary fan inserts
    st = check(mode, pts)
    assert st["inserted"] == len(pts)
    assert st["n_ho_pocket"] >= 1, st
