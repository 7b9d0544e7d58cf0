"""Subdiv2D's hand-over insert (the previous insert's star walked through arrays, subdiv2d.h) against the swap
loop: two instances get the same points, one with the hand-over on and one forced onto OpenCV's swap loop, and
their complete state (rings, end points, firstEdge, recentEdge, free lists) must be equal after every insert.
CPU-only: subdiv2d.cpp is compiled here into a throw-away library, as in test_subdiv_host.py."""
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
enum { NST = 16 };   // counters per instance
// stats: inserts that returned true, n_handover, n_cavity, n_loop, n_ho_bail, hand-over inserts whose located fan
// triangle sat at ring slot 0, and at slot m - 1, n_deferred, inserts after which a star was pending
static void count(const aos::Subdiv2D& a, bool ok, long* st) {
    st[0] += ok;
    st[1] = a.n_handover; st[2] = a.n_cavity; st[3] = a.n_loop; st[4] = a.n_ho_bail;
    if (a.last_ho_slot == 0) st[5]++;
    if (a.last_ho_slot >= 0 && a.last_ho_slot == a.last_ho_ring - 1) st[6]++;
    st[7] = a.n_deferred;
    st[8] += a.star_pending();
}
// returns -1 when the states were equal after every insert, else the index of the first insert after which they differ
extern "C" int ho_check(const double* s, int n, float rx, float ry, float rw, float rh, int handover, long* st) {
    aos::Subdiv2D a, r;
    a.set_handover(handover != 0);
    r.set_swap_loop(true);
    a.init_delaunay(rx, ry, rw, rh, 0); r.init_delaunay(rx, ry, rw, rh, 0);
    for (int i = 0; i < NST; ++i) st[i] = 0;
    for (int i = 0; i < n; ++i) {
        const bool ka = a.insert((float)s[2 * i], (float)s[2 * i + 1]), kr = r.insert((float)s[2 * i], (float)s[2 * i + 1]);
        if (ka != kr || !a.same_state(r)) return i;
        count(a, ka, st);
    }
    return -1;
}
// two hand-over instances fed alternately (set 1, set 2, set 1, ...), each against a swap-loop instance of its own
extern "C" int ho_check2(const double* s1, int n1, const double* s2, int n2, float rx, float ry, float rw, float rh, long* st) {
    aos::Subdiv2D a[2], r[2];
    const double* s[2] = {s1, s2};
    const int n[2] = {n1, n2};
    for (int k = 0; k < 2; ++k) {
        r[k].set_swap_loop(true);
        a[k].init_delaunay(rx, ry, rw, rh, 0); r[k].init_delaunay(rx, ry, rw, rh, 0);
    }
    for (int i = 0; i < 2 * NST; ++i) st[i] = 0;
    for (int i = 0; i < n1 || i < n2; ++i)
        for (int k = 0; k < 2; ++k) {
            if (i >= n[k]) continue;
            const float x = (float)s[k][2 * i], y = (float)s[k][2 * i + 1];
            const bool ka = a[k].insert(x, y), kr = r[k].insert(x, y);
            if (ka != kr || !a[k].same_state(r[k])) return 2 * i + k;
            count(a[k], ka, st + NST * k);
        }
    return -1;
}
extern "C" int ho_available() { return aos::Subdiv2D::simd_ok() ? 1 : 0; }
"""

_lib = None


def shim():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="subdiv_ho_shim_")
        src = os.path.join(d, "shim.cpp")
        open(src, "w").write(SHIM)
        so = os.path.join(d, "libshim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                               "-I", os.path.dirname(SRC), "-o", so, src, SRC])
        _lib = ctypes.CDLL(so)
        _lib.ho_check.restype = ctypes.c_int
        _lib.ho_check.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_float] * 4 + [ctypes.c_int, ctypes.c_void_p]
        _lib.ho_check2.restype = ctypes.c_int
        _lib.ho_check2.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_float] * 4 + [
            ctypes.c_void_p]
        assert _lib.ho_available() == 1, "the hand-over needs AVX2 (every supported host has it)"
    return _lib


RECT = (-5.0, -5.0, 60.0, 40.0)   # x, y, w, h: every row set below lies inside it

NST = 16   # counters per instance (the shim's NST)
STAT = ("inserted", "n_handover", "n_cavity", "n_loop", "n_ho_bail", "seam_first", "seam_last", "n_deferred", "pending_after")


def check(pts, handover=1):
    """Runs pts through a hand-over instance and a swap-loop instance; returns the hand-over instance's counters."""
    s = np.ascontiguousarray(pts, np.float64).reshape(-1)
    st = np.zeros(NST, np.int64)
    bad = shim().ho_check(s.ctypes.data, s.size // 2, *RECT, handover, st.ctypes.data)
    assert bad == -1, f"state differs from the swap loop's after insert {bad} of {s.size // 2}"
    return dict(zip(STAT, (int(v) for v in st)))


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


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("n_rows", [2, 3, 5])
@pytest.mark.parametrize("n", [6, 13, 40])
def test_rows_equal_swap_loop(n_rows, n, order):
    st = check(rows(n_rows, n, order))
    assert st["inserted"] == n_rows * n
    assert st["n_handover"] > 0
    off = check(rows(n_rows, n, order), handover=0)
    assert off["n_handover"] == 0 and off["inserted"] == n_rows * n
    # with the hand-over off no star is ever left pending: every insert runs its ring pass
    assert off["pending_after"] == 0 and off["n_deferred"] == 0


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("n", [3, 4, 5, 6, 7])
def test_rows_shorter_than_a_vector(n, order):
    st = check(rows(4, n, order, dx=0.9, dy=1.0))
    assert st["inserted"] == 4 * n and st["n_handover"] > 0


def test_fan_triangle_at_the_array_seam():
    """Inserts whose located fan triangle is slot 0 or slot m - 1 of the ring arrays (the cyclic padding)."""
    first = last = 0
    for order in (0, 1, 2):
        for seed in range(4):
            st = check(rows(3, 40, order, seed=seed))
            first += st["seam_first"]
            last += st["seam_last"]
    assert first > 0 and last > 0, (first, last)


def test_duplicate_between_fan_inserts():
    pts = rows(3, 20, 2)
    rep = []
    for i, p in enumerate(pts):
        rep.append(p)
        if i % 5 == 2:
            rep.extend([p, p])          # located as an existing vertex (loc = 1): nothing is inserted
    st = check(np.array(rep))
    assert st["inserted"] == len(rep)   # insert() returns true for an existing vertex
    assert st["n_cavity"] + st["n_loop"] == len(pts)
    assert st["n_handover"] > 0.5 * len(pts)


def test_on_edge_insert_then_fan_insert():
    """Exactly collinear rows in the order 0, 2, 1, 4, 3, ...: the odd points fall on the edge between their
    neighbours (loc = 2, swap-loop path), and the next point is a fan insert again."""
    out = []
    for r in range(3):
        idx = [0]
        for i in range(2, 24, 2):
            idx += [i, i - 1]
        out.append(np.stack([np.array(idx) * 0.5, np.full(len(idx), r * 2.0)], -1))
    pts = np.concatenate(out)
    st = check(pts)
    assert st["inserted"] == len(pts)
    assert st["n_loop"] >= 20 and st["n_handover"] > 0


def test_point_outside_the_rectangle_in_mid_row():
    pts = rows(3, 20, 0)
    pts = np.insert(pts, [25, 26, 47], [[500.0, 3.0], [-100.0, -100.0], [7.0, 1000.0]], axis=0)
    st = check(pts)
    assert st["inserted"] == len(pts) - 3
    assert st["n_handover"] > 0.5 * len(pts)


def test_uniform_random():
    rng = np.random.default_rng(7)
    pts = np.stack([rng.uniform(-4, 54, 2000), rng.uniform(-4, 34, 2000)], -1)
    st = check(pts)
    assert st["inserted"] == 2000


def test_two_instances_fed_alternately():
    a, b = rows(3, 40, 2, seed=1), rows(5, 13, 1, seed=2, dx=0.7, dy=1.9) + np.array([3.0, 1.0])
    s1 = np.ascontiguousarray(a, np.float64).reshape(-1)
    s2 = np.ascontiguousarray(b, np.float64).reshape(-1)
    st = np.zeros(2 * NST, np.int64)
    bad = shim().ho_check2(s1.ctypes.data, len(a), s2.ctypes.data, len(b), *RECT, st.ctypes.data)
    assert bad == -1, f"state differs after alternating insert {bad}"
    assert st[0] == len(a) and st[NST] == len(b)
    assert st[1] > 0.8 * len(a) and st[NST + 1] > 0.5 * len(b)


@pytest.mark.parametrize("order", [0, 1, 2])
def test_most_row_inserts_take_the_hand_over(order):
    st = check(rows(3, 40, order))
    assert st["n_handover"] > 0.8 * st["inserted"], st
