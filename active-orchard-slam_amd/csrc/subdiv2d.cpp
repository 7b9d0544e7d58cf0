// Host Delaunay with cv::Subdiv2D semantics — see subdiv2d.h. Compiled -ffp-contract=off.
#include "subdiv2d.h"

#if defined(__x86_64__)
#include <immintrin.h>
#define AOS_AVX2 __attribute__((target("avx2")))
#else
#define AOS_AVX2
#endif

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <functional>

// AOS_SD_PROF (tools/sdcheck/sdprof.cpp only): per-phase TSC accumulators of the insert path
#ifdef AOS_SD_PROF
#include <x86intrin.h>
namespace aos { SdProf g_sdprof; }
#define SDP_T0(v) const unsigned long long v = __rdtsc()
#define SDP_ADD(field, t0) (aos::g_sdprof.field += __rdtsc() - (t0))
#define SDP_INC(field) (++aos::g_sdprof.field)
#else
#define SDP_T0(v)
#define SDP_ADD(field, t0)
#define SDP_INC(field)
#endif

namespace aos {

#ifdef AOS_SD_POISON
long sd_poison_reads = 0;
#endif

namespace {
// triangleArea (double from float coordinates)
inline double tri_area(float ax, float ay, float bx, float by, float cx, float cy) {
    return ((double)bx - ax) * ((double)cy - ay) - ((double)by - ay) * ((double)cx - ax);
}
// computeVoronoiPoint; returns false for det == 0 or a huge result (the vertex is not created)
inline bool voronoi_point(float o0x, float o0y, float d0x, float d0y, float o1x, float o1y, float d1x, float d1y,
                          float &rx, float &ry) {
    double a0 = d0x - o0x, b0 = d0y - o0y;
    double c0 = -0.5 * (a0 * (d0x + o0x) + b0 * (d0y + o0y));
    double a1 = d1x - o1x, b1 = d1y - o1y;
    double c1 = -0.5 * (a1 * (d1x + o1x) + b1 * (d1y + o1y));
    double det = a0 * b1 - a1 * b0;
    if (det != 0) {
        det = 1. / det;
        rx = (float)((b0 * c1 - b1 * c0) * det);
        ry = (float)((a1 * c0 - a0 * c1) * det);
        return std::abs(rx) < FLT_MAX * 0.5 && std::abs(ry) < FLT_MAX * 0.5;
    }
    return false;
}

// The swap loop's flip test of a link edge O -> D whose right triangle has the apex T, against the new point P:
//   isRightOf(T, edge) > 0 && isPtInCircle3(pt = O, a = T, b = D, c = P) < 0, eps = FLT_EPSILON / 8.
// Every operand has x, y and n2 = x*x + y*y as exact double copies of the float coordinates (the float -> double
// conversions are exact, so every product and sum rounds as in triangleArea / isPtInCircle3, and |p|^2 is formed once
// per vertex in the same order). This is the one scalar statement of the test: bit-exactness against OpenCV rests on
// these operands in this operation order. It is evaluated whole and combined without a branch: the orientation test
// is nearly always true and the in-circle sum's operands are already loaded; the sum is only compared, so where the
// orientation fails the result is false whatever the sum is.
template <class TT, class TO, class TD, class TP>
inline bool flips(const TT &T, const TO &O, const TD &D, const TP &P) {
    auto area = [](const auto &a, const auto &b, const auto &c) { return (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x); };
    const double aTDO = area(T, D, O);
    double val = T.n2 * area(D, P, O);
    val -= D.n2 * area(T, P, O);
    val += P.n2 * aTDO;
    val -= O.n2 * area(T, D, P);
    return (aTDO > 0) & (val < -(FLT_EPSILON * 0.125));
}
struct HoS { double x, y, n2; };   // an operand of flips() put together from the ring arrays

#if defined(__x86_64__)
// Four flip tests at once (bit i = lane i swaps): each lane is flips(), the same plain IEEE double subtractions,
// products and sums in the same order, no FMA.
struct HoV { __m256d x, y, n; };
AOS_AVX2 inline HoV ho_ld(const double *x, const double *y, const double *n, int i) {
    return HoV{_mm256_loadu_pd(x + i), _mm256_loadu_pd(y + i), _mm256_loadu_pd(n + i)};
}
AOS_AVX2 inline __m256d area4(__m256d ax, __m256d ay, __m256d bx, __m256d by, __m256d cx, __m256d cy) {
    return _mm256_sub_pd(_mm256_mul_pd(_mm256_sub_pd(bx, ax), _mm256_sub_pd(cy, ay)),
                         _mm256_mul_pd(_mm256_sub_pd(by, ay), _mm256_sub_pd(cx, ax)));
}
AOS_AVX2 inline int ho_test4(const HoV &T, const HoV &O, const HoV &D, const HoV &P) {
    const __m256d aTDO = area4(T.x, T.y, D.x, D.y, O.x, O.y);
    __m256d val = _mm256_mul_pd(T.n, area4(D.x, D.y, P.x, P.y, O.x, O.y));
    val = _mm256_sub_pd(val, _mm256_mul_pd(D.n, area4(T.x, T.y, P.x, P.y, O.x, O.y)));
    val = _mm256_add_pd(val, _mm256_mul_pd(P.n, aTDO));
    val = _mm256_sub_pd(val, _mm256_mul_pd(O.n, area4(T.x, T.y, D.x, D.y, P.x, P.y)));
    const __m256d right = _mm256_cmp_pd(aTDO, _mm256_setzero_pd(), _CMP_GT_OQ);
    const __m256d inside = _mm256_cmp_pd(val, _mm256_set1_pd(-(FLT_EPSILON * 0.125)), _CMP_LT_OQ);
    return _mm256_movemask_pd(_mm256_and_pd(right, inside));
}
#endif
}  // namespace

void Subdiv2D::reserve(size_t n) {
    vp.reserve(2 * n + 8); vd.reserve(2 * n + 8); vfirst.reserve(2 * n + 8); vtype.reserve(2 * n + 8);
    rec.reserve(3 * n + 8);
}

int Subdiv2D::right_of(float px, float py, int e) const {   // isRightOf: sign of triangleArea(p, dst, org)
    const V2d &o = vd[org(e)], &d = vd[dst(e)];
    const double x = px, y = py;
    const double cw = (d.x - x) * (o.y - y) - (d.y - y) * (o.x - x);
    return (cw > 0) - (cw < 0);
}

// newEdge: a fresh quad-edge whose primal edges are singleton rings; free quad-edges are reused LIFO
int Subdiv2D::new_edge() {
    if (free_q <= 0) {
        rec.push_back(Rec{});
        free_q = (int)rec.size() - 1;
    }
    const int q = free_q, e = q * 4;
    free_q = rec[q].h[0].x;
    rec[q] = Rec{{Half{e, e, 0, 0}, Half{e + 2, e + 2, 0, 0}}};
    return e;
}

int Subdiv2D::new_point(float x, float y, int type) {
    if (free_p == 0) {
        vp.push_back(V2f{0.f, 0.f}); vfirst.push_back(0); vtype.push_back(-1); vd.push_back(V2d{0.0, 0.0, 0.0, 0, 0});
        free_p = (int)vp.size() - 1;
    }
    const int v = free_p;
    free_p = vfirst[v];
    vp[v] = V2f{x, y}; vfirst[v] = 0; vtype[v] = type;
    vd[v] = V2d{(double)x, (double)y, (double)x * x + (double)y * y, 0, 0};
    return v;
}

void Subdiv2D::set_pts(int e, int o, int d) {   // setEdgePoints
    orgr(e) = o;
    orgr(sym(e)) = d;
    vfirst[o] = e;
    vfirst[d] = sym(e);
}

int Subdiv2D::connect(int a, int b) {   // connectEdges
    const int e = new_edge();
    splice(e, lnext(a));
    splice(sym(e), b);
    set_pts(e, dst(a), org(b));
    return e;
}

void Subdiv2D::swap_edge(int e) {   // swapEdges
    const int se = sym(e);
    const int a = oprev(e), b = oprev(se);
    splice(e, a);
    splice(se, b);
    set_pts(e, dst(a), dst(b));
    splice(e, lnext(a));
    splice(se, lnext(b));
}

void Subdiv2D::delete_edge(int e) {   // deleteEdge
    splice(e, oprev(e));
    const int se = sym(e);
    splice(se, oprev(se));
    const int q = e >> 2;
    rec[q].h[0].on = 0;        // free marker (OpenCV: next[0] = 0)
    rec[q].h[0].x = free_q;
    free_q = q;
}

Subdiv2D::Subdiv2D() = default;

void Subdiv2D::init_delaunay(float rx, float ry, float rw, float rh, int rect_mode) {
    if (rect_mode == 1) {  // Rect_<float> -> Rect_<int>: saturate_cast<int> = cvRound (nearest even)
        rx = (float)(int)std::lrint(rx); ry = (float)(int)std::lrint(ry);
        rw = (float)(int)std::lrint(rw); rh = (float)(int)std::lrint(rh);
    }
    const float big = 3.f * std::max(rw, rh);
    vp.clear(); vd.clear(); vfirst.clear(); vtype.clear(); rec.clear();
    recent = 0;
    ho_valid = false;
    pending = false;   // a pending star of the previous point set is dropped with its records
    loc_k = -1;
    tlx = rx; tly = ry; brx = rx + rw; bry = ry + rh;
    vp.push_back(V2f{0.f, 0.f}); vd.push_back(V2d{0.0, 0.0, 0.0, 0, 0}); vfirst.push_back(0); vtype.push_back(-1);
    rec.push_back(Rec{});                                                      // quad-edge 0 (NULL)
    free_q = 0; free_p = 0;
    const int pA = new_point(rx + big, ry, 0), pB = new_point(rx, ry + big, 0), pC = new_point(rx - big, ry - big, 0);
    const int eAB = new_edge(), eBC = new_edge(), eCA = new_edge();
    set_pts(eAB, pA, pB); set_pts(eBC, pB, pC); set_pts(eCA, pC, pA);
    splice(eAB, sym(eCA)); splice(eBC, sym(eAB)); splice(eCA, sym(eBC));
    recent = eAB;
}

// Subdiv2D::locate: 0 inside, 1 vertex, 2 on edge, -1 outside rect, -2 error
int Subdiv2D::locate(float px, float py, int &out_edge, int &out_vertex) {
    int vertex = 0;
    const int max_edges = (int)rec.size() * 4;
    if (px < tlx || py < tly || px >= brx || py >= bry) return -1;
    loc_k = -1;
    if (pending) {
        if (locate_star(px, py, out_edge)) { out_vertex = 0; return 0; }
        flush();   // the walk below starts again from the same recentEdge
    }
    SDP_T0(t_loc);
    // The walk carries the current edge's end points o = Org(edge), d = Dst(edge): Onext(edge) keeps the origin and
    // Dprev(edge) the destination, and both end at the left face's third vertex a (Dst Onext = Org Dprev), so a step
    // loads one vertex. right_of(p, x -> y) is the sign of (y.x - p.x) (x.y - p.y) - (y.y - p.y) (x.x - p.x), as before.
    // (Checked against the round-4 walk on every locate of tools/sdcheck's 241 cases and the C2 seeds: same location,
    // edge, vertex and recentEdge; the C2 replay 17.4 -> 17.1 ms on the box, profiles/r05s_sdprof.txt.)
    const double x = px, y = py;
    auto rof = [&](int oi, int di) {
        const V2d &o = vd[oi], &d = vd[di];
        const double cw = (d.x - x) * (o.y - y) - (d.y - y) * (o.x - x);
        return (cw > 0) - (cw < 0);
    };
    int edge = recent;
    int location = -2;
    int o = org(edge), d = dst(edge);
    int roc = rof(o, d);
    if (roc > 0) { edge = sym(edge); roc = -roc; std::swap(o, d); }
    for (int i = 0; i < max_edges; i++) {
        SDP_INC(loc_iters);
        const int on_ = onext(edge);
        const int a = dst(on_);
        const int ron = rof(o, a);   // Onext: o -> a
        const int rod = rof(a, d);   // Dprev: a -> d
        if (rod > 0) {
            if (ron > 0 || (ron == 0 && roc == 0)) { location = 0; break; }
            roc = ron; edge = on_; d = a;
        } else {
            if (ron > 0) {
                if (rod == 0 && roc == 0) { location = 0; break; }
                roc = rod; edge = dprev(edge); o = a;
            } else if (roc == 0 && right_of(vp[a].x, vp[a].y, edge) >= 0) {
                edge = sym(edge); std::swap(o, d);
            } else {
                roc = ron; edge = on_; d = a;
            }
        }
    }
    recent = edge;
    if (location == 0) {
        const float ox = vp[o].x, oy = vp[o].y, dx = vp[d].x, dy = vp[d].y;
        double t1 = std::fabs(px - ox); t1 += std::fabs(py - oy);
        double t2 = std::fabs(px - dx); t2 += std::fabs(py - dy);
        double t3 = std::fabs(ox - dx); t3 += std::fabs(oy - dy);
        if (t1 < FLT_EPSILON) { location = 1; vertex = o; edge = 0; }
        else if (t2 < FLT_EPSILON) { location = 1; vertex = d; edge = 0; }
        else if ((t1 < t3 || t2 < t3) && std::fabs(tri_area(px, py, ox, oy, dx, dy)) < FLT_EPSILON) { location = 2; vertex = 0; }
    }
    if (location == -2) { edge = 0; vertex = 0; }
    out_edge = edge; out_vertex = vertex;
    SDP_ADD(t_locate, t_loc);
    return location;
}

bool Subdiv2D::insert(float x, float y) {
    int curr_edge = 0, curr_point = 0;
    last_ho_slot = -1;
    const int loc = locate(x, y, curr_edge, curr_point);
    if (loc < 0) return false;        // PTLOC_ERROR (CV_StsBadSize) / outside rect (CV_StsOutOfRange)
    if (loc == 1) return true;        // existing vertex: nothing inserted
    if (loc == 2) {
        const int deleted = curr_edge;
        recent = curr_edge = oprev(curr_edge);
        delete_edge(deleted);
    }
    if (curr_edge == 0) return false;  // CV_Assert
    curr_point = new_point(x, y, 0);
    if (loc == 0 && !force_loop && insert_cavity(curr_edge, curr_point)) {
        ++n_cavity;
        return true;
    }
    ++n_loop;
    flush();
    ho_valid = false;   // the swap loop leaves no ring arrays behind
    int base = new_edge();
    const int first_point = org(curr_edge);
    set_pts(base, first_point, curr_point);
    splice(base, curr_edge);
    do {
        base = connect(curr_edge, sym(base));
        curr_edge = oprev(base);
    } while (dst(curr_edge) != first_point);
    swap_loop(oprev(base), first_point, curr_point);
    return true;
}

// OpenCV's swap loop (Subdiv2D::insert after the connects), the reference path.
void Subdiv2D::swap_loop(int curr_edge, int first_point, int curr_point) {
    const int max_edges = (int)rec.size() * 4;
    const V2d P = vd[curr_point];
    for (int i = 0; i < max_edges; i++) {
        const int temp = oprev(curr_edge);
        const int corg = org(curr_edge);
        if (flips(vd[dst(temp)], vd[corg], vd[dst(curr_edge)], P)) {
            swap_edge(curr_edge);
            curr_edge = oprev(curr_edge);
        } else if (corg == first_point) {
            break;
        } else {
            curr_edge = lprev(onext(curr_edge));
        }
    }
}

// ---- the ring of an insert's star as arrays (subdiv2d.h) ----
static constexpr int HO_PAD = 4;   // spare entries before position 0 and after position cap - 1 (the cyclic copies)

Subdiv2D::RingP Subdiv2D::ring_ptrs(Ring &r) {   // indexed from the window's first slot
    const size_t at = (size_t)HO_PAD + r.b;
    return RingP{r.bd.data() + at, r.bu.data() + at, r.ba.data() + at, r.sp.data() + at, r.x.data() + at,
                 r.y.data() + at,  r.n.data() + at,  r.ax.data() + at, r.ay.data() + at, r.an.data() + at};
}

void Subdiv2D::ring_reserve(Ring &r, int slots) {   // room for slots from the window's first on; keeps the contents
    const int need = r.b + slots;
    if (need <= r.cap) return;
    const int cap = std::max(64, 2 * need);
    const size_t n = (size_t)cap + 2 * HO_PAD;
    r.bd.resize(n); r.bu.resize(n); r.ba.resize(n); r.sp.resize(n);
    r.x.resize(n); r.y.resize(n); r.n.resize(n); r.ax.resize(n); r.ay.resize(n); r.an.resize(n);
    r.cap = cap;
}

// The one statement of what slot k of a ring around p owns in the records, and so of what is pending while its star
// is deferred (subdiv2d.h): f(field, value) for Onext(L_k), the slot int of L_k (how the next insert finds its fan
// triangle's slot), Oprev(Sym L_k+1), every field of the spoke S_k = x_k -> p and of Sym S_k, and firstEdge of x_k.
// k is the slot's position in the buffer. L = L_k, Ln = L_k+1, x = x_k, Sm / S / Sn = S_k-1 / S_k / S_k+1. R is the
// Rec array as ints (a directed edge e's fields at R[2 e]: onext, oprev, origin, slot). The ring pass, retire() and
// for_pending() all go through it.
template <class F>
static inline void slot_fields(int *R, int *vfirst, int k, int L, int Ln, int x, int Sm, int S, int Sn, int p, F f) {
    const int sLn = Ln ^ 2, sS = S ^ 2;
    f(R[2 * (ptrdiff_t)L], S);                                     // Onext(L_k) = S_k
    f(R[2 * (ptrdiff_t)L + 3], k);                                 // slot of L_k
    f(R[2 * (ptrdiff_t)sLn + 1], S);                               // Oprev(Sym L_k+1) = S_k
    int *a = R + 2 * (ptrdiff_t)S, *b = R + 2 * (ptrdiff_t)sS;
    f(a[0], sLn); f(a[1], L); f(a[2], x);                          // S_k: x_k -> p
    f(b[0], Sm ^ 2); f(b[1], Sn ^ 2); f(b[2], p);                  // Sym S_k: around p, counter-clockwise
    f(vfirst[x], S);
}
static inline void slot_write(int *R, int *vfirst, int k, int L, int Ln, int x, int Sm, int S, int Sn, int p) {
    slot_fields(R, vfirst, k, L, Ln, x, Sm, S, Sn, p, [](int &field, int v) { field = v; });
}

// The ring pass: one pass over the boundary L_k (k in walk order from the window's first slot, at position base;
// bd / sp padded cyclically at m) writes every slot's fields. OpenCV's swapEdges' setEdgePoints(e, apex, p) and
// vtx[apex].firstEdge = e, and the rings of the final star, are all in it. In a function of its own over plain
// restrict pointers the compiler keeps the loop's values (the carried S_k-1, S_k, S_k+1) in registers (DESIGN.md 6.1,
// round 5).
__attribute__((noinline)) static void ring_pass(int *__restrict R, int *__restrict vfirst, const int *__restrict bd,
                                                const int *__restrict bu, const int *__restrict sp, int m, int p,
                                                int base) {
    int Sm = sp[m - 1], S = sp[0];
    for (int k = 0; k < m; ++k) {
        const int Sn = sp[k + 1];
        slot_write(R, vfirst, base + k, bd[k], bd[k + 1], bu[k], Sm, S, Sn, p);
        Sm = S; S = Sn;
    }
}

// The cavity walk from one link edge e (the generic form: the swap loop's tests read off the records); every leaf
// goes into ring N at slot q with its apex and both vertices' coordinates. Returns the next free slot, or -1 when an
// apex is already a cavity vertex (the cavity would wrap a vertex: the caller runs the connects and the swap loop);
// the last swap (or last_flip, if there was none) is left in ho_lf.
//  * Pre-order: the first child (w -> v) is walked at once, the second (u -> w) waits on the stack, which is the swap
//    loop's order. Every test reads the old triangle right of the link edge, never one incident to p, so the walk
//    changes no record.
//  * The marks live in the vertex's own line (V2d::stamp / spoke): the walk reads them right after the vertex's
//    coordinates. w is never p (p has no edge yet), and the stack cannot overflow: every swap adds a distinct vertex,
//    so the swaps are fewer than the vertices (dfs_stack is sized by them).
//  * Why no certification of the boundary is needed: by induction over the walk, a tested edge u -> v emits leaves
//    forming a chain from v back to u (a leaf emits itself; a swapped edge with apex w emits the chain of w -> v, then
//    that of u -> w), whose origins are u and the apexes below it. So the three root chains always close into one
//    cycle of 3 + (swaps) edges, and its vertices are distinct exactly when every apex is new, which is checked at
//    each swap. (tools/sdcheck still compares every insert's full state with the swap loop.)
//  * The stack is a bumped pointer and no flip counter is kept (last_flip < 0: no flip): with fewer live values the
//    walk keeps them in registers.
__attribute__((noinline)) int Subdiv2D::cavity_walk(int e, const V2d &Pin, int sA, Ring &N, int q, int last_flip) {
    const V2d P = Pin;
    int *const stk = dfs_stack.data();
    int *top = stk;
    RingP n = ring_ptrs(N);
    int cap = N.cap - N.b;
    const int hz = ho_hz;
    for (;;) {
        SDP_INC(dfs_steps);
        const int t = oprev(e), w = dst(t), o = org(e);
        const V2d &T = vd[w], &O = vd[o];
        if (flips(T, O, vd[dst(e)], P)) {
            V2d &W = vd[w];
            if (W.stamp == sA) return -1;
            // a ring vertex of the pending star outside the cavity: the child edges may be Sym L_i (subdiv2d.h)
            if (W.stamp == hz) { ho_pocket = true; return -1; }
            W.stamp = sA;
            W.spoke = e;                                       // e becomes w -> p
            last_flip = e;
            *top++ = t;                                        // u -> w, after the w -> v subtree
            e = sym(onext(sym(e)));                            // w -> v
            continue;
        }
        if (q >= cap) { ring_reserve(N, q + 1); n = ring_ptrs(N); cap = N.cap - N.b; }
        n.bd[q] = e; n.bu[q] = o; n.ba[q] = w; n.sp[q] = O.spoke;
        n.x[q] = O.x; n.y[q] = O.y; n.n[q] = O.n2;
        n.ax[q] = T.x; n.ay[q] = T.y; n.an[q] = T.n2;
        ++q;
        if (top == stk) break;
        e = *--top;
    }
    ho_lf = last_flip;
    return q;
}

// ---- hand-over: the previous insert's star walked through its arrays (subdiv2d.h) ----
AOS_AVX2 static int find_int(const int *a, int m, int v);
#if defined(__x86_64__)
#ifndef AOS_HO_VEC
#define AOS_HO_VEC 1   // 0: every hand-over test and copy one slot at a time (the A/B of DESIGN.md 6.1)
#endif


// Walk of the three roots when p lies in the fan triangle (x_k, x_k-1, c) of the previous star O (subdiv2d.h): the
// roots are L_k (link), S_k-1 (descending chain) and Sym S_k (ascending chain); shift rotates the order
// (ascending, descending, link) to the walk order eA, eB, e0. Writes the new ring into N; 0: bail out, 1: done.
// INPLACE: the same tests, stamps and bail-outs in the same order, but nothing is stored into a ring but the leaves
// of swapped links, which go into N as scratch (ho_plan says where). 2 (seam), 3 (swapped links) and 4 (no room) say
// that ho_apply cannot build this ring in place: the caller takes a fresh stamp and runs the copying form, whose tests
// up to that point repeat this walk's.
template <bool INPLACE>
AOS_AVX2 int Subdiv2D::ho_fast(Ring &Oring, Ring &N, int k, int shift, int p, int c, int sA, int &q_out) {
    const RingP o = ring_ptrs(Oring);
    RingP n = ring_ptrs(N);
    const int m = Oring.m;
    V2d *const V = vd.data();
    const V2d Pv = V[p], Cv = V[c];
    const HoS Ps{Pv.x, Pv.y, Pv.n2}, Cs{Cv.x, Cv.y, Cv.n2};
    const HoV P4{_mm256_set1_pd(Pv.x), _mm256_set1_pd(Pv.y), _mm256_set1_pd(Pv.n2)};
    const HoV C4{_mm256_set1_pd(Cv.x), _mm256_set1_pd(Cv.y), _mm256_set1_pd(Cv.n2)};
    int q = 0, lf = -1;
    const int km1 = k ? k - 1 : m - 1;
    if (INPLACE) { ho_plan.k = k; ho_plan.nsl = 0; }

#define HO_ROOM(cnt) do { if (N.b + q + (cnt) > N.cap) { ring_reserve(N, q + (cnt)); n = ring_ptrs(N); } } while (0)
#define HO_XS(i) HoS{o.x[i], o.y[i], o.n[i]}
#define HO_AS(i) HoS{o.ax[i], o.ay[i], o.an[i]}
// a swap onto ring vertex v (the apex), whose spoke becomes s
#define HO_SWAP(v, s) do { V2d &W_ = V[v]; if (W_.stamp == sA) return 0; W_.stamp = sA; W_.spoke = (s); lf = (s); } while (0)
// link slot j: a leaf is copied from the old ring (its right triangle is untouched), a swap leaves the star
#define HO_LINK(j, swaps) do { \
        if (swaps) { \
            if (INPLACE) { if (ho_plan.nsl == 2) return 3; ho_plan.sl[ho_plan.nsl] = HoLink{(j), q, 0}; } \
            q = cavity_walk(o.bd[j], Pv, sA, N, q, lf); \
            if (q < 0) return 0; \
            lf = ho_lf; n = ring_ptrs(N); \
            if (INPLACE) { HoLink &l_ = ho_plan.sl[ho_plan.nsl++]; l_.cnt = q - l_.s0; } \
        } else if (!INPLACE) { \
            HO_ROOM(1); \
            n.bd[q] = o.bd[j]; n.bu[q] = o.bu[j]; n.ba[q] = o.ba[j]; n.sp[q] = V[o.bu[j]].spoke; \
            n.x[q] = o.x[j]; n.y[q] = o.y[j]; n.n[q] = o.n[j]; n.ax[q] = o.ax[j]; n.ay[q] = o.ay[j]; n.an[q] = o.an[j]; \
            ++q; \
        } } while (0)
// link slots j .. j + 3, all leaves: one copy per array (the spokes are the caller's)
#define HO_COPY4(j) do { \
        HO_ROOM(4); \
        _mm_storeu_si128((__m128i *)(n.bd + q), _mm_loadu_si128((const __m128i *)(o.bd + (j)))); \
        _mm_storeu_si128((__m128i *)(n.bu + q), _mm_loadu_si128((const __m128i *)(o.bu + (j)))); \
        _mm_storeu_si128((__m128i *)(n.ba + q), _mm_loadu_si128((const __m128i *)(o.ba + (j)))); \
        _mm256_storeu_pd(n.x + q, _mm256_loadu_pd(o.x + (j)));   _mm256_storeu_pd(n.y + q, _mm256_loadu_pd(o.y + (j))); \
        _mm256_storeu_pd(n.n + q, _mm256_loadu_pd(o.n + (j)));   _mm256_storeu_pd(n.ax + q, _mm256_loadu_pd(o.ax + (j))); \
        _mm256_storeu_pd(n.ay + q, _mm256_loadu_pd(o.ay + (j))); _mm256_storeu_pd(n.an + q, _mm256_loadu_pd(o.an + (j))); \
    } while (0)

    for (int r = 0; r < 3; ++r) {
        const int kind = (r + shift) % 3;   // 0 ascending, 1 descending, 2 link
        if (kind == 2) {
            SDP_INC(dfs_steps);
            const bool f = flips(HO_AS(k), HO_XS(k), HO_XS(k - 1), Ps);
            HO_LINK(k, f);
        } else if (kind == 1) {
            // S_j = x_j -> c for j = k - 1, k - 2, ...: T = x_j-1, O = x_j, D = c; a swap stacks L_j and goes on to S_j-1
            int j = km1, nsw = 0;
            for (;;) {
                if (AOS_HO_VEC && j >= 3) {
                    const int b = j - 3;   // lanes: slots b .. j
                    int mask = ho_test4(ho_ld(o.x, o.y, o.n, b - 1), ho_ld(o.x, o.y, o.n, b), C4, P4);
#ifdef AOS_SD_PROF
                    g_sdprof.dfs_steps += 4;
#endif
                    if (mask == 0xf) {
                        for (int i = 3; i >= 0; --i) HO_SWAP(o.bu[b - 1 + i], o.sp[b + i]);
                        nsw += 4;
                        j = b ? b - 1 : m - 1;
                        continue;
                    }
                    while (mask & 8) { HO_SWAP(o.bu[j - 1], o.sp[j]); --j; ++nsw; mask <<= 1; }
                    break;
                }
                SDP_INC(dfs_steps);
                const int jm = j ? j - 1 : m - 1;
                if (!flips(HO_XS(jm), HO_XS(j), Cs, Ps)) break;
                HO_SWAP(o.bu[jm], o.sp[j]);
                ++nsw;
                j = jm;
            }
            // the leaf S_j (apex x_j-1), then the stacked links L_j+1 .. L_k-1
            ho_jD = j;
            if (!INPLACE) {
                HO_ROOM(1);
                n.bd[q] = o.sp[j]; n.bu[q] = o.bu[j]; n.ba[q] = o.bu[j - 1]; n.sp[q] = V[o.bu[j]].spoke;
                n.x[q] = o.x[j]; n.y[q] = o.y[j]; n.n[q] = o.n[j]; n.ax[q] = o.x[j - 1]; n.ay[q] = o.y[j - 1]; n.an[q] = o.n[j - 1];
                ++q;
            }
            int i = j + 1 == m ? 0 : j + 1;
            for (int cnt = nsw; cnt > 0;) {
                if (AOS_HO_VEC && cnt >= 4 && i + 4 <= m) {
                    const int mask = ho_test4(ho_ld(o.ax, o.ay, o.an, i), ho_ld(o.x, o.y, o.n, i), ho_ld(o.x, o.y, o.n, i - 1), P4);
#ifdef AOS_SD_PROF
                    g_sdprof.dfs_steps += 4;
#endif
                    if (mask == 0) {
                        if (!INPLACE) {
                            HO_COPY4(i);
                            _mm_storeu_si128((__m128i *)(n.sp + q), _mm_loadu_si128((const __m128i *)(o.sp + i + 1)));   // x_i took S_i+1
                            q += 4;
                        }
                    } else {
                        for (int l = 0; l < 4; ++l) HO_LINK(i + l, (mask >> l) & 1);
                    }
                    i += 4; cnt -= 4;
                    if (i == m) i = 0;
                } else {
                    SDP_INC(dfs_steps);
                    const bool f = flips(HO_AS(i), HO_XS(i), HO_XS(i - 1), Ps);
                    HO_LINK(i, f);
                    i = i + 1 == m ? 0 : i + 1; --cnt;
                }
            }
            if (!INPLACE && nsw) n.sp[q - 1] = V[o.bu[km1]].spoke;   // the last link's origin x_k-1 is a root
        } else {
            // Sym S_j = c -> x_j for j = k, k + 1, ...: T = x_j+1, O = c, D = x_j; a swap walks L_j+1 at once, then Sym S_j+1
            int j = k;
            for (;;) {
                if (AOS_HO_VEC && j + 4 <= m - 1) {
                    const HoV X0 = ho_ld(o.x, o.y, o.n, j), X1 = ho_ld(o.x, o.y, o.n, j + 1);
                    const int smask = ho_test4(X1, C4, X0, P4);
                    const int lmask = ho_test4(ho_ld(o.ax, o.ay, o.an, j + 1), X1, X0, P4);   // links j + 1 .. j + 4
#ifdef AOS_SD_PROF
                    g_sdprof.dfs_steps += 8;
#endif
                    if (smask == 0xf && lmask == 0) {
                        for (int i = 0; i < 4; ++i) HO_SWAP(o.bu[j + 1 + i], o.sp[j + i] ^ 2);
                        if (!INPLACE) {
                            HO_COPY4(j + 1);
                            _mm_storeu_si128((__m128i *)(n.sp + q),
                                             _mm_xor_si128(_mm_loadu_si128((const __m128i *)(o.sp + j)), _mm_set1_epi32(2)));   // x_j+1 took Sym S_j
                            q += 4;
                        }
                        j += 4;
                        continue;
                    }
                    int i = 0;
                    for (; i < 4 && ((smask >> i) & 1); ++i) {
                        HO_SWAP(o.bu[j + 1], o.sp[j] ^ 2);
                        HO_LINK(j + 1, (lmask >> i) & 1);
                        ++j;
                    }
                    if (i < 4) break;
                    continue;
                }
                SDP_INC(dfs_steps);
                const int jn = j + 1 == m ? 0 : j + 1;
                if (!flips(HO_XS(jn), Cs, HO_XS(j), Ps)) break;
                HO_SWAP(o.bu[jn], o.sp[j] ^ 2);
                SDP_INC(dfs_steps);
                const bool f = flips(HO_AS(jn), HO_XS(jn), HO_XS(j), Ps);
                HO_LINK(jn, f);
                j = jn;
            }
            // the leaf Sym S_j (apex x_j+1)
            ho_jA = j;
            if (!INPLACE) {
                HO_ROOM(1);
                n.bd[q] = o.sp[j] ^ 2; n.bu[q] = c; n.ba[q] = o.bu[j + 1]; n.sp[q] = Cv.spoke;
                n.x[q] = Cv.x; n.y[q] = Cv.y; n.n[q] = Cv.n2; n.ax[q] = o.x[j + 1]; n.ay[q] = o.y[j + 1]; n.an[q] = o.n[j + 1];
                ++q;
            }
        }
    }
#undef HO_ROOM
#undef HO_XS
#undef HO_AS
#undef HO_SWAP
#undef HO_LINK
#undef HO_COPY4
    ho_lf = lf;
    q_out = q;
    if (INPLACE) {
        // a chain that crossed the seam: its end unwrapped, below the window's first slot or above its last. The kept
        // run is then jD + 1 .. jA; a swapped link goes to the end it lies at most one slot from (sl[0] low, sl[1] high)
        HoPlan &pl = ho_plan;
        int jD = ho_jD, jA = ho_jA, wrap = 0;
        if (jD >= k) { jD -= m; wrap = -1; }
        if (jA < k) { if (wrap) return 2; jA += m; wrap = 1; }
        if (wrap && !seam_copy) return 2;
        for (int i = 0; i < pl.nsl; ++i) {
            if (wrap < 0 && pl.sl[i].j > ho_jD) pl.sl[i].j -= m;
            if (wrap > 0 && pl.sl[i].j <= ho_jA) pl.sl[i].j += m;
        }
        pl.jD = jD; pl.jA = jA; pl.wrap = wrap;
        pl.lo = pl.hi = false;
        if (pl.nsl == 2) {
            if (pl.sl[0].j > pl.sl[1].j) std::swap(pl.sl[0], pl.sl[1]);
            if (pl.sl[0].j - (jD + 1) > 1 || jA - pl.sl[1].j > 1) return 3;
            pl.lo = pl.hi = true;
        } else if (pl.nsl == 1) {
            if (pl.sl[0].j - (jD + 1) <= 1) pl.lo = true;
            else if (jA - pl.sl[0].j <= 1) { pl.hi = true; pl.sl[1] = pl.sl[0]; }
            else return 3;
        }
        const int first = jD - (pl.lo ? pl.sl[0].cnt - 1 : 0) - (wrap < 0), end = jA + 2 + (pl.hi ? pl.sl[1].cnt - 1 : 0);
        if (Oring.b + first < 0 || Oring.b + end > Oring.cap) return 4;   // no room: the copying walk re-bases
    }
    return 1;
}

// The new ring of an in-place insert, built in the old ring's window after retire() has read it (subdiv2d.h): O is the
// old ring, S the scratch buffer with the swapped links' leaves, ho_plan / ho_jD / ho_jA what ho_fast<true> found.
// Leaves the position (relative to the new window) and kind of recentEdge = e0 in s_out / kind_out.
AOS_AVX2 void Subdiv2D::ho_apply(Ring &Oring, Ring &Sring, int shift, int e0, int c, int &s_out, int &kind_out) {
    const RingP o = ring_ptrs(Oring), sc = ring_ptrs(Sring);
    const HoPlan &pl = ho_plan;
    const V2d *const V = vd.data();
    const int k = pl.k, jD = pl.jD, jA = pl.jA;
    const int dlo = pl.lo ? pl.sl[0].cnt - 1 : 0, dhi = pl.hi ? pl.sl[1].cnt - 1 : 0;
    const bool mlo = pl.lo && pl.sl[0].j == jD + 2, mhi = pl.hi && pl.sl[1].j == jA - 1;   // L_jD+1 / L_jA moves
    auto put = [&](int d, int bd, int bu, int ba, int sp, double x, double y, double n, double ax, double ay, double an) {
        o.bd[d] = bd; o.bu[d] = bu; o.ba[d] = ba; o.sp[d] = sp;
        o.x[d] = x; o.y[d] = y; o.n[d] = n; o.ax[d] = ax; o.ay[d] = ay; o.an[d] = an;
    };
    auto move = [&](const RingP &f, int from, int d) {
        put(d, f.bd[from], f.bu[from], f.ba[from], f.sp[from], f.x[from], f.y[from], f.n[from], f.ax[from], f.ay[from], f.an[from]);
    };
    if (pl.wrap) {   // the slots beyond the seam (and the one whose vertex is the end leaf's apex) to the other end
        const int m = Oring.m;
        if (pl.wrap < 0) for (int i = ho_jD - 1; i < m; ++i) move(o, i, i - m);
        else for (int i = 0; i <= ho_jA + 1; ++i) move(o, i, i + m);
#ifdef AOS_SD_PROF
        g_sdprof.ho_slots_written += pl.wrap < 0 ? m - ho_jD + 1 : ho_jA + 2;
        ++g_sdprof.ip_unwrapped;
#endif
        ++n_ip_unwrap;
    }
    // the old values the two end leaves are made of, before anything is written
    const int spD = o.sp[jD], spA = o.sp[jA], uD = o.bu[jD], aD = o.bu[jD - 1], aA = o.bu[jA + 1];
    const double xD = o.x[jD], yD = o.y[jD], nD = o.n[jD], axD = o.x[jD - 1], ayD = o.y[jD - 1], anD = o.n[jD - 1];
    const double axA = o.x[jA + 1], ayA = o.y[jA + 1], anA = o.n[jA + 1];
    // sp over the kept run and slot jD: x_i took S_i+1 for i < k - 1 (ascending copy), Sym S_i-1 for i > k (descending
    // copy: the source overlaps the destination from below); x_k-1 and x_k are roots
    {
        int i = jD;
        for (; i + 8 <= k - 1; i += 8)
            _mm256_storeu_si256((__m256i *)(o.sp + i), _mm256_loadu_si256((const __m256i *)(o.sp + i + 1)));
        for (; i < k - 1; ++i) o.sp[i] = o.sp[i + 1];
        const __m256i two = _mm256_set1_epi32(2);
        for (i = jA; i - 7 >= k + 1; i -= 8)
            _mm256_storeu_si256((__m256i *)(o.sp + i - 7), _mm256_xor_si256(_mm256_loadu_si256((const __m256i *)(o.sp + i - 8)), two));
        for (; i >= k + 1; --i) o.sp[i] = o.sp[i - 1] ^ 2;
    }
    o.sp[k - 1] = V[o.bu[k - 1]].spoke;
    o.sp[k] = V[o.bu[k]].spoke;
    // the low end, in ascending positions: the leaf S_jD, the moved L_jD+1, the swapped link's leaves
    const int pD = jD - dlo;
    put(pD, spD, uD, aD, o.sp[jD], xD, yD, nD, axD, ayD, anD);
    if (mlo) move(o, jD + 1, jD + 1 - dlo);
    if (pl.lo)
        for (int i = 0, d = pl.sl[0].j - dlo; i < pl.sl[0].cnt; ++i) move(sc, pl.sl[0].s0 + i, d + i);
    // the high end, in descending positions: the leaf Sym S_jA, the moved L_jA, the swapped link's leaves
    const int pA = jA + 1 + dhi;
    const V2d &Cv = V[c];
    put(pA, spA ^ 2, c, aA, Cv.spoke, Cv.x, Cv.y, Cv.n2, axA, ayA, anA);
    if (mhi) move(o, jA, jA + dhi);
    if (pl.hi)
        for (int i = pl.sl[1].cnt - 1, d = pl.sl[1].j; i >= 0; --i) move(sc, pl.sl[1].s0 + i, d + i);
#ifdef AOS_SD_PROF
    g_sdprof.ho_slots_written += 2 + mlo + mhi + (pl.lo ? pl.sl[0].cnt : 0) + (pl.hi ? pl.sl[1].cnt : 0);
#endif
    // recentEdge = e0: a leaf (L_k, or a chain's root that did not swap), else the spoke of the vertex that took it
    int s, kind = 0;
    if (shift == 0) s = k == jD + 1 && mlo ? k - dlo : k == jA && mhi ? k + dhi : k;
    else if (shift == 2) {   // e0 = S_k-1: taken by x_k-2
        if (jD == k - 1) s = pD;
        else { kind = 2; s = k - 2 == jD ? pD : k - 2 == jD + 1 && mlo ? k - 2 - dlo : k - 2; }
    } else {                 // e0 = Sym S_k: taken by x_k+1
        if (jA == k) s = pA;
        else { kind = 2; s = k + 1 == jA && mhi ? k + 1 + dhi : pl.hi && pl.sl[1].j == k + 1 ? k + dhi + 1 : k + 1; }
    }
    if ((kind == 0 ? o.bd[s] : o.sp[s]) != e0) {   // (L_k swapped: the spoke of its apex, among its leaves)
        const int m = pA + 1 - pD;
        s = find_int(o.bd + pD, m, e0);
        if (s >= 0) kind = 0; else { kind = 2; s = find_int(o.sp + pD, m, e0); }
        s = s >= 0 ? s + pD : INT_MIN;
    }
    s_out = s == INT_MIN ? -1 : s - pD;
    kind_out = kind;
    Oring.b += pD;
    Oring.m = pA + 1 - pD;
}
#endif   // __x86_64__

AOS_AVX2 static int find_int(const int *a, int m, int v) {   // the first i < m with a[i] == v, or -1
    int i = 0;
#if defined(__x86_64__)
    const __m256i V = _mm256_set1_epi32(v);
    for (; i + 8 <= m; i += 8) {
        const int mask = _mm256_movemask_ps(_mm256_castsi256_ps(_mm256_cmpeq_epi32(_mm256_loadu_si256((const __m256i *)(a + i)), V)));
        if (mask) return i + __builtin_ctz(mask);
    }
#endif
    for (; i < m; ++i) if (a[i] == v) return i;
    return -1;
}

// Cavity form of an INSIDE insert (subdiv2d.h). e0 = locate's edge: p lies left of it, inside the triangle (e0,
// Lnext e0, Lnext^2 e0). The walk starts either through the previous star's arrays (ho_fast, with the hand-over on)
// or, when p does not lie in a fan triangle of the previous insert, from the three roots by cavity_walk; both leave
// the new star's ring in the other buffer, but for a hand-over insert that can build it in the old ring's window
// (ho_fast<true> and ho_apply, subdiv2d.h). Returns false, with nothing of the new star in the records, when the walk meets an apex that
// is already a cavity vertex; the caller then runs the connects and the swap loop.
bool Subdiv2D::insert_cavity(int e0, int p) {
    if (++stamp >= (1 << 29)) {
        flush();   // (the pocket test needs the pending ring's stamps)
        for (V2d &x : vd) x.stamp = 0;
        stamp = 1; ho_stamp = -1;
    }
    int sA = 2 * stamp;
    Ring &O = ho[ho_cur], &N = ho[ho_cur ^ 1];
    int eA = 0, eB = 0, first, v1, v2;
    int shift = -1, k = -1;
    if (loc_k >= 0) {
        // located on the ring arrays (locate_star): slot, rotation and corners without a record read
        const RingP o = ring_ptrs(O);
        k = loc_k - O.b; shift = loc_shift;
        const int xk = o.bu[k], xk1 = o.bu[k - 1], c = ho_c;
        if (shift == 0) { first = xk; v1 = xk1; v2 = c; }         // e0 = L_k
        else if (shift == 2) { first = xk1; v1 = c; v2 = xk; }    // e0 = S_k-1
        else { first = c; v1 = xk; v2 = xk1; }                    // e0 = Sym S_k
    } else {
        eB = lnext(e0); eA = lnext(eB);                // root link edges in walk order: eA, eB, e0
        if (lnext(eA) != e0) return false;
        first = org(e0); v1 = org(eB); v2 = org(eA);
    }
    if (first == v1 || v1 == v2 || v2 == first) { flush(); return false; }
    const size_t cap = vp.size() + 8;
    if (dfs_stack.size() < cap) dfs_stack.resize(2 * cap);
    // the quad-edges the three new_edge() calls below will hand out, so that the roots' spokes are known to the walk
    int cn[3];
    {
        int f = free_q, fresh = (int)rec.size();
        for (int i = 0; i < 3; ++i) {
            if (f > 0) { cn[i] = 4 * f; f = rec[f].h[0].x; }
            else cn[i] = 4 * fresh++;
        }
    }
    V2d &F = vd[first], &A = vd[v1], &B = vd[v2];
    F.stamp = A.stamp = B.stamp = sA;
    F.spoke = cn[0]; A.spoke = cn[1]; B.spoke = cn[2];           // first -> p, v1 -> p, v2 -> p
    const V2d P = vd[p];
    N.b = ring_slack;   // (a walk into the other buffer puts the window back at the slack)
    ring_reserve(N, 8);
    int q = 0, lf = -1;
    bool inplace = false;
    SDP_T0(t_dfs);
    bool fast = loc_k >= 0;
    if (!fast && ho_valid) {
        // the guard: a corner is the previous centre, and the opposite root is the link edge of the slot it carries
        // (the star is not pending here: the generic locate has flushed it)
        int L = 0, asc = 0, desc = 0;
        const int c = ho_c;
        if (v2 == c) { shift = 0; asc = eA; desc = eB; L = e0; }
        else if (v1 == c) { shift = 2; L = eA; asc = eB; desc = e0; }
        else if (first == c) { shift = 1; desc = eA; L = eB; asc = e0; }
        if (shift >= 0) {
            k = (int)((unsigned)chk(ri()[2 * (ptrdiff_t)L + 3]) - (unsigned)O.b);
            const RingP o = ring_ptrs(O);
            fast = (unsigned)k < (unsigned)O.m && o.bd[k] == L && (o.sp[k] ^ 2) == asc && o.sp[k - 1] == desc;
        }
    }
#if defined(__x86_64__)
    if (fast) {
        last_ho_slot = k; last_ho_ring = O.m;
        ho_hz = pending ? ho_stamp : -1;
        ho_pocket = false;
        int res = 1;
        if (use_inpl) {
            res = ho_fast<true>(O, N, k, shift, p, ho_c, sA, q);
            inplace = res == 1;
            if (res == 0) SDP_INC(ip_bail);
            if (res >= 2) {
                ++n_ip_fallback;
                n_rebase += res == 4;
                n_ip_seam += res == 2;
#ifdef AOS_SD_PROF
                ++(res == 2 ? g_sdprof.ip_seam : res == 3 ? g_sdprof.ip_interior : g_sdprof.ip_rebase);
#endif
                // a fresh stamp: the copying walk repeats the tests, and finds the stamps of this attempt older than
                // its own as it would have found the ones before them
                ++stamp;
                sA = 2 * stamp;
                F.stamp = A.stamp = B.stamp = sA;
            }
        }
        if (res >= 1 && !inplace) res = ho_fast<false>(O, N, k, shift, p, ho_c, sA, q);
        if (res == 0) {
            if (ho_pocket) ++n_ho_pocket; else ++n_ho_bail;
            flush();   // (ho_fast has changed no record: the pending ring is still the whole truth)
            ho_valid = false; last_ho_slot = -1;
            return false;
        }
        lf = ho_lf;
    } else
#endif
    {
        flush();
        ho_hz = -1;
        if ((q = cavity_walk(eA, P, sA, N, 0, -1)) < 0 || (q = cavity_walk(eB, P, sA, N, q, ho_lf)) < 0 ||
            (q = cavity_walk(e0, P, sA, N, q, ho_lf)) < 0) {
            ho_valid = false;
            return false;
        }
        lf = ho_lf;
    }
    SDP_ADD(t_dfs, t_dfs);
    SDP_T0(t_wr);
    // The outcome. OpenCV's two connectEdges (after the first newEdge + splice) number the three new quad-edges
    // first -> p, v1 -> p, v2 -> p in that order; everything else they write (the rings of first, v1, v2 and p next to
    // the new edges, their end points, firstEdge) is rewritten by the ring pass, which sets every field of every spoke
    // and the ring links of the boundary edges on both sides of it. So only their allocations are kept.
    const int c0 = new_edge(), c1 = new_edge(), c2 = new_edge();   // (= cn[0 .. 2])
    (void)c0; (void)c1;
    vfirst[p] = sym(lf >= 0 ? lf : c2);   // the last setEdgePoints with p as destination
    if (pending) retire(O, ho_jA, ho_jD);   // (fast: what survives of the old star; the rest is the new ring's to write)
    // only now, with the old ring read for the last time, may an in-place insert write into its window
    int rs = -1, rkind = 0;
#if defined(__x86_64__)
    if (inplace) { ho_apply(O, N, shift, e0, ho_c, rs, rkind); ++n_inplace; SDP_INC(ip_done); }
    else
#endif
    {
        N.m = q;
        ho_cur ^= 1;
#ifdef AOS_SD_PROF
        if (fast) g_sdprof.ho_slots_written += q;
#endif
    }
    Ring &Rn = ho[ho_cur];
    const int m = Rn.m;
    const RingP n = ring_ptrs(Rn);   // (the cyclic copies at the window's ends: HO_PAD spare entries lie outside the buffer's slots)
    n.bd[m] = n.bd[0]; n.bu[m] = n.bu[0]; n.sp[m] = n.sp[0]; n.x[m] = n.x[0]; n.y[m] = n.y[0]; n.n[m] = n.n[0];
    n.bd[-1] = n.bd[m - 1]; n.bu[-1] = n.bu[m - 1]; n.sp[-1] = n.sp[m - 1];
    n.x[-1] = n.x[m - 1]; n.y[-1] = n.y[m - 1]; n.n[-1] = n.n[m - 1];
    ho_c = p; ho_valid = use_ho; ho_stamp = sA;
    n_handover += fast;
    pending = false;
    if (use_ho & use_def) {   // (a star is left pending only where the next insert can walk it)
        // recentEdge = e0 in the new ring: the last leaf if its test did not swap, else the spoke of its apex
        int s = rs, kind = rkind;
        if (!inplace) {
            s = m - 1; kind = 0;
            if (n.bd[s] != e0) { kind = 2; s = find_int(n.sp, m, e0); }
        }
        if (s >= 0) {
            pending = true; rs_kind = kind; rs_slot = Rn.b + s;
            ++n_deferred;
#ifdef AOS_SD_POISON
            for_pending([](int &f) { f = INT_MIN; });
#endif
        }
    }
    static_assert(sizeof(Rec) == 32 && sizeof(Half) == 16 && offsetof(Half, op) == 4 && offsetof(Half, org) == 8 &&
                  offsetof(Half, x) == 12, "slot_fields: Rec layout");
    if (!pending) ring_pass(ri(), vfirst.data(), n.bd, n.bu, n.sp, m, p, Rn.b);
    SDP_ADD(t_write, t_wr);
    return true;
}

// The ring pass on the pending star.
void Subdiv2D::flush() {
    if (!pending) return;
    SDP_T0(t_wr);
    Ring &R = ho[ho_cur];
    const RingP r = ring_ptrs(R);
    ring_pass(ri(), vfirst.data(), r.bd, r.bu, r.sp, R.m, ho_c, R.b);
    pending = false;
    SDP_ADD(t_write, t_wr);
}

// The pending ring O after the next insert has been walked through it: slots jA .. jD (cyclic) kept their spokes. The
// pass restricted to them writes a superset of what the new ring's pass will not write again: of these slots' fields
// only Onext(L_jA), Oprev(Sym L_jD+1) (both links were tested: leaves or spokes of the new ring), Onext / Oprev of
// S_jD and Sym S_jA (link edges of the new ring now) and firstEdge of x_jA, x_jD (new ring vertices) are rewritten.
void Subdiv2D::retire(Ring &O, int jA, int jD) {
    const RingP o = ring_ptrs(O);
    int *const R = ri();
    const int m = O.m, c = ho_c;
#ifdef AOS_SD_PROF
    g_sdprof.ring_slots += m;
    g_sdprof.kept_slots += (jD - jA + m) % m + 1;
#endif
    for (int j = jA;; j = j + 1 == m ? 0 : j + 1) {
        slot_write(R, vfirst.data(), O.b + j, o.bd[j], o.bd[j + 1], o.bu[j], o.sp[j - 1], o.sp[j], o.sp[j + 1], c);
        if (j == jD) break;
    }
}

// f(int &field) over every pending field of ho[ho_cur] (the checkers' poison, and same_state's save and restore)
template <class Fn> void Subdiv2D::for_pending(Fn f) {
    Ring &Rg = ho[ho_cur];
    const RingP r = ring_ptrs(Rg);
    for (int k = 0; k < Rg.m; ++k)
        slot_fields(ri(), vfirst.data(), Rg.b + k, r.bd[k], r.bd[k + 1], r.bu[k], r.sp[k - 1], r.sp[k], r.sp[k + 1], ho_c,
                    [&](int &field, int) { f(field); });
}

// locate()'s loop while it stays inside the pending star of c = ho_c (subdiv2d.h): the current edge is (kind, slot) of
// the ring, its end points and the left face's third vertex come from the ring arrays and c. The predicates are
// locate()'s (same operands, same order); with every sign non-zero its branches reduce to: both right -> found;
// right of Onext only -> Dprev; else Onext. Returns false, having changed nothing, where the generic walk has to run.
bool Subdiv2D::locate_star(float px, float py, int &out_edge) {
    SDP_T0(t_loc);
    Ring &Rg = ho[ho_cur];
    const RingP r = ring_ptrs(Rg);
    const int m = Rg.m;
    const V2d C = vd[ho_c];
    const double x = px, y = py;
    auto rof = [&](double ox, double oy, double dx, double dy) {
        const double cw = (dx - x) * (oy - y) - (dy - y) * (ox - x);
        return (cw > 0) - (cw < 0);
    };
    int kind = rs_kind, s = rs_slot - Rg.b;
    SDP_INC(star_loc);
    double ox = r.x[s], oy = r.y[s], dx, dy;
    if (kind == 0) { dx = r.x[s - 1]; dy = r.y[s - 1]; } else { dx = C.x; dy = C.y; }
    const int roc = rof(ox, oy, dx, dy);
    bool found = false;
    if (roc < 0 || (roc > 0 && kind == 2)) {   // (zero: generic; right of a link edge: Sym L leaves the star)
        if (roc > 0) { kind = 3; std::swap(ox, dx); std::swap(oy, dy); }
        for (int it = 0; it < 2 * m + 8; ++it) {
            SDP_INC(loc_iters);
            SDP_INC(star_steps);
            double ax, ay;
            if (kind == 0) { ax = C.x; ay = C.y; }
            else if (kind == 2) { ax = r.x[s + 1]; ay = r.y[s + 1]; }
            else { ax = r.x[s - 1]; ay = r.y[s - 1]; }
            const int ron = rof(ox, oy, ax, ay);   // Onext: o -> a
            const int rod = rof(ax, ay, dx, dy);   // Dprev: a -> d
            if (ron == 0 || rod == 0) break;
            if (ron > 0 && rod > 0) { found = true; break; }
            if (ron > 0) {   // Dprev
                if (kind == 3) break;                                       // Sym L_s
                if (kind == 0) { kind = 3; s = s ? s - 1 : m - 1; }         // L_s -> Sym S_s-1
                else s = s + 1 == m ? 0 : s + 1;                            // S_s -> S_s+1
                ox = ax; oy = ay;
            } else {         // Onext
                if (kind == 2) break;                                       // Sym L_s+1
                if (kind == 0) kind = 2;                                    // L_s -> S_s
                else s = s ? s - 1 : m - 1;                                 // Sym S_s -> Sym S_s-1
                dx = ax; dy = ay;
            }
        }
    }
    if (found) {
        const float fox = (float)ox, foy = (float)oy, fdx = (float)dx, fdy = (float)dy;   // (exact: they were floats)
        double t1 = std::fabs(px - fox); t1 += std::fabs(py - foy);
        double t2 = std::fabs(px - fdx); t2 += std::fabs(py - fdy);
        double t3 = std::fabs(fox - fdx); t3 += std::fabs(foy - fdy);
        if (t1 < FLT_EPSILON || t2 < FLT_EPSILON ||
            ((t1 < t3 || t2 < t3) && std::fabs(tri_area(px, py, fox, foy, fdx, fdy)) < FLT_EPSILON))
            found = false;   // a vertex or on an edge
    }
    if (found) {
        // the left face of L_s and of Sym S_s is fan triangle s, that of S_s is triangle s + 1
        if (kind == 0) { recent = r.bd[s]; loc_k = s; loc_shift = 0; }
        else if (kind == 2) { recent = r.sp[s]; loc_k = s + 1 == m ? 0 : s + 1; loc_shift = 2; }
        else { recent = r.sp[s] ^ 2; loc_k = s; loc_shift = 1; }
        loc_k += Rg.b;
        out_edge = recent;
        SDP_INC(star_found);
    }
    SDP_ADD(t_locate, t_loc);
    return found;
}

// Compared through a flushed view: a pending star's fields are saved, the pass is run, and after the comparison the
// fields are put back, so that the live instance stays exactly as deferred as it was.
bool Subdiv2D::same_state(const Subdiv2D &o) const {
    Subdiv2D *const both[2] = {const_cast<Subdiv2D *>(this), const_cast<Subdiv2D *>(&o)};
    std::vector<int> saved[2];
    for (int i = 0; i < 2; ++i) {
        Subdiv2D &t = *both[i];
        if (!t.pending || (i == 1 && both[1] == both[0])) continue;
        t.for_pending([&](int &f) { saved[i].push_back(f); });
        t.flush();
        t.pending = true;
    }
    const bool eq = same_records(o);
    for (int i = 1; i >= 0; --i) {
        if (saved[i].empty()) continue;
        size_t at = 0;
        both[i]->for_pending([&](int &f) { f = saved[i][at++]; });
    }
    return eq;
}

bool Subdiv2D::same_records(const Subdiv2D &o) const {
    if (rec.size() != o.rec.size() || vp.size() != o.vp.size() || recent != o.recent || free_q != o.free_q ||
        free_p != o.free_p)
        return false;
    for (size_t q = 0; q < rec.size(); ++q)
        for (int d = 0; d < 2; ++d)
            if (rec[q].h[d].on != o.rec[q].h[d].on || rec[q].h[d].op != o.rec[q].h[d].op || rec[q].h[d].org != o.rec[q].h[d].org)
                return false;
    for (size_t v = 0; v < vp.size(); ++v)
        if (vfirst[v] != o.vfirst[v] || vtype[v] != o.vtype[v] || vp[v].x != o.vp[v].x || vp[v].y != o.vp[v].y)
            return false;
    return true;
}

// OpenCV quad-edge layout: next[r] = Onext of rotation r of quad-edge q. Primal rotations come
// straight from the rings; Onext(Rot e) = Rot^-1 Oprev(e) gives the dual ones. pt[0] / pt[2] are
// the primal end points; the dual pt[1] / pt[3] (Voronoi vertices) start unset (calcVoronoi).
Subdiv2D::Raw Subdiv2D::raw() {
    flush();
    const int n = (int)rec.size();
    qx.assign(8 * (size_t)n, 0);
    auto rot3 = [](int x) { return (x & ~3) + ((x + 3) & 3); };
    for (int q = 1; q < n; ++q) {
        const Rec &r = rec[q];
        int *o = &qx[8 * (size_t)q];
        if (r.h[0].on <= 0) continue;   // free
        o[0] = r.h[0].on; o[1] = rot3(r.h[0].op); o[2] = r.h[1].on; o[3] = rot3(r.h[1].op);
        o[4] = r.h[0].org; o[6] = r.h[1].org;
    }
    return Raw{qx.data(), n, reinterpret_cast<const float *>(vp.data()), vfirst.data(), vtype.data(), (int)vp.size()};
}

// Records [q0, q1) in OpenCV's layout {next[4], pt[4]} (free ones and #0 as zeros). The AVX2 form moves a record
// with one load, one permute and one store (round 5: the export is on the frame's path between the last insert and
// the GPU facet builder).
static void export_recs_scalar(const int *R, int *out, int q0, int q1) {
    auto rot3 = [](int x) { return (x & ~3) + ((x + 3) & 3); };
    for (int q = q0; q < q1; ++q) {
        const int *r = R + 8 * (size_t)q;   // {on, op, org, x} of Sym-direction 0, then 1
        int o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (q > 0 && r[0] > 0) {
            o[0] = r[0]; o[1] = rot3(r[1]); o[2] = r[4]; o[3] = rot3(r[5]);
            o[4] = r[2]; o[6] = r[6];
        }
        std::memcpy(out + 8 * (size_t)q, o, sizeof(o));
    }
}
#if defined(__x86_64__)
AOS_AVX2 static void export_recs_avx2(const int *R, int *out, int q0, int q1) {
    if (q0 == 0 && q1 > 0) { export_recs_scalar(R, out, 0, 1); q0 = 1; }
    const __m256i perm = _mm256_setr_epi32(0, 1, 4, 5, 2, 0, 6, 0);   // on0 op0 on1 op1 org0 . org1 .
    const __m256i keep = _mm256_setr_epi32(-1, -1, -1, -1, -1, 0, -1, 0);
    const __m256i m3 = _mm256_set1_epi32(3), not3 = _mm256_set1_epi32(~3), zero = _mm256_setzero_si256();
    for (int q = q0; q < q1; ++q) {
        const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(R + 8 * (size_t)q));
        const __m256i w = _mm256_permutevar8x32_epi32(v, perm);
        const __m256i rot = _mm256_add_epi32(_mm256_and_si256(w, not3), _mm256_and_si256(_mm256_add_epi32(w, m3), m3));
        __m256i o = _mm256_and_si256(_mm256_blend_epi32(w, rot, 0x0a), keep);
        const __m256i live = _mm256_cmpgt_epi32(_mm256_permutevar8x32_epi32(v, zero), zero);   // on0 > 0
        o = _mm256_and_si256(o, live);
        _mm256_storeu_si256(reinterpret_cast<__m256i *>(out + 8 * (size_t)q), o);
    }
}
#else
static void export_recs_avx2(const int *R, int *out, int q0, int q1) { export_recs_scalar(R, out, q0, q1); }   // (simd_ok() is false)
#endif

Subdiv2D::Raw Subdiv2D::raw_into(void *dst, int chunk_recs, const std::function<void(size_t, size_t)> &written) const {
    const_cast<Subdiv2D *>(this)->flush();   // (pending state is not observable: the export sees the written star)
    const int n = (int)rec.size(), nv = (int)vp.size();
    int *qe = static_cast<int *>(dst);
    static const bool avx2 = simd_ok();
    const int step = chunk_recs > 0 ? chunk_recs : std::max(n, 1);
    for (int q0 = 0; q0 < n; q0 += step) {
        const int q1 = std::min(n, q0 + step);
        if (avx2) export_recs_avx2(ri(), qe, q0, q1);
        else export_recs_scalar(ri(), qe, q0, q1);
        if (written && q1 < n) written(sizeof(int) * 8 * (size_t)q0, sizeof(int) * 8 * (size_t)(q1 - q0));
    }
    char *p = reinterpret_cast<char *>(qe + 8 * (size_t)n);
    float *vpo = reinterpret_cast<float *>(p);
    std::memcpy(vpo, vp.data(), sizeof(V2f) * (size_t)nv);
    int *vf = reinterpret_cast<int *>(p + sizeof(V2f) * (size_t)nv), *vt = vf + nv;
    std::memcpy(vf, vfirst.data(), sizeof(int) * (size_t)nv);
    std::memcpy(vt, vtype.data(), sizeof(int) * (size_t)nv);
    return Raw{qe, n, vpo, vf, vt, nv};
}

// calcVoronoi on the exported layout (host reference of gvd.hip's builder): quad-edges from #4;
// the first quad-edge touching a triangle computes its circumcentre (pt[3] left face, pt[1] right).
int Subdiv2D::facet_next(int e) const {   // getEdge(e, NEXT_AROUND_LEFT = 0x13) on the exported layout
    const int x = qx[8 * (size_t)(e >> 2) + ((e + 3) & 3)];
    return (x & ~3) + ((x + 1) & 3);
}

void Subdiv2D::calc_voronoi() {
    flush();
    raw();
    const int total = (int)rec.size();
    auto next = [&](int e) { return qx[8 * (size_t)(e >> 2) + (e & 3)]; };
    auto get_e = [&](int e, int t) { const int x = next((e & ~3) + ((e + t) & 3)); return (x & ~3) + ((x + (t >> 4)) & 3); };
    auto pt = [&](int e) -> int & { return qx[8 * (size_t)(e >> 2) + 4 + (e & 3)]; };
    for (size_t i = 0; i < vp.size(); ++i)
        if (vtype[i] > 0) { vfirst[i] = free_p; vtype[i] = -1; free_p = (int)i; }
    for (int q = 4; q < total; q++) {
        if (qx[8 * (size_t)q] <= 0) continue;  // free
        const int e0 = q * 4;
        if (!pt(e0 + 3)) {   // left face
            const int e1 = get_e(e0, 0x13), e2 = get_e(e1, 0x13);
            const V2f a = vp[pt(e0)], b = vp[pt(e0 + 2)], c = vp[pt(e1)], d = vp[pt(e1 ^ 2)];
            float rx, ry;
            if (voronoi_point(a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y, rx, ry)) {
                const int p = new_point(rx, ry, 1);
                pt(e0 + 3) = p;
                qx[8 * (size_t)(e1 >> 2) + 4 + 3 - (e1 & 2)] = p;
                qx[8 * (size_t)(e2 >> 2) + 4 + 3 - (e2 & 2)] = p;
            }
        }
        if (!pt(e0 + 1)) {   // right face
            const int e1 = get_e(e0, 0x31), e2 = get_e(e1, 0x31);
            const V2f a = vp[pt(e0)], b = vp[pt(e0 + 2)], c = vp[pt(e1)], d = vp[pt(e1 ^ 2)];
            float rx, ry;
            if (voronoi_point(a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y, rx, ry)) {
                const int p = new_point(rx, ry, 1);
                pt(e0 + 1) = p;
                qx[8 * (size_t)(e1 >> 2) + 4 + 1 + (e1 & 2)] = p;
                qx[8 * (size_t)(e2 >> 2) + 4 + 1 + (e2 & 2)] = p;
            }
        }
    }
}

// getVoronoiFacetList: per real vertex (vertex order) the ring of Voronoi points, starting at
// rotateEdge(firstEdge, 1) and walking NEXT_AROUND_LEFT; vtx[edgeOrg(t)] (index 0 = the (0,0)
// NULL vertex when a circumcentre was not created).
void Subdiv2D::voronoi_facets(std::vector<int> &off, std::vector<float> &xy) {
    flush();
    calc_voronoi();
    off.assign(1, 0);
    xy.clear();
    const size_t nv = vp.size();
    for (size_t k = 4; k < nv; k++) {
        if (vtype[k] != 0) continue;  // free or virtual
        const int f = vfirst[k], start = (f & ~3) + ((f + 1) & 3);
        int t = start;
        do {
            const int p = qx[8 * (size_t)(t >> 2) + 4 + (t & 3)];
            xy.push_back(vp[p].x); xy.push_back(vp[p].y);
            t = facet_next(t);
        } while (t != start);
        off.push_back((int)(xy.size() / 2));
    }
}

void Subdiv2D::voronoi_edges(std::vector<float> &edges) {
    std::vector<int> off;
    std::vector<float> xy;
    voronoi_facets(off, xy);
    edges.clear();
    for (size_t f = 0; f + 1 < off.size(); ++f) {
        const int b = off[f], n = off[f + 1] - b;
        if (n < 2) continue;
        for (int i = 0; i < n; ++i) {
            const int a = b + i, c = b + (i + 1) % n;
            edges.push_back(xy[2 * a]); edges.push_back(xy[2 * a + 1]); edges.push_back(xy[2 * c]); edges.push_back(xy[2 * c + 1]);
        }
    }
}

}  // namespace aos
