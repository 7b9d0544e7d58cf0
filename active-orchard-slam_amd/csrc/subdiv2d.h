// Incremental Delaunay / Voronoi facets with OpenCV 4.5.4 cv::Subdiv2D semantics
// (modules/imgproc/src/subdivision2d.cpp, used by aos::VoronoiDiagram::compute,
// src/utils/voronoi_diagram.cpp:51-94).
//
// Why on the host: insertion is inherently sequential and history-dependent — the quad-edge
// numbering, vtx[].firstEdge (which decides where each facet starts) and which edge pair computes
// each circumcentre (float rounding) all depend on the exact locate walk and flip order. Each
// insert's locate walk starts where the previous one ended, so there is no independent work to
// spread. GvdGraph node order follows that history, so bit-identical topology needs this exact
// replay; the GPU takes over from the facet list on (gvd.hip: k_vor_faces, k_facet_*).
//
// Representation: OpenCV stores all four rotations of a quad-edge (primal and dual rings). Only the
// primal rings are stored here, doubly linked (onext and its inverse oprev per directed edge), with
// the same quad-edge ids (directed edge e = 4q + {0, 2}). Every navigation the algorithm uses is an
// identity of the edge algebra (Oprev = Rot Onext Rot):
//   Lnext(e) = Oprev(Sym e),  Dprev(e) = Sym Oprev(Sym e),  Lprev(e) = Sym Onext(e),
// and splice(a, b) = swap(Onext a, Onext b) plus the two inverse links: two independent loads and
// four stores instead of OpenCV's two-level dependent chain through the dual ring. The dual links
// are recovered when the structure is exported (Onext(Rot e) = Rot^-1 Oprev(e)). On orchard seed rows
// an insert performs ~56 swaps (~115 flip-loop steps) as each new seed on the next tree line takes
// over the fan of the previous one, so these constant factors are the replay's cost.
//
// Cavity form of the swap loop (insert_cavity, cavity_walk). Every triangle the swap loop tests lies across a
// link edge from the new point p, so it is never incident to p: it is an *old* triangle, untouched
// when it is tested. Each test is therefore a pure function of the triangulation before the insert,
// and the loop is a depth-first pre-order walk of the cavity tree (children in clockwise order
// around p). A read-only DFS over the old structure replays exactly the same tests with the same
// arguments, then the outcome is written in one pass:
//   * the internal edge e through which the walk entered cavity triangle T (directed as the loop's
//     curr_edge) becomes T's apex -> p with pt[dir(e)] = apex (setEdgePoints in swapEdges);
//   * vtx[apex].firstEdge = e, and vtx[p].firstEdge = Sym of the last swap in walk order;
//   * the rings are the cyclic orders of the final star, which the walk order of the boundary
//     (link) edges fixes; the unique onext/oprev values are stored directly.
// The swap loop stays as the reference path (on-edge inserts, and any walk that meets an apex that is
// already a cavity vertex). tools/sdcheck compares the two paths' complete state after every insert.
// There is one form of each part: the flip test (flips(), and ho_test4 whose lanes are that function), the walk
// (cavity_walk, from a link edge, reading the records), and the write (ring_pass over slot_fields()). The walk
// leaves the boundary (link) edges in walk order as a ring in arrays (struct Ring: per slot k the link edge
// L_k = x_k -> x_k-1, its origin, the apex of its untouched right triangle, the spoke S_k = x_k -> centre, and the
// double coordinates and |.|^2 of x_k and of the apex, padded cyclically), and ring_pass writes the star from them:
//   Oprev(S_j) = L_j,  Oprev(Sym S_j) = Sym S_j+1,  Sym Onext(Sym S_j) = S_j-1,  Sym Onext(S_j) = L_j+1.
//
// Hand-over (ho_fast, on by default where the CPU has AVX2; set_handover). On seed rows nearly every point lands in
// a fan triangle of the previous insert's star, and nearly all of the walk's tests lie in that star or on its ring.
// The ring a cavity insert left behind stays valid for the next one (two buffers alternate), and the next insert
// walks the star through it: the same tests with the same operands in the same order, four slots at a time, without
// following oprev / dst / vertex loads, and the new ring is copied from the old one in runs. A link edge that swaps
// leaves the star: cavity_walk runs from it. With the hand-over off, or where the new point does not lie in the
// previous star, cavity_walk runs from the three roots. All of this state is per instance.
//
// Deferred star (set_deferred, on by default with the hand-over). The next insert's pass rewrites about nine tenths of
// what ring_pass writes (on seed rows a ring of 60 slots keeps 4-5 of its spokes), and between two inserts only
// locate() reads records, nearly always inside that star. So with the hand-over on a cavity insert does not run its
// ring pass: the star stays *pending*, described by the ring arrays alone (never with the hand-over off). Pending are
// exactly the fields ring_pass writes, which slot_fields() names: per slot k Onext(L_k), Oprev(Sym L_k+1), the slot
// int of L_k, every field of S_k and Sym S_k, and firstEdge of x_k. All that faces outward from the ring
// (Oprev(L_k), Onext(Sym L_k), the link edges' end points) is valid in the records.
//   * locate() walks its loop on the arrays while it stays in the star (locate_star: same predicate arithmetic and
//     branch order; transitions Onext L_s = S_s, Dprev L_s = Sym S_s-1, Dprev S_s = S_s+1, Onext Sym S_s = Sym S_s-1;
//     Onext S_s and Dprev Sym S_s are Sym L, which leaves the star). Any zero predicate, a step out of the star, or a
//     vertex / on-edge result flushes and restarts the generic walk from the same recentEdge.
//   * The next hand-over insert reads the pending ring O, builds N, and retires O: the spokes between the ends of the
//     ascending and descending chains (slots jA .. jD) did not flip, and the ring pass restricted to those slots writes
//     every field of O's pass that N's pass will not write again. N stays pending.
//   * The generic walk from a swapped link L_j reads only outward fields, unless a swap's apex is a ring vertex of O
//     that is not in the cavity yet (a pocket of a non-convex star): its child edge can be Sym L_i, whose Oprev is
//     pending. Ring vertices carry O's stamp, so the swap sees it for free: flush, swap loop (n_ho_pocket).
//   * flush() runs the pass on the pending ring. Everything that reads records generically calls it first.
//
// The ring as a window, and the in-place hand-over (set_inplace, on by default with the hand-over). A ring lives in a
// linear buffer as a window [b, b + m) with slack on both sides, cyclic from its last slot to its first; the cyclic pad
// entries sit at the window's ends. Slot positions are absolute buffer positions: the slot int of a link edge, rs_slot
// and loc_k are positions (the code indexes the window from its first slot). The new ring of a hand-over insert is the
// old ring's run of link slots jD + 1 .. jA carried over unchanged, between two new leaves: S_jD in position jD (same
// origin, new edge and apex) and Sym S_jA in position jA + 1. Where the fan triangle is known and every swapped link
// lies at most one slot from an end of the run, the insert runs in place: ho_fast<true> makes the same tests in the same order with the same stamps but stores nothing into a
// ring (a swapped link's leaves go into the other buffer as scratch), retire() reads the old ring, and only then
// ho_apply() trims the window, shifts sp toward k from both sides (x_i took S_i+1 below k, Sym S_i-1 above it; the
// roots' spokes come from the vertices), writes the two end leaves and moves the leaves of an end-adjacent swapped
// link (and the one carried slot outside it) into place. The seam normally lies in the dropped range jA + 1 .. jD - 1
// (it is where the centre before last sits in the ring); where one chain has crossed it, ho_apply first copies the
// slots beyond the seam to the window's other end, which makes the run contiguous again. Any other outcome (both
// chains across the seam, a swapped link further in, three or more swapped links, no room left in the buffer) takes a
// fresh stamp and runs the copying
// walk into the other buffer, which puts the window back at the slack (that copy is the re-base). A walk that bails
// out has changed neither a record nor a ring in either form.
// -DAOS_SD_POISON (checkers only) stores INT_MIN in every field as it becomes pending and counts record reads that
// return it (sd_poison_reads): a stale read fails deterministically.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#define AOS_SD_HANDOVER 1   // set_handover(), n_handover and n_ho_bail exist (tools/sdcheck/sdprof.cpp)
#define AOS_SD_DEFERRED 1   // set_deferred(), flush(), n_deferred and n_ho_pocket exist
#define AOS_SD_INPLACE 1    // set_inplace(), n_inplace, n_ip_fallback and n_rebase exist

namespace aos {

// per-phase counters of a build with -DAOS_SD_PROF (tools/sdcheck/sdprof.cpp); TSC ticks
struct SdProf {
    unsigned long long t_locate = 0, t_dfs = 0, t_write = 0, loc_iters = 0, dfs_steps = 0;
    // deferred star: locates started on the ring arrays, those that ended there, their steps; slots of the rings that
    // were retired and how many of them kept their spoke
    unsigned long long star_loc = 0, star_found = 0, star_steps = 0, ring_slots = 0, kept_slots = 0;
    // in-place hand-over: inserts done in place, and those of them with a chain across the seam; attempts redone by the copying walk because the seam lay in the kept
    // run, because of a swapped link further in than one slot from an end (or a third one), and for want of room (the
    // re-bases); attempts that bailed out (swap loop); ring slots written by hand-over inserts of either form
    unsigned long long ip_done = 0, ip_unwrapped = 0, ip_seam = 0, ip_interior = 0, ip_rebase = 0, ip_bail = 0, ho_slots_written = 0;
};
extern SdProf g_sdprof;
#ifdef AOS_SD_POISON
extern long sd_poison_reads;   // record reads that returned a pending field's poison (must stay 0)
#endif

class Subdiv2D {
  public:
    Subdiv2D();
    // rect: Subdiv2D(Rect2f) (mode 0) or the implicit Rect2f -> Rect conversion (mode 1)
    void init_delaunay(float rx, float ry, float rw, float rh, int rect_mode);
    // Subdiv2D::insert; returns false where OpenCV throws (the reference catches and skips).
    bool insert(float x, float y);
    // 0: cavity DFS + bulk write (default); 1: always OpenCV's swap loop (reference / cross-check)
    void set_swap_loop(bool on) { flush(); force_loop = on; }
    // walk the previous insert's star through the arrays it left (see above); needs AVX2. Off: every cavity insert
    // walks from its three roots (n_handover stays 0) and no star is left pending
    void set_handover(bool on) { flush(); use_ho = on && simd_ok(); ho_valid = false; }
    // leave a cavity insert's star pending in the ring arrays (see above; only with the hand-over on); off: every
    // insert runs its ring pass
    void set_deferred(bool on) { flush(); use_def = on; }
    // build a hand-over insert's ring in the previous ring's window where that is possible (see above); off: every
    // hand-over insert copies into the other buffer
    void set_inplace(bool on) { flush(); use_inpl = on; }
    // test hook: slots of slack the copying walk leaves below a new window (and at least as many above); small values
    // force re-bases
    void set_ring_slack(int slots) { flush(); ho_valid = false; ring_slack = slots < 1 ? 1 : slots; }
    // test hook: off: an insert with a chain across the window's seam is redone by the copying walk and not built in
    // place from copied ends
    void set_seam_copy(bool on) { seam_copy = on; }
    void flush();                    // writes a pending star into the records (no-op without one)
    bool star_pending() const { return pending; }
    static bool simd_ok() {
#if defined(__x86_64__)
        return __builtin_cpu_supports("avx2");
#else
        return false;
#endif
    }
    // full internal state (for the equivalence checker): rings, end points, firstEdge, recentEdge
    bool same_state(const Subdiv2D &o) const;
    long n_cavity = 0, n_loop = 0;   // inserts done by each path
    long n_handover = 0;             // cavity inserts that walked the previous star's arrays (part of n_cavity)
    long n_ho_bail = 0;              // hand-over walks that met a cavity vertex twice: redone by the swap loop
    long n_deferred = 0;             // inserts that left their star pending (part of n_cavity)
    long n_ho_pocket = 0;            // hand-over walks whose swap had a ring vertex of the pending star as apex: flushed, swap loop
    long n_inplace = 0;              // hand-over inserts that built their ring in place (part of n_handover)
    long n_ip_fallback = 0;          // in-place attempts redone by the copying walk (seam, interior swapped link, re-base)
    long n_rebase = 0;               // of those, the ones that only lacked room in the buffer
    long n_ip_seam = 0;              // and the ones with the window's seam inside the kept run
    long n_ip_unwrap = 0;            // in-place inserts that copied the slots beyond the seam to the window's other end
    int last_ho_slot = -1, last_ho_ring = 0;   // the last insert's fan-triangle slot and ring length (-1: no hand-over)
    // getVoronoiFacetList(idx = {}): per real vertex (in vertex order) the facet polygon.
    // Emits the reference's edge list directly: (p_i, p_{i+1 mod n}) for facets with >= 2 points
    // (voronoi_diagram.cpp:97-114), as float x0, y0, x1, y1. Host reference of the GPU builder.
    void voronoi_edges(std::vector<float> &edges);
    // getVoronoiFacetList(idx = {}) as polygons: facet f (real vertices in vertex order) is the float
    // points xy[2 * off[f] .. 2 * off[f + 1]) (extractCellBoundaries, voronoi_diagram.cpp:288-290).
    void voronoi_facets(std::vector<int> &off, std::vector<float> &xy);
    size_t num_vertices() const { return vp.size(); }
    void reserve(size_t n_points);
    // OpenCV-layout quad-edge state after the inserts, for the GPU facet builder:
    // qe = 8 ints per quad-edge {next[4], pt[4]} (free quad-edges have next[0] = 0), vp = float2.
    struct Raw { const int *qe; int n_rec; const float *vp; const int *vfirst, *vtype; int n_vtx; };
    Raw raw();
    // the same state written straight into dst (raw_bytes() bytes: qe | vp | vfirst | vtype), e.g. the
    // pinned staging buffer of the GPU facet builder: no zero-fill, export buffer or second copy
    size_t raw_bytes() const { return (8 * sizeof(int) * rec.size()) + (sizeof(V2f) + 2 * sizeof(int)) * vp.size(); }
    // written(offset, bytes): called after each chunk_recs records but the last, so that the caller can start
    // copying what is written (the rest, from the last call's end to raw_bytes(), once raw_into returns)
    Raw raw_into(void *dst, int chunk_recs = 0, const std::function<void(size_t, size_t)> &written = {}) const;

  private:
    // (32-byte aligned: a record or a vertex never straddles two cache lines; the C2 replay 26.3-27.0 ->
    // 26.0-26.6 ms on the box, profiles/r04z_replay_dfs.txt)
    // A quad-edge's record holds its two primal directed edges, 16 bytes each: directed edge e (always even, 4q or
    // 4q + 2) sits at byte 8 e of the array, so a field is one load at [base + 8 e + field] with no index arithmetic
    // (round 5: the replay's field accessors took 3-4 instructions each in the {on[2], op[2], org[2]} layout)
    struct alignas(16) Half { int on, op, org, x; };   // x: the free-list link in half 0 of a free record;
                                                       // in a live half: its slot in the last ring it bounded (hand-over)
    struct alignas(32) Rec { Half h[2]; };
    struct V2f { float x, y; };
    struct alignas(32) V2d { double x, y, n2; int stamp, spoke; };   // stamp / spoke: insert_cavity scratch
    std::vector<Rec> rec;
    std::vector<V2f> vp;
    std::vector<V2d> vd;   // exact double copies of vp plus x*x + y*y, for the predicates
    std::vector<int> vfirst, vtype;   // type: -1 free, 0 real, 1 virtual
    std::vector<int> qx;              // export buffer (Raw::qe)
    int free_q = 0, free_p = 0, recent = 0;
    bool force_loop = false;
    // cavity walk scratch: stack of link edges; per vertex (V2d) the spoke, valid while its stamp is this insert's
    std::vector<int> dfs_stack;
    int stamp = 0;
    // the walk's output, and the hand-over's input: two ring buffers that alternate (ho[ho_cur] describes the star of
    // vertex ho_c while ho_valid)
    struct Ring {
        std::vector<int> bd, bu, ba, sp;
        std::vector<double> x, y, n, ax, ay, an;
        int cap = 0, m = 0, b = 0;   // slots in the buffer; the window [b, b + m)
    };
    struct RingP { int *bd, *bu, *ba, *sp; double *x, *y, *n, *ax, *ay, *an; };   // the window's first slot in each array
    Ring ho[2];
    int ho_cur = 0, ho_c = 0, ho_lf = -1;
    bool ho_valid = false, use_ho = simd_ok(), use_inpl = true;
    int ring_slack = 256;
    bool seam_copy = true;
    // what ho_fast<true> found, for ho_apply: the fan triangle's slot, the chain ends and up to two swapped links (slot,
    // first scratch slot in the other buffer, leaves), all relative to the window and unwrapped: where a chain crossed
    // the seam, wrap says which end of the window the slots beyond it are copied to (-1: the top ones below the first
    // slot, 1: the bottom ones above the last), and jD < 0 or jA >= m
    struct HoLink { int j, s0, cnt; };
    struct HoPlan { int k = 0, nsl = 0, jD = 0, jA = 0, wrap = 0; bool lo = false, hi = false; HoLink sl[2]; } ho_plan;   // sl[0]: low end, sl[1]: high end
    // deferred star: ho[ho_cur] is pending; recentEdge as (kind, slot) of that ring; the fan triangle locate_star found
    bool pending = false, use_def = true, ho_pocket = false;
    int rs_kind = 0, rs_slot = 0;    // kind: 0 L_s, 2 S_s, 3 Sym S_s; rs_slot: a position
    int loc_k = -1, loc_shift = 0;   // set by locate_star: the fan triangle's position (loc_k < 0: the generic locate ran)
    int ho_stamp = -1, ho_hz = -1;   // the pending ring's vertex stamp; the stamp cavity_walk treats as a pocket (-1: none)
    int ho_jA = 0, ho_jD = 0;        // ho_fast: the slots where the ascending and descending chains ended
    float tlx = 0, tly = 0, brx = 0, bry = 0;

    static int sym(int e) { return e ^ 2; }
    static int dir(int e) { return (e >> 1) & 1; }
    int *ri() { return reinterpret_cast<int *>(rec.data()); }
    const int *ri() const { return reinterpret_cast<const int *>(rec.data()); }
    int &on(int e) { return ri()[2 * (ptrdiff_t)e]; }
    int &op(int e) { return ri()[2 * (ptrdiff_t)e + 1]; }
    int &orgr(int e) { return ri()[2 * (ptrdiff_t)e + 2]; }
#ifdef AOS_SD_POISON
    static int chk(int v) { sd_poison_reads += v == INT32_MIN; return v; }
#else
    static int chk(int v) { return v; }
#endif
    int onext(int e) const { return chk(ri()[2 * (ptrdiff_t)e]); }
    int oprev(int e) const { return chk(ri()[2 * (ptrdiff_t)e + 1]); }
    int org(int e) const { return chk(ri()[2 * (ptrdiff_t)e + 2]); }
    int dst(int e) const { return chk(ri()[2 * (ptrdiff_t)(e ^ 2) + 2]); }
    int lnext(int e) const { return oprev(sym(e)); }          // NEXT_AROUND_LEFT
    int dprev(int e) const { return sym(oprev(sym(e))); }     // PREV_AROUND_DST
    int lprev(int e) const { return sym(onext(e)); }          // PREV_AROUND_LEFT
    int right_of(float px, float py, int e) const;
    int new_edge();
    int new_point(float x, float y, int type);
    void splice(int a, int b) {
        const int an = chk(on(a)), bn = chk(on(b));
        on(a) = bn; on(b) = an;
        op(bn) = a; op(an) = b;
    }
    void set_pts(int e, int o, int d);
    int connect(int a, int b);
    void swap_edge(int e);
    void delete_edge(int e);
    int locate(float px, float py, int &edge, int &vertex);
    bool locate_star(float px, float py, int &edge);
    void retire(Ring &O, int jA, int jD);
    template <class F> void for_pending(F f);   // f(int &field) over every pending field of ho[ho_cur]
    bool same_records(const Subdiv2D &o) const;
    void swap_loop(int curr_edge, int first_point, int curr_point);
    static RingP ring_ptrs(Ring &r);
    static void ring_reserve(Ring &r, int slots);
    bool insert_cavity(int e0, int curr_point);
    int cavity_walk(int e, const V2d &P, int sA, Ring &N, int q, int last_flip);
    // (x86-64 only) 0: bailed out, 1: done; 2 / 3 / 4: not possible in place (seam / swapped links / no room)
    template <bool INPLACE> int ho_fast(Ring &O, Ring &N, int k, int shift, int p, int c, int sA, int &q_out);
    void ho_apply(Ring &O, Ring &S, int shift, int e0, int c, int &s_out, int &kind_out);
    void calc_voronoi();   // calcVoronoi on the exported layout (qx), creating the virtual vertices
    int facet_next(int e) const;
};

}  // namespace aos
