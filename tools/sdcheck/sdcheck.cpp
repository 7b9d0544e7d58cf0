// Equivalence checker for aos::Subdiv2D's cavity insert (subdiv2d.h): the same seeds go into two
// instances, one forced onto OpenCV's swap loop, and the complete internal state (rings, end points,
// firstEdge, recentEdge, free lists) must be equal after every insert. Also times both paths.
// The deferred leg (a hand-over insert's star stays pending in arrays, subdiv2d.h) runs twice: compared after every
// insert (same_state looks through a flushed view and leaves the star pending), and compared only after the last
// insert, so that pending stars follow each other with no call in between. Built with -DAOS_SD_POISON, every pending
// field holds INT_MIN and a record read that returns it fails the case.
// The in-place leg (a hand-over insert builds its ring in the previous ring's window, subdiv2d.h) runs in the same two
// forms; the other legs run with it off, so the copying walk stays the reference it is compared with.
// usage: sdcheck [seeds.bin]   (seeds.bin: int n, n double pairs, 4 double bounds)
#include "subdiv2d.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t sm_state;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni() { return (splitmix() >> 11) * (1.0 / 9007199254740992.0); }

struct Case { const char *name; std::vector<double> s; double b[4]; };

static long g_inplace = 0, g_fallback = 0, g_rebase = 0;   // summed over an in-place leg's cases

static bool check(const Case &c, bool verbose, bool handover, bool deferred, bool every, bool inplace) {
    float rx = (float)(c.b[0] - 1.0), ry = (float)(c.b[2] - 1.0);
    float rw = (float)(std::abs(c.b[1] - c.b[0]) + 2.0), rh = (float)(std::abs(c.b[3] - c.b[2]) + 2.0);
    aos::Subdiv2D a, r;
    a.set_handover(handover);
    a.set_deferred(deferred);
    a.set_inplace(inplace);
    r.set_swap_loop(true);
    const int n = (int)c.s.size() / 2;
    a.reserve(n); r.reserve(n);
    a.init_delaunay(rx, ry, rw, rh, 0); r.init_delaunay(rx, ry, rw, rh, 0);
    for (int i = 0; i < n; ++i) {
        float x = (float)c.s[2 * i], y = (float)c.s[2 * i + 1];
        x = std::max(rx + 0.1f, std::min(rx + rw - 0.1f, x)); y = std::max(ry + 0.1f, std::min(ry + rh - 0.1f, y));
        const bool ka = a.insert(x, y), kr = r.insert(x, y);
        if (ka != kr || ((every || i + 1 == n) && !a.same_state(r))) {
            printf("FAIL %s: state differs after insert %d of %d (%.9g, %.9g)\n", c.name, i, n, x, y);
            return false;
        }
    }
    if (!inplace && a.n_inplace) { printf("FAIL %s: %ld inserts in place with the switch off\n", c.name, a.n_inplace); return false; }
    g_inplace += a.n_inplace; g_fallback += a.n_ip_fallback; g_rebase += a.n_rebase;
    if (!deferred && a.n_deferred) { printf("FAIL %s: %ld stars deferred with the switch off\n", c.name, a.n_deferred); return false; }
    std::vector<float> ea, er;
    a.voronoi_edges(ea); r.voronoi_edges(er);
    if (ea.size() != er.size() || memcmp(ea.data(), er.data(), ea.size() * 4)) {
        printf("FAIL %s: facet edges differ\n", c.name);
        return false;
    }
#ifdef AOS_SD_POISON
    if (aos::sd_poison_reads) {
        printf("FAIL %s: %ld record reads returned a pending field\n", c.name, aos::sd_poison_reads);
        aos::sd_poison_reads = 0;
        return false;
    }
#endif
    if (verbose)
        printf("ok   %-22s n=%-7d cavity inserts %ld (hand-over %ld, in place %ld, deferred %ld, bailed out %ld, pockets %ld), swap-loop inserts %ld\n",
               c.name, n, a.n_cavity, a.n_handover, a.n_inplace, a.n_deferred, a.n_ho_bail, a.n_ho_pocket, a.n_loop);
    return true;
}

static double time_inserts(const Case &c, bool loop, bool handover, bool deferred, bool inplace, uint64_t &hash) {
    float rx = (float)(c.b[0] - 1.0), ry = (float)(c.b[2] - 1.0);
    float rw = (float)(std::abs(c.b[1] - c.b[0]) + 2.0), rh = (float)(std::abs(c.b[3] - c.b[2]) + 2.0);
    const int n = (int)c.s.size() / 2;
    double best = 1e30;
    for (int rep = 0; rep < 7; ++rep) {
        aos::Subdiv2D sd;
        sd.set_swap_loop(loop);
        sd.set_handover(handover);
        sd.set_deferred(deferred);
        sd.set_inplace(inplace);
        sd.reserve(n);
        auto t0 = std::chrono::steady_clock::now();
        sd.init_delaunay(rx, ry, rw, rh, 0);
        for (int i = 0; i < n; ++i) {
            float x = (float)c.s[2 * i], y = (float)c.s[2 * i + 1];
            x = std::max(rx + 0.1f, std::min(rx + rw - 0.1f, x)); y = std::max(ry + 0.1f, std::min(ry + rh - 0.1f, y));
            sd.insert(x, y);
        }
        auto t1 = std::chrono::steady_clock::now();
        best = std::min(best, std::chrono::duration<double, std::milli>(t1 - t0).count());
        std::vector<float> e;
        sd.voronoi_edges(e);
        hash = 1469598103934665603ull;
        for (float v : e) { uint32_t u; memcpy(&u, &v, 4); hash = (hash ^ u) * 1099511628211ull; }
    }
    return best;
}

int main(int argc, char **argv) {
    std::vector<Case> cases;
    // random uniform, lattices (co-circular everywhere), lattice rows in row-by-row order (orchard-like),
    // jittered lattices, duplicates / near-duplicates, collinear runs, tiny clusters
    const char *reps_env = getenv("AOS_SDCHECK_REPS");   // (the sanitizer build runs a few repetitions)
    const int reps = reps_env ? atoi(reps_env) : 40;
    for (int rep = 0; rep < reps; ++rep) {
        sm_state = 1000 + rep;
        Case u{"uniform", {}, {0, 50, 0, 50}};
        const int n = 200 + (int)(uni() * 3000);
        for (int i = 0; i < n; ++i) { u.s.push_back(uni() * 50); u.s.push_back(uni() * 50); }
        cases.push_back(u);
        Case g{"lattice", {}, {0, 30, 0, 30}};
        const double sp = 0.25 + uni();
        for (double y = 0; y <= 30; y += sp) for (double x = 0; x <= 30; x += sp) { g.s.push_back(x); g.s.push_back(y); }
        cases.push_back(g);
        Case o{"orchard-rows", {}, {0, 120, 0, 60}};
        const double dx = 0.3 + 0.7 * uni(), dy = 1.5 + 2.5 * uni();
        for (double y = 1; y < 60; y += dy) {
            const bool rev = uni() < 0.5;
            for (double x0 = 1; x0 < 119; x0 += dx) {
                const double x = rev ? 120 - x0 : x0;
                o.s.push_back(x + (uni() < 0.2 ? 0.05 * (uni() - 0.5) : 0)); o.s.push_back(y + (uni() < 0.3 ? 0.3 * (uni() - 0.5) : 0));
                if (uni() < 0.3) { o.s.push_back(x); o.s.push_back(y + dy * 0.5); }
            }
        }
        cases.push_back(o);
        Case j{"jitter-lattice", {}, {0, 40, 0, 40}};
        for (double y = 0; y <= 40; y += 0.5) for (double x = 0; x <= 40; x += 0.5) {
            j.s.push_back(x + 1e-6 * (uni() - 0.5)); j.s.push_back(y + 1e-6 * (uni() - 0.5));
        }
        cases.push_back(j);
        Case d{"dups-collinear", {}, {0, 20, 0, 20}};
        for (int i = 0; i < 1500; ++i) {
            const double r = uni();
            if (r < 0.2 && d.s.size() >= 2) { size_t k = 2 * (size_t)(uni() * (d.s.size() / 2)); d.s.push_back(d.s[k] + (uni() < 0.5 ? 0 : 1e-7)); d.s.push_back(d.s[k + 1]); }
            else if (r < 0.5) { d.s.push_back(uni() * 20); d.s.push_back(10.0); }
            else if (r < 0.6) { const double t = uni() * 20; d.s.push_back(t); d.s.push_back(t); }
            else { d.s.push_back(uni() * 20); d.s.push_back(uni() * 20); }
        }
        cases.push_back(d);
        Case c{"clamped-border", {}, {0, 10, 0, 10}};
        for (int i = 0; i < 800; ++i) { c.s.push_back(uni() * 14 - 2); c.s.push_back(uni() * 14 - 2); }
        cases.push_back(c);
    }
    Case file{"seeds.bin", {}, {0, 0, 0, 0}};
    const char *path = argc > 1 ? argv[1] : nullptr;
    if (path) {
        FILE *f = fopen(path, "rb");
        int n = 0;
        if (!f || fread(&n, 4, 1, f) != 1) { printf("cannot read %s\n", path); return 2; }
        file.s.resize(2 * (size_t)n);
        if (fread(file.s.data(), 8, 2 * (size_t)n, f) != 2 * (size_t)n || fread(file.b, 8, 4, f) != 4) { printf("short %s\n", path); return 2; }
        fclose(f);
        cases.push_back(file);
    }
    int fails = 0;
    // legs: the hand-over with the deferred star and the copying walk (it needs AVX2) compared after every insert and
    // only at the end, the hand-over with a ring pass per insert, then the hand-over off (the cavity walk from the
    // three roots of every insert), then the in-place hand-over (the default path) compared after every insert and only
    // at the end; each against a swap-loop instance fed in step with it.
    static const char *const leg[6] = {"hand-over on, star deferred", "hand-over on, star deferred, compared at the end only",
                                       "hand-over on, ring pass per insert", "hand-over off",
                                       "in place, star deferred", "in place, star deferred, compared at the end only"};
    const bool simd = aos::Subdiv2D::simd_ok();
    for (int pass = simd ? 0 : 3; pass < (simd ? 6 : 4); ++pass) {
        g_inplace = g_fallback = g_rebase = 0;
        for (size_t i = 0; i < cases.size(); ++i)
            fails += !check(cases[i], (pass == 0 || pass == 4) && (i < 6 || i + 1 == cases.size()), pass != 3, pass <= 1 || pass >= 4,
                            pass != 1 && pass != 5, pass >= 4);
        if (pass >= 4) printf("in place %ld, redone by the copying walk %ld (re-bases %ld)\n", g_inplace, g_fallback, g_rebase);
        printf("%zu cases (%s), %d failed so far\n", cases.size(), leg[pass], fails);
    }
    if (path) {
        uint64_t hi = 0, hd = 0, hh = 0, hs = 0, hr = 0;
        const double ti = time_inserts(file, false, true, true, true, hi), td = time_inserts(file, false, true, true, false, hd),
                     th = time_inserts(file, false, true, false, false, hh), ts = time_inserts(file, false, false, false, false, hs),
                     tr = time_inserts(file, true, false, false, false, hr);
        const bool eq = hi == hr && hd == hr && hh == hr && hs == hr;
        printf("%s inserts: in place %.2f ms, deferred %.2f ms, hand-over %.2f ms, hand-over off %.2f ms, swap loop %.2f ms (x%.2f); "
               "facet-edge hash %016llx %s\n",
               path, ti, td, th, ts, tr, tr / ti, (unsigned long long)hi, eq ? "equal" : "DIFFERENT");
        if (!eq) fails++;
    }
    return fails ? 1 : 0;
}
