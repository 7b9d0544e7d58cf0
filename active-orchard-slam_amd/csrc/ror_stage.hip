// The ROR stage of a frame (a1-a4) on the handle's stream: what the three frame drivers (the plain frame, the
// streaming map, a tiled rank) run between the cloud and the raster bits. The kernels are ror.hip's; the state is
// aos_ctx::ror (ror.h). ror_stage queues the passes, the frame's end reads the stats back, ror_collect judges them.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <stdexcept>

#include "aos_ctx.h"

using namespace aos;

namespace aos {

float ror_margin(const aos_params &P) { return (float)(P.ror_radius * 1.01) + 1e-4f; }

void ror_binned_box(const FrameGeom &g, const aos_params &P, const RorOwn *own, float b[6]) {
    const float m = ror_margin(P);
    b[0] = g.minx - m; b[1] = g.maxx + m; b[2] = g.miny - m; b[3] = g.maxy + m;
    b[4] = P.clipping_minz - m; b[5] = P.clipping_maxz + m;
    if (own && own->limit_box) {   // a tile: only the neighbourhood of its own cells
        b[0] = std::max(b[0], own->box[0]); b[2] = std::max(b[2], own->box[1]);
        b[1] = std::min(b[1], own->box[2]); b[3] = std::min(b[3], own->box[3]);
    }
}

}  // namespace aos

// ------------------------------------------------------------------ the steps of ror_stage
// Launch geometry from the frame and the owner's box: the cloud view, the clip and binned boxes, the keep
// test's radii, the grid and the owned cells. (L.n is the whole cloud; ror_stage narrows a split host cloud.)
static RorLaunch launch_geometry(const aos_ctx &c, const FrameGeom &g, const RorOwn &o) {
    const aos_params &P = c.P;
    RorLaunch L{};
    L.cloud = c.d_cloud; L.n = c.n_points; L.step = c.step; L.ox = c.ox; L.oy = c.oy; L.oz = c.oz;
    L.is_dense = c.is_dense;
    L.cminx = g.minx; L.cmaxx = g.maxx; L.cminy = g.miny; L.cmaxy = g.maxy;
    L.cminz = P.clipping_minz; L.cmaxz = P.clipping_maxz;
    float b[6];
    ror_binned_box(g, P, &o, b);
    L.bminx = b[0]; L.bmaxx = b[1]; L.bminy = b[2]; L.bmaxy = b[3]; L.bminz = b[4]; L.bmaxz = b[5];
    L.r2 = P.ror_radius * P.ror_radius;
    L.r2f = (float)(P.ror_radius * P.ror_radius);
    L.r2df = (float)L.r2;
    if ((double)L.r2df > L.r2) L.r2df = std::nextafter(L.r2df, 0.0f);
    L.need = P.ror_min_neighbors + 1;
    L.origin_x = g.origin_x; L.origin_y = g.origin_y; L.res = g.res; L.W = g.W; L.H = g.H;
    L.rx0 = o.rx0; L.ry0 = o.ry0; L.rx1 = o.rx1; L.ry1 = o.ry1; L.wx0 = o.wx0; L.wy0 = o.wy0; L.Wr = o.Wr;
    return L;
}

// The bin grid over the binned box: square bins of side just above r, at most kMaxBinsPerAxis along the longer
// axis (coarser bins stay exact: a neighbour still lies in the 3 x 3 bins), then coarsened by kBinCoarsen until
// the tiles of 32 x 32 bins are within the tile walk's capacity.
constexpr double kMaxBinsPerAxis = 8192.0;
constexpr float kBinCoarsen = 1.25f;
static void bin_grid(RorLaunch &L, double ror_radius) {
    float cs_ = (float)(ror_radius * 1.001);
    const double ext = std::max((double)L.bmaxx - L.bminx, (double)L.bmaxy - L.bminy);
    if (ext / cs_ > kMaxBinsPerAxis) cs_ = (float)(ext / kMaxBinsPerAxis);
    for (;;) {
        L.inv_cs = 1.0f / cs_;
        L.nbx = std::max(1, (int)((L.bmaxx - L.bminx) * L.inv_cs) + 1);
        L.nby = std::max(1, (int)((L.bmaxy - L.bminy) * L.inv_cs) + 1);
        if ((long long)((L.nbx + 31) / 32) * ((L.nby + 31) / 32) <= kRtMaxTiles) break;
        cs_ *= kBinCoarsen;
    }
}

// What a tile store remembers of a launch: its geometry, without the pointers, counts and per-frame choices
static RorLaunch geom_of(RorLaunch x) {
    x.cloud = nullptr; x.n = 0; x.step = x.ox = x.oy = x.oz = 0; x.staged_cap = 0; x.overflow = nullptr;
    x.big_ok = 0;
    return x;
}

// The committed store covers the map up to the last append and was built with this very geometry: the frame
// needs the appended scan only (ror_stage_append), or nothing (ror_stage_unchanged)
static bool store_continues(const aos_ctx &c, const RorLaunch &L) {
    const MapStore &ms = c.ror.ms;
    if (!(ms.dense == c.is_dense && ms.n_points == c.ror.scan_begin && c.n_points >= ms.n_points)) return false;
    const RorLaunch a = geom_of(L), b = ms.L;
    return !std::memcmp(&a, &b, sizeof(RorLaunch));
}

// The staged array holds own + halo copies. With a capacity from an earlier frame that leaves kGuessHeadroom
// over the largest total seen, the scatter runs at once and reports an overflow (the frame is then redone with
// the size it read back, run_seedgen); without one, or when the caller cannot redo (a tiled frame), the size is
// read back first (a host wait) and the array gets kStagedSlack of it plus kStagedPad records.
constexpr double kGuessHeadroom = 1.1, kStagedSlack = 1.15;
constexpr size_t kStagedPad = 1024;
static void size_staged(aos_ctx &c, RorLaunch &L, DevBuf &stage_buf, const int *d_staged_total, const RorStatus *d_st,
                        bool allow_guess, bool map_mode) {
    RorStage &R = c.ror;
    const size_t cap_now = stage_buf.cap / sizeof(float4);
    if (allow_guess && R.staged_max > 0 && cap_now >= (size_t)(R.staged_max * kGuessHeadroom)) return;
    RorHostStats *h = R.stats();
    // the staged total and the largest tile (the latter's slot is rewritten by ror_stats_to_host later)
    peek_to_host(&h->staged, {d_staged_total, reinterpret_cast<const int *>(&d_st->largest_tile)}, c.stream);
    AOS_HIP(hipStreamSynchronize(c.stream));
    // the big-tile kernels only for a frame that has a tile beyond the LDS cap (a tiled rank launched all six
    // on every frame: ~27 us per rank, profiles/r06/r06d_tiling.json)
    if (!map_mode && h->largest_tile <= rt_lds_tile_cap()) L.big_ok = 0;
    const size_t need = (size_t)std::max(h->staged, 1);
    R.staged_max = std::max<double>(R.staged_max, (double)need);
    stage_buf.ensure(sizeof(float4) * (size_t)(need * kStagedSlack + kStagedPad));
}

// The count pass's column-scan look-back: its err word is the frame's flags word (read back with the frame's
// stats), kRorStuckLookBack = a stuck wait (ror_collect throws).
LookBack aos_ctx::ror_lookback(const RorLaunch &L, int G, RorStatus *d_st) {
    LookBack lb = ror.lb.take(rt_colscan_words(L, G), stream);
    lb.err = reinterpret_cast<int *>(&d_st->flags);
    return lb;
}

// a1-a4: ROR restricted to the points that can reach the (own) cells, clip, exclusion discs, raster
// straight into the bit-packed window rbits (o.Hr rows of ceil(o.Wr / 64) words, zeroed here), by the
// tile walk of ror.hip. Records kEvRorCountBegin / CountEnd / ScatterBegin / TilesBegin / TilesEnd around its
// passes and queues the read-back of its stats (RorHostStats; ror_collect reads them after the frame's sync).
void aos_ctx::ror_stage(const FrameGeom &g, const RorOwn &o, uint64_t *rbits, bool allow_guess) {
    hipStream_t s = stream;
    MapStore &ms = ror.ms;
    // binned, staged, ror_collect's status words: all the stage's peeks write
    std::memset(ror.stats(), 0, offsetof(RorHostStats, st.largest_tile));
    RorLaunch L = launch_geometry(*this, g, o);
    if (d_cloud == cloud_copy.as<uint8_t>() && n_points) {   // a host cloud: its split front, or all of it
        const float b[6] = {L.bminx, L.bmaxx, L.bminy, L.bmaxy, L.bminz, L.bmaxz};
        L.n = cloud_for_box(b);
    }
    ror.read = L.n;
    bin_grid(L, P.ror_radius);
    const int WWr = (o.Wr + 63) / 64;

    // ---- which path: the streaming map keeps a tile store across appends (its tile size stays fixed); a tiled
    // rank's map (limit_box) holds the points of its box only
    const bool map_mode = map_n > 0 && d_cloud == map_buf.as<uint8_t>() && n_points == map_n && map_boxed == o.limit_box;
    // the store becomes valid again only in ror_collect, once this frame's read-back shows no overflow
    // (a frame that fails in between leaves it invalid: the next append reprocesses the whole map)
    const bool store_ok = map_mode && ms.valid;
    ms.valid = false;
    ms.pend.on = false;
    // a streaming store keeps its tile size, but only while the bin grid is the one it was built on
    const bool same_bins = store_ok && ms.L.nbx == L.nbx && ms.L.nby == L.nby && ms.L.inv_cs == L.inv_cs &&
                           ms.L.bminx == L.bminx && ms.L.bminy == L.bminy;
    rt_configure(L, o.Hr, WWr, ror.est_binned > 0 ? ror.est_binned : 0.5 * (double)n_points, same_bins ? ms.L.TB : 0);
    // the big-tile kernels run once a frame of this handle has needed them, and on every frame that cannot
    // be redone (a tiled rank, a redo); a frame that finds a big tile without them is redone (ror_collect)
    L.big_ok = ror.big_seen || !allow_guess || o.limit_box;
    if (store_ok && store_continues(*this, L)) {
        ror.read = n_points - ms.n_points;   // (the scan)
        if (n_points > ms.n_points) ror_stage_append(L, rbits);
        else ror_stage_unchanged();
        return;
    }

    // ---- the whole stage: buffers
    const int nt = L.ntiles;
    const int G = rt_part_blocks(L);
    int *d_H = static_cast<int *>(ror.bin_count.ensure(sizeof(int) * rt_h_ints(L, G)));
    int *d_ts = static_cast<int *>(ror.bin_start.ensure(sizeof(int) * (nt + 1)));
    if (map_mode) d_ts = static_cast<int *>(ms.ts[ms.cur].ensure(sizeof(int) * (nt + 1)));
    int *d_kept = map_mode ? static_cast<int *>(ms.kept.ensure(sizeof(int) * nt)) : nullptr;
    DevBuf &stage_buf = map_mode ? ms.st[ms.cur] : ror.sorted;
    RorCounters *d_cnt = static_cast<RorCounters *>(ror.counters.ensure(sizeof(RorCounters)));
    // PCL dense kNN needs k = min_pts + 1 points in the whole cloud (else every point is removed).
    // A tile's shard holds every neighbour of its own candidates, so a shard with fewer points has
    // no keepable candidate either: the local test is exact.
    const bool any = L.n > 0 && !(is_dense && n_points < (uint64_t)L.need);
    // the counters, raster bits and kept counts start at zero: cleared by the count launch (no fills)
    RtClear clr;
    clr.w = rbits; clr.nw = (size_t)o.Hr * WWr;
    clr.c = d_cnt->kept; clr.nc = sizeof(RorCounters) / 8;
    clr.k = d_kept; clr.nk = d_kept ? nt : 0;
    if (!any) {
        AOS_HIP(hipMemsetAsync(d_cnt, 0, sizeof(RorCounters), s));
        AOS_HIP(hipMemsetAsync(rbits, 0, sizeof(uint64_t) * clr.nw, s));
        if (d_kept) AOS_HIP(hipMemsetAsync(d_kept, 0, sizeof(int) * nt, s));
        return;
    }

    // ---- the launches: count, (size the staged array,) scatter, tile pass
    AOS_HIP(hipEventRecord(ev[kEvRorCountBegin], s));
    launch_rt_count(L, d_H, G, d_ts, &d_cnt->st, ror_lookback(L, G, &d_cnt->st), s, clr);
    AOS_HIP(hipEventRecord(ev[kEvRorCountEnd], s));
    size_staged(*this, L, stage_buf, d_ts + nt, &d_cnt->st, allow_guess, map_mode);
    float4 *d_staged = stage_buf.as<float4>();
    L.staged_cap = (int)std::min<size_t>(stage_buf.cap / sizeof(float4), (size_t)INT_MAX);
    // Records are float4 (x, y, z, w = the class). Round 5 measured and removed two other forms (rorbench, C2 cloud,
    // identical raster hashes): 12-byte records with the class recomputed by the tile pass (scatter 89-90 -> 96-97 us,
    // tile pass 122 -> 126: 12-byte accesses are not 16-byte aligned, profiles/r05k_rorbench.txt), and w carrying the
    // record's local bin in its tile so the tile pass does not recompute it (tile pass unchanged at 113-115 us, scatter
    // +2-4 us: the tile pass is not bound by that arithmetic, profiles/r05n_ror_ab.txt).
    float4 *d_scratch = static_cast<float4 *>(ror.scratch.ensure(sizeof(float4) * (size_t)L.staged_cap));
    L.overflow = reinterpret_cast<int *>(&d_cnt->st.flags);
    AOS_HIP(hipEventRecord(ev[kEvRorScatterBegin], s));
    launch_rt_scatter(L, d_H, d_ts, G, d_staged, s);
    AOS_HIP(hipEventRecord(ev[kEvRorTilesBegin], s));
    int *d_big = static_cast<int *>(ror.bigbins.ensure(sizeof(int) * rt_bigbins_ints(L)));
    launch_rt_ror(L, d_ts, d_staged, d_scratch, d_big, rbits, d_cnt->kept, d_kept, nullptr, s);
    AOS_HIP(hipEventRecord(ev[kEvRorTilesEnd], s));
    ror_stats_to_host(d_ts + nt, &d_cnt->st);

    // ---- the pending commit: the store will hold the whole map (committed by ror_collect: no overflow)
    if (map_mode) ms.pend = MapStore::Pending{true, false, geom_of(L), is_dense, n_points, ms.cur};
}

// Streaming map, one appended scan: the keep decision is monotone in the point set
// (adding points only adds neighbours: PCL's kNN distance can only shrink, a radius count only grow),
// and a candidate's neighbours all sit in its own tile's list. So only the scan is partitioned; each
// tile's list becomes old run + scan run (k_rt_merge); only tiles that received scan points (own or
// halo copies) are recounted, OR-ing into the raster bits the map already has; the kept count is the
// sum of the per-tile counts. Equal to reprocessing the whole map (tests/test_gpu_stream.py).
constexpr size_t kScanCopiesMax = 4, kScanPad = 1024;   // a point lands in at most 4 tiles (own + 3 halo)
void aos_ctx::ror_stage_append(RorLaunch L, uint64_t *rbits) {
    hipStream_t s = stream;
    MapStore &ms = ror.ms;
    const int nt = L.ntiles;
    const uint64_t scan_n = n_points - ms.n_points;
    RorLaunch Ls = L;   // the scan's float4 records in the map buffer
    Ls.cloud = map_buf.as<uint8_t>() + sizeof(float4) * ms.n_points;
    Ls.n = scan_n; Ls.step = 16; Ls.ox = 0; Ls.oy = 4; Ls.oz = 8;
    const int G = rt_part_blocks(Ls);
    int *d_H = static_cast<int *>(ms.scan_H.ensure(sizeof(int) * rt_h_ints(Ls, G)));
    int *d_sts = static_cast<int *>(ms.scan_ts.ensure(sizeof(int) * (nt + 1)));
    RorCounters *d_cnt = static_cast<RorCounters *>(ror.counters.ensure(sizeof(RorCounters)));
    // so the scan's staging and the merged store cannot overflow
    const size_t scan_cap = kScanCopiesMax * (size_t)scan_n + kScanPad;
    float4 *d_scan = static_cast<float4 *>(ms.scan_st.ensure(sizeof(float4) * scan_cap));
    const int nxt = ms.cur ^ 1;
    const size_t cap = ms.n_staged + scan_cap;
    if (cap > (size_t)INT_MAX) throw std::runtime_error("streaming map: ROR store exceeds 2^31 points");
    float4 *d_new = static_cast<float4 *>(ms.st[nxt].ensure(sizeof(float4) * cap));
    int *d_nts = static_cast<int *>(ms.ts[nxt].ensure(sizeof(int) * (nt + 1)));
    float4 *d_scratch = static_cast<float4 *>(ror.scratch.ensure(sizeof(float4) * cap));
    Ls.staged_cap = (int)scan_cap;
    Ls.overflow = reinterpret_cast<int *>(&d_cnt->st.flags);
    AOS_HIP(hipEventRecord(ev[kEvRorCountBegin], s));
    RtClear clr;
    clr.c = d_cnt->kept; clr.nc = sizeof(RorCounters) / 8;
    launch_rt_count(Ls, d_H, G, d_sts, &d_cnt->st, ror_lookback(Ls, G, &d_cnt->st), s, clr);
    AOS_HIP(hipEventRecord(ev[kEvRorCountEnd], s));
    AOS_HIP(hipEventRecord(ev[kEvRorScatterBegin], s));
    launch_rt_scatter(Ls, d_H, d_sts, G, d_scan, s);
    AOS_HIP(hipEventRecord(ev[kEvRorTilesBegin], s));
    launch_rt_merge(ms.st[ms.cur].as<float4>(), ms.ts[ms.cur].as<int>(), d_scan, d_sts, d_new, d_nts, nt, (int)cap,
                    Ls.overflow, s);
    L.staged_cap = (int)cap;
    L.overflow = Ls.overflow;
    int *d_big = static_cast<int *>(ror.bigbins.ensure(sizeof(int) * rt_bigbins_ints(L)));
    launch_rt_ror(L, d_nts, d_new, d_scratch, d_big, rbits, d_cnt->kept, ms.kept.as<int>(), d_sts, s);
    launch_rt_sum_kept(ms.kept.as<int>(), nt, d_cnt->kept, s);
    AOS_HIP(hipEventRecord(ev[kEvRorTilesEnd], s));
    ror_stats_to_host(d_nts + nt, &d_cnt->st);
    // committed by ror_collect (the old store ms.st[ms.cur] stays intact until then)
    ms.pend = MapStore::Pending{true, true, ms.L, ms.dense, n_points, nxt};
}

// A streaming map's frame with no new points in the map (a tiled rank whose box the scan missed: ADVICE
// r03): the kept set, the raster bits (ORed into across appends) and the kept count (counters) are the last
// frame's, so the stage is skipped; the store is recommitted as it is.
void aos_ctx::ror_stage_unchanged() {
    for (FrameEvent e : {kEvRorCountBegin, kEvRorCountEnd, kEvRorScatterBegin, kEvRorTilesBegin, kEvRorTilesEnd})
        AOS_HIP(hipEventRecord(ev[e], stream));
    MapStore &ms = ror.ms;
    ror.stats()->staged = (int)ms.n_staged;   // (binned 0 new points and no flags: zeroed by ror_stage)
    ms.pend = MapStore::Pending{true, true, ms.L, ms.dense, n_points, ms.cur};
    ++ror.skipped;
}

// The stage's staged total and its binned count + flags (RorStatus) into the pinned stats, read after the
// frame's sync (ror_collect): one kernel store instead of two copy-engine read-backs
void aos_ctx::ror_stats_to_host(const int *d_staged_total, const RorStatus *d_st) {
    const int *b = reinterpret_cast<const int *>(&d_st->binned), *f = reinterpret_cast<const int *>(&d_st->flags);
    // staged, largest_tile's slot (a filler: the peek writes consecutive ints), st.binned, st.flags
    peek_to_host(&ror.stats()->staged, {d_staged_total, d_staged_total, b, b + 1, f, f + 1}, stream);
}

// After the frame's sync: binned count, staged size, and whether the attempt failed (true: the scatter overflowed
// its guess, or a big tile met a frame without the big-tile kernels; the caller redoes the frame). A stuck
// look-back throws unless throw_stuck is false (a tiled rank: its flags go to every rank first, so all ranks
// fail the frame together instead of one leaving the others in a collective: ADVICE r04).
bool aos_ctx::ror_collect(bool throw_stuck) {
    RorHostStats *h = ror.stats();
    MapStore &ms = ror.ms;
    const unsigned long long flags = h->st.flags;
    double binned = (double)h->st.binned;
    if (ms.pend.on && ms.pend.incremental) binned += ms.n_binned;   // the scan's binned points on top of the map's
    h->binned = (int)binned;
    ror.est_binned = binned;
    ror.staged_max = std::max<double>(ror.staged_max, (double)h->staged);
    if (flags & kRorStuckLookBack) {
        ms.pend.on = false;
        if (throw_stuck) throw std::runtime_error("ROR column scan: a look-back wait exceeded its cap (kSpinCap)");
        return true;
    }
    if (flags & kRorBigTileSeen) ror.big_seen = true;
    if (ms.pend.on && flags == 0) {   // commit the streaming map's tile store
        ms.valid = true;
        ms.L = ms.pend.L;
        ms.dense = ms.pend.dense;
        ms.n_points = ms.pend.n_points;
        ms.cur = ms.pend.cur;
        ms.n_binned = binned;
        ms.n_staged = (size_t)h->staged;
    }
    ms.pend.on = false;
    return flags != 0;
}

// The ABI's names against the passes: ms_ror_bin is the count pass (count + column scan), ms_ror_scatter the
// sizing read-back (if any) + scatter, ms_ror_count the tile pass (the neighbour counts). All 0 for a frame
// that binned nothing (its events may be another frame's). After ror_collect.
void aos_ctx::ror_times(aos_seedgen_out &out) {
    out.n_binned = ror.stats()->binned;
    out.ms_ror_count = out.n_binned ? ms_ev(kEvRorTilesBegin, kEvRorTilesEnd) : 0.0f;
    out.ms_ror_bin = out.n_binned ? ms_ev(kEvRorCountBegin, kEvRorCountEnd) : 0.0f;
    out.ms_ror_scatter = out.n_binned ? ms_ev(kEvRorScatterBegin, kEvRorTilesBegin) : 0.0f;
}
