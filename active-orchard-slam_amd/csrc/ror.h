// The radius-outlier-removal (ROR) stage, a1-a4: the kernels' launchers (ror.hip), the status words the
// kernels and the host share, and the stage's per-handle state (ror_stage.hip). Not part of the ABI.
#pragma once
#include <cstddef>

#include "aos_internal.h"
#include "dev_prims.h"

namespace aos {

// ------------------------------------------------------------------ status words
constexpr int kRorCounters = 256;   // spread n_clipped counter slots (k_rt_ror)
// Bits of the stage's flags word (RorStatus::flags, written through RorLaunch::overflow and the column scan's
// look-back err word; read back with the frame's stats, ror_collect). Any bit fails the frame's attempt.
enum RorFlag : int {
    kRorStagedOverflow = 1,   // the scatter (or a streaming store's merge) exceeded the staged capacity: redone
    kRorBigTileSeen = 2,      // a tile beyond the LDS capacity was found with big_ok = 0: redone with the big kernels
    kRorStuckLookBack = 4,    // a look-back wait of the column scan exceeded kSpinCap: the frame throws
};
// The device status block (RorStage::counters): the kept-candidate slots, then the three status words.
struct RorStatus { unsigned long long binned, flags, largest_tile; };   // largest_tile: its record count
struct RorCounters {
    unsigned long long kept[kRorCounters];
    RorStatus st;
};
static_assert(sizeof(RorCounters) == 8 * (kRorCounters + 3), "kept slots + three status words, no padding");
// The pinned stats (RorStage::h_stats). peek_to_host fills consecutive ints, so member order is the contract:
// the sizing read-back writes staged, largest_tile; the frame's (ror_stats_to_host) staged, staged again (a
// filler), st.binned, st.flags. binned is ror_collect's result (aos_seedgen_out::n_binned).
struct RorHostStats {
    int binned, unused;
    int staged, largest_tile;
    RorStatus st;
    unsigned long long unused2[3];
    unsigned long long kept[kRorCounters];   // RorCounters::kept, copied with the frame's read-backs
};
static_assert(offsetof(RorHostStats, staged) == 8 && offsetof(RorHostStats, largest_tile) == 12, "peek order");
static_assert(offsetof(RorHostStats, st) == 16 && offsetof(RorHostStats, st.flags) == 24, "peek order");
static_assert(offsetof(RorHostStats, kept) == 64 && sizeof(RorHostStats) == 64 + 8 * kRorCounters, "kept counters");

// ------------------------------------------------------------------ kernels (launchers, ror.hip)
struct RorLaunch {
    const uint8_t *cloud; uint64_t n; uint32_t step, ox, oy, oz; int is_dense;
    float bminx, bminy, bminz, bmaxx, bmaxy, bmaxz, inv_cs; int nbx, nby;
    float cminx, cmaxx, cminy, cmaxy, cminz, cmaxz;
    double r2; float r2f, r2df; int need;   // r2df: largest float f with (double)f <= r2
    float r2cmp;   // the keep test as one compare, d2 <= r2cmp (rt_configure: r2df, or the float below r2f)
    double origin_x, origin_y; float res; int W, H;
    // Ownership (tiled frames, tiled.hip): a kept candidate is counted iff its cell, clamped to the
    // grid, lies in [rx0, rx1) x [ry0, ry1); it is rastered (if inside the grid) into the byte window
    // whose cell (wx0, wy0) is element 0, row pitch Wr. Single-GPU frames own the whole grid.
    int rx0, ry0, rx1, ry1, wx0, wy0, Wr;
    // tile walk (ror.hip): TB x TB bins per tile, ntx x nty tiles; the raster window as bits (Hr rows
    // of WWr words, wx0 a multiple of 64); a tile's LDS raster window (win_rows x win_w words, 0: none)
    int TB, TBs, ntx, nty, ntiles, Hr, WWr, win_rows, win_w;   // TB = 1 << TBs
    int staged_cap; int *overflow;   // staged array capacity; the flags word (RorFlag: | kRorStagedOverflow when the
                                     // scatter exceeds it, | kRorBigTileSeen when a big tile meets big_ok = 0)
    int big_ok;                      // launch the big-tile kernels (ror.hip); 0 skips their five launches
};
constexpr int kRtMaxTiles = 36000;   // tiles per frame (LDS histogram of the partition passes: 144 KB)
void rt_configure(RorLaunch &L, int Hr, int WWr, double est_binned, int force_tb = 0);
int rt_part_blocks(const RorLaunch &L);   // G: workgroups (= cloud chunks) of the partition passes
// H: rt_h_ints ints, G x ntiles (row per workgroup) + G per-workgroup binned counts. The count pass (two
// launches: count, k_rt_colscan) leaves per-tile prefixes over the workgroups in H, the tile starts in ts
// (ntiles + 1 entries, ts[ntiles] = staged total), the binned count and the largest tile in *st; lb: a
// look-back of rt_colscan_words words whose err word gets kRorStuckLookBack on a stuck wait.
size_t rt_h_ints(const RorLaunch &L, int G);
int rt_colscan_words(const RorLaunch &L, int G);
// clr: buffers the count launch zeroes before the stage's later kernels write them (no fill launches)
struct RtClear { uint64_t *w = nullptr; size_t nw = 0; unsigned long long *c = nullptr; int nc = 0; int *k = nullptr; int nk = 0; };
void launch_rt_count(const RorLaunch &L, int *H, int G, int *ts, RorStatus *st, const LookBack &lb, hipStream_t s,
                     const RtClear &clr = RtClear{});
void launch_rt_scatter(const RorLaunch &L, int *H, const int *tstart, int G, float4 *staged, hipStream_t s);
// kept_tile (nullable): per-tile kept counts; dirty (nullable): a tile is counted iff dirty[t+1] > dirty[t]
// scratch: staged-sized; bigbins: rt_bigbins_ints(L) ints (tiles beyond the LDS capacity are sorted there)
size_t rt_bigbins_ints(const RorLaunch &L);
int rt_lds_tile_cap();   // records a tile may hold for k_rt_ror<false> (LDS); larger tiles take the big-tile kernels
// kept_tile != nullptr (a streaming map's store): kept candidates are marked (w = 2) in staged, which
// is rewritten bin-sorted per tile
void launch_rt_ror(const RorLaunch &L, const int *tstart, float4 *staged, float4 *scratch, int *bigbins,
                   uint64_t *rbits, unsigned long long *counters, int *kept_tile, const int *dirty, hipStream_t s);
// streaming map: merge the map's tile store with a scan's partition; n_clipped from per-tile counts
// (cap: new_st capacity in records; a merge that would exceed it writes nothing past it and sets *overflow)
void launch_rt_merge(const float4 *old_st, const int *old_ts, const float4 *scan_st, const int *scan_ts, float4 *new_st,
                     int *new_ts, int ntiles, int cap, int *overflow, hipStream_t s);
void launch_rt_sum_kept(const int *kept_tile, int ntiles, unsigned long long *counters, hipStream_t s);
// reads n staged records (brings their lines into the Infinity Cache before the scatter writes them)
void launch_rt_touch(const float4 *p, size_t n, hipStream_t s);

// ------------------------------------------------------------------ the stage (ror_stage.hip)
// Half-width of the band around the clip box (or a tile's cells) whose points can be ROR
// neighbours of a candidate: r plus slack for the float box arithmetic.
float ror_margin(const aos_params &P);
// Cells a frame rasterises / counts: [rx0, rx1) x [ry0, ry1) (clamped cell), stored into the
// Wr x Hr bit window at cell (wx0, wy0), wx0 a multiple of 64; limit_box: bin only points in box
// (a tile's shard).
struct RorOwn { int rx0, ry0, rx1, ry1, wx0, wy0, Wr, Hr; bool limit_box; float box[4]; };
// The stage's binned box for a frame's geometry and parameters: bminx, bmaxx, bminy, bmaxy, bminz, bmaxz (the
// clip box widened by ror_margin; own (nullable): clamped to a tiled rank's points box). The split upload keeps
// only the points inside it on the device, so the stage and the upload take it from here.
void ror_binned_box(const FrameGeom &g, const aos_params &P, const RorOwn *own, float b[6]);

// Tile store of the streaming map (incremental ROR, ror_stage_append): the map's binned points partitioned by
// ROR tile (own + halo copies, ping-pong), tile starts, kept candidates per tile; valid while the geometry,
// density and raster bits are the ones it was built with
struct MapStore {
    bool valid = false;
    RorLaunch L{};               // geometry it was built with (pointers / counts cleared)
    DevBuf st[2], ts[2], kept, scan_st, scan_H, scan_ts;
    int cur = 0, dense = 1;
    uint64_t n_points = 0;       // map points it covers
    double n_binned = 0;         // binned (own) points it holds
    size_t n_staged = 0;         // staged copies it holds
    // what this frame's ROR stage built, committed by ror_collect after the read-back
    struct Pending {
        bool on = false, incremental = false;
        RorLaunch L{};
        int dense = 1;
        uint64_t n_points = 0;
        int cur = 0;
    } pend;
};

// Per-handle state of the stage (aos_ctx::ror). An aggregate; every buffer frees itself with the handle.
struct RorStage {
    DevBuf bin_count, bin_start;           // H (rt_h_ints) and the tile starts
    DevBuf sorted, scratch, bigbins;       // the staged records, their bin-sorted copy, the big tiles' bins
    DevBuf counters;                       // RorCounters
    LookBackScratch lb;                    // look-back words of the column scan (k_rt_colscan)
    PinnedBuf h_stats;                     // RorHostStats
    RorHostStats *stats() { return static_cast<RorHostStats *>(h_stats.ensure(sizeof(RorHostStats))); }
    double est_binned = 0;                 // binned points of the last frame (sizes the ROR tiles)
    double staged_max = 0;                 // largest staged (own + halo) count seen (sizes the scatter)
    bool big_seen = false;                 // a frame had a ROR tile beyond the LDS capacity (ror.hip big_ok)
    uint64_t skipped = 0;                  // frames that skipped the stage (ror_stage_unchanged)
    uint64_t read = 0;                     // points this frame's partition passes read (aos_seedgen_out::n_ror_read)
    MapStore ms;
    uint64_t scan_begin = 0;               // map points before the last aos_map_append
};

}  // namespace aos
