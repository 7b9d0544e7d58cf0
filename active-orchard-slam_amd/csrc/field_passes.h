// Device code of the two exact distance passes, shared by clearance.hip (the squared distance) and regions.hip (the
// squared distance with its site): the sizes, the wave reductions, the column pass's nearest rows and the row pass's
// block walk. Device only: the host programs read clearance.h and regions.h, never this file.
#pragma once
#include <hip/hip_runtime.h>

#include "clearance.h"

namespace aos {

// (tests/clearance_scenes.py and tests/regions_scenes.py name these sizes: their sweeps run +-1 around each)
constexpr int kFieldBand = 64;     // rows per band: one bit per row of a (band, column) word
constexpr int kFieldTB = 256;      // threads per workgroup, every kernel of the two files
constexpr int kFieldBlock = 64;    // columns per block minimum of the row pass (a wave's cells)
constexpr unsigned kFieldMagNone = 0xFFFF;   // a block minimum's magnitude of a column without an occupied cell

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
    return v;
}

// The column's nearest occupied rows above (<= y) and below (>= y) row y = y0 + r of a band: from the band's word m
// (k_clr_bands) where it has one, else the carries cu / cd (k_clr_carry); -1: none
struct NearestRows { int above, below; };
__device__ __forceinline__ NearestRows band_nearest_rows(unsigned long long m, int cu, int cd, int y0, int r) {
    const unsigned long long lo = m & (~0ull >> (63 - r)), hi = m & (~0ull << r);
    const int above = lo ? y0 + 63 - __clzll((long long)lo) : cu;
    const int below = hi ? y0 + __ffsll((long long)hi) - 1 : cd;
    return {above, below};
}

// The row pass of one workgroup (kFieldTB threads) on row y: the row's column values in LDS with the least magnitude
// of every kFieldBlock columns; a cell scans its own block, then the blocks left and right of it outwards. A block
// whose (distance to the block)^2 + (its least magnitude)^2 cannot win is skipped, and the walk ends once
// (distance to the block)^2 alone cannot win on either side. A wave's 64 cells share their block, so every LDS read
// of the walk is a broadcast. done(x, best) takes each cell's result; returns the thread's maximum d2.
// The policy P:
//   Stored, kNone        a column value and the one of a column without an occupied cell
//   mag(v)               |v| for the block minimum (kFieldMagNone for kNone)
//   Cand                 the best candidate so far, d2 its squared distance (kNone at first)
//   update(c, v, x, xp, y, W)   column xp's value v (from LDS) against c
//   kTies                the prunes admit a bound equal to c.d2 (a candidate of equal d2 may still win)
template <class P, class Done>
__device__ __forceinline__ unsigned field_row_pass(const typename P::Stored *row, int y, int W, Done &&done) {
    __shared__ typename P::Stored vs[clr::kMaxDim];
    __shared__ uint16_t bmin[clr::kMaxDim / kFieldBlock];
    const int tid = threadIdx.x;
    for (int x0 = 0; x0 < W; x0 += kFieldTB) {   // (uniform bounds: every lane takes part in the wave minimum)
        const int x = x0 + tid;
        const int v = x < W ? row[x] : P::kNone;
        if (x < W) vs[x] = (typename P::Stored)v;
        const unsigned wm = wave_min_u32(P::mag(v));
        if ((tid & 63) == 0 && x < W) bmin[x / kFieldBlock] = (uint16_t)wm;
    }
    __syncthreads();
    const int nblk = (W + kFieldBlock - 1) / kFieldBlock;
    auto admits = [](unsigned bound, unsigned best) { return P::kTies ? bound <= best : bound < best; };
    unsigned row_max = 0;
    for (int x = tid; x < W; x += kFieldTB) {
        typename P::Cand c;
        auto scan = [&](int B) {
            const int a = B * kFieldBlock, e = min(W, a + kFieldBlock);
            for (int xp = a; xp < e; ++xp) P::update(c, vs[xp], x, xp, y, W);
        };
        const int bx = x / kFieldBlock;
        scan(bx);
        for (int k = 1;; ++k) {
            const int bl = bx - k, br = bx + k;
            bool any = false;
            if (bl >= 0) {
                const unsigned db = (unsigned)(x - (bl * kFieldBlock + kFieldBlock - 1));
                if (admits(db * db, c.d2)) {
                    any = true;
                    const unsigned gm = bmin[bl];
                    if (gm != kFieldMagNone && admits(db * db + gm * gm, c.d2)) scan(bl);
                }
            }
            if (br < nblk) {
                const unsigned db = (unsigned)(br * kFieldBlock - x);
                if (admits(db * db, c.d2)) {
                    any = true;
                    const unsigned gm = bmin[br];
                    if (gm != kFieldMagNone && admits(db * db + gm * gm, c.d2)) scan(br);
                }
            }
            if (!any) break;
        }
        done(x, c);
        row_max = max(row_max, c.d2);
    }
    return row_max;
}

}  // namespace aos
