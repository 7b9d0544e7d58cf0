// The frame's input: a host PointCloud2 uploaded into HBM (split by the ROR stage's binned box while it is
// gathered), the prefetch of the next frame's cloud, and the streaming map's ingest (aos_map_append,
// aos_tiled_map_append). seedgen.hip runs the frame on what these leave in the handle's cloud view.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <thread>

#include "aos_ctx.h"
#include "cloud_split.h"
#include "host_pool.h"

using namespace aos;

// Host PointCloud2 -> HBM. A pageable hipMemcpyAsync of the 160 MB C2 cloud runs at ~20 GB/s: the runtime
// stages it through pinned memory on one thread. Here up_threads() threads each take a range of points,
// gather their x, y, z floats (12 of the record's point_step bytes: the only fields the path reads) into
// a ring of kUpSlots pinned 2 MB slots and DMA them on their own streams, so 25 % fewer bytes cross PCIe
// for the common 16-byte record and the device gets a packed float3 cloud (step 12). With the split
// (CloudSplit, default) only the points inside the binned box go into the slots (C2: 49.5 % of the cloud);
// the others go to the (pageable) rest buffer (cloud_split.cpp: AVX-512 compress, 4 records per register). The
// handle's stream waits for all of them. The caller's buffer is only read during the call.
// Round 4 (profiles/r04v_split_ab.txt): C2's upload ends 2.2-2.8 ms after it starts with the split at 8
// threads, 2.4-3.8 ms without it (4 / 8 / 16 threads); the DMA no longer trails the gather.
// Default 16 (the box's core share per GPU): the gather is bound by each core's memory bandwidth (10 M points: 160 MB
// read, 120 MB written), and 16 threads took ~0.8 ms off the C2 frame against 8 (bench A/B, two rounds alternating:
// frame p50 23.19-23.32 -> 22.09-22.13 ms on one box, profiles/r05zb_upload_threads.txt).
int aos_ctx::up_threads() {
    static const int n = [] {
        const char *e = getenv("AOS_UP_THREADS");
        return e ? std::max(1, std::min(kUpThreads, atoi(e))) : std::min(kUpThreads, host_cpu_share());
    }();
    return n;
}

// AOS_STAGED_TOUCH: 1 (default) the staged array is read while the upload DMAs run; 0 never. (Round 4 also
// measured it beside the count pass on a second stream and on the stage's stream before the count pass: both
// slower, profiles/r04h_ror_variants_touch_ab.txt, r04t_touch_placement_ab.txt.)
static int staged_touch_mode() {
    static const int m = [] { const char *e = getenv("AOS_STAGED_TOUCH"); return e ? atoi(e) : 1; }();
    return m;
}

bool aos_ctx::split_enabled() {
    static const bool on = [] { const char *e = getenv("AOS_UP_SPLIT"); return !e || atoi(e) != 0; }();
    return on;
}

// The split's box: the ROR stage's binned box for polygon pg (ror_binned_box: the stage takes its own from there)
bool aos_ctx::split_box(const Poly &pg, float box[6]) const {
    if (!split_enabled()) return false;
    ror_binned_box(frame_geom(pg, P), P, nullptr, box);
    for (int i = 0; i < 6; ++i)
        if (!std::isfinite(box[i])) return false;
    return box[0] <= box[1] && box[2] <= box[3] && box[4] <= box[5];
}

void aos_ctx::CloudSplit::swap_with(CloudSplit &o) {
    std::swap(rest.p, o.rest.p); std::swap(rest.cap, o.rest.cap);
    std::swap(rbeg, o.rbeg); std::swap(rn, o.rn); std::swap(nth, o.nth);
    std::swap(n_front, o.n_front); std::swap(n_all, o.n_all); std::swap(box, o.box);
    std::swap(on, o.on); std::swap(whole, o.whole); std::swap(copied, o.copied); std::swap(copy_pending, o.copy_pending);
}

// Device points of the handle's host cloud that a ROR stage with binned box b reads: the front when b lies
// inside the split's box, else (first time) the rest is copied behind the front on the handle's stream.
uint64_t aos_ctx::cloud_for_box(const float b[6]) {
    CloudSplit &sp = split_cur;
    if (!sp.on || sp.whole) return sp.n_all;
    if (b[0] >= sp.box[0] && b[1] <= sp.box[1] && b[2] >= sp.box[2] && b[3] <= sp.box[3] && b[4] >= sp.box[4] &&
        b[5] <= sp.box[5])
        return sp.n_front;
    uint64_t at = sp.n_front;
    for (int t = 0; t < sp.nth; ++t) {
        if (!sp.rn[t]) continue;
        AOS_HIP(hipMemcpyAsync(cloud_copy.as<char>() + 12 * at, sp.rest.as<char>() + sp.rbeg[t], 12 * sp.rn[t],
                               hipMemcpyHostToDevice, stream));
        at += sp.rn[t];
    }
    if (!sp.copied) AOS_HIP(hipEventCreateWithFlags(&sp.copied, hipEventDisableTiming));
    AOS_HIP(hipEventRecord(sp.copied, stream));
    sp.copy_pending = true;
    sp.whole = true;
    return sp.n_all;
}

void aos_ctx::upload_pack(void *dst, const aos_cloud_view &v, CloudSplit &sp, bool prefetch) {
    // chunks of 2 MB: the last DMAs start soon after the last gather, so the upload ends ~one chunk's DMA after
    // the gather instead of one slot per thread later (8 MB slots: ~1 ms). Every gather thread copies on a stream
    // of its own. (Both were measured with AOS_UP_CHUNK_KB and AOS_UP_STREAMS, removed.)
    constexpr uint64_t kChunkPts = (2048u << 10) / 12;
    const uint64_t n = v.n_points;
    const int nth = up_threads();
    for (int t = 0; t < nth; ++t)
        if (!up.st[t]) {
            AOS_HIP(hipStreamCreateWithFlags(&up.st[t], hipStreamNonBlocking));
            for (int k = 0; k < kUpSlots; ++k) AOS_HIP(hipEventCreateWithFlags(&up.ev[t][k], hipEventDisableTiming));
            AOS_HIP(hipEventCreateWithFlags(&up.done[t], hipEventDisableTiming));
            for (int k = 0; k < kUpSlots; ++k) up.slot[t][k].ensure(12 * kChunkPts);
        }
    // the handle's stream may still read dst (the previous frame): the copies start after it (a prefetch
    // writes the spare buffer, which no queued work reads)
    if (!prefetch) {
        AOS_HIP(hipEventRecord(ev[kEvUploadGate], stream));
        // while the DMAs run (they wait for the gate only): the last frame's staged array is read once so that
        // the scatter's partial-line writes hit the Infinity Cache (launch_rt_touch)
        if (staged_touch_mode() == 1 && ror.staged_max > 0)   // (the last frame's records)
            launch_rt_touch(ror.sorted.as<float4>(),
                            std::min(ror.sorted.cap / sizeof(float4), (size_t)ror.staged_max + 1), stream);
    }
    const uint64_t per = (n + nth - 1) / nth;
    const uint8_t *src = static_cast<const uint8_t *>(v.data);
    // split (CloudSplit): points inside the box go to the slot (the device front), the others to the rest
    const bool split = sp.on;
    if (sp.copy_pending) { AOS_HIP(hipEventSynchronize(sp.copied)); sp.copy_pending = false; }   // rest is read
    float *rest = split ? static_cast<float *>(sp.rest.ensure(12 * (size_t)n + kPackSlack * (nth + 1))) : nullptr;
    const float *box = sp.box;
    const PackLayout lay{v.point_step, v.off_x, v.off_y, v.off_z};
    std::atomic<uint64_t> front{0};
    uint64_t rn[kUpThreads] = {};
    std::exception_ptr err[kUpThreads];
    auto work = [&](int t) {
        try {
            AOS_HIP(hipSetDevice(device));
            hipStream_t ust = up.st[t];
            if (!prefetch) AOS_HIP(hipStreamWaitEvent(ust, ev[kEvUploadGate], 0));
            const uint64_t p0 = std::min(n, per * t), p1 = std::min(n, per * (t + 1));
            float *rr = split ? rest + 3 * p0 + (kPackSlack / 4) * t : nullptr;   // (kPackSlack between runs)
            uint64_t nr = 0;
            int k = 0;
            for (uint64_t c = p0; c < p1; c += kChunkPts, k = (k + 1) % kUpSlots) {
                const uint64_t m = std::min(kChunkPts, p1 - c);
                if (up.used[t][k]) AOS_HIP(hipEventSynchronize(up.ev[t][k]));   // its last DMA is done
                float *o = static_cast<float *>(up.slot[t][k].p);
                uint64_t f = m;
                if (split) {
                    uint64_t r = 0;
                    f = pack_split(src + c * (uint64_t)v.point_step, m, lay, box, o, rr + 3 * nr, &r);
                    nr += r;
                } else {
                    pack_all(src + c * (uint64_t)v.point_step, m, lay, o);
                }
                if (!f) continue;   // (the slot's last DMA, if any, stays its event)
                const uint64_t at = split ? front.fetch_add(f) : c;
                AOS_HIP(hipMemcpyAsync(static_cast<char *>(dst) + 12 * at, o, 12 * f, hipMemcpyHostToDevice, ust));
                AOS_HIP(hipEventRecord(up.ev[t][k], ust));
                up.used[t][k] = true;
            }
            rn[t] = nr;
            AOS_HIP(hipEventRecord(up.done[t], ust));
        } catch (...) { err[t] = std::current_exception(); }
    };
    HostTrace tr{"upload"};
    up_pool.run(nth, work);   // (parked workers: round 4 spawned nth - 1 threads per upload)
    for (int t = 0; t < nth; ++t)
        if (err[t]) std::rethrow_exception(err[t]);
    sp.nth = nth; sp.n_all = n; sp.n_front = split ? front.load() : n; sp.whole = !split;
    for (int t = 0; t < kUpThreads; ++t) {   // (byte offsets of the threads' rest runs)
        sp.rbeg[t] = t < nth ? 12 * std::min(n, per * t) + kPackSlack * t : 0;
        sp.rn[t] = t < nth ? rn[t] : 0;
    }
    tr.mark("gathered");
    if (tr.on) {   // (AOS_TRACE only: wait for the DMAs to see when the cloud is in HBM)
        for (int t = 0; t < nth; ++t) AOS_HIP(hipEventSynchronize(up.done[t]));
        tr.mark("dma_done");
    }
    if (!prefetch)
        for (int t = 0; t < nth; ++t) AOS_HIP(hipStreamWaitEvent(stream, up.done[t], 0));
}

// aos_cloud_prefetch: the host stages and DMAs the next cloud into cloud_next on a background thread
// (the same four-thread uploader), while this frame's kernels and the GVD jobs run.
void aos_ctx::prefetch_start(const aos_cloud_view &v) {
    prefetch_join();
    const size_t bytes = (size_t)v.n_points * v.point_step;
    if (v.on_device || bytes < (32u << 20)) return;   // nothing to hide
    void *dst = cloud_next.ensure(12 * (size_t)v.n_points);
    split_next.on = split_box(poly, split_next.box);   // (the polygon now; ror_stage checks it still holds)
    pf.view = v;
    pf.src = v.data;
    pf.bytes = bytes;
    pf.err = nullptr;
    pf.active = true;
    pf.th = std::thread([this, dst]() {
        try { upload_pack(dst, pf.view, split_next, true); } catch (...) { pf.err = std::current_exception(); }
    });
}

bool aos_ctx::prefetch_join() {
    if (!pf.active) return false;
    pf.th.join();
    pf.active = false;
    if (pf.err) { std::exception_ptr e = pf.err; pf.err = nullptr; std::rethrow_exception(e); }
    return true;
}

void aos_ctx::release_uploader() {
    up_pool.stop();
    for (int t = 0; t < kUpThreads; ++t) {
        if (up.st[t]) {
            (void)hipStreamSynchronize(up.st[t]);
            for (int k = 0; k < kUpSlots; ++k) (void)hipEventDestroy(up.ev[t][k]);
            (void)hipEventDestroy(up.done[t]);
            (void)hipStreamDestroy(up.st[t]);
            up.st[t] = nullptr;
        }
    }
}

// The cloud state is committed only after the upload succeeded: a failed upload leaves no cloud
// (aos_seedgen_reprocess then fails instead of reading a partly copied buffer).
void aos_ctx::set_cloud(const aos_cloud_view &v) {
    have_cloud = false;
    ror.ms.valid = false;
    const uint8_t *dc;
    if (v.on_device) {
        dc = static_cast<const uint8_t *>(v.data);
    } else {
        size_t bytes = (size_t)v.n_points * v.point_step;
        const void *pf_src = pf.src;
        const size_t pf_bytes = pf.bytes;
        const bool same_view = pf_src == v.data && pf_bytes == bytes;
        bool pf_ok = false;
        try {
            pf_ok = prefetch_join();
        } catch (...) {
            if (same_view) throw;   // the prefetch of this very cloud failed; another view's is dropped
        }
        if (pf_ok && same_view) {
            // the prefetched copy of this very view: it becomes the frame's cloud once its DMAs are done
            std::swap(cloud_copy.p, cloud_next.p);
            std::swap(cloud_copy.cap, cloud_next.cap);
            split_cur.swap_with(split_next);
            for (int t = 0; t < up_threads(); ++t) AOS_HIP(hipStreamWaitEvent(stream, up.done[t], 0));
        } else {
            void *dst = cloud_copy.ensure(std::max<size_t>(12 * (size_t)v.n_points, 16));
            split_cur.on = bytes && split_box(poly, split_cur.box);
            split_cur.whole = true; split_cur.n_all = split_cur.n_front = 0;   // (until the upload succeeds)
            if (bytes) upload_pack(dst, v, split_cur);
        }
        dc = cloud_copy.as<uint8_t>();
    }
    n_points = v.n_points;
    if (v.on_device) { step = v.point_step; ox = v.off_x; oy = v.off_y; oz = v.off_z; }
    else { step = 12; ox = 0; oy = 4; oz = 8; }   // packed by upload_pack
    is_dense = v.is_dense ? 1 : 0;
    d_cloud = dc;
    have_cloud = true;
}

// Streaming ingest: append one scan to the device-resident map (aos_map_append) and make the map
// this frame's cloud. Only the scan crosses PCIe; the map grows by 1.5x when full.
void aos_ctx::map_grow(uint64_t n) {
    if (map_n + n <= map_buf.cap / sizeof(float4)) return;
    const uint64_t want = std::max<uint64_t>(map_n + n, map_n + map_n / 2);
    DevBuf grown;
    void *dst = grown.ensure(sizeof(float4) * std::max<uint64_t>(want, 1));
    if (map_n) AOS_HIP(hipMemcpyAsync(dst, map_buf.p, sizeof(float4) * map_n, hipMemcpyDeviceToDevice, stream));
    AOS_HIP(hipStreamSynchronize(stream));
    std::swap(map_buf.p, grown.p);
    std::swap(map_buf.cap, grown.cap);
}

// Room in the map for the scan's points, and the scan's records on the device (a host scan is staged first)
static const uint8_t *map_scan_on_device(aos_ctx &c, const aos_cloud_view &v) {
    const uint64_t n = v.n_points;
    c.map_grow(n);   // (a boxed map: an upper bound, every point of the scan may be in the box)
    if (!n || v.on_device) return static_cast<const uint8_t *>(v.data);
    void *st = c.scan_stage.ensure((size_t)n * v.point_step);
    AOS_HIP(hipMemcpyAsync(st, v.data, (size_t)n * v.point_step, hipMemcpyHostToDevice, c.stream));
    return static_cast<const uint8_t *>(st);
}

// The map, `added` packed points longer, becomes the frame's cloud
static void map_becomes_cloud(aos_ctx &c, uint64_t added, bool scan_dense) {
    c.ror.scan_begin = c.map_n;
    c.map_n += added;
    c.map_dense = c.map_dense && scan_dense;
    c.n_points = c.map_n;
    c.step = 16; c.ox = 0; c.oy = 4; c.oz = 8;
    c.is_dense = c.map_dense;
    c.d_cloud = c.map_buf.as<uint8_t>();
    c.have_cloud = true;
}

void aos_ctx::map_append(const aos_cloud_view &v) {
    const uint64_t n = v.n_points;
    if (map_boxed && map_n) throw std::logic_error("aos_map_append on a tiled streaming map (aos_map_reset first)");
    map_boxed = false;
    const uint8_t *src = map_scan_on_device(*this, v);
    launch_pack_xyz(src, n, v.point_step, v.off_x, v.off_y, v.off_z, map_buf.as<float4>() + map_n, stream);
    map_becomes_cloud(*this, n, v.is_dense);
    map_total = map_n;
}

// Tiled streaming map (aos_tiled_map_append, BASELINE configs[4] over several GPUs): every rank receives
// the whole scan (each subscriber of /global_map does) and keeps, on its GPU, the points inside its tile's
// points box — all its tile can rasterise or count as ROR neighbours (make_tile_plan) — so the ROR stage
// of the tiled frame sees exactly the points it would see in the whole map. The box is fixed by the
// polygon the map was started with.
void aos_ctx::map_append_box(const aos_cloud_view &v, const float box[4]) {
    hipStream_t s = stream;
    const uint64_t n = v.n_points;
    if (map_n && (!map_boxed || std::memcmp(map_box, box, sizeof(map_box)))) {
        throw std::invalid_argument(map_boxed ? "tiled streaming map: the tile's points box changed (polygon or tiling); "
                                                "aos_map_reset and append the map again"
                                              : "aos_tiled_map_append on a whole streaming map (aos_map_reset first)");
    }
    map_boxed = true;
    std::memcpy(map_box, box, sizeof(map_box));
    const uint8_t *src = map_scan_on_device(*this, v);
    unsigned long long *d_cnt = static_cast<unsigned long long *>(map_count.ensure(8));
    unsigned long long *h_cnt = static_cast<unsigned long long *>(h_map_count.ensure(8));
    AOS_HIP(hipMemsetAsync(d_cnt, 0, 8, s));
    launch_pack_xyz_box(src, n, v.point_step, v.off_x, v.off_y, v.off_z, box, map_buf.as<float4>() + map_n, d_cnt, s);
    AOS_HIP(hipMemcpyAsync(h_cnt, d_cnt, 8, hipMemcpyDeviceToHost, s));
    AOS_HIP(hipStreamSynchronize(s));
    map_becomes_cloud(*this, *h_cnt, v.is_dense);
    map_total += n;
}
