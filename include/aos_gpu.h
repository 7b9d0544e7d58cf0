/*
 * aos_gpu.h — C ABI of libaos_gpu.so, the MI355X (gfx950) implementation of the AOS
 * seed-gen + GVD hot path.
 *
 * The reference has no plugin/FFI boundary: the path is two rclcpp nodes wired by topics.
 * Each entry point below replaces one reference callback; the rclcpp drop-in wrapper
 * (active-orchard-slam_amd/node/) maps the same topics, QoS and parameter
 * names onto these calls.
 *
 *   aos_seedgen_process   <- AosSeedGenNode::globalMapCallback   src/aos_seed_gen_node.cpp:230-248
 *   aos_set_polygon       <- AosSeedGenNode::explorationAreaCallback (polygon part) :250-277
 *   aos_seedgen_reprocess <- explorationAreaCallback -> processPointCloud(last_cloud) :282-285
 *   aos_gvd_process       <- AosGvdNode::processGraph on the settled inputs of
 *                            voronoiSeedsCallback :84-128, explorationTreeRowsInfoCallback :130-150,
 *                            skeletonizedGridCallback :173-177  (src/aos_gvd_node.cpp:255-318)
 *   aos_gvd_from_seedgen  <- the same, fed directly from this handle's last seed-gen frame
 *                            (device-resident, no serialisation) — the fused pipeline.
 *
 * Conventions
 *  - Plain C types only; no torch / HIP types cross this boundary.
 *  - Status: 0 = OK, < 0 = error (AOS_E_*); aos_last_error() returns a thread-local message.
 *    No C++ exception crosses the ABI. Empty input -> empty outputs with status 0, mirroring the
 *    reference's early returns (gvd:257-259, 273-275, 284-287).
 *  - Inputs are caller-owned and only read during the call. Output arrays are library-owned and
 *    valid until the next call on the same handle or aos_destroy.
 *  - One handle = one device + one HIP stream; a handle is not re-entrant, different handles may
 *    run concurrently (one per GPU).
 *  - There is no CPU fallback: without a usable gfx950 device aos_create fails.
 */
#ifndef AOS_GPU_H
#define AOS_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AOS_OK 0
#define AOS_E_INVALID -1
#define AOS_E_NOMEM -2
#define AOS_E_HIP -3
#define AOS_E_STATE -4
#define AOS_E_RCCL -5

/* Parameters: names and defaults of the reference nodes (seed_gen:69-100, gvd:26,
 * config/aos_planner_params.yaml:55-89). */
typedef struct aos_params {
    float clipping_minz, clipping_maxz;      /* -0.4, 0.5  (seed-gen node override)     */
    float clipping_minx, clipping_maxx;      /* -5, 72    (only used without polygon)   */
    float clipping_miny, clipping_maxy;      /* -10, 20                                  */
    float grid_resolution;                   /* 0.05                                     */
    float inflation_radius;                  /* 0.8                                      */
    double cluster_min_length;               /* 2.0                                      */
    double ror_radius;                       /* 0.2 (hard-coded, seed_gen:238)           */
    int32_t ror_min_neighbors;               /* 2   (hard-coded, seed_gen:239)           */
    int32_t subdiv_rect_mode;                /* 0: Subdiv2D(Rect2f); 1: Rect2f->Rect      */
    double max_graph_publish_rate;           /* 10 Hz (throttle is the wrapper's job)    */
    int32_t gvd_markers;                     /* 1: also publishMarkers' Voronoi cells (gvd:1098-1194),
                                                a second Subdiv2D on its own host thread */
    int32_t thin_graph;                      /* 1 (default): the first thinning batch of a frame is a
                                                replayed hipGraph; 0: plain kernel launches */
    int32_t gvd_count_evals;                 /* 0 (default); 1: the GVD graph phase counts the work of its
                                                searches (aos_gvd_evals_get; a few atomics per workgroup) */
} aos_params;

void aos_default_params(aos_params *p);

typedef struct aos_ctx aos_ctx;

/* PointCloud2 view (fields x, y, z float32 at the given byte offsets). */
typedef struct aos_cloud_view {
    const void *data;        /* n_points * point_step bytes                                   */
    uint64_t n_points;
    uint32_t point_step, off_x, off_y, off_z;
    int32_t is_dense;        /* PointCloud2.is_dense: selects PCL's kNN vs radius ROR branch   */
    int32_t on_device;       /* 1: data is a device pointer on this handle's GPU (no H2D copy) */
} aos_cloud_view;

/* OccupancyGrid.info subset. */
typedef struct aos_grid_info {
    double origin_x, origin_y;
    float resolution;
    uint32_t width, height;
} aos_grid_info;

/* Seed-gen frame outputs. Host arrays are filled only when want_host != 0 (aos_seedgen_process
 * argument); device arrays are always valid (HBM, library-owned). */
typedef struct aos_seedgen_out {
    aos_grid_info info;
    int32_t thin_iters;                  /* Zhang-Suen iterations incl. the final no-change pass */
    uint64_t n_input, n_ror_kept, n_clipped;
    /* grids, int8 {0,100}, row-major x + y*width */
    const int8_t *occupancy;             /* /occupancy_grid (inflated + 5-cell frame)            */
    const int8_t *skeleton;              /* /skeletonized_occupancy_grid (with polygon frame)    */
    const int8_t *d_occupancy, *d_skeleton;
    /* clusters after the length filter, discovery order */
    int32_t n_clusters_all;              /* before the length filter                             */
    int32_t n_bfs_replayed;              /* clusters without the order-free certificate (exact BFS) */
    int32_t n_rows;                      /* tree rows (all_tree_rows order)                      */
    const double *row_center, *row_start, *row_end, *row_length;  /* 2, 2, 2, 1 per row         */
    /* /voronoi_seeds = virtual ++ real(empty) ++ ray ++ endpoint seeds (x, y) */
    int32_t n_virtual, n_ray, n_endpoint, n_voronoi;
    const double *voronoi_xy;
    /* /exploration_tree_rows_info: sorted (start.x, start.y, end.x, end.y) per row */
    const double *rows_info_xy;
    /* /cluster_info: exploration cluster centres sorted by y */
    int32_t n_cluster_info;
    const double *cluster_info_xy;
    /* per-stage device time (ms), HIP events */
    float ms_ror, ms_grid, ms_thin, ms_cluster, ms_seeds, ms_total;
    /* ROR stage (ror.hip): points it binned (near the clip box); device time of the per-tile
     * neighbour counts (k_rt_ror + the big-tile kernels), of the count pass + tile scan (ms_ror_bin)
     * and of the scatter pass (ms_ror_scatter), HIP events on the handle's stream */
    uint64_t n_binned;
    float ms_ror_count;
    float ms_ror_bin, ms_ror_scatter;
    /* thinning launches of this frame: thin_graph = 0 plain launches, 1 the first batch replayed from
     * a hipGraph, 2 that graph captured this frame (then launched); thin_launches = k_thin_block
     * launches issued (8 Zhang-Suen iterations each, launches past convergence return at once) */
    int32_t thin_graph, thin_launches;
    /* points the ROR stage's partition passes read: a host cloud's upload keeps on the device only the
     * points near the clip box of the polygon current at upload time (the others stay in pinned host
     * memory until a frame's box needs them); otherwise every point of the cloud / map */
    uint64_t n_ror_read;
} aos_seedgen_out;

/* GVD inputs when not fed from this handle's seed-gen frame. */
typedef struct aos_gvd_in {
    const double *seeds_xy; int32_t n_seeds;          /* /voronoi_seeds poses (x, y)            */
    const double *rows_info_xy; int32_t n_rows_poses;  /* /exploration_tree_rows_info poses      */
    aos_grid_info info;
    const int8_t *skeleton;                            /* /skeletonized_occupancy_grid data      */
} aos_gvd_in;

/* msg/GvdGraph.msg fields. */
typedef struct aos_gvd_out {
    int32_t published;                   /* 0 when processGraph returns early                   */
    double resolution, origin_x, origin_y;
    int32_t num_nodes, num_edges;
    const double *nodes_xy;
    const int32_t *node_labels, *node_cluster_indices, *node_label_counts;
    int32_t n_label_entries;
    const int32_t *node_label_clusters, *node_label_types;
    const int32_t *edges;                /* 2 per edge                                          */
    const float *edge_lengths, *edge_clearances;
    int32_t n_merged_seeds, n_voronoi_edges, n_boundary_points;
    float ms_merge, ms_delaunay, ms_graph, ms_total;
    float ms_cells;                      /* always 0: the cells finish after the call returns;
                                            see aos_gvd_markers.ms_cells                          */
} aos_gvd_out;

const char *aos_last_error(void);
int aos_create(const aos_params *p, int device, aos_ctx **out);
void aos_destroy(aos_ctx *ctx);
int aos_set_polygon(aos_ctx *ctx, const double *xy, uint32_t n_points);  /* n < 3: ignored (:253) */
int aos_seedgen_process(aos_ctx *ctx, const aos_cloud_view *cloud, int want_host, aos_seedgen_out *out);
int aos_seedgen_reprocess(aos_ctx *ctx, int want_host, aos_seedgen_out *out);
/* aos_gvd_process: AOS_E_INVALID for a negative count or a null array behind a non-empty seed / row list or
 * grid; empty lists are processGraph's early returns (status 0, published 0); non-finite seeds are filtered. */
int aos_gvd_process(aos_ctx *ctx, const aos_gvd_in *in, aos_gvd_out *out);
int aos_gvd_from_seedgen(aos_ctx *ctx, aos_gvd_out *out);
/* Pipelined form: the reference runs seed-gen and the GVD as two nodes, so frame k + 1's seed-gen
 * overlaps frame k's graph. _async snapshots the last seed-gen frame's GVD inputs (seeds, rows,
 * skeleton) and starts the GVD on a worker thread and its own stream; aos_seedgen_process /
 * aos_map_append may run meanwhile. aos_gvd_wait returns that graph (the same as
 * aos_gvd_from_seedgen would have). A synchronous GVD call supersedes every job in flight.
 * Frames are independent, so up to `depth` jobs (aos_gvd_pipeline_depth, default 1) may be in flight,
 * each replaying its Subdiv2D on its own host thread; aos_gvd_wait collects them in start order, and
 * starting one more than `depth` supersedes the oldest. aos_gvd_markers_get / aos_path_plan on the
 * handle's graph use the job aos_gvd_wait collected last, or the newest job if none was collected
 * since it started (they wait for it without collecting it). */
/* Starts copying a host PointCloud2 to the device in the background (a node can start as soon as the
 * message arrives, while the previous frame is processed). The next aos_seedgen_process with a host view
 * joins it: the same view (same data pointer and size) uses that copy instead of uploading (a failed
 * prefetch of it is raised there); another host view drops it (and any error it had) and uploads
 * normally. aos_cloud_prefetch (another cloud or NULL) joins it too and raises its error; aos_destroy
 * joins and drops it;
 * aos_seedgen_process with a device view and aos_map_append leave it in flight. The caller keeps the
 * bytes unchanged until it is joined. Device views and clouds under 32 MB are ignored.
 * cloud = NULL waits for the prefetch in flight and drops it. */
int aos_cloud_prefetch(aos_ctx *ctx, const aos_cloud_view *cloud);
/* The last seed-gen frame's two published OccupancyGrids (W*H bytes each, x + y*width), copied from HBM
 * straight into caller memory — e.g. the data vectors of the outgoing nav_msgs/OccupancyGrid messages
 * (seed_gen:552-577), so a frame run with want_host = 0 publishes without the library's host copies.
 * Either pointer may be null. */
int aos_seedgen_grids_copy(aos_ctx *ctx, int8_t *occupancy, int8_t *skeleton);
int aos_gvd_from_seedgen_async(aos_ctx *ctx);
int aos_gvd_wait(aos_ctx *ctx, aos_gvd_out *out);
int aos_gvd_pipeline_depth(aos_ctx *ctx, int32_t depth);   /* 1..16 GVD jobs in flight */
/* publishMarkers' cells for the GVD calls that follow (aos_params.gvd_markers): 1 = computed in the
 * background after each graph, 0 = not computed. The reference throttles publishGraph + publishMarkers
 * (gvd:306-314, max_graph_publish_rate): a wrapper that publishes 1 frame in n turns them on for the
 * published frames only. A background job keeps the value it had when it started. With 0,
 * aos_gvd_markers_get computes the cells of the current frame on demand (synchronously). */
int aos_gvd_set_markers(aos_ctx *ctx, int32_t on);
/* SURVEY §8d's GVD figure, "pair evaluations": the distance / sample evaluations of the graph phase's searches
 * in the last GVD call that ran with aos_params.gvd_count_evals = 1 (aos_gvd_set_count_evals). ref_* are what
 * the reference evaluates for the same inputs: findNearestBoundaryPoint scans every boundary point for each of
 * the 2E edge ends (gvd:812-824), the pair loop every i < j (gvd:861-894), findVoronoiBoundaryPointNearEndpoint
 * every filtered node once per radius it tries (gvd:686-790); gpu_* are the candidates this build's kernels
 * examined (k_nearest, k_pairs' two passes, k_occupancy's grid samples, k_label_points). */
typedef struct aos_gvd_evals {
    int32_t counted;                      /* 1: the last GVD call counted                                  */
    int32_t n_label_jobs;                 /* 4 per exploration row                                         */
    uint64_t edge_ends, boundary_points, filtered_nodes;   /* 2E, M, M'                                   */
    uint64_t ref_nearest, ref_pairs, ref_labels;
    uint64_t gpu_nearest, gpu_pairs, gpu_samples, gpu_labels;
} aos_gvd_evals;
int aos_gvd_set_count_evals(aos_ctx *ctx, int32_t on);
int aos_gvd_evals_get(aos_ctx *ctx, aos_gvd_evals *out);

/* ---------------------------------------------------------------------------------------------
 * Streaming ingest (BASELINE.json configs[4]). The handle keeps the global
 * map device-resident. Each aos_map_append call uploads only the new scan (packed to x, y, z float4
 * on the GPU), then processes the frame on the whole accumulated map. The outputs equal
 * aos_seedgen_process on the concatenation of the scans (the reference reprocesses its whole
 * global map on every callback, seed_gen:230-248). The map is dense iff every scan was.
 * ------------------------------------------------------------------------------------------- */
int aos_map_reset(aos_ctx *ctx, uint64_t reserve_points);
int aos_map_append(aos_ctx *ctx, const aos_cloud_view *scan, int want_host, aos_seedgen_out *out);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU tiled frame (BASELINE.json configs[3]: 8192^2 in 2 x 4 tiles).
 * One map is split into tiles_x x tiles_y tiles, one rank (process or thread) per tile, each with
 * its own handle on its own GPU. Ranks refresh the halos of their bit-packed grids by all-gathering
 * every tile's border strips, and max-reduce the thinning convergence flags. After thinning, the
 * skeleton and inflated tiles are all-gathered and the root rank finishes the frame on the whole
 * map. The root's outputs are byte-identical to aos_seedgen_process on the whole cloud. The
 * reference has no counterpart: its node processes the whole map on one core (seed_gen:230-248).
 * ------------------------------------------------------------------------------------------- */

/* Communicator supplied by the caller: RCCL over xGMI in production (torch.distributed 'nccl', or
 * ncclAllGather / ncclAllReduce on the same buffers). send_buf / recv_buf are device memory on
 * this rank's GPU, registered once; the library packs into send_buf and reads recv_buf. Both
 * callbacks are collective (every rank makes the same calls in the same order), are called with
 * the handle's stream idle, and must have completed when they return. Return 0 on success.
 * The library calls every non-NULL callback, including the optional ones at the end: fill the struct
 * from a zeroed one (aos_comm_init, or `aos_comm c = {0};`) so that a caller built against an older
 * header leaves the newer fields NULL. aos_rccl_comm's communicator is the library's own: with it, a
 * tiled frame enqueues its collectives on the handle's stream instead (no host wait around them). */
typedef struct aos_comm {
    void *user;
    int32_t rank, world;                 /* world = tiles_x * tiles_y; rank r = tile (r % tiles_x, r / tiles_x) */
    void *send_buf;                      /* >= buf_bytes                                       */
    void *recv_buf;                      /* >= world * buf_bytes                               */
    uint64_t buf_bytes;                  /* >= aos_tile_plan.exchange_bytes                    */
    /* recv_buf[r * bytes, (r + 1) * bytes) = send_buf[0, bytes) of rank r, for every rank r */
    int (*all_gather)(void *user, uint64_t bytes);
    /* element-wise max over ranks of n int32 values in host memory, in place */
    int (*all_reduce_max)(void *user, int32_t *values, int32_t n);
    /* Optional (NULL: the library routes through all_gather instead). Personalised exchange:
     * counts[s * world + d] = bytes rank s sends to rank d, the same world x world matrix on every rank.
     * send_buf holds this rank's blocks for d = 0, 1, ... back to back; on return recv_buf holds the blocks
     * addressed to this rank from s = 0, 1, ... back to back. The library keeps every row sum <= buf_bytes
     * and every column sum <= world * buf_bytes (larger exchanges are split into rounds). RCCL: grouped
     * ncclSend / ncclRecv; torch.distributed: all_to_all_single. Used by the distributed cluster stage to
     * send each long cluster's cells to the one rank that measures (and replays) it. */
    int (*all_to_all)(void *user, const uint64_t *counts);
} aos_comm;
void aos_comm_init(aos_comm *comm);   /* all fields zero / NULL */

/* RCCL communicator (one process per GPU, e.g. a torch.distributed launch): an aos_comm whose
 * exchange buffers live in HBM, all-gather = ncclAllGather over xGMI, max all-reduce =
 * ncclAllReduce(ncclMax) of the int32 flags. Rank 0 makes the id (NCCL_UNIQUE_ID_BYTES = 128 bytes)
 * and hands it to every rank out of band; aos_rccl_create is collective (every rank, at once).
 * RCCL (librccl.so.1) is loaded at run time by aos_rccl_unique_id / aos_rccl_create only. This
 * replaces the in-process group's peer copies when the ranks are separate processes. */
typedef struct aos_rccl aos_rccl;
int aos_rccl_unique_id(uint8_t *id128);
int aos_rccl_create(const uint8_t *id128, int32_t rank, int32_t world, int32_t device, uint64_t buf_bytes,
                    aos_rccl **out);
const aos_comm *aos_rccl_comm(aos_rccl *comm);   /* valid until aos_rccl_destroy */
void aos_rccl_destroy(aos_rccl *comm);

typedef struct aos_tile_plan {
    int32_t tiles_x, tiles_y, rank, tile_x, tile_y;
    int32_t halo_rows, halo_words;       /* halo depth (0 along an untiled dimension)          */
    int32_t row0, row1, word0, word1;    /* own rows and 64-cell words of the map              */
    int32_t win_row0, win_row1, win_word0, win_word1;   /* own tile + halo, clamped to the map */
    double points_box[4];                /* xmin, ymin, xmax, ymax: the points this rank needs  */
    uint64_t exchange_bytes;             /* minimum aos_comm.buf_bytes                         */
    aos_grid_info info;                  /* the whole map                                      */
} aos_tile_plan;

/* Host arithmetic only (no device needed): the tile of `rank` for this polygon (n_poly < 3: the
 * reference's default polygon, seed_gen:196-199) and these parameters. */
int aos_tile_plan_compute(const aos_params *p, const double *poly_xy, uint32_t n_poly, int32_t tiles_x,
                          int32_t tiles_y, int32_t rank, aos_tile_plan *out);
/* One tiled frame on this rank (uses the handle's polygon, see aos_set_polygon). `cloud` must hold
 * every point inside this rank's points_box; points outside it are ignored, so the whole cloud
 * also works. Root: the full aos_seedgen_out, and aos_gvd_from_seedgen works afterwards. Other
 * ranks: info, thin_iters, n_clipped (whole map) and timings only. */
int aos_tiled_seedgen_process(aos_ctx *ctx, const aos_comm *comm, int32_t tiles_x, int32_t tiles_y, int32_t root,
                              const aos_cloud_view *cloud, int want_host, aos_seedgen_out *out);

/* Streaming ingest on a tiled map (BASELINE.json configs[4] over several GPUs). Every rank keeps its own
 * device-resident map of the points inside its tile's points_box (aos_map_reset on the rank's handle
 * starts it) and its own incremental ROR tile store. Each call hands every rank the whole scan (as every
 * subscriber of /global_map receives it); the rank keeps its box's points on the GPU, then runs the tiled
 * frame on its map (halo all-gathers, global thinning convergence, root finishes the frame). The root's
 * outputs equal aos_map_append of the same scans on one GPU (n_input counts every appended point). The
 * box follows from the polygon and the tiling: changing either needs aos_map_reset and a new map. */
int aos_tiled_map_append(aos_ctx *ctx, const aos_comm *comm, int32_t tiles_x, int32_t tiles_y, int32_t root,
                         const aos_cloud_view *scan, int want_host, aos_seedgen_out *out);

/* Where this rank's last tiled frame (aos_tiled_seedgen_process / aos_tiled_map_append) spent its time
 * (no reference counterpart: the reference runs one map on one core). Host wall clock; a collective's
 * time includes the wait for the slowest rank. */
typedef struct aos_tiled_stats {
    float ms_frame;            /* the whole call on this rank                                        */
    float ms_comm_gather;      /* inside aos_comm.all_gather / all_to_all (halo strips, tables, the final
                                  grids, the long clusters' cells)                                    */
    float ms_comm_reduce;      /* inside aos_comm.all_reduce_max (thinning flags, counts, sizes)     */
    int32_t n_gather, n_reduce;
    uint64_t bytes_gather;     /* all-gather / all-to-all payload sent by this rank                  */
    float ms_ror, ms_thin;     /* device stage times (HIP events), as aos_seedgen_out                */
    float ms_cluster;          /* cluster stage, from the final all-gather (device events)           */
    float ms_seeds;            /* root: rows + seeds                                                 */
    float ms_cluster_local;    /* own-tile labelling and piece tables (host clock)                   */
    float ms_cluster_global;   /* union-find, long-cluster statistics and replays (incl. collectives) */
    float ms_replay;           /* of which: this rank's exact BFS replays                            */
    int32_t n_replayed;        /* clusters replayed on this rank                                     */
    int32_t ror_skipped;       /* streaming: 1 if no new point reached this rank's box (stage skipped) */
    int32_t is_root;
    uint64_t bytes_recv;       /* payload this rank received (halo strips, tables, the final tiles on the root, the
                                  owned clusters' cells, records)                                     */
} aos_tiled_stats;
int aos_tiled_stats_get(aos_ctx *ctx, aos_tiled_stats *out);

/* Border union-find of per-tile cluster pieces: the numbering step of the tiled frame's distributed
 * cluster stage (csrc/cluster_dist.hip; it replaces clusterOccupiedCells' whole-map raster scan + BFS
 * labelling, aos_seed_gen_node.cpp:970-1049, for clusters that cross tiles). Host code: no GPU needed.
 * A piece is a tile's 8-connected component of foreground cells, named by its first cell in raster
 * order (y * width + x, distinct over pieces); border_cell[i] (a piece's cell on its tile's edge)
 * belongs to the piece named border_root[i]. Two pieces are one cluster iff two of their border cells
 * are 8-adjacent. piece_cluster[i] = the cluster of piece i, clusters numbered in raster order of
 * their first cell (the reference's discovery order); *n_clusters = their number. */
int aos_cluster_union(int32_t width, int32_t height, int32_t n_pieces, const int32_t *piece_root, int32_t n_border,
                      const int32_t *border_cell, const int32_t *border_root, int32_t *piece_cluster,
                      int32_t *n_clusters);

/* One map over several GPUs from one process (SURVEY §8b's multi-GPU handle). The group owns one
 * handle per tile (devices[r] for rank r = tile (r % tiles_x, r / tiles_x); devices may repeat) and
 * drives the ranks with its own threads and an in-process aos_comm (peer copies over xGMI, host
 * max-reduction). clouds[r] must hold every point in rank r's points_box (aos_group_plan); the whole
 * cloud works too. The root's outputs equal aos_seedgen_process on the whole cloud; aos_group_rank
 * returns a rank's handle for aos_gvd_from_seedgen, markers and path planning on the root. */
typedef struct aos_group aos_group;
int aos_group_create(const aos_params *p, const int32_t *devices, int32_t tiles_x, int32_t tiles_y, aos_group **out);
void aos_group_destroy(aos_group *group);
int aos_group_set_polygon(aos_group *group, const double *xy, uint32_t n_points);
int aos_group_plan(aos_group *group, int32_t rank, aos_tile_plan *out);
aos_ctx *aos_group_rank(aos_group *group, int32_t rank);
int aos_group_process(aos_group *group, const aos_cloud_view *clouds, int32_t root, int want_host,
                      aos_seedgen_out *root_out);
/* The group's tiled streaming map (aos_tiled_map_append on every rank with the same scan). */
int aos_group_map_reset(aos_group *group, uint64_t reserve_points_per_rank);
int aos_group_map_append(aos_group *group, const aos_cloud_view *scan, int32_t root, int want_host,
                         aos_seedgen_out *root_out);

/* /gvd/markers content of the last GVD call (publishMarkers gvd:1012-1591) that is not already in
 * aos_gvd_out; the wrapper adds styles, ids and text. Needs aos_params.gvd_markers = 1.
 * The reference publishes the graph before the markers (gvd:310-313). Likewise a GVD call returns
 * once the graph is ready, and the cells (a second Subdiv2D) finish on a background thread: this
 * call waits for them, and raises their error if they failed. They overlap the next seed-gen
 * frame; the next GVD call and aos_destroy wait for them. The pointers stay valid until then. */
typedef struct aos_gvd_markers {
    int32_t n_seeds; const double *seeds_xy;   /* /gvd_voronoi_seeds: the merged seeds (gvd:1019-1041)        */
    int32_t n_rows;                            /* exploration rows (sorted rows_info pairs)                   */
    const double *row_label_xy;                /* TL, TR, BL, BR boundary points per row, (x, y) x 4          */
    const int32_t *row_label_valid;            /* 4 per row (gvd:1370-1450 draws the valid ones)             */
    int32_t n_cells;                           /* VoronoiDiagram::extractCellBoundaries voronoi_diagram.cpp:209-311 */
    const int32_t *cell_offsets;               /* n_cells + 1, into cell_xy points                            */
    const double *cell_xy;                     /* cell boundary, closed when its ends are > 1 cm apart        */
    const double *cell_center_xy;              /* seeds_[i]: the centre publishMarkers pairs with cell i      */
    const float *cell_rgba;                    /* /gvd_voronoi_cells i colour: HSV(i / n_cells, 0.7, 0.9), a 0.4 */
    float ms_cells;                            /* host time of the cells' Subdiv2D + facets (parallel thread) */
} aos_gvd_markers;
int aos_gvd_markers_get(aos_ctx *ctx, aos_gvd_markers *out);
/* The markers of the frame last returned by aos_gvd_wait (or the last synchronous GVD call), without
 * waiting for the jobs started since: a pipelined caller collects a frame's cells one step later,
 * while the next frames' jobs run (aos_gvd_markers_get would wait for the newest job). */
int aos_gvd_collected_markers_get(aos_ctx *ctx, aos_gvd_markers *out);

/* ---------------------------------------------------------------------------------------------
 * Path planning over the GvdGraph (aos_path_gen_node): graphCallback
 * (path_gen:418-579) = cluster waypoint mapping (:704-765) + waypoint sequence (:588-702) + target
 * restore (:496-560), then planAndPublishPath (:976-1567): weighted A* (:800-896) from the 5 nodes
 * nearest the start (:914-932), the straight 0.2 m segments, orientations, and
 * trimPathNearOccupiedRegions (:1570-1630) on the skeleton. The node's state goes in as
 * aos_path_query; the published /path poses, the status and the indices come out.
 * ------------------------------------------------------------------------------------------- */
typedef struct aos_path_graph {          /* msg/GvdGraph.msg */
    int32_t num_nodes; const double *nodes_xy;
    const int32_t *node_labels, *node_cluster_indices, *node_label_counts;
    int32_t n_label_entries; const int32_t *node_label_clusters, *node_label_types;
    int32_t num_edges; const int32_t *edges; const float *edge_lengths;
} aos_path_graph;

typedef struct aos_path_query {
    int32_t initial_waypoint_reached;    /* 0: straight line (0, 0) -> initial waypoint (:983-1031) */
    double initial_waypoint_xy[2];       /* (8, 0) in the reference (:81-83)                      */
    int32_t target_waypoint_index;       /* current_target_waypoint_index_ before this graph (-1)  */
    int32_t have_saved_target;           /* that index was valid: its position follows            */
    double saved_target_xy[2];
    int32_t previous_waypoint_index;     /* previous_waypoint_index_ (-1: start at the initial waypoint) */
    int32_t use_current_position;        /* service call with a received position (:1062-1066)    */
    double current_xy[2];
    int32_t exploration_completed;       /* the origin (0, 0) ends the sequence (node -1, :1096-1280);
                                            modelled as this graph's sequence plus the origin      */
} aos_path_query;

typedef struct aos_path_out {
    int32_t status;                      /* publishPlanningStatus: 1 "Success", 0 "Failed"          */
    int32_t target_waypoint_index;       /* after the restore                                       */
    int32_t cluster_index;               /* calculateClusterIndex (:1633-1652)                      */
    int32_t n_clusters;                  /* cluster_waypoint_nodes_, ascending cluster id           */
    const int32_t *cluster_ids, *cluster_nodes;   /* 4 per cluster: TL, TR, BL, BR node (-1: none) */
    int32_t n_waypoints; const double *waypoints_xy; const int32_t *waypoint_nodes;
    int32_t n_node_path; const int32_t *node_path;   /* the chosen A* node path                   */
    int32_t n_poses; const double *poses;            /* x, y, qz, qw per /path pose (z = 0)       */
    int32_t trimmed_from;                /* pose count before the trim, or -1                       */
    float ms_plan;
} aos_path_out;

/* graph: NULL = this handle's last GVD graph. skeleton: /skeletonized_occupancy_grid bytes, host
 * memory (skeleton_on_device = 0) or device memory on the handle's GPU (1), with `info`; NULL = the
 * skeleton that graph was built on (AOS_E_STATE if a later seed-gen frame replaced it). On
 * "Failed" the outputs hold no poses: the node republishes its last path. */
int aos_path_plan(aos_ctx *ctx, const aos_path_graph *graph, const int8_t *skeleton, int skeleton_on_device,
                  const aos_grid_info *info, const aos_path_query *query, aos_path_out *out);

/* ---------------------------------------------------------------------------------------------
 * /aos/path -> /plan (aos_path_linearization_node): the path the controller drives on.
 * At most 4 straight segments fitted by regression (10 when the path ends at the origin), resampled at 5 cm.
 * aos_path_linearize <- AosPathLinearizationNode::pathCallback + convertToLinearSegments
 *                       src/aos_path_linearization_node.cpp:372-395, 248-370
 * The node's 1 Hz republish timer, stamps and header copies stay in the wrapper.
 * ------------------------------------------------------------------------------------------- */
typedef struct aos_linear_path_out {
    int32_t published;        /* 0: empty input (pathCallback returns, :373-375)                     */
    int32_t long_distance;    /* last pose within 1e-6 of (0, 0) on both axes: 10 segments, else 4    */
    int32_t n_breakpoints; const int32_t *breakpoints;  /* input indices the output is drawn through,
                                 ascending, incl. 0 and n - 1; every index for 2 <= n <= 4; empty for n <= 1 */
    int32_t n_poses; const double *poses;               /* x, y, qz, qw per /plan pose (z = 0)        */
    int32_t n_split_searches; /* findBestSplitPoint calls (each one kernel launch)                    */
    float ms_linearize;
} aos_linear_path_out;
/* poses: x, y, qz, qw per /aos/path pose, the layout of aos_path_out.poses (z = 0, qx = qy = 0). poses = NULL with
 * n_poses = 0 is the fused form: the poses of the last aos_path_plan on this handle (AOS_E_STATE if none has run;
 * after a "Failed" plan, which holds no poses: status 0 with published = 0); that plan's arrays stay valid and
 * unchanged. The outputs are library-owned, in buffers of their own, valid until the next aos_path_linearize on the
 * handle or aos_destroy. AOS_E_INVALID: a null out, a negative count, a null array with a count above 0,
 * n_poses > 65536, a non-finite x or y, a segment longer than 2^22 x 0.05 m or an output above 2^22 poses (bounded
 * as 1 + the sum over the segments of floor(length / 0.05) + 1): the node casts floor(distance / 0.05) to int,
 * which is undefined there. */
int aos_path_linearize(aos_ctx *ctx, const double *poses, int32_t n_poses, aos_linear_path_out *out);

/* ---------------------------------------------------------------------------------------------
 * Clearances of the GvdGraph (GvdGraph.msg float32[] edge_clearances). The reference declares the field and never
 * computes it: EdgeRecord::min_clearance_m stays 0 (gvd:466, :1000-1006, :1637), and aos_gvd_out.edge_clearances
 * keeps that zero. aos_gvd_clearance computes the real value from an exact distance field.
 *  - Occupied cell: the byte is 100 (the test of edgePassesThroughOccupiedPixels and trimPathNearOccupiedRegions);
 *    every other value is free.
 *  - Field: d2[y * width + x] = min over occupied (cx, cy) of (x - cx)^2 + (y - cy)^2, uint32 in cell units;
 *    AOS_D2_NONE everywhere when no cell is occupied. width, height <= 16384, so d2 < 2^29.
 *  - A point's cell: fx = (px - origin_x) / res, fy likewise (res = (double)info.resolution); the point has a cell
 *    iff -1 < fx < width, -1 < fy < height and the truncation toward zero of (fx, fy) lies in the grid.
 *  - node_d2 = d2 at the node's cell. edge_d2 = the minimum of d2 over the samples of edgePassesThroughOccupiedPixels
 *    (gvd:320-359) from node edges[2k] to node edges[2k + 1] that have a cell: num = (int)(len / (res * 0.5)) + 1,
 *    samples s + (t * u) * len for t = i / num, i = 0 .. num (t = 1 at i = num); an edge shorter than 1e-6 has the
 *    sample s; num out of int range: no samples. AOS_D2_NONE: no sample has a cell, or the field is empty.
 *  - Metres: (float)(sqrt((double)d2) * res), +inf for AOS_D2_NONE. The distance runs between cell centres: it is
 *    quantised to the grid on purpose (a point takes its cell's value; no sub-cell distances).
 * graph: NULL = this handle's last GVD graph; only nodes_xy, num_nodes, edges and num_edges are read. grid: int8
 * bytes, host memory (grid_on_device = 0) or device memory on the handle's GPU (1), with `info`; NULL = the skeleton
 * that graph was built on, with its info (AOS_E_STATE if there was no GVD call, or a later seed-gen frame replaced
 * it). AOS_E_INVALID: a null out, a negative count, a null array behind a positive count, a grid without info, width
 * or height above 16384, a resolution that is not finite or <= 0, a non-finite node coordinate, an edge index
 * outside [0, num_nodes). width * height = 0: status 0, n_occupied 0, d2_device NULL, every clearance AOS_D2_NONE
 * (+inf). Every call recomputes its field. The outputs are library-owned and valid until the next aos_gvd_clearance
 * on the handle or aos_destroy.
 * ------------------------------------------------------------------------------------------- */
#define AOS_D2_NONE 0xFFFFFFFFu
typedef struct aos_clearance_out {
    aos_grid_info info;
    uint64_t n_occupied;
    uint32_t max_d2;                                 /* over the field; AOS_D2_NONE if n_occupied == 0        */
    const uint32_t *d2_device;                       /* width * height words on the handle's GPU              */
    int32_t num_nodes, num_edges;
    const uint32_t *node_d2, *edge_d2;               /* host, library-owned                                   */
    const float *node_clearances, *edge_clearances;  /* metres; what a wrapper puts into GvdGraph.msg         */
    float ms_field, ms_graph;                        /* device time of the field passes / the sampling        */
} aos_clearance_out;
int aos_gvd_clearance(aos_ctx *ctx, const aos_path_graph *graph, const int8_t *grid, int grid_on_device,
                      const aos_grid_info *info, aos_clearance_out *out);
/* The last aos_gvd_clearance's field copied to host memory. AOS_E_STATE before any field exists; AOS_E_INVALID for
 * a capacity_cells below width * height. */
int aos_clearance_field_copy(aos_ctx *ctx, uint32_t *dst, uint64_t capacity_cells);
/* d2 and metres of n points (x, y) against the last aos_gvd_clearance's field, by the node rule (e.g. /plan poses).
 * Either output may be null. AOS_E_STATE before any field exists; a non-finite point has no cell. */
int aos_clearance_points(aos_ctx *ctx, const double *xy, int32_t n, uint32_t *d2_out, float *metres_out);

/* ---------------------------------------------------------------------------------------------
 * Nearest-obstacle regions and the grid GVD ridge. The reference approximates the ridge between the tree rows with
 * point seeds (virtual, ray and endpoint seeds); aos_gvd_regions computes the ridge itself on the grid, so a caller
 * can tell how far a graph node or a /plan pose lies from it. Every quantity is an integer: the definitions below fix
 * every word of the result.
 *  - Grid: int8 bytes with `info`; a cell is occupied iff its byte is 100. width, height <= 16384. The linear index
 *    of cell (x, y) is i = y * width + x (< 2^28).
 *  - Sites and labels, labels = NULL: the occupied cells are split into 8-connected components; a component's label
 *    is the least linear index of its cells. With opts.min_component_cells > 1 the components with fewer cells are
 *    dropped: their cells stay occupied and are not sites. n_occupied = the occupied cells, n_components = all
 *    components, n_sites = the site cells, n_regions = the components kept.
 *  - Sites and labels, labels given (int32[width * height], in the same kind of memory as grid, read only at occupied
 *    cells): an occupied cell with label >= 0 is a site with that label; a negative label: not a site. Equal labels
 *    on separate components are one region. min_component_cells > 1 with labels is AOS_E_INVALID. n_components and
 *    n_regions are -1.
 *  - Nearest site: site[c] = the linear index of the site cell s with the least pair (squared distance between the
 *    centres of c and s in cells, linear index of s), compared lexicographically; AOS_SITE_NONE everywhere when there
 *    is no site. A site cell is its own site. d2[c] is that squared distance (AOS_D2_NONE without a site): it follows
 *    from site[c] and is not stored. max_d2 = its maximum (AOS_D2_NONE without a site). region[c] = the label of
 *    site[c], or AOS_REGION_NONE.
 *  - Ridge (the grid GVD; int8, 0 or 100): take every pair of 4-adjacent cells (c, n), n = (x + 1, y) or (x, y + 1),
 *    whose regions are both not AOS_REGION_NONE and differ. The pair marks c if c is not a site cell; otherwise it
 *    marks n if n is not a site cell; otherwise it marks neither. A cell is a ridge cell iff some pair marks it;
 *    n_ridge = their count.
 *  - Ridge distance (opts.want_ridge_distance != 0): ridge_d2 = the field of aos_gvd_clearance with the ridge cells
 *    as the occupied cells; AOS_D2_NONE everywhere without a ridge.
 *  - Nodes and points: by the cell rule of aos_gvd_clearance, node_site / node_region / node_d2 / node_ridge_d2 are
 *    the values at the node's cell (AOS_SITE_NONE, AOS_REGION_NONE, AOS_D2_NONE, AOS_D2_NONE without a cell; every
 *    node_ridge_d2 is AOS_D2_NONE when the ridge distance was not asked for). node_ridge_offset, metres:
 *    (float)(sqrt((double)ridge_d2) * res), +inf for AOS_D2_NONE. A non-finite point has no cell.
 * graph and grid = NULL are those of aos_gvd_clearance (the handle's last GVD graph; the skeleton that graph was
 * built on), with AOS_E_STATE under the same conditions; labels must be NULL when grid is. opts = NULL is {0, 0}.
 * AOS_E_INVALID: every case of aos_gvd_clearance, labels without a grid, min_component_cells > 1 with labels.
 * width * height = 0: status 0, nothing launched, the counts 0 (n_components and n_regions -1 with labels), max_d2
 * AOS_D2_NONE, the device pointers NULL, every node value NONE / +inf. Every call recomputes its fields; the outputs
 * are library-owned and valid until the next aos_gvd_regions on the handle or aos_destroy. The call has buffers of
 * its own: the field of an earlier aos_gvd_clearance stays valid across it.
 * ------------------------------------------------------------------------------------------- */
#define AOS_SITE_NONE 0xFFFFFFFFu
#define AOS_REGION_NONE (-1)
typedef struct aos_regions_opts {
    int32_t min_component_cells;   /* <= 1: every component is kept                                            */
    int32_t want_ridge_distance;   /* != 0: ridge_d2 is computed                                               */
} aos_regions_opts;
typedef struct aos_regions_out {
    aos_grid_info info;
    uint64_t n_occupied, n_sites, n_ridge;
    int64_t n_components, n_regions;                 /* -1 with caller labels                                  */
    uint32_t max_d2;                                 /* AOS_D2_NONE if n_sites == 0                            */
    const uint32_t *site_device;                     /* width * height words each, on the handle's GPU         */
    const int32_t *region_device;
    const int8_t *ridge_device;
    const uint32_t *ridge_d2_device;                 /* NULL unless opts.want_ridge_distance                   */
    int32_t num_nodes;
    const uint32_t *node_site;                       /* host, library-owned                                    */
    const int32_t *node_region;
    const uint32_t *node_d2, *node_ridge_d2;
    const float *node_ridge_offset;                  /* metres                                                 */
    float ms_label, ms_field, ms_ridge, ms_graph;    /* device time: sites and labels / the site field / region,
                                                        ridge and ridge distance / the node sampling           */
} aos_regions_out;
int aos_gvd_regions(aos_ctx *ctx, const aos_path_graph *graph, const int8_t *grid, int grid_on_device,
                    const aos_grid_info *info, const int32_t *labels, const aos_regions_opts *opts,
                    aos_regions_out *out);
/* A field of the last aos_gvd_regions copied to host memory. which: "site" (uint32), "region" (int32), "ridge" (int8),
 * "ridge_d2" (uint32). AOS_E_STATE before any field exists; AOS_E_INVALID for an unknown name, a capacity_cells below
 * width * height, a null dst behind cells, or "ridge_d2" when the last call did not compute it. */
int aos_regions_field_copy(aos_ctx *ctx, const char *which, void *dst, uint64_t capacity_cells);
/* The values of n points (x, y) against the last aos_gvd_regions' fields, by the node rule (e.g. /plan poses). Any
 * output may be null. AOS_E_STATE before any field exists. */
int aos_regions_points(aos_ctx *ctx, const double *xy, int32_t n, uint32_t *site, int32_t *region, uint32_t *d2,
                       uint32_t *ridge_d2, float *ridge_offset_m);

/* ---------------------------------------------------------------------------------------------
 * Clearance-limited cost-to-go. aos_gvd_clearance and aos_gvd_regions are straight-line quantities; aos_gvd_reach is
 * the field that knows obstacles are in the way: for a robot that must keep a given distance from every occupied
 * cell, which cells and graph nodes it can reach from a set of sources, how far it is to drive there, and along which
 * cells. Every quantity is an integer: the definitions below fix every word of the result.
 *  - Grid: int8 bytes with `info`, width, height <= 16384; a cell is occupied iff its byte is 100. The linear index of
 *    cell (x, y) is y * width + x.
 *  - Passable: a cell is passable iff its byte is not 100 and its d2 >= opts.min_d2, d2 being aos_gvd_clearance's
 *    field of the same grid (AOS_D2_NONE counts as >= anything). With min_d2 <= 1 the second condition follows from
 *    the first, and no distance field is computed. n_passable = the passable cells.
 *  - Moves: from a passable cell to a passable 8-neighbour inside the grid. An axis move costs 5, a diagonal move 7;
 *    a diagonal move from (x, y) to (x + dx, y + dy) is allowed only if (x + dx, y) and (x, y + dy) are passable too
 *    (no corner cutting). The move relation is symmetric.
 *  - Sources: n_sources world points (x, y), 0 <= n_sources <= 2^20, each mapped to its cell by the cell rule of
 *    aos_gvd_clearance. A source that is not finite, has no cell or falls on an impassable cell is dropped.
 *    n_sources_used = the sources kept (sources, not distinct cells: duplicates count).
 *  - Cost: cost[c] = the least sum of move costs from any source cell to c, uint32; 0 at a source cell; AOS_COST_NONE
 *    at an impassable cell and at a passable cell that no source reaches. width * height <= 2^28, so every finite
 *    cost is below 7 * 2^28 < 2^31. n_reached = the cells with a finite cost; max_cost = the largest finite cost,
 *    AOS_COST_NONE if n_reached == 0.
 *  - Nodes and points: the cost at the node's or point's cell, AOS_COST_NONE without a cell. Metres:
 *    (float)((double)cost * res / 5.0), +inf for AOS_COST_NONE.
 *  - Descent from a start point whose cell c has a finite cost: the cell sequence starts at c; each further cell is
 *    the first neighbour n reachable by an allowed move with cost[n] + w(c, n) == cost[c], the neighbours (dx, dy)
 *    tried in the order (1,0), (-1,0), (0,1), (0,-1), (1,1), (-1,1), (1,-1), (-1,-1); one always exists. The sequence
 *    ends at the first cell of cost 0 and has at most cost / 5 + 1 cells. A start without a cell or with cost
 *    AOS_COST_NONE has 0 cells.
 * graph and grid = NULL are those of aos_gvd_clearance (the handle's last GVD graph, of which only nodes_xy and
 * num_nodes are read; the skeleton that graph was built on), with AOS_E_STATE under the same conditions. opts = NULL
 * is {0, 0}. AOS_E_INVALID: every grid and info case of aos_gvd_clearance, n_sources negative or above 2^20, a null
 * sources_xy behind a positive count. width * height = 0: status 0, nothing launched, the counts 0, max_cost
 * AOS_COST_NONE, cost_device NULL, every node value AOS_COST_NONE / +inf.
 * The field is computed as a fixed point in rounds (n_rounds: the rounds in which some tile of the grid ran); the
 * call returns once a round ran no tile. opts.max_rounds > 0: at most that many rounds are issued, and if a tile still
 * ran in the last of them the call fails with AOS_E_STATE, "reach did not converge in N rounds", and leaves no field
 * behind (aos_reach_field_copy: AOS_E_STATE). Every call recomputes its field; the outputs are library-owned and valid
 * until the next aos_gvd_reach on the handle or aos_destroy. The call has buffers of its own: the fields of earlier
 * aos_gvd_clearance and aos_gvd_regions calls stay valid across it.
 * ------------------------------------------------------------------------------------------- */
#define AOS_COST_NONE 0xFFFFFFFFu
typedef struct aos_reach_opts {
    uint32_t min_d2;        /* a passable cell's d2 is at least this (<= 1: every free cell is passable)          */
    int32_t max_rounds;     /* <= 0: no limit                                                                      */
} aos_reach_opts;
typedef struct aos_reach_out {
    aos_grid_info info;
    uint64_t n_passable, n_reached;
    int32_t n_sources_used;
    uint32_t max_cost;                               /* AOS_COST_NONE if n_reached == 0                        */
    const uint32_t *cost_device;                     /* width * height words on the handle's GPU               */
    int32_t num_nodes;
    const uint32_t *node_cost;                       /* host, library-owned                                    */
    const float *node_metres;
    int32_t n_rounds;                                /* diagnostics, not part of the definition                */
    uint64_t n_tile_runs;                            /* tile workgroups that ran, over all rounds              */
    float ms_mask, ms_wave, ms_graph;                /* device time: mask and seeding (with the distance field
                                                        where min_d2 >= 2) / the rounds / statistics, sampling */
} aos_reach_out;
int aos_gvd_reach(aos_ctx *ctx, const aos_path_graph *graph, const int8_t *grid, int grid_on_device,
                  const aos_grid_info *info, const double *sources_xy, int32_t n_sources, const aos_reach_opts *opts,
                  aos_reach_out *out);
/* The last aos_gvd_reach's field copied to host memory. AOS_E_STATE before any field exists; AOS_E_INVALID for a
 * capacity_cells below width * height or a null dst behind cells. */
int aos_reach_field_copy(aos_ctx *ctx, uint32_t *dst, uint64_t capacity_cells);
/* cost and metres of n points (x, y) against the last aos_gvd_reach's field, by the node rule. Either output may be
 * null. AOS_E_STATE before any field exists; a non-finite point has no cell. */
int aos_reach_points(aos_ctx *ctx, const double *xy, int32_t n, uint32_t *cost, float *metres);
/* The descent from start_xy on the last aos_gvd_reach's field: the cells' linear indices into cells and, if xy is not
 * null, their centres origin + (index + 0.5) * res as doubles (x, y) into xy; at most capacity_cells of them are
 * written, and *n_cells is always the full length. AOS_E_STATE before any field exists; AOS_E_INVALID for a null
 * start_xy or n_cells, or a null cells behind a capacity above 0. */
int aos_reach_descend(aos_ctx *ctx, const double start_xy[2], uint32_t *cells, double *xy, uint64_t capacity_cells,
                      uint64_t *n_cells);

/* ---------------------------------------------------------------------------------------------
 * Line of sight and taut descents. A descent is a staircase of 8-connected cells; aos_reach_sight answers whether a
 * robot that keeps reach's clearance can drive a straight segment, and aos_reach_pull turns a descent into the few
 * waypoints a controller wants while every leg keeps that clearance. Everything is integer, as above: the definitions
 * fix every word of the result.
 *  - Passable is the mask of the last successful aos_gvd_reach on the handle (its grid, its min_d2). Both calls return
 *    AOS_E_STATE before any aos_gvd_reach on the handle and after one that failed ("did not converge").
 *  - Touched cells: for cells a = (ax, ay) and b = (bx, by) let dx = bx - ax, dy = by - ay. T(a, b) is the set of
 *    cells (x, y) with min(ax, bx) <= x <= max(ax, bx), min(ay, by) <= y <= max(ay, by) and
 *        2 * |dx * (y - ay) - dy * (x - ax)| <= |dx| + |dy|.
 *    Every term is below 2^30 (width, height <= 16384). These are exactly the cells whose closed unit square meets
 *    the closed segment between the two centres. T contains a and b; T(a, a) = {a}; T(a, b) = T(b, a); an axis
 *    segment of n steps touches n + 1 cells, a pure diagonal of n steps 3 n + 1 (the two cells beside every corner it
 *    passes through included); (0,0)->(2,1) touches 4 cells, (0,0)->(6,3) touches 10. A move of aos_gvd_reach is
 *    allowed iff the segment between the two cells touches only passable cells: the corner rule is the diagonal case.
 *  - aos_reach_sight: n segments, from_xy and to_xy n points (x, y) each, every end mapped to its cell by the cell
 *    rule of aos_gvd_clearance. n_touched[k] = |T|; n_blocked[k] = the cells of T that are not passable: the segment is
 *    free iff it is 0. An end that is not finite or has no cell gives n_touched 0 and n_blocked AOS_COST_NONE. Either
 *    output may be null. n = 0: AOS_OK, nothing launched. AOS_E_INVALID: n negative, a null array behind a positive n.
 *  - aos_reach_pull: let c_0 .. c_(m-1) be the descent of aos_reach_descend from start_xy (m = 0 when the start has no
 *    cell or no finite cost). The waypoints are the steps k_0 = 0 and, while k_i < m - 1,
 *        k_(i+1) = max { j : k_i < j <= hi and n_blocked(c_(k_i), c_j) = 0 },
 *    hi = m - 1 when opts.max_span <= 0, else min(m - 1, k_i + max_span). The set is never empty, since j = k_i + 1 is
 *    an allowed move. The rule is the farthest visible step, not the step before the first invisible one: visibility
 *    along a descent is not monotone. opts = NULL is {0}.
 *    n_cells = m; start_cost = the start cell's cost (AOS_COST_NONE for m = 0); n_waypoints (0 for m = 0, 1 for
 *    m = 1); waypoint_steps = the k_i; waypoint_cells = the linear indices of c_(k_i); waypoints_xy = their centres
 *    origin + (index + 0.5) * res; length_m = the sum over the legs in order of sqrt((double)(dx^2 + dy^2)),
 *    accumulated in double, times res once at the end (0 for fewer than two waypoints); descent_m =
 *    (double)start_cost * res / 5 (+inf for m = 0). Both are host arithmetic on the integers.
 *    m > 65536 is AOS_E_INVALID, "descent longer than 65536 cells" (aos_path_linearize's limit on its poses), and
 *    leaves nothing behind. The pull's worst case is quadratic in m; this limit and max_span are the caller's bound.
 *    AOS_E_INVALID also for a null start_xy or out.
 *    The outputs are library-owned, in buffers of their own, and valid until the next aos_reach_pull or aos_gvd_reach on
 *    the handle or aos_destroy; the field and the outputs of the other reach calls are not touched.
 * Guarantee: every cell touched by every leg is passable. So the robot's centre keeps reach's clearance along the
 * whole polyline, quantised to the grid as aos_gvd_clearance is. Neither the staircase of cell centres joined by
 * anything but its own moves nor a regressed segment of aos_path_linearize gives this.
 * ------------------------------------------------------------------------------------------- */
int aos_reach_sight(aos_ctx *ctx, const double *from_xy, const double *to_xy, int32_t n, uint32_t *n_touched,
                    uint32_t *n_blocked);
typedef struct aos_pull_opts {
    int32_t max_span;       /* > 0: a leg spans at most this many steps of the descent; <= 0: no limit           */
} aos_pull_opts;
typedef struct aos_pull_out {
    uint64_t n_cells;                                /* m, the descent's length                                 */
    uint32_t start_cost;                             /* AOS_COST_NONE for m = 0                                 */
    int32_t n_waypoints;
    const uint32_t *waypoint_steps;                  /* host, library-owned: n_waypoints words each             */
    const uint32_t *waypoint_cells;
    const double *waypoints_xy;                      /* n_waypoints x (x, y)                                    */
    double length_m, descent_m;
    int32_t n_steps_launched;                        /* diagnostics, not part of the definition: anchor steps   */
    uint64_t n_sight_tests;                          /* candidates the anchor steps tested                      */
    float ms_descend, ms_pull;                       /* stream time: the descent / the anchor steps with their
                                                        host looks                                              */
} aos_pull_out;
int aos_reach_pull(aos_ctx *ctx, const double start_xy[2], const aos_pull_opts *opts, aos_pull_out *out);

/* ---------------------------------------------------------------------------------------------
 * The widest robot that can reach each cell and node. aos_gvd_reach answers "given this robot, where can it go?" for
 * one clearance threshold; aos_gvd_width answers the inverse for every cell and node at once: the largest min_d2 at
 * which aos_gvd_reach from the same sources still reaches it. It is the max-min (bottleneck) closure of
 * aos_gvd_clearance's d2 over aos_gvd_reach's move relation. Every quantity is an integer: the definitions below fix
 * every word of the result and no algorithm does.
 *  - Grid, cell rule, info and graph checks: aos_gvd_clearance's.
 *  - cap[c]: 0 if the cell's byte is 100; otherwise aos_gvd_clearance's d2[c] of the same grid, which is at least 1,
 *    and AOS_D2_NONE = 0xFFFFFFFF everywhere when no cell is occupied, which is simply the largest value.
 *  - Moves: aos_gvd_reach's, to an 8-neighbour inside the grid. The bottleneck of an axis move a -> b is
 *    min(cap[a], cap[b]); of a diagonal move min(cap[a], cap[b], cap[(bx, ay)], cap[(ax, by)]): the two cells beside
 *    the diagonal count (aos_gvd_reach's corner rule). The relation is symmetric.
 *  - Sources: as aos_gvd_reach, 0 <= n_sources <= 2^20 world points mapped by the cell rule. A source that is not
 *    finite, has no cell or has cap 0 is dropped. n_sources_used = the sources kept (duplicates count).
 *  - width[c], uint32: the maximum, over all move paths from a kept source cell to c, of the minimum bottleneck along
 *    the path; a path of one cell has value cap[c]. 0 (AOS_WIDTH_NONE) if no path has a bottleneck above 0: occupied
 *    cells, and free cells that no source can reach, have width 0.
 *  - Equivalence: for every m >= 1, width[c] >= m iff aos_gvd_reach on the same grid and sources with min_d2 = m gives
 *    c a finite cost (for m <= 1 reach's passable is "byte != 100", which is width >= 1).
 *  - Counts: n_free = the cells with cap > 0; n_reached = the cells with width > 0; max_width and min_width run over
 *    the reached cells and are 0 when there are none.
 *  - Nodes and points: the width at the node's or point's cell by the node rule, 0 without a cell. radius_m =
 *    (float)(sqrt((double)width) * res), +inf for 0xFFFFFFFF and 0.0f for 0: host arithmetic on the integer, the form of
 *    aos_gvd_clearance's metres.
 * graph and grid = NULL are the handle's own, as in aos_gvd_reach, with AOS_E_STATE under the same conditions. opts =
 * NULL is {0}. AOS_E_INVALID: a null ctx or out, a grid without info, every grid and info case of aos_gvd_clearance,
 * n_sources negative or above 2^20, a null sources_xy behind a positive count. width * height = 0: status 0, nothing
 * launched, the counts 0, width_device NULL, every node value 0.
 * The field is the unique fixed point of width[c] = max(width[c], min(width[n], bottleneck(n -> c))) over the moves
 * with width = cap at the kept source cells, computed in rounds (n_rounds: the rounds in which some tile ran).
 * opts.max_rounds works as in aos_gvd_reach: > 0, at most that many rounds are issued, and if a tile still ran in the
 * last of them the call fails with AOS_E_STATE, "width did not converge in N rounds", and leaves no field behind.
 * Every call recomputes its field; the outputs are library-owned and valid until the next aos_gvd_width on the handle
 * or aos_destroy. The state is the call's own: the fields and outputs of earlier aos_gvd_clearance, aos_gvd_regions,
 * aos_gvd_reach, aos_reach_descend and aos_reach_pull calls stay valid across it, and it stays valid across them.
 * With w = width at a start cell, aos_gvd_reach(min_d2 = w) followed by aos_reach_pull(start) is the widest route and
 * its waypoints.
 * ------------------------------------------------------------------------------------------- */
#define AOS_WIDTH_NONE 0u
typedef struct aos_width_opts {
    int32_t max_rounds;     /* <= 0: no limit                                                                      */
} aos_width_opts;
typedef struct aos_width_out {
    aos_grid_info info;
    uint64_t n_free, n_reached;
    int32_t n_sources_used;
    uint32_t min_width, max_width;                   /* over the reached cells; 0 if n_reached == 0            */
    const uint32_t *width_device;                    /* width * height words on the handle's GPU               */
    int32_t num_nodes;
    const uint32_t *node_width;                      /* host, library-owned                                    */
    const float *node_radius_m;
    int32_t n_rounds;                                /* diagnostics, not part of the definition                */
    uint64_t n_tile_runs;                            /* tile workgroups that ran, over all rounds              */
    float ms_field, ms_wave, ms_graph;               /* device time: the distance field, cap and seeding / the
                                                        rounds / statistics, sampling                          */
} aos_width_out;
int aos_gvd_width(aos_ctx *ctx, const aos_path_graph *graph, const int8_t *grid, int grid_on_device,
                  const aos_grid_info *info, const double *sources_xy, int32_t n_sources, const aos_width_opts *opts,
                  aos_width_out *out);
/* The last aos_gvd_width's field copied to host memory. AOS_E_STATE before any field exists; AOS_E_INVALID for a
 * capacity_cells below width * height or a null dst behind cells. */
int aos_width_field_copy(aos_ctx *ctx, uint32_t *dst, uint64_t capacity_cells);
/* width and radius_m of n points (x, y) against the last aos_gvd_width's field, by the node rule. Either output may be
 * null. AOS_E_STATE before any field exists; AOS_E_INVALID for a negative n or a null xy behind a positive n. */
int aos_width_points(aos_ctx *ctx, const double *xy, int32_t n, uint32_t *width, float *radius_m);

/* ---------------------------------------------------------------------------------------------
 * Cost-to-go that pays for driving close to obstacles. A shortest path under a hard clearance (aos_gvd_reach) runs
 * along the obstacles' inflation rim; aos_gvd_soft is reach's field with a weight per cell that rises towards the
 * obstacles, so its descent leaves the rim where the detour is cheap and squeezes through where it is not: the
 * costmap-weighted plan. Every quantity is an integer: the definitions below fix every word of the result.
 *  - Grid, cell rule, info and graph checks: aos_gvd_clearance's. Passable: aos_gvd_reach's rule, the byte is not 100
 *    and d2 >= opts.min_d2 (AOS_D2_NONE counts as >= anything). n_passable = the passable cells.
 *  - Weight: r[c] = floor(sqrt(d2[c])), the exact integer square root of aos_gvd_clearance's field; pen[c] =
 *    max(0, soft_cells - r[c]), and 0 where d2[c] is AOS_D2_NONE; wt[c] = 1 + gain * pen[c] on passable cells.
 *    0 <= soft_cells <= 255, 0 <= gain <= 254, and 1 + gain * max(0, soft_cells - 1) <= 255: a free cell has r >= 1,
 *    so wt fits a byte. With soft_cells <= 1 or gain == 0 every weight is 1, and then no distance field is computed
 *    unless min_d2 >= 2. n_soft = the passable cells with wt > 1; max_weight = the largest wt over the passable
 *    cells, 0 if there are none.
 *  - Moves: aos_gvd_reach's, to an 8-neighbour inside the grid, no corner cutting. A move a -> b costs base * the
 *    largest wt over the cells it touches, base 5 (axis) or 7 (diagonal); an axis move touches a and b, a diagonal
 *    move a, b and the two cells beside the diagonal (the set T(a, b) of aos_reach_sight, the cells whose least
 *    clearance is aos_gvd_width's bottleneck). The relation is symmetric; with all weights 1 the cost is reach's.
 *  - Sources: as aos_gvd_reach, 0 <= n_sources <= 2^20 world points; a source that is not finite, has no cell or falls
 *    on an impassable cell is dropped. n_sources_used = the sources kept (duplicates count).
 *  - Cost: cost[c], uint32 = the least sum of move costs from a kept source cell to c; 0 at a source cell;
 *    AOS_COST_NONE at an impassable cell and at a passable cell that no source reaches. n_reached = the cells with a
 *    finite cost; max_cost = the largest finite cost, AOS_COST_NONE if n_reached == 0.
 *  - Bound: a least-cost path visits no cell twice, so every finite cost is below 7 * max_weight * n_passable. If that
 *    product is >= 2^31 the call fails with AOS_E_INVALID, the message names both factors, and no field is left
 *    behind. With all weights 1 this is reach's own bound (width * height <= 2^28).
 *  - Nodes and points: the cost at the node's or point's cell by the node rule, AOS_COST_NONE without a cell. No
 *    metres are given: a weighted cost is not a length.
 *  - Descent: aos_gvd_reach's rule with this call's move costs: from cell c the first neighbour n, in reach's order
 *    of the eight moves, that an allowed move reaches with cost[n] + w(c, n) == cost[c]; down to the first cell of
 *    cost 0; at most cost / 5 + 1 cells. plain_cost = the sum of 5 and 7 over the descent's moves (host arithmetic on
 *    the cells): beside reach's cost at the same start it is the length of the detour paid for clearance.
 * graph and grid = NULL are the handle's own, as in aos_gvd_reach, with AOS_E_STATE under the same conditions. opts =
 * NULL is {0, 0, 0, 0}. AOS_E_INVALID: reach's cases, soft_cells or gain out of range, a weight above 255, and the
 * bound above. width * height = 0: status 0, nothing launched, the counts 0, max_cost AOS_COST_NONE, cost_device NULL,
 * every node value AOS_COST_NONE.
 * The field is the unique fixed point of cost[c] = min(cost[c], cost[n] + w(n, c)) over the moves, computed in rounds
 * as reach's (n_rounds: the rounds in which some tile ran). opts.max_rounds > 0: at most that many rounds are issued,
 * and if a tile still ran in the last of them the call fails with AOS_E_STATE, "soft did not converge in N rounds",
 * and leaves no field behind. Every call recomputes its field; the outputs are library-owned and valid until the next
 * aos_gvd_soft on the handle or aos_destroy. The state is the call's own: the fields and outputs of aos_gvd_clearance,
 * aos_gvd_regions, aos_gvd_reach, aos_reach_descend, aos_reach_pull and aos_gvd_width stay valid across it, and it
 * stays valid across them; aos_reach_sight and aos_reach_pull stay bound to the last aos_gvd_reach's mask. No pull is
 * offered for soft descents: pulling a descent taut undoes the centring it paid for.
 * ------------------------------------------------------------------------------------------- */
typedef struct aos_soft_opts {
    uint32_t min_d2;        /* a passable cell's d2 is at least this (<= 1: every free cell is passable)          */
    int32_t soft_cells;     /* cells nearer than this to an obstacle (r < soft_cells) weigh more; 0..255           */
    int32_t gain;           /* weight per cell of that nearness; 0..254                                            */
    int32_t max_rounds;     /* <= 0: no limit                                                                      */
} aos_soft_opts;
typedef struct aos_soft_out {
    aos_grid_info info;
    uint64_t n_passable, n_reached, n_soft;
    int32_t n_sources_used;
    uint32_t max_cost, max_weight;                   /* AOS_COST_NONE if n_reached == 0; 0 if n_passable == 0  */
    const uint32_t *cost_device;                     /* width * height words on the handle's GPU               */
    int32_t num_nodes;
    const uint32_t *node_cost;                       /* host, library-owned                                    */
    int32_t n_rounds;                                /* diagnostics, not part of the definition                */
    uint64_t n_tile_runs;                            /* tile workgroups that ran, over all rounds              */
    float ms_mask, ms_wave, ms_graph;                /* device time: distance field, weights and seeding / the
                                                        rounds / statistics, sampling                          */
} aos_soft_out;
int aos_gvd_soft(aos_ctx *ctx, const aos_path_graph *graph, const int8_t *grid, int grid_on_device,
                 const aos_grid_info *info, const double *sources_xy, int32_t n_sources, const aos_soft_opts *opts,
                 aos_soft_out *out);
/* The last aos_gvd_soft's field copied to host memory. AOS_E_STATE before any field exists; AOS_E_INVALID for a
 * capacity_cells below width * height or a null dst behind cells. */
int aos_soft_field_copy(aos_ctx *ctx, uint32_t *dst, uint64_t capacity_cells);
/* The cost of n points (x, y) against the last aos_gvd_soft's field, by the node rule. AOS_E_STATE before any field
 * exists; AOS_E_INVALID for a negative n or a null xy behind a positive n. */
int aos_soft_points(aos_ctx *ctx, const double *xy, int32_t n, uint32_t *cost);
/* The descent from start_xy on the last aos_gvd_soft's field: the cells' linear indices into cells and, if xy is not
 * null, their centres into xy; at most capacity_cells of them are written, and *n_cells is always the full length.
 * *plain_cost (may be NULL) is summed over the full descent whatever the capacity, 0 for an empty one. AOS_E_STATE
 * before any field exists; AOS_E_INVALID for a null start_xy or n_cells, or a null cells behind a capacity above 0. */
int aos_soft_descend(aos_ctx *ctx, const double start_xy[2], uint32_t *cells, double *xy, uint64_t capacity_cells,
                     uint64_t *n_cells, uint32_t *plain_cost);

/* Diagnostics: copy an internal device grid of the last frame to host as int8 {0,100}.
 * which: "raster", "inflated", "opened", "skeleton_frameless". */
int aos_debug_grid(aos_ctx *ctx, const char *which, int8_t *dst, uint64_t capacity);
/* Diagnostics: the library's single-pass exclusive scan (its counting sorts' and compactions' primitive) on the
 * handle's stream: d_out[i] = d_in[0] + ... + d_in[i - 1] for i in [0, n] (n + 1 outputs), device int32 arrays on
 * the handle's GPU; zero_in: d_in is left zero. Returns once done. */
int aos_debug_scan(aos_ctx *ctx, int32_t *d_in, int32_t *d_out, int32_t n, int zero_in);
/* Stream of the handle (hipStream_t as void*) for callers that time with their own events. */
void *aos_stream(aos_ctx *ctx);
/* Test hooks (fault injection for the tiled path's error tests; process-wide, not for production use):
 * ror_stuck_rank >= 0: that tiled rank reports a stuck look-back wait in its ROR column scan (every rank
 * must then fail the frame together); a2a_round_bytes > 0: the distributed cluster stage's personalised
 * exchange moves at most that many bytes per rank pair and round. (-1, 0) turns both off (the default). */
void aos_debug_faults(int32_t ror_stuck_rank, uint64_t a2a_round_bytes);
/* Test hook (process-wide): a seed-gen frame replays its clusters without the order-free certificate on the GPU
 * (one wave per cluster) once it has at least gpu_min_clusters of them, else on host threads. -1: the default
 * (never: the host walk is faster); 0: always on the GPU (where a cluster's box fits the wave's LDS
 * bitmap).
 * ring_cap in [1, 63]: the GPU walk gives a cluster up to the host once more than that many cells are queued
 * (default 0: 64), so tests reach the fallback. replay_all != 0: every cluster is replayed, also those with the
 * order-free certificate (whose records the replay must reproduce). (-1, 0, 0): the defaults. */
void aos_debug_replay(int32_t gpu_min_clusters, int32_t ring_cap, int32_t replay_all);
/* Test hook (process-wide; a negative value restores the default): thin_cap_launches >= 0: a whole-map frame
 * issues at most max(1, thin_cap_launches) thinning launches, so a test reaches "thinning did not converge";
 * ccl_edge_cap >= 0: the cluster stage's link list holds max(2, ccl_edge_cap) links, so a test reaches its
 * overflow fall-back; stats_lds == 0: the cluster statistics kernel reads the cluster table from global memory
 * instead of its LDS copy. (-1, -1, -1): the defaults. */
void aos_debug_limits(int32_t thin_cap_launches, int32_t ccl_edge_cap, int32_t stats_lds);
/* Diagnostics: the last single-GPU seed-gen frame's exact BFS replays: out[0] = all of them (n_bfs_replayed),
 * out[1] = on the GPU, out[2] = on host threads over the skeleton bits, out[3] = on host threads from the clusters'
 * cells. */
int aos_replay_counts(aos_ctx *ctx, int32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* AOS_GPU_H */
