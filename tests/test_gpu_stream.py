"""Streaming ingest (BASELINE.json configs[4]): scans appended to the
device-resident map with aos_map_append must give exactly the frame of aos_seedgen_process on the
concatenated cloud, and the oracle's frame. The C2 test also covers configs[4]'s hipGraph-captured
thinning: the appending handle replays its first thinning batch from hipGraphs (aos_params.thin_graph),
the reprocessing handle launches plainly, over 20 frames whose T changes."""
import json
import os

import numpy as np
import pytest

import aos_gpu
import oracle_py as O
import orchard
from parity_util import assert_golden_hashes, assert_gvd_parity, assert_seedgen_parity

pytestmark = pytest.mark.gpu

GVD_KEYS = ("nodes", "edges", "edge_lengths", "node_labels", "node_cluster_indices", "node_label_clusters")


def test_stream_appends_equal_full_reprocessing_and_oracle():
    cfg = orchard.CONFIGS["C1"]
    poly = orchard.polygon(cfg)
    scans = [orchard.generate_scan(cfg, k * 40, n_points=150_000) for k in range(4)]
    s = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res))
    s.set_polygon(poly)
    s.map_reset(reserve_points=200_000)      # forces one growth of the map buffer
    ref = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res))
    ref.set_polygon(poly)
    for k in range(len(scans)):
        g = s.map_append(scans[k])
        gg = s.gvd_from_seedgen()
        full = np.concatenate(scans[:k + 1])
        r = ref.seedgen(full)
        rg = ref.gvd_from_seedgen()
        assert_seedgen_parity(g, {**r, "cluster_length": np.zeros(r["n_clusters_all"])})
        assert g["n_clipped"] == r["n_clipped"] and g["n_input"] == full.shape[0]
        for key in GVD_KEYS:
            assert np.array_equal(gg[key], rg[key]), (k, key)
    o = O.seedgen(full, poly, O.default_params(grid_resolution=cfg.res))
    assert_seedgen_parity(g, o)
    assert_gvd_parity(gg, O.gvd(o["voronoi_seeds"], o["rows_info"], o))
    s.close()
    ref.close()


def test_stream_custom_layout_and_non_dense_scan():
    """A scan with point_step 32 and swapped offsets, then a non-dense scan: the map turns non-dense."""
    cfg = orchard.CONFIGS["C0"]
    poly = orchard.polygon(cfg)
    a = orchard.generate(cfg, n_points=40000)
    b = orchard.generate(cfg, seed=9, n_points=30000)
    f = a.view(np.float32).reshape(-1, 4)
    rec = np.zeros((len(f), 8), np.float32)
    rec[:, 3], rec[:, 1], rec[:, 5] = f[:, 0], f[:, 1], f[:, 2]
    wide = rec.view(np.uint8).reshape(len(f), 32)
    s = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res))
    s.set_polygon(poly)
    s.map_reset()
    s.map_append(wide, point_step=32, offs=(12, 4, 20))
    g = s.map_append(b, is_dense=False)
    full = np.concatenate([a, b])
    o = O.seedgen(full, poly, O.default_params(grid_resolution=cfg.res), is_dense=False)
    assert_seedgen_parity(g, o)
    s.map_reset()
    g2 = s.map_append(a)
    assert_seedgen_parity(g2, O.seedgen(a, poly, O.default_params(grid_resolution=cfg.res)))
    s.close()


def test_stream_c2_map_20_scans_incremental_equals_full_reprocessing():
    """BASELINE configs[4] at full size: the C2 map (10 M points) then 20 scans of 1 M points. From the
    second frame on each append only partitions the scan and recounts the tiles it reached (the
    incremental ROR, ror_stage.hip ror_stage_append), and its first thinning batch is a replayed hipGraph;
    the reference handle reprocesses the whole concatenated cloud with plain launches. Every frame must be
    equal (grids, T, counts, rows, seeds), the GvdGraph every fourth scan; the frames after 5 and 20 scans
    must match the oracle's SHA-256 fixtures (tests/golden/c4_stream_sha256.json), and on the last frame
    the oracle's Zhang-Suen on the GPU's opened grid must give the same T and skeleton."""
    import torch
    cfg = orchard.CONFIGS["C2"]
    poly = orchard.polygon(cfg)
    base = orchard.generate(cfg)
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c4_stream_sha256.json")))
    assert {"scans_5", "scans_20"} <= set(gold)
    n_scans = 20
    s = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res, thin_graph=1))
    s.set_polygon(poly)
    s.map_reset(reserve_points=base.shape[0] + n_scans * orchard.SCAN_POINTS)
    ref = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res, thin_graph=0))
    ref.set_polygon(poly)
    g = s.map_append(base)
    full = torch.from_numpy(base).to("cuda:0")
    ror_inc, ror_full, Ts, graph_use = [], [], [], []
    for k in range(n_scans):
        scan = orchard.generate_scan(cfg, 40 * k)
        g = s.map_append(scan)
        full = torch.cat([full, torch.from_numpy(scan).to("cuda:0")])
        torch.cuda.synchronize()   # the library reads on its own stream
        r = ref.seedgen(full.data_ptr(), n_points=full.shape[0], on_device=True)
        assert r["thin_graph"] == 0
        assert_seedgen_parity(g, {**r, "cluster_length": np.zeros(r["n_clusters_all"])})
        assert (g["n_clipped"], g["n_binned"], g["n_input"]) == (r["n_clipped"], r["n_binned"], full.shape[0]), k
        Ts.append(g["thin_iters"])
        graph_use.append(g["thin_graph"])
        ror_inc.append(g["ms"]["ror"])
        ror_full.append(r["ms"]["ror"])
        if k % 4 == 3 or k == n_scans - 1 or k + 1 in (5, 20):
            gg, rg = s.gvd_from_seedgen(), ref.gvd_from_seedgen()
            for key in GVD_KEYS:
                assert np.array_equal(gg[key], rg[key]), (k, key)
            if f"scans_{k + 1}" in gold:   # the accumulated 15 M / 30 M-point frames vs the oracle
                assert_golden_hashes(g, gg, gold[f"scans_{k + 1}"])
    print("T per scan:", Ts, "graph use per scan:", graph_use)
    assert all(x in (1, 2) for x in graph_use) and graph_use.count(1) >= 10, graph_use
    assert len(set(Ts)) >= 3, Ts   # the replayed batches saw different thinning depths
    # the oracle's ximgproc thinning on the last frame's opened grid: same T, same skeleton
    H, W = g["height"], g["width"]
    opened = (s.debug_grid("opened", (H, W)) != 0).astype(np.uint8)
    skel_o, T_o = O.thin(opened)
    assert T_o == g["thin_iters"], (T_o, g["thin_iters"])
    assert np.array_equal(skel_o != 0, s.debug_grid("skeleton_frameless", (H, W)) != 0)
    # the appends do not reprocess the map: their ROR stage stays below the whole-map one
    print("ROR stage ms, incremental:", np.round(ror_inc, 2).tolist(), "whole map:", np.round(ror_full, 2).tolist())
    assert np.median(ror_inc) < np.median(ror_full), (ror_inc, ror_full)
    s.close()
    ref.close()
