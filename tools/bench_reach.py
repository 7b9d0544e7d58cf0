"""Latency of aos_gvd_reach (the clearance-limited cost-to-go field) and of one aos_reach_descend beside the same
definitions on one CPU core.

Inputs: the C2 skeleton with its graph (one seed-gen + GVD frame, then the call with no graph and no grid: the handle's
own graph and device skeleton) with the graph's nodes as the sources at min_d2 0 and at min_d2 16 (a robot that keeps
four cells away), and with one source in a corner (the long wavefront); the C0 golden skeleton with its nodes as the
sources and an empty 4096 x 4096 grid with one corner source, both as an explicit graph and a grid already on the device.
GPU columns: the median of 20 calls after 5 warm-up calls, host clock around the call (it ends in a stream synchronise),
the call's own device times ms_mask / ms_wave / ms_graph, n_rounds and n_tile_runs; descend_ms and descend_cells: one
aos_reach_descend from the reached cell farthest from the sources' corner (the last one with the maximum cost). Host
column: tests/reach_host/reach_host_main.cpp built without sanitizers at the library Makefile's host flags, the median
of 7 runs of its Dijkstra inside that one process. Both outputs are compared bit for bit. Prints one JSON line per row.

    python tools/bench_reach.py
"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tools", "tests", "active-orchard-slam_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

WARMUP, CALLS, HOST_RUNS = 5, 20, 7
RADIUS_D2 = 16


def build_host(out_dir):
    csrc = os.path.join(ROOT, "active-orchard-slam_amd", "csrc")
    exe = os.path.join(out_dir, "reach_host_main")
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3",
                    "-mtune=znver5", "-Wall", "-I", csrc, "-x", "c++",
                    os.path.join(ROOT, "tests", "reach_host", "reach_host_main.cpp"),
                    os.path.join(csrc, "reach_host.cpp"), os.path.join(csrc, "clearance_host.cpp"), "-o", exe], check=True)
    return exe


def main():
    import torch
    import numpy as np

    import aos_gpu
    import clearance_scenes as CS
    import orchard
    import reach_scenes as S
    from test_reach_cpu import COUNTS, blob, parse_host_output

    cfg = orchard.CONFIGS["C2"]
    c = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res))
    c.set_polygon(orchard.polygon(cfg))
    f = c.seedgen(orchard.generate(cfg))
    gg = c.gvd_from_seedgen()
    sk, org, res = f["skeleton_framed"], f["origin"], f["resolution"]
    H2, W2 = sk.shape
    free = np.argwhere(np.asarray(sk) != 100)
    corner = [S.centre(int(free[0][1]), int(free[0][0]), org, float(np.float32(res)))]   # the first free cell in raster order
    mk = lambda grid, src, m, nodes, o, r: S.scene(grid, src, m, nodes=nodes, starts=[], origin=o, resolution=r, cells=False)  # noqa: E731
    c0 = CS.c0_scene()
    empty = np.zeros((4096, 4096), np.int8)
    e_org, e_res = (3.5, -7.25), 0.05
    rows = [("c2_nodes", mk(sk, gg["nodes"], 0, gg["nodes"], org, res), "own"),
            (f"c2_nodes_min_d2_{RADIUS_D2}", mk(sk, gg["nodes"], RADIUS_D2, gg["nodes"], org, res), "own"),
            ("c2_corner_source", mk(sk, corner, 0, gg["nodes"], org, res), "own"),
            ("c0_nodes", mk(c0["grid"], c0["nodes"], 0, c0["nodes"], c0["origin"], c0["resolution"]), "device"),
            ("empty_4096_corner_source", mk(empty, [S.centre(0, 0, e_org, float(np.float32(e_res)))], 0, None, e_org, e_res),
             "device")]
    scenes = [r[1] for r in rows]
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_host(tmp)
        fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fi, "wb") as fh:
            fh.write(blob(scenes))
        r = subprocess.run([exe, fi, fo, str(HOST_RUNS)], capture_output=True, text=True, check=True)   # (one thread)
        host_ms = {int(l.split()[1]): float(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("ms ")}
        with open(fo, "rb") as fh:
            host = parse_host_output(fh.read(), scenes)
    ok = True
    p50 = lambda v: round(sorted(v)[len(v) // 2], 4)  # noqa: E731
    for k, (name, sc, form) in enumerate(rows):
        H, W = sc["grid"].shape
        info = {"origin": sc["origin"], "resolution": sc["resolution"], "width": W, "height": H}
        if form == "device":
            d = torch.from_numpy(np.ascontiguousarray(sc["grid"]).reshape(-1)).cuda()
            torch.cuda.synchronize()
            run = lambda: c.gvd_reach(sc["sources"], graph=sc, grid=d.data_ptr(), info=info, on_device=True, min_d2=sc["min_d2"])  # noqa: E731
        else:
            run = lambda: c.gvd_reach(sc["sources"], min_d2=sc["min_d2"])  # noqa: E731
        ms, parts = [], {"mask": [], "wave": [], "graph": []}
        for i in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            g = run()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                ms.append(dt)
                for key, v in parts.items():
                    v.append(g["ms"][key])
        h = host[k]
        fld = c.reach_field()
        equal = h["status"] == 0 and all(g[key] == h[key] for key in COUNTS) and fld.tobytes() == h["field"].tobytes()
        equal = equal and g["node_cost"].tobytes() == h["node_cost"].tobytes()
        equal = equal and g["node_metres"].tobytes() == h["node_metres"].tobytes()
        # one descent from the last cell with the maximum cost
        far = int(np.flatnonzero(h["field"].ravel() == h["max_cost"])[-1])
        start = S.centre(far % W, far // W, sc["origin"], sc["resolution"])
        n = aos_gpu.c_u64(0)
        cells = np.empty(h["max_cost"] // 5 + 1, np.uint32)
        s_xy = np.array(start, np.float64)
        t0 = time.perf_counter()
        aos_gpu._check(aos_gpu.lib().aos_reach_descend(c.h, s_xy.ctypes.data, cells.ctypes.data, None, cells.size,
                                                       ctypes.byref(n)))
        descend_ms = (time.perf_counter() - t0) * 1e3
        path = cells[:n.value].astype(np.int64)
        costs = h["field"].ravel()[path].astype(np.int64)
        equal = equal and n.value > 0 and path[0] == far and costs[-1] == 0 and set((costs[:-1] - costs[1:]).tolist()) <= {5, 7}
        ok &= bool(equal)
        ms.sort()
        out = {"input": name, "width": W, "height": H, "form": form, "min_d2": sc["min_d2"], "sources": len(sc["sources"]),
               "nodes": len(sc["nodes"])}
        out.update({key: g[key] for key in COUNTS})
        out.update({"n_rounds": g["n_rounds"], "n_tile_runs": g["n_tile_runs"]})
        out.update({"gpu_call_ms_p50": p50(ms), "gpu_call_ms_min": round(ms[0], 4), "gpu_call_ms_max": round(ms[-1], 4)})
        out.update({"gpu_ms_" + key + "_p50": p50(v) for key, v in parts.items()})
        out.update({"descend_ms": round(descend_ms, 4), "descend_cells": n.value, "host_ms_p50": host_ms[k],
                    "host_over_gpu": round(host_ms[k] / max(p50(ms), 1e-9), 2), "bit_equal": bool(equal)})
        print(json.dumps(out), flush=True)
    c.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
