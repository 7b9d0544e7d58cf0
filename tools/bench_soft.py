"""Latency of aos_gvd_soft (the cost-to-go field that pays for driving close to obstacles) and of one aos_soft_descend
beside the same definitions on one CPU core and beside aos_gvd_reach on the same inputs.

Inputs: the C2 skeleton with its graph (one seed-gen + GVD frame, then the call with no graph and no grid: the handle's
own graph and device skeleton) with the graph's nodes as the sources and with one source in a corner (the first passable
cell in raster order: the long wavefront); the C0 golden skeleton with its nodes as the sources and an empty 4096 x 4096 grid with one corner source,
both as an explicit graph and a grid already on the device. Every input at soft_cells 10, gain 2 and min_d2 0 and 16.
An input that the call refuses at those options (7 * max_weight * n_passable reaches 2^31: a 4096 x 4096 map with cells
of weight 19) is reported as a row with "refused" and the message, by the GPU call and the host statement alike, and is
then measured at gain 1 in a row named "..._gain_1".
GPU columns: the median of 20 calls after 5 warm-up calls, host clock around the call (it ends in a stream synchronise),
the call's own device times ms_mask / ms_wave / ms_graph, n_rounds and n_tile_runs; descend_ms, descend_cells and
plain_cost: one aos_soft_descend from the last reached cell with the maximum cost. reach_*: aos_gvd_reach with the same
grid, sources and min_d2 in the same job, measured the same way: its rounds and milliseconds beside soft's are the price
of the weights. Host column: tests/soft_host/soft_host_main.cpp built without sanitizers at the library Makefile's host
flags, the median of 3 runs of its Dijkstra inside that one process. The outputs of the GPU call and the host statement
are compared bit for bit. Prints one JSON line per row.

    python tools/bench_soft.py
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

WARMUP, CALLS, HOST_RUNS = 5, 20, 3
SOFT_CELLS, GAIN, MIN_D2 = 10, 2, (0, 16)


def build_host(out_dir):
    csrc = os.path.join(ROOT, "active-orchard-slam_amd", "csrc")
    exe = os.path.join(out_dir, "soft_host_main")
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3",
                    "-mtune=znver5", "-Wall", "-I", csrc, "-x", "c++",
                    os.path.join(ROOT, "tests", "soft_host", "soft_host_main.cpp"),
                    os.path.join(csrc, "soft_host.cpp"), os.path.join(csrc, "clearance_host.cpp"), "-o", exe], check=True)
    return exe


def main():
    import torch
    import numpy as np

    import aos_gpu
    import clearance_scenes as CS
    import orchard
    import soft_scenes as S
    from test_soft_cpu import COUNTS, blob, parse_host_output

    cfg = orchard.CONFIGS["C2"]
    c = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res))
    c.set_polygon(orchard.polygon(cfg))
    f = c.seedgen(orchard.generate(cfg))
    gg = c.gvd_from_seedgen()
    sk, org, res = f["skeleton_framed"], f["origin"], f["resolution"]
    c.gvd_clearance()
    d2 = c.clearance_field()
    # the first cell in raster order that is passable at each min_d2
    first = {m: np.argwhere((np.asarray(sk) != 100) & (d2 >= m))[0] for m in MIN_D2}
    corner = {m: [S.centre(int(first[m][1]), int(first[m][0]), org, float(np.float32(res)))] for m in MIN_D2}
    mk = lambda grid, src, m, nodes, o, r, gain=GAIN: S.scene(grid, src, SOFT_CELLS, gain, m, nodes=nodes, starts=[],  # noqa: E731
                                                              origin=o, resolution=r, cells=False)
    c0 = CS.c0_scene()
    empty = np.zeros((4096, 4096), np.int8)
    e_org, e_res = (3.5, -7.25), 0.05
    rows = []
    for m in MIN_D2:
        rows += [(f"c2_nodes_min_d2_{m}", mk(sk, gg["nodes"], m, gg["nodes"], org, res), "own"),
                 (f"c2_corner_source_min_d2_{m}", mk(sk, corner[m], m, gg["nodes"], org, res), "own"),
                 (f"c0_nodes_min_d2_{m}", mk(c0["grid"], c0["nodes"], m, c0["nodes"], c0["origin"], c0["resolution"]), "device"),
                 (f"empty_4096_corner_source_min_d2_{m}",
                  mk(empty, [S.centre(0, 0, e_org, float(np.float32(e_res)))], m, None, e_org, e_res), "device")]
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_host(tmp)

        def run_host(scene_list):
            fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(fi, "wb") as fh:
                fh.write(blob(scene_list))
            r = subprocess.run([exe, fi, fo, str(HOST_RUNS)], capture_output=True, text=True, check=True)   # (one thread)
            times = {int(l.split()[1]): float(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("ms ")}
            with open(fo, "rb") as fh:
                return parse_host_output(fh.read(), scene_list), times

        host, host_ms = run_host([r[1] for r in rows])
        # a row the bound refuses at GAIN is followed by the same input at gain 1
        extra = [(name + "_gain_1", dict(sc, gain=1), form) for (name, sc, form), h in zip(rows, host) if h["status"] != 0]
        more, more_ms = run_host([r[1] for r in extra]) if extra else ([], {})
    for j, row in enumerate(extra):
        at = [r[0] for r in rows].index(row[0][:-len("_gain_1")]) + 1
        rows.insert(at, row)
        host.insert(at, more[j])
        host_ms = {(k if k < at else k + 1): v for k, v in host_ms.items()}
        if j in more_ms:
            host_ms[at] = more_ms[j]
    ok = True
    p50 = lambda v: round(sorted(v)[len(v) // 2], 4)  # noqa: E731

    def measure(run):
        ms, parts, g = [], {"mask": [], "wave": [], "graph": []}, None
        for i in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            g = run()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                ms.append(dt)
                for key, v in parts.items():
                    v.append(g["ms"][key])
        return sorted(ms), parts, g

    for k, (name, sc, form) in enumerate(rows):
        H, W = sc["grid"].shape
        info = {"origin": sc["origin"], "resolution": sc["resolution"], "width": W, "height": H}
        opts = {"min_d2": sc["min_d2"], "soft_cells": SOFT_CELLS, "gain": sc["gain"]}
        if form == "device":
            d = torch.from_numpy(np.ascontiguousarray(sc["grid"]).reshape(-1)).cuda()
            torch.cuda.synchronize()
            run = lambda: c.gvd_soft(sc["sources"], graph=sc, grid=d.data_ptr(), info=info, on_device=True, **opts)  # noqa: E731
            run_reach = lambda: c.gvd_reach(sc["sources"], graph=sc, grid=d.data_ptr(), info=info, on_device=True,  # noqa: E731
                                            min_d2=sc["min_d2"])
        else:
            run = lambda: c.gvd_soft(sc["sources"], **opts)  # noqa: E731
            run_reach = lambda: c.gvd_reach(sc["sources"], min_d2=sc["min_d2"])  # noqa: E731
        h = host[k]
        if h["status"] != 0:   # the host statement refuses it: so must the call, with the bound's message
            try:
                run()
                message, ok = "not refused by the GPU call", False
            except RuntimeError as e:
                message = str(e)
                ok &= "n_passable" in message and "max_weight" in message
            print(json.dumps({"input": name, "width": W, "height": H, "form": form, "min_d2": sc["min_d2"],
                              "soft_cells": SOFT_CELLS, "gain": sc["gain"], "refused": message}), flush=True)
            continue
        ms, parts, g = measure(run)
        r_ms, r_parts, rg = measure(run_reach)
        fld = c.soft_field()
        equal = h["status"] == 0 and all(g[key] == h[key] for key in COUNTS) and fld.tobytes() == h["field"].tobytes()
        equal = equal and g["node_cost"].tobytes() == h["node_cost"].tobytes()
        # the same cells are reached as by reach, at no lower cost
        rf = c.reach_field()
        equal = equal and np.array_equal(rf == 0xFFFFFFFF, fld == 0xFFFFFFFF) and bool((fld >= rf).all())
        # one descent from the last cell with the maximum cost
        far = int(np.flatnonzero(h["field"].ravel() == h["max_cost"])[-1])
        start = np.array(S.centre(far % W, far // W, sc["origin"], sc["resolution"]), np.float64)
        n, plain = aos_gpu.c_u64(0), ctypes.c_uint32(0)
        aos_gpu._check(aos_gpu.lib().aos_soft_descend(c.h, start.ctypes.data, None, None, 0, ctypes.byref(n), None))
        cells = np.empty(n.value, np.uint32)
        t0 = time.perf_counter()
        aos_gpu._check(aos_gpu.lib().aos_soft_descend(c.h, start.ctypes.data, cells.ctypes.data, None, cells.size,
                                                      ctypes.byref(n), ctypes.byref(plain)))
        descend_ms = (time.perf_counter() - t0) * 1e3
        path = cells[:n.value].astype(np.int64)
        costs = h["field"].ravel()[path].astype(np.int64)
        equal = equal and n.value > 0 and path[0] == far and costs[-1] == 0 and bool((np.diff(costs) <= -5).all())
        equal = equal and plain.value >= int(rf.ravel()[far])
        ok &= bool(equal)
        out = {"input": name, "width": W, "height": H, "form": form, "min_d2": sc["min_d2"], "soft_cells": SOFT_CELLS,
               "gain": sc["gain"], "sources": len(sc["sources"]), "nodes": len(sc["nodes"])}
        out.update({key: g[key] for key in COUNTS})
        out.update({"n_rounds": g["n_rounds"], "n_tile_runs": g["n_tile_runs"]})
        out.update({"gpu_call_ms_p50": p50(ms), "gpu_call_ms_min": round(ms[0], 4), "gpu_call_ms_max": round(ms[-1], 4)})
        out.update({"gpu_ms_" + key + "_p50": p50(v) for key, v in parts.items()})
        out.update({"descend_ms": round(descend_ms, 4), "descend_cells": n.value, "plain_cost": plain.value,
                    "reach_cost_at_start": int(rf.ravel()[far]), "reach_call_ms_p50": p50(r_ms),
                    "reach_ms_wave_p50": p50(r_parts["wave"]), "reach_n_rounds": rg["n_rounds"],
                    "reach_n_tile_runs": rg["n_tile_runs"], "soft_over_reach": round(p50(ms) / max(p50(r_ms), 1e-9), 2),
                    "host_ms_p50": host_ms[k], "host_over_gpu": round(host_ms[k] / max(p50(ms), 1e-9), 2),
                    "bit_equal": bool(equal)})
        print(json.dumps(out), flush=True)
    c.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
