"""Latency of aos_gvd_clearance (the exact distance field and the GvdGraph's clearances) beside the same definitions on
one CPU core.

Inputs: the C2 skeleton with its graph (one seed-gen + GVD frame, then the call with no arguments: the handle's own
graph and device skeleton), a 4096 x 4096 grid with a single occupied cell (the row pass's worst case: every cell's
search crosses the whole row) and the C0 golden skeleton with its graph; the last two as an explicit graph and a grid
already on the device. GPU columns: the median of 20 calls after 5 warm-up calls, host clock around the call (it ends
in a stream synchronise), and the call's own device times ms_field / ms_graph. Host column:
tests/clearance_host/clear_host_main.cpp built without sanitizers at the library Makefile's host flags, the median of
20 runs inside that one process (field and graph timed apart). Both outputs are compared bit for bit. Prints one JSON
line per input.

    python tools/bench_clearance.py
"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("tools", "tests", "active-orchard-slam_amd"):
    sys.path.insert(0, os.path.join(ROOT, sub))

WARMUP, CALLS = 5, 20


def build_host(out_dir):
    csrc = os.path.join(ROOT, "active-orchard-slam_amd", "csrc")
    exe = os.path.join(out_dir, "clear_host_main")
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3",
                    "-mtune=znver5", "-Wall", "-I", csrc, "-x", "c++",
                    os.path.join(ROOT, "tests", "clearance_host", "clear_host_main.cpp"),
                    os.path.join(csrc, "clearance_host.cpp"), "-o", exe], check=True)
    return exe


def main():
    import torch
    import numpy as np

    import aos_gpu
    import clearance_scenes as S
    import orchard
    from test_clearance_cpu import blob, parse_host_output

    cfg = orchard.CONFIGS["C2"]
    c = aos_gpu.Ctx(aos_gpu.default_params(grid_resolution=cfg.res))
    c.set_polygon(orchard.polygon(cfg))
    f = c.seedgen(orchard.generate(cfg))
    gg = c.gvd_from_seedgen()
    c2 = S.scene(f["skeleton_framed"], gg["nodes"], gg["edges"], f["origin"], f["resolution"])
    single = np.zeros((4096, 4096), np.int8)
    single[0, 0] = 100
    inputs = [("c2", c2, "own"), ("single_cell_4096", S.scene(single), "device"), ("c0", S.c0_scene(), "device")]
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_host(tmp)
        fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fi, "wb") as fh:
            fh.write(blob([sc for _, sc, _ in inputs]))
        r = subprocess.run([exe, fi, fo, str(CALLS)], capture_output=True, text=True, check=True)   # (one thread)
        host_ms = {int(l.split()[1]): (float(l.split()[3]), float(l.split()[4]))
                   for l in r.stdout.splitlines() if l.startswith("ms ")}
        with open(fo, "rb") as fh:
            host = parse_host_output(fh.read(), [sc for _, sc, _ in inputs])
    ok = True
    for k, (name, sc, form) in enumerate(inputs):
        H, W = sc["grid"].shape
        info = {"origin": sc["origin"], "resolution": sc["resolution"], "width": W, "height": H}
        if form == "device":
            d = torch.from_numpy(np.ascontiguousarray(sc["grid"]).reshape(-1)).cuda()
            torch.cuda.synchronize()
            run = lambda: c.gvd_clearance(graph=sc, grid=d.data_ptr(), info=info, on_device=True)  # noqa: E731
        else:
            run = lambda: c.gvd_clearance()  # noqa: E731
        ms, msf, msg = [], [], []
        for i in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            g = run()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                ms.append(dt)
                msf.append(g["ms"]["field"])
                msg.append(g["ms"]["graph"])
        fld = c.clearance_field()
        h = host[k]
        equal = (h["status"] == 0 and fld.tobytes() == h["field"].tobytes() and g["n_occupied"] == h["n_occupied"]
                 and g["max_d2"] == h["max_d2"]
                 and all(g[key].tobytes() == h[key].tobytes()
                         for key in ("node_d2", "edge_d2", "node_clearances", "edge_clearances")))
        ok &= bool(equal)
        for v in (ms, msf, msg):
            v.sort()
        p50 = lambda v: round(v[len(v) // 2], 4)  # noqa: E731
        print(json.dumps({"input": name, "width": W, "height": H, "n_occupied": g["n_occupied"], "max_d2": g["max_d2"],
                          "nodes": len(sc["nodes"]), "edges": len(sc["edges"]), "form": form,
                          "gpu_call_ms_p50": p50(ms), "gpu_call_ms_min": round(ms[0], 4), "gpu_call_ms_max": round(ms[-1], 4),
                          "gpu_ms_field_p50": p50(msf), "gpu_ms_graph_p50": p50(msg),
                          "host_ms_field_p50": host_ms[k][0], "host_ms_graph_p50": host_ms[k][1], "bit_equal": bool(equal)}),
              flush=True)
    c.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
