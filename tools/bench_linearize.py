"""Latency of aos_path_linearize (the /aos/path -> /plan step) beside the same host code with the
node's own O(n^2) split search on the CPU.

Paths: zigzags of 25-pose legs at 0.2 m spacing with n = 250, 500, 1000 and 2000 poses, as they are (4 segments, up
to 3 searches) and shifted to end at the origin (10 segments, up to 9 searches), and the 5-pose path `five`, whose
searches have one candidate each: the call's fixed cost. GPU column: the median of 20 calls after 5 warm-up calls,
host clock around the call (it ends in a stream synchronise). Host column: tests/linearize_host/lin_host_main.cpp built
without sanitizers at the library Makefile's host flags, the median of 20 runs inside that one process. Both outputs
are compared bit for bit. Prints one JSON line per path.

    python tools/bench_linearize.py
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
    exe = os.path.join(out_dir, "lin_host_main")
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3",
                    "-mtune=znver5", "-Wall", "-I", csrc, "-x", "c++",
                    os.path.join(ROOT, "tests", "linearize_host", "lin_host_main.cpp"),
                    os.path.join(csrc, "linearize_host.cpp"), "-o", exe], check=True)
    return exe


def main():
    import torch  # noqa: F401  (shared HIP runtime first)
    import numpy as np

    import aos_gpu
    import linearize_scenes as S
    from test_linearize_cpu import _blob, parse_host_output

    paths = [("five", 0, S.five())]
    for n in (250, 500, 1000, 2000):
        paths.append((f"zigzag{n}", 0, S.zigzag(n // 25, 25)))
        paths.append((f"zigzag{n}_home", 1, S.zigzag_ending_at(0.0, 0.0, n // 25, 25)))
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_host(tmp)
        fi, fo = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fi, "wb") as f:
            f.write(_blob([p for _, _, p in paths]))
        r = subprocess.run([exe, fi, fo, str(CALLS)], capture_output=True, text=True, check=True)
        host_ms = {int(l.split()[1]): float(l.split()[3]) for l in r.stdout.splitlines() if l.startswith("ms ")}
        with open(fo, "rb") as f:
            host = parse_host_output(f.read(), len(paths))
    c = aos_gpu.Ctx(aos_gpu.default_params())
    ok = True
    for k, (name, home, p) in enumerate(paths):
        ms, inner = [], []
        for i in range(WARMUP + CALLS):
            t0 = time.perf_counter()
            g = c.path_linearize(p)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= WARMUP:
                ms.append(dt)
                inner.append(g["ms"])
        h = host[k]
        equal = (h["status"] == 0 and g["long_distance"] == h["long_distance"] == home
                 and np.array_equal(g["breakpoints"], h["breakpoints"])
                 and g["poses"].tobytes() == h["poses"].tobytes() and g["n_split_searches"] == h["n_split_searches"])
        ok &= bool(equal)
        ms.sort()
        inner.sort()
        print(json.dumps({"path": name, "n": len(p), "ends_at_origin": home, "n_split_searches": g["n_split_searches"],
                          "poses_out": len(g["poses"]), "gpu_call_ms_p50": round(ms[len(ms) // 2], 4),
                          "gpu_call_ms_min": round(ms[0], 4), "gpu_call_ms_max": round(ms[-1], 4),
                          "gpu_ms_linearize_p50": round(inner[len(inner) // 2], 4),
                          "host_ms_p50": host_ms[k], "bit_equal": bool(equal)}), flush=True)
    c.close()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
