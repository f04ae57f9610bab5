"""Timing of CLIPPER's affinity matrix as CSR: the dense path (k_clipper_affinity writing m x m doubles, k_clq_csr
reading them twice) against the sparse build (k_affinity_csr count + emit) in one process and one build, on the bench's generator
(bench.py's affinity leg: an eighth of the associations true, sigma 0.1, epsilon 0.3) at m = 256, 4096, 16 384.  Device times from
slide_last_device_ms (HIP events around the launches), wall times around the calls: median and range of REPS runs after a warm-up.

    python tools/affinity_csr_timing.py [m ...]                   # both tables
    SLIDE_AFFINITY_CSR_GATHER=0 python tools/affinity_csr_timing.py --sparse-only   # points read through A (the variant not taken)
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/affinity_csr_timing.py --once [--sparse-only]
    python tools/affinity_csr_timing.py --summarise DIR           # per-launch device time of every kernel of that trace
(the kernel trace is a run of its own; --once runs every size one time after the warm-up; --sparse-only leaves the dense path out)
"""
import glob
import os
import re
import sqlite3
import sys
import time
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = r"(k_affinity_csr<[^>]*>|k_affinity_csr|k_affinity_gather|k_clipper_affinity|k_clq_csr<[^>]*>|k_clq_csr|k_clq_solve_coop|k_clq_solve)"
REPS = 5
SIZES = (256, 4096, 16384)


def summarise(d):
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    agg = defaultdict(list)
    try:
        rows = list(c.execute("select name, start, end, grid_x from kernels"))
    except sqlite3.OperationalError:          # (a trace database without the launch geometry: one line per kernel)
        rows = [(n, a, b, 0) for n, a, b in c.execute("select name, start, end from kernels")]
    for name, start, end, gx in rows:
        m = re.search(KERNELS, name)
        if m:
            agg[(m.group(1), gx)].append((end - start) * 1e-3)
    for (k, gx), us in sorted(agg.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        us.sort()
        print(f"{k:40s} grid_x {gx:9d}  launches {len(us):4d}  median {us[len(us) // 2]:11.1f} us  ({us[0]:.1f} - {us[-1]:.1f})")


def problem(m):
    import numpy as np
    rng = np.random.default_rng(20240229 + m)
    D1 = rng.uniform(-100, 100, (m, 2))
    D2 = D1 + rng.normal(0, 0.02, (m, 2))
    A = np.column_stack([np.arange(m), rng.permutation(m)]).astype(np.int32)
    A[: m // 8, 1] = A[: m // 8, 0]
    return D1, D2, A, rng.uniform(0, 1, m)


def fmt(v):
    import numpy as np
    return f"{np.median(v):10.3f} ({min(v):.3f} - {max(v):.3f})"


def main(sizes, once, sparse_only):
    import numpy as np
    import torch
    torch.zeros(1, device="cuda:0")      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from slide_slam_amd import api
    p = s.clipper_params(sigma=0.1, epsilon=0.3)
    gather = os.environ.get("SLIDE_AFFINITY_CSR_GATHER") != "0"
    print(f"sparse build reads the points {'pre-gathered per association' if gather else 'through the association list'}; "
          f"ms, median (min - max) of {1 if once else REPS} after a warm-up", flush=True)
    for m in sizes:
        D1, D2, A, u0 = problem(m)

        def dense():
            t0 = time.perf_counter()
            M = s.clipper_affinity(D1, D2, A, sigma=0.1, epsilon=0.3)
            ms = api.last_device_ms(api.MS_AFFINITY)
            out = s.clipper_dense_clique(M, u0, p)
            t1 = time.perf_counter()
            return out, ms, api.last_device_ms(api.MS_CLQ_CSR), api.last_device_ms(api.MS_CLQ_SOLVE), 1e3 * (t1 - t0)

        def sparse():
            t0 = time.perf_counter()
            out = s.clipper_match(D1, D2, A, u0, p)
            t1 = time.perf_counter()
            return out, api.last_device_ms(api.MS_AFFINITY_CSR), api.last_device_ms(api.MS_CLQ_SOLVE), 1e3 * (t1 - t0)
        got = sparse()[0]
        nnz = api.last_device_ms(api.MS_CLQ_NNZ)
        if not sparse_only:
            want = dense()[0]
            assert all(np.array_equal(a, b) for a, b in zip(got[:2], want[:2])) and got[2] == want[2], "the two paths disagree"
        d_aff, d_csr, d_solve, d_wall, s_csr, s_solve, s_wall = [], [], [], [], [], [], []
        for _ in range(1 if once else REPS):
            if not sparse_only:
                _, a, c, sv, w = dense()
                d_aff.append(a); d_csr.append(c); d_solve.append(sv); d_wall.append(w)
            _, c, sv, w = sparse()
            s_csr.append(c); s_solve.append(sv); s_wall.append(w)
        print(f"m = {m}: nnz {int(nnz)} ({100 * nnz / max(m * m, 1):.2f} % of m^2), clique {len(got[0])}")
        if not sparse_only:
            both = [a + c for a, c in zip(d_aff, d_csr)]
            print(f"  dense   device: k_clipper_affinity {fmt(d_aff)}  + k_clq_csr x 2 {fmt(d_csr)}  = {fmt(both)}")
        print(f"  sparse  device: {'k_affinity_gather + ' if gather else ''}k_affinity_csr x 2 {fmt(s_csr)}")
        if not sparse_only:
            print(f"  solve   device: after dense {fmt(d_solve)}   after sparse {fmt(s_solve)}")
            print(f"  wall: clipper_affinity + clipper_dense_clique {fmt(d_wall)}   clipper_match {fmt(s_wall)}", flush=True)
        else:
            print(f"  solve   device: {fmt(s_solve)}   wall: clipper_match {fmt(s_wall)}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        ms = tuple(int(a) for a in sys.argv[1:] if a.isdigit()) or SIZES
        main(ms, "--once" in sys.argv, "--sparse-only" in sys.argv)
