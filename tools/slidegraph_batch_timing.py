"""Timing of inter-robot SlideGraph place recognition over a list of robot pairs: one reference map against 1, 7 and 28
query maps, at 45, 200 and 792 objects per map, each set once as a loop over the existing single call (run_semantic_clipper: the path
a caller had before) and once as one find_inter_loop_closures_clipper call, in one process.  The query maps are views of the reference
map from other frames (all objects, another order, 1 cm noise) at the object density of the 45-object test maps.  Wall times: median and
range of REPS runs after a warm-up.

    python tools/slidegraph_batch_timing.py [sizes ...]          # wall times (default sizes: 45 200 792)
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/slidegraph_batch_timing.py --once 45 200
    python tools/slidegraph_batch_timing.py --summarise DIR      # device time and launches per kernel from that trace
(the kernel trace is a run of its own, with no counters alongside; --once runs every set one time after the warm-up)
"""
import glob
import os
import re
import sqlite3
import sys
import time
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = (r"(k_tri_match_seg|k_tri_match|k_tri_prepare|k_seg_scan|k_affinity_csr_seg|k_affinity_csr|k_affinity_gather|k_clq_pack_u|"
           r"k_clq_solve_coop|k_clq_solve_b|k_clq_solve)")
REPS = 5
KW = dict(sigma=0.05, epsilon=0.15, num_inliers_threshold=4, matching_threshold=0.1)


def summarise(d):
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    agg = defaultdict(lambda: [0, 0.0])
    tables = [r[0] for r in c.execute("select name from sqlite_master where type in ('table', 'view') and name like 'kernels%'")]
    for name, start, end in c.execute(f"select name, start, end from {tables[0]}"):
        m = re.search(KERNELS, name)
        if m:
            agg[m.group(1)][0] += 1
            agg[m.group(1)][1] += (end - start) * 1e-6
    for k, (n, ms) in sorted(agg.items()):
        print(f"{k:20s} launches {n:6d}  total {ms:9.3f} ms  mean {1e3 * ms / n:8.2f} us")


def make_maps(n, n_query):
    import numpy as np
    span = 30.0 * (n / 45.0) ** 0.5
    rng = np.random.default_rng(n)
    ref = np.zeros((n, 7)); ref[:, 0] = 1; ref[:, 1:3] = rng.uniform(-span, span, (n, 2))
    qrys = []
    for _ in range(n_query):
        yaw, t = rng.uniform(-np.pi, np.pi), rng.uniform(-5, 5, 2)
        R = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
        q = np.zeros((n, 7)); q[:, 0] = 1
        q[:, 1:3] = (ref[rng.permutation(n), 1:3] - t) @ R + rng.normal(0, 0.01, (n, 2))
        qrys.append(q)
    return ref, qrys


def main(sizes, once):
    import numpy as np
    import torch
    torch.zeros(1, device=torch.device("cuda", 0))      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    p = s.slidegraph_params(**KW)
    for n in sizes:
        for n_query in (1, 7, 28):
            ref, qrys = make_maps(n, n_query)
            maps, pairs = [ref] + qrys, [(0, k + 1) for k in range(n_query)]
            loop = lambda: [s.run_semantic_clipper(ref, q, sigma=KW["sigma"], epsilon=KW["epsilon"], min_num_pairs=KW["num_inliers_threshold"],
                                                   matching_threshold=KW["matching_threshold"]) for q in qrys]
            batch = lambda: s.find_inter_loop_closures_clipper(maps, pairs, p)
            one, many = loop(), batch()                    # (the warm-up)
            assert [r["n_putative"] for r in one] == [r["n_putative"] for r in many] and [r["n_inliers"] for r in one] == [r["n_inliers"] for r in many]
            assert all(np.abs(m["tf"] - np.linalg.inv(o["tf"])).max() <= 1e-12 for o, m in zip(one, many))
            t_one, t_many = [], []
            for _ in range(1 if once else REPS):
                t0 = time.perf_counter(); loop(); t1 = time.perf_counter(); batch(); t2 = time.perf_counter()
                t_one.append(1e3 * (t1 - t0)); t_many.append(1e3 * (t2 - t1))
            m = [r["n_putative"] for r in many]
            print(f"{n:4d} objects x {n_query:2d} queries  associations {min(m)} - {max(m)}, found {sum(r['found'] for r in many)}   "
                  f"loop of single calls {np.median(t_one):9.2f} ms ({min(t_one):.2f} - {max(t_one):.2f})   one list call {np.median(t_many):9.2f} ms "
                  f"({min(t_many):.2f} - {max(t_many):.2f})   ratio {np.median(t_one) / np.median(t_many):5.2f}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        args = [a for a in sys.argv[1:] if not a.startswith("--")]
        main([int(a) for a in args] or [45, 200, 792], "--once" in sys.argv)
