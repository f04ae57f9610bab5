"""Timing of the joint-graph marginals on the exact joint pass's factor at C4 size on one GPU: eight robots of 625
poses in one CholBatch (as bench.py's exact leg builds them, with its relative-pose factors), one pass, then every pose of every robot
(the first call includes the selected inversion over the pass's elimination tree) and every robot's marginal_traces.

    python tools/joint_marginals_timing.py                 # wall times (stream synchronised), the pass's own time beside them
    rocprofv3 --kernel-trace -d DIR -o run -- python tools/joint_marginals_timing.py
    python tools/joint_marginals_timing.py --summarise DIR # device time and launches per kernel of joint_cov_kernels.hip from that trace
"""
import glob
import os
import re
import sqlite3
import sys
import time
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = r"(k_jsinv_prep|k_jsinv_tile|k_jsig_gather|k_sym_blocks|k_lm_cov|k_pose_blocks)"


def summarise(d):
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    agg = defaultdict(lambda: [0, 0.0])
    for name, start, end in c.execute("select name, start, end from kernels"):
        m = re.search(KERNELS, name)
        if m:
            key = m.group(1) + ("<true>" if m.group(1) == "k_jsinv_tile" and "ILb1" in name else "")
            agg[key][0] += 1
            agg[key][1] += (end - start) * 1e-6
    tot_n, tot_ms = 0, 0.0
    for k, (n, ms) in sorted(agg.items()):
        print(f"{k:20s} launches {n:6d}  total {ms:9.3f} ms  mean {1e3 * ms / n:8.2f} us")
        tot_n += n
        tot_ms += ms
    print(f"{'all':20s} launches {tot_n:6d}  total {tot_ms:9.3f} ms")


def main():
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from slide_slam_amd.distributed import PassDriver, gpu_matcher, setup_local_shards
    from slide_slam_amd.replay import replay_single
    from slide_slam_amd.synth import SynthConfig, make_relmeas, make_robot_log, make_world
    cfg = SynthConfig.preset("C4")
    world = make_world(cfg)
    logs = [make_robot_log(cfg, world, r) for r in range(cfg.robots)]
    shards = []
    for lg in logs:
        gb = s.SlideBackend(s.default_params(), 1)
        replay_single(gb, lg, collect=False)
        shards.append(gb)
    batch = s.CholBatch(len(shards))
    for t, gb in enumerate(shards):
        gb.graph.join_chol_batch(batch, t)
    bufs, info = setup_local_shards(shards, gpu_matcher, device=dev)
    drv = PassDriver(shards, bufs, info["n_slots"], batch=batch, device=dev, arrow=True, sep_dim=info["sep_dim"], sep_prof=info.get("sep_prof"))
    drv.setup_ghosts(make_relmeas(cfg, logs))
    P = [gb.graph.stats()["n_pose"] for gb in shards]
    print("robots", len(shards), "poses", P, "shared slots", info["n_slots"], "separator coordinates", info["sep_dim"])
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); drv.one_pass(); torch.cuda.synchronize(); t1 = time.perf_counter()
        cov = drv.get_pose_covariances(0, np.arange(P[0])); t2 = time.perf_counter()
        for r in range(1, len(shards)):
            drv.get_pose_covariances(r, np.arange(P[r]))
        t3 = time.perf_counter()
        tr = [drv.marginal_traces(r) for r in range(len(shards))]; t4 = time.perf_counter()
        assert np.isfinite(cov).all() and all(np.isfinite(t).all() for t in tr)
        print(f"rep {rep}: pass {1e3 * (t1 - t0):.2f} ms; robot 0's {P[0]} pose marginals incl. the joint selected inversion "
              f"{1e3 * (t2 - t1):.2f} ms; the other robots' poses (cached) {1e3 * (t3 - t2):.2f} ms; marginal_traces x {len(shards)} "
              f"{1e3 * (t4 - t3):.2f} ms ({int(tr[0][3])} point landmarks); pose trace robot 0 {tr[0][0]:.6g}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        main()
