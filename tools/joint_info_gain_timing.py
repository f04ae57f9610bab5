"""Timing of loop-closure information gain on the joint graph at C4 size on one GPU: eight robots of 625 poses in
one CholBatch (as tools/joint_marginals_timing.py builds them), one exact pass, then gain queries of m = 1, 3 and 64 steps on robot 0
and one inter-robot candidate (robot 0 to robot 1, m = 1).  The substitutions through the pass's elimination tree are the device part;
C^-1 of the 6m x 6m C runs on the host.

    python tools/joint_info_gain_timing.py                 # wall times (stream synchronised)
    rocprofv3 --kernel-trace -d DIR -o run -- python tools/joint_info_gain_timing.py
    python tools/joint_info_gain_timing.py --summarise DIR # device time and launches per kernel of the gain queries from that trace
"""
import glob
import os
import re
import sqlite3
import sys
import time
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = r"(k_jms_push|k_jms_pull|k_jms_sum|k_jms_gather|k_jt_scatter|k_gram|k_lm_V)"


def summarise(d):
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    agg = defaultdict(lambda: [0, 0.0])
    groups, last = [], None          # (the queries, told apart by the host's gaps between them: allocations, C^-1)
    for name, start, end in c.execute("select name, start, end from kernels order by start"):
        m = re.search(KERNELS, name)
        if m:
            if last is None or start - last > 5e5:
                groups.append([0, 0.0])
            last = end
            groups[-1][0] += 1
            groups[-1][1] += (end - start) * 1e-6
            key = m.group(1) + (("<bwd>" if "ILb1" in name or "<true>" in name else "<fwd>") if m.group(1) in ("k_jms_push", "k_jms_pull") else "")
            agg[key][0] += 1
            agg[key][1] += (end - start) * 1e-6
    tot_n, tot_ms = 0, 0.0
    for k, (n, ms) in sorted(agg.items()):
        print(f"{k:20s} launches {n:6d}  total {ms:9.3f} ms  mean {1e3 * ms / n:8.2f} us")
        tot_n += n
        tot_ms += ms
    print(f"{'all':20s} launches {tot_n:6d}  total {tot_ms:9.3f} ms  (every query of the run: {QUERIES} per rep, {REPS} reps)")
    for q, (n, ms) in enumerate(groups):
        print(f"query {q:2d}: launches {n:5d}  device {ms:8.3f} ms")


REPS = 3
QUERIES = "m = 1, 3, 64, inter-robot m = 1"


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
    torch.cuda.synchronize()
    t0 = time.perf_counter(); drv.one_pass(); torch.cuda.synchronize(); t1 = time.perf_counter()
    print(f"pass {1e3 * (t1 - t0):.2f} ms")
    p0 = P[0]
    qs = [("m=1", 0, [p0 - 1, 0], None), ("m=3", 0, [p0 - 1, 2 * p0 // 3, p0 // 3, 0], None),
          ("m=64", 0, list(np.linspace(p0 - 1, 0, 65).astype(int)), None), ("inter m=1", 0, [P[1] - 1, p0 - 1], [1, 0])]
    for rep in range(REPS):
        line = []
        for name, slot, traj, rob in qs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g = drv.closure_info_gain(slot, traj, [5.0] * (len(traj) - 1), None, rob)
            t1 = time.perf_counter()
            assert np.isfinite(g).all() and g[0] > 0
            line.append(f"{name} {1e3 * (t1 - t0):.2f} ms (gain {g[0]:.4g}, all robots' poses {g[3]:.4g})")
        print(f"rep {rep}: " + "; ".join(line))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        main()
