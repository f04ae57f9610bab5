"""Timing of many loop-closure candidates in one call: K = 1, 8, 32, 64 one-step candidates and 8 candidates of 8
steps (with --wide also 8 candidates of 17 and of 64 steps, which take the Woodbury step's global-memory path), each set once as a loop over the single-candidate call and once as one batch call, on the 625-pose C4shard graph
(`single`) and on the C4 batch of eight robots (`joint`).  Wall times: median and range of REPS runs after a warm-up.

    python tools/info_gain_batch_timing.py single|joint [--wide] # wall times
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/info_gain_batch_timing.py single|joint --once
    python tools/info_gain_batch_timing.py --summarise DIR       # device time and launches per kernel from that trace
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

KERNELS = r"(k_sub_fwd|k_sub_bwd|k_jms_push|k_jms_pull|k_jms_sum|k_jms_gather|k_jt_scatter|k_gram_blocks|k_gram_reduce|k_gram|k_woodbury_blocks|k_lm_V)"
REPS = 5


def summarise(d):
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    agg = defaultdict(lambda: [0, 0.0])
    for name, start, end in c.execute("select name, start, end from kernels"):
        m = re.search(KERNELS, name)
        if m:
            agg[m.group(1)][0] += 1
            agg[m.group(1)][1] += (end - start) * 1e-6
    for k, (n, ms) in sorted(agg.items()):
        print(f"{k:20s} launches {n:6d}  total {ms:9.3f} ms  mean {1e3 * ms / n:8.2f} us")


def sets(P, wide):
    """(name, trajectories) over the poses 0 .. P-1 of one robot."""
    out = [(f"{K} x 1 step", [[P - 1 - (7 * k) % (P // 2), (3 * k) % (P // 2)] for k in range(K)]) for K in (1, 8, 32, 64)]
    out.append(("8 x 8 steps", [[(P - 1 - 11 * k - (P // 9) * i) % P for i in range(9)] for k in range(8)]))
    if wide:      # k_woodbury_blocks factors these in global memory, one workgroup each; every candidate of 64 steps is a sweep of its own
        out.append(("8 x 17 steps", [[(P - 1 - 11 * k - (P // 18) * i) % P for i in range(18)] for k in range(8)]))
        out.append(("8 x 64 steps", [[(P - 1 - 11 * k - 9 * i) % P for i in range(65)] for k in range(8)]))
    return out


def report(name, single, batch, once):
    import numpy as np
    one, many = single(), batch()                    # (the warm-up)
    assert np.allclose(one, many, rtol=1e-6, atol=1e-6 * np.abs(one).max())
    t_one, t_many = [], []
    for _ in range(1 if once else REPS):
        t0 = time.perf_counter(); single(); t1 = time.perf_counter(); batch(); t2 = time.perf_counter()
        t_one.append(1e3 * (t1 - t0)); t_many.append(1e3 * (t2 - t1))
    print(f"{name:12s} single calls {np.median(t_one):8.2f} ms ({min(t_one):.2f} - {max(t_one):.2f})   one batch {np.median(t_many):7.2f} ms "
          f"({min(t_many):.2f} - {max(t_many):.2f})   ratio {np.median(t_one) / np.median(t_many):5.1f}", flush=True)


def main(which, once, wide):
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from slide_slam_amd.synth import SynthConfig, make_relmeas, make_robot_log, make_world
    from slide_slam_amd.replay import replay_single
    if which == "single":
        cfg = SynthConfig.preset("C4shard")
        gb = s.SlideBackend(s.default_params(), 1)
        replay_single(gb, make_robot_log(cfg, make_world(cfg), 0), collect=False)
        G = gb.graph
        G.gauss_newton(1)
        P = G.stats()["n_pose"]
        print("single graph:", P, "poses,", len(G.tile_profile()), "block columns")
        for name, trajs in sets(P, wide):
            travels = [[5.0] * (len(t) - 1) for t in trajs]
            report(name, lambda: np.array([G.closure_info_gain(0, t, d) for t, d in zip(trajs, travels)]),
                   lambda: G.closure_info_gain_batch(0, trajs, travels)[0], once)
        return
    from slide_slam_amd.distributed import PassDriver, gpu_matcher, setup_local_shards
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
    drv.one_pass()
    torch.cuda.synchronize()
    P = shards[0].graph.stats()["n_pose"]
    print("joint graph:", len(shards), "robots,", P, "poses in slot 0, separator coordinates", info["sep_dim"])
    for name, trajs in sets(P, wide):
        travels = [[5.0] * (len(t) - 1) for t in trajs]
        report(name, lambda: np.array([drv.closure_info_gain(0, t, d) for t, d in zip(trajs, travels)]),
               lambda: drv.closure_info_gain_batch(0, trajs, travels)[0], once)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else "single", "--once" in sys.argv, "--wide" in sys.argv)
