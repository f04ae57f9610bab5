"""Timing of CholBatch.closure_mahalanobis and CholBatch.get_pose_pair_covariances on the C4 eight-robot batch (as
tools/joint_info_gain_timing.py builds it): 1, 64 and 512 inter-robot gate candidates and 32 inter-robot pose pairs after one exact
joint pass, and beside each closure_info_gain_batch with the same number of one-step inter-robot candidates — the same column count
walked through BOTH halves of the same plan, plus the Woodbury step.  The gate walks the forward half alone; the expectation to check
is "about half the substitution launches", and the condition only that the gate's range for 64 closures lies below the information
gain's range for 64 candidates.  No number is fixed in advance.  Wall times with the device synchronised around the timed region, both
calls alternating in one process: the median of 21 repetitions after three warm-ups.

    timeout -k 10 900 python tools/joint_closure_gate_timing.py > profiles/joint_closure_gate_timing.txt
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/joint_closure_gate_timing.py      # (a run of its own)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 21, 3


def main():
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from slide_slam_amd.distributed import PassDriver, gpu_matcher, setup_local_shards
    from slide_slam_amd.replay import IDENT7, replay_single
    from slide_slam_amd.synth import SynthConfig, make_relmeas, make_robot_log, make_world
    cfg = SynthConfig.preset("C4")
    world = make_world(cfg)
    logs = [make_robot_log(cfg, world, r) for r in range(cfg.robots)]
    shards = []
    for lg in logs:
        gb = s.SlideBackend(s.default_params(), 1)
        replay_single(gb, lg, collect=False)
        shards.append(gb)
    R = len(shards)
    batch = s.CholBatch(R)
    for t, gb in enumerate(shards):
        gb.graph.join_chol_batch(batch, t)
    bufs, info = setup_local_shards(shards, gpu_matcher, device=dev)
    drv = PassDriver(shards, bufs, info["n_slots"], batch=batch, device=dev, arrow=True, sep_dim=info["sep_dim"], sep_prof=info.get("sep_prof"))
    drv.setup_ghosts(make_relmeas(cfg, logs))
    P = [gb.graph.stats()["n_pose"] for gb in shards]
    drv.one_pass()
    torch.cuda.synchronize()
    print(f"{R} robots, poses {P}, shared slots {info['n_slots']}, separator coordinates {info['sep_dim']}, lambda coordinates {getattr(drv, 'lam_dim', 0)}")
    sigma = np.array([0.01] * 3 + [0.05] * 3)
    rng = np.random.default_rng(0)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def ends(n):
        out = []
        for _ in range(n):
            a = int(rng.integers(R))
            b = (a + 1 + int(rng.integers(R - 1))) % R
            out.append((a, int(rng.integers(P[a] // 2, P[a])), b, int(rng.integers(0, P[b] // 2))))
        return out
    print(f"closure_mahalanobis / get_pose_pair_covariances against closure_info_gain_batch (one-step inter-robot candidates); ms wall, "
          f"median of {REPS} after {WARM} warm-ups, the two calls alternating")
    for what, n in (("gate", 1), ("gate", 64), ("gate", 512), ("pairs", 32)):
        e = ends(n)
        closures = [(a, i, b, j, IDENT7, sigma) for a, i, b, j in e]
        trajs, slots, travels = [[i, j] for _, i, _, j in e], [[a, b] for a, _, b, _ in e], [[5.0]] * n

        def query():
            if what == "gate":
                return batch.closure_mahalanobis(closures)["status"]
            return batch.get_pose_pair_covariances(e)[1]

        def gain():
            return batch.closure_info_gain_batch(0, trajs, travels, sigma, slots)[1]
        for _ in range(WARM):
            sq, sg = query(), gain()
        assert (sq == 0).all() and (sg == 0).all()
        tq, tg = [], []
        for _ in range(REPS):
            tq.append(timed(query))
            tg.append(timed(gain))
        cols = (6 if what == "gate" else 12) * n
        print(f"({n} {what}, {cols} columns, {(cols + 383) // 384} sweep(s)) {what} {np.median(tq):8.3f} ms ({min(tq):.3f} - {max(tq):.3f}); "
              f"info gain of {n} candidates ({6 * n} columns) {np.median(tg):8.3f} ms ({min(tg):.3f} - {max(tg):.3f}); "
              f"ratio {np.median(tq) / np.median(tg):.2f}", flush=True)


if __name__ == "__main__":
    main()
