"""Timing of SlideGraph.closure_mahalanobis: 1, 64 and 512 gate candidates on the 625-pose C4shard robot graph, and
beside each closure_info_gain_batch with the same number of one-step candidates — the nearest existing query: the same six columns per
candidate, but both substitution directions.  The expectation to check is roughly half its launch chain per sweep; no number is fixed
in advance.  Wall times with the device synchronised around the timed region: the median of 21 repetitions after three warm-ups.

    timeout -k 10 500 python tools/closure_gate_timing.py > profiles/closure_gate_timing.txt
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
    torch.zeros(1, device=torch.device("cuda", 0))      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from slide_slam_amd.replay import IDENT7
    from slide_slam_amd.synth import SynthConfig, frame_detections, make_robot_log, make_world
    cfg = SynthConfig.preset("C4shard")
    log = make_robot_log(cfg, make_world(cfg), 0)
    b = s.SlideBackend(s.default_params(), 1)
    prev = IDENT7.copy()
    for k in range(cfg.poses_per_robot):
        r = b.process_frame(0, log["rel7"][k], prev, frame_detections(log, k), 0)
        assert r["status"] == 0
        prev = r["pose7"].copy()
    G = b.graph
    P = cfg.poses_per_robot
    T = len(G.tile_profile())
    sigma = np.array([0.01] * 3 + [0.05] * 3)
    rng = np.random.default_rng(0)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    print(f"closure_mahalanobis against closure_info_gain_batch (one-step candidates), {P} poses, {T} tile columns; ms wall, median of "
          f"{REPS} after {WARM} warm-ups")
    for n in (1, 64, 512):
        ends = [(int(rng.integers(P // 2, P)), int(rng.integers(0, P // 2))) for _ in range(n)]
        closures = [(0, i, 0, j, IDENT7, sigma) for i, j in ends]
        trajs, travels = [[i, j] for i, j in ends], [[5.0]] * n

        def gate():
            return G.closure_mahalanobis(closures)

        def gain():
            return G.closure_info_gain_batch(0, trajs, travels, sigma)
        for _ in range(WARM):
            og, (_, st) = gate(), gain()
        assert (og["status"] == 0).all() and (st == 0).all()
        tg = [timed(gate) for _ in range(REPS)]
        ti = [timed(gain) for _ in range(REPS)]
        sweeps = (n + 63) // 64
        print(f"({n} candidates, {sweeps} sweep(s)) gate {np.median(tg):8.3f} ms ({min(tg):.3f} - {max(tg):.3f}), {T + 4} launches per sweep; "
              f"info gain {np.median(ti):8.3f} ms ({min(ti):.3f} - {max(ti):.3f}), {2 * T} substitution launches per sweep; "
              f"ratio {np.median(tg) / np.median(ti):.2f}", flush=True)


if __name__ == "__main__":
    main()
