"""Timing of the robust loss on the exact joint pass: ms per PassDriver.one_pass() of the C4 job (8 robots of 625
poses in one CholBatch, the pass one replayed hipGraph) with the batch's loss off and on (Huber on the relative-measurement class:
the inter-robot relative-pose factors), off and on alternating in one process, and the device time of the one added launch,
k_robust_reweight_b, between two events (CholBatch.profile_robust_reweight).  An event pair around one short launch mostly measures
the launch itself (a few microseconds of dispatch), not the kernel's work.  Reported only.  Wall times with the device synchronised
around the timed region: the median (min - max) of 21 repetitions after three warm-ups.

    timeout -k 10 900 python tools/joint_robust_timing.py >> profiles/joint_robust_loss_timing.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM, PROF = 21, 3, 20


def main():
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from slide_slam_amd.distributed import PassDriver, gpu_matcher, setup_local_shards
    from slide_slam_amd.replay import replay_single
    from slide_slam_amd.synth import SynthConfig, make_relmeas, make_robot_log, make_world
    cfg = SynthConfig.preset(sys.argv[1] if len(sys.argv) > 1 else "C4")
    wm = make_world(cfg)
    logs = [make_robot_log(cfg, wm, r) for r in range(cfg.robots)]
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
    rel = make_relmeas(cfg, logs)
    drv.setup_ghosts(rel)
    for _ in range(3):
        drv.one_pass()

    def timed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        drv.one_pass()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    t = {"off": [], "on": []}
    for rep in range(WARM + REPS):
        for tag in ("off", "on"):
            drv.set_robust_loss("huber" if tag == "on" else None, closures=False)
            timed()                                    # (the first pass after a change of the loss captures the pass again)
            ms = timed()
            if rep >= WARM:
                t[tag].append(ms)
    print(f"one_pass(), {cfg.robots} robots x {cfg.poses_per_robot} poses, {len(rel)} inter-robot relative-pose factors, {info['n_slots']} shared "
          f"landmarks; ms wall, median (min - max) of {REPS} after {WARM} warm-ups, loss off and on (Huber, relative measurements) alternating")
    for tag in ("off", "on"):
        print(f"loss {tag:3s}: {np.median(t[tag]):8.3f} ms ({min(t[tag]):.3f} - {max(t[tag]):.3f})")
    drv.set_robust_loss("huber", closures=False)
    drv.one_pass()
    us = [1e3 * batch.profile_robust_reweight(drv.ptrs) for _ in range(PROF)]
    print(f"k_robust_reweight_b: {np.median(us):.2f} us ({min(us):.2f} - {max(us):.2f}) between two events around the launch, {PROF} launches "
          "(an event pair around one short launch mostly measures the launch)")
    drv.one_pass()                                     # (the profiled launches wrote weights of no pass: the read-back wants a pass)
    cw = drv.closure_weights()["relmeas"]
    print(f"weights of the last pass: {int((cw['weight'] == 1.0).sum())} of {len(cw['weight'])} at 1, smallest {np.nanmin(cw['weight']):.3e}")
    for gb in shards:
        gb.graph.join_chol_batch(None)


if __name__ == "__main__":
    main()
