"""Timing of the observation loss on the exact joint pass: ms per PassDriver.one_pass() of the C4 job (8 robots of 625
poses in one CholBatch, the pass one replayed hipGraph).  Wall times with the device synchronised around the timed region: the
median (min - max) of 21 repetitions after three warm-ups.  Reported only.

  (i)   the batch's loss off and on (Huber on all classes), off and on alternating in one process;
  (ii)  the linearisation launch alone between two events (CholBatch.profile_linearize: k_lin_lf_b with the loss off,
        k_lin_lf_robust_b with it on), off and on alternating.  An event pair around one short launch mostly measures the launch;
  (iii) `--off-only`: the loss never set, nothing else - one process per run, for a comparison of this library against another
        build of it (SLIDE_LIB_VARIANT=<name> loads _lib/<name>.so: the parent commit's library built from its own sources), the
        two alternating.

    timeout -k 10 900 python tools/joint_observation_loss_timing.py >> profiles/joint_observation_loss_timing.txt
    timeout -k 10 300 python tools/joint_observation_loss_timing.py --off-only >> profiles/joint_observation_loss_timing.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM, PROF = 21, 3, 21


def main():
    off_only = "--off-only" in sys.argv
    preset = next((a for a in sys.argv[1:] if not a.startswith("--")), "C4")
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from slide_slam_amd.distributed import PassDriver, gpu_matcher, setup_local_shards
    from slide_slam_amd.replay import replay_single
    from slide_slam_amd.synth import SynthConfig, make_relmeas, make_robot_log, make_world
    cfg = SynthConfig.preset(preset)
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

    def fmt(v):
        return f"{np.median(v):8.3f} ms ({min(v):.3f} - {max(v):.3f})"
    head = (f"one_pass(), {cfg.robots} robots x {cfg.poses_per_robot} poses, {info['n_slots']} shared landmarks; ms wall, median (min - max) "
            f"of {REPS} after {WARM} warm-ups")
    if off_only:
        t = [timed() for _ in range(WARM + REPS)][WARM:]
        print(f"{head}; library {os.environ.get('SLIDE_LIB_VARIANT') or 'this change'}, loss never set: {fmt(t)}")
    else:
        t = {"off": [], "on": []}
        for rep in range(WARM + REPS):
            for tag in ("off", "on"):
                drv.set_observation_loss("huber" if tag == "on" else None)
                timed()                                    # (the first pass after a change of the loss captures the pass again)
                ms = timed()
                if rep >= WARM:
                    t[tag].append(ms)
        print(f"{head}, loss off and on (Huber, all classes) alternating")
        for tag in ("off", "on"):
            print(f"loss {tag:3s}: {fmt(t[tag])}")
        us = {"off": [], "on": []}
        for rep in range(WARM + PROF):
            for tag in ("off", "on"):
                drv.set_observation_loss("huber" if tag == "on" else None)
                drv.one_pass()
                v = 1e3 * batch.profile_linearize(drv.ptrs)
                if rep >= WARM:
                    us[tag].append(v)
        for tag, name in (("off", "k_lin_lf_b"), ("on", "k_lin_lf_robust_b")):
            print(f"{name}: {np.median(us[tag]):.2f} us ({min(us[tag]):.2f} - {max(us[tag]):.2f}) between two events around the launch, "
                  f"{PROF} launches after {WARM} (an event pair around one short launch mostly measures the launch)")
        drv.set_observation_loss("huber")
        drv.one_pass()
        ow = drv.observation_weights()
        print(f"weights of the last pass: {ow['n']} landmark factors, {int((ow['weight'] == 1.0).sum())} at 1, smallest {ow['weight'].min():.3e}")
    for gb in shards:
        gb.graph.join_chol_batch(None)


if __name__ == "__main__":
    main()
