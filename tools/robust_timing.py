"""Timing of the robust loss: ms per SlideGraph.gauss_newton(1) with the loss off and on (Huber) on the 625-pose C4shard
robot graph with 64 loop closures added, and the device time of k_robust_reweight itself beside the linearisation launch it precedes
(SlideGraph.get_profile).  Reported only; the expectation to check is one short launch of a few microseconds per iteration.  Wall
times with the device synchronised around the timed region: the median of 21 repetitions after three warm-ups, off and on alternating.

    timeout -k 10 500 python tools/robust_timing.py > profiles/robust_loss_timing.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM, NCLOSE, PROF_ITERS = 21, 3, 64, 20


def rel7(a12, b12, dt):
    """a^-1 b of two poses (R row-major, t) as (t, quaternion xyzw), its translation moved by dt."""
    from scipy.spatial.transform import Rotation
    Ra, Rb = a12[:9].reshape(3, 3), b12[:9].reshape(3, 3)
    q = Rotation.from_matrix(Ra.T @ Rb).as_quat()
    return np.concatenate([Ra.T @ (b12[9:] - a12[9:]) + dt, q if q[3] >= 0 else -q])


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
    rng = np.random.default_rng(0)
    # closures on the graph's own estimate, a few closure sigmas off; every eighth one 2 m off
    for n in range(NCLOSE):
        i, j = int(rng.integers(0, P // 2)), int(rng.integers(P // 2, P))
        dt = rng.normal(0, 3e-3, 3) + (np.array([2.0, 0.0, 0.0]) if n % 8 == 7 else 0.0)
        G.add_loop_closure(rel7(G.get_pose12(0, i)[1], G.get_pose12(0, j)[1], dt), i, 0, j, 0)

    G.set_robust_loss("huber")
    assert G.gauss_newton(1) == 0
    w0 = G.closure_weights()["weight"]                 # (before the plain steps of the alternation below bend the chain onto the offsets)
    G.set_robust_loss(None)

    def timed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert G.gauss_newton(1) == 0
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    t = {"off": [], "on": []}
    for rep in range(WARM + REPS):
        for tag in ("off", "on"):
            G.set_robust_loss("huber" if tag == "on" else None)
            timed()                                    # (the first step after a change of the loss re-captures the pass)
            ms = timed()
            if rep >= WARM:
                t[tag].append(ms)
    nf = G.stats()["n_factors"]
    print(f"gauss_newton(1), {P} poses, {nf} factors of which {NCLOSE} loop closures, {len(G.tile_profile())} tile columns; ms wall, median of "
          f"{REPS} after {WARM} warm-ups, loss off and on alternating")
    for tag in ("off", "on"):
        print(f"loss {tag:3s}: {np.median(t[tag]):8.3f} ms ({min(t[tag]):.3f} - {max(t[tag]):.3f})")
    G.set_robust_loss("huber")
    G.set_profiling(True)
    for _ in range(PROF_ITERS):
        assert G.gauss_newton(1) == 0
    prof = G.get_profile()
    for name in ("k_robust_reweight", "linearize"):
        p = prof[name]
        print(f"{name}: {1e3 * p['ms'] / p['launches']:.2f} us per launch over {p['launches']} launches (HIP events around the launch)")
    print(f"weights of the first reweighted step: {int((w0 == 1.0).sum())} at 1, {int((w0 < 0.1).sum())} below 0.1, smallest {w0.min():.3e}")


if __name__ == "__main__":
    main()
