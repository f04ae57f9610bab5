"""Timing of CholBatch.observation_mahalanobis on the C4 eight-robot batch (as tools/joint_closure_gate_timing.py builds
it) after one exact joint pass: 20 point candidates at each robot's newest pose against its nearest landmarks (one frame's worth per
robot), 128 points at robot 0's newest pose (one full sweep), and 1024 candidates of all three classes across the trajectories, about
half of them a pose of one robot against a landmark of another's graph; beside each, CholBatch.closure_mahalanobis with the same number
of COLUMNS of B (three per point, nine per cube, seven per cylinder against six per closure): both walk the forward half of the same
plan and form the same grams.  No number is fixed in advance.  Wall times with the device synchronised around the timed region, the two
calls alternating in one process: the median (min - max) of 21 repetitions after three warm-ups.

    timeout -k 10 900 python tools/joint_observation_gate_timing.py > profiles/joint_observation_gate_timing.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

REPS, WARM = 21, 3


def main():
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from observation_gate_timing import quat
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
    cnt = [gb.counts() for gb in shards]
    print(f"{R} robots, poses {P}, shared slots {info['n_slots']}, separator coordinates {info['sep_dim']}, lambda coordinates {getattr(drv, 'lam_dim', 0)}")
    sigma = np.array([0.01] * 3 + [0.05] * 3)
    rng = np.random.default_rng(0)

    def pose(sl, p):
        st, x = shards[sl].graph.get_pose12(0, p)
        assert st == 0
        return x[:9].reshape(3, 3), x[9:12]

    def pose7(sl, p):
        Rm, t = pose(sl, p)
        return np.concatenate([t, quat(Rm)])

    def lm(sl, cls, l):
        st, v = shards[sl].graph.get_landmark(cls, l)
        assert st == 0
        return v

    def point(sl, p, ls, l):
        Rm, t = pose(sl, p)
        q = Rm.T @ (lm(ls, 2, l)[:3] - t)
        return ("point", sl, p, l, q / np.linalg.norm(q), float(np.linalg.norm(q)), ls)

    def cube(sl, p, ls, l):
        v = lm(ls, 1, l)
        return ("cube", sl, p, l, pose7(sl, p), np.concatenate([v[9:12], quat(v[:9].reshape(3, 3))]), v[12:15], ls)

    def cylinder(sl, p, ls, l):
        v = lm(ls, 0, l)
        return ("cylinder", sl, p, l, pose7(sl, p), v[:3], v[3:6], float(v[6]), ls)

    def nearest(sl):
        xyz, _ = shards[sl].landmark_table(2)
        return np.argsort(np.linalg.norm(xyz - pose(sl, P[sl] - 1)[1], axis=1))
    frames = [point(sl, P[sl] - 1, sl, int(l)) for sl in range(R) for l in nearest(sl)[:20]]
    near0 = nearest(0)
    sweep = [point(0, P[0] - 1, 0, int(near0[i % len(near0)])) for i in range(128)]
    mixed = []
    for i in range(1024):
        kind = ("point", "cube", "point", "cylinder")[i % 4]
        sl = int(rng.integers(R))
        ls = sl if i % 2 == 0 else (sl + 1 + int(rng.integers(R - 1))) % R
        p = int(rng.integers(P[sl]))
        if kind == "cube" and cnt[ls]["cube"] > 0:
            mixed.append(cube(sl, p, ls, int(rng.integers(cnt[ls]["cube"]))))
        elif kind == "cylinder" and cnt[ls]["cyl"] > 0:
            mixed.append(cylinder(sl, p, ls, int(rng.integers(cnt[ls]["cyl"]))))
        else:
            mixed.append(point(sl, p, ls, int(rng.integers(cnt[ls]["point"]))))

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
    print(f"observation_mahalanobis against closure_mahalanobis on the joint graph (the same number of columns); ms wall, median (min - max) of "
          f"{REPS} after {WARM} warm-ups, the two calls alternating")
    dims = {"point": 3, "cube": 9, "cylinder": 7}
    per = {"point": 128, "cube": 42, "cylinder": 54}
    for name, cands in ((f"one frame per robot: 20 points at each of {R} newest poses", frames), ("128 points at robot 0's newest pose", sweep),
                        ("1024 mixed across the trajectories, half of them cross-robot", mixed)):
        cols = sum(dims[c[0]] for c in cands)
        ncl = (cols + 5) // 6
        closures = [(a, i, b, j, IDENT7, sigma) for a, i, b, j in ends(ncl)]
        sweeps = sum((sum(c[0] == k for c in cands) + per[k] - 1) // per[k] for k in per)

        def gate():
            return batch.observation_mahalanobis(cands)["status"]

        def closure():
            return batch.closure_mahalanobis(closures)["status"]
        for _ in range(WARM):
            sg, sc = gate(), closure()
        assert (sg == 0).all() and (sc == 0).all(), (sg, sc)
        tg, tc = [], []
        for _ in range(REPS):
            tg.append(timed(gate))
            tc.append(timed(closure))
        print(f"({name}: {len(cands)} candidates, {cols} columns, {sweeps} sweep(s)) gate {np.median(tg):8.3f} ms ({min(tg):.3f} - {max(tg):.3f}); "
              f"closure gate, {ncl} closures = {6 * ncl} columns, {(ncl + 63) // 64} sweep(s), {np.median(tc):8.3f} ms ({min(tc):.3f} - {max(tc):.3f}); "
              f"ratio {np.median(tg) / np.median(tc):.2f}", flush=True)


if __name__ == "__main__":
    main()
