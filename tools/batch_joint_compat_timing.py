"""Timing of CholBatch.observation_joint_compatibility on the C4 eight-robot batch (as tools/joint_closure_gate_timing.py
builds it) after one exact joint pass: one group of 20 point candidates at robot 0's newest pose against its nearest landmarks (one
frame's hypothesis), 6 such groups in one call (the newest poses of six robots), and one group of 128 points (384 rows: a whole sweep,
the chain's longest run); beside each, CholBatch.observation_mahalanobis on the same candidates.  Each at prob = 0.99.  No number is
fixed in advance.  Wall times with the device synchronised around the timed region, the two calls alternating in one process: the
median (min - max) of 21 repetitions after three warm-ups.

    timeout -k 10 900 python tools/batch_joint_compat_timing.py > profiles/batch_joint_compat_timing.txt

--summarise DIR: from a `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/batch_joint_compat_timing.py` run (a run
of its own, no counters), the device time of each joint-compatibility sweep by part (fill, walk, signed gram, chain), medians per
number of candidates in the sweep.
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

    def point(sl, p, ls, l):
        st, x = shards[sl].graph.get_pose12(0, p)
        assert st == 0
        Rm, t = x[:9].reshape(3, 3), x[9:12]
        st, v = shards[ls].graph.get_landmark(2, l)
        assert st == 0
        q = Rm.T @ (v[:3] - t)
        return ("point", sl, p, l, q / np.linalg.norm(q), float(np.linalg.norm(q)), ls)

    def nearest(sl, n):
        """The n points nearest to robot sl's newest pose: its own graph's first, then (where it holds fewer) the next robots', named
        cross-robot."""
        st, x = shards[sl].graph.get_pose12(0, P[sl] - 1)
        out = []
        for ls in [(sl + i) % R for i in range(R)]:
            xyz, _ = shards[ls].landmark_table(2)
            near = np.argsort(np.linalg.norm(xyz - x[9:12], axis=1))
            out += [point(sl, P[sl] - 1, ls, int(l)) for l in near[:n - len(out)]]
            if len(out) == n:
                return out
        raise AssertionError((sl, n, len(out)))
    frame = nearest(0, 20)
    six = [nearest(sl, 20) for sl in range(min(6, R))]
    sweep = nearest(0, 128)
    print(f"of the 128 points {sum(x[6] != 0 for x in sweep)} are named cross-robot")

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    print(f"observation_joint_compatibility against observation_mahalanobis on the joint graph (the same candidates), prob 0.99; ms wall, median "
          f"(min - max) of {REPS} after {WARM} warm-ups, the two calls alternating")
    for name, groups in (("one group of 20 points at robot 0's newest pose", [frame]), (f"{len(six)} such groups in one call, one robot each", six),
                         ("one group of 128 points at robot 0's newest pose", [sweep])):
        flat = [x for g in groups for x in g]

        def joint():
            return batch.observation_joint_compatibility(groups, prob=0.99)

        def gate():
            return batch.observation_mahalanobis(flat)
        for _ in range(WARM):
            oj, og = joint(), gate()
        assert (oj["status"] == 0).all() and (oj["group_status"] == 0).all() and (og["status"] == 0).all()
        tj, tg = [], []
        for _ in range(REPS):
            tj.append(timed(joint))
            tg.append(timed(gate))
        print(f"({name}: {len(flat)} candidates, {3 * len(flat)} rows, accepted {oj['group_count'].tolist()}) joint compatibility "
              f"{np.median(tj):8.3f} ms ({min(tj):.3f} - {max(tj):.3f}); individual gate {np.median(tg):8.3f} ms ({min(tg):.3f} - {max(tg):.3f}); "
              f"ratio {np.median(tj) / np.median(tg):.2f}", flush=True)


def summarise(d):
    import csv
    import glob
    rows = list(csv.DictReader(open(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    grid = [k for k in rows[0] if "Grid_Size" in k][0]
    recs, cur = {}, None

    def close(cur):
        if cur and cur["chain"] > 0:
            recs.setdefault(cur["key"], []).append([cur[k] for k in ("fill", "walk", "gram", "chain")])
    for r in rows:
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "k_joint_obs_joint_lin" in name:           # a sweep starts with its fill and ends behind its chain launches
            close(cur)
            cur = dict(key=int(r[grid]) // 64, fill=us, walk=0.0, gram=0.0, chain=0.0)
        elif cur is None:
            continue
        elif "k_gram_" in name:
            cur["gram"] += us
        elif "k_joint_compat_chain" in name:
            cur["chain"] += us
        elif cur["chain"] > 0:
            close(cur)
            cur = None
        else:
            cur["walk"] += us
    close(cur)
    for key, v in sorted(recs.items()):
        m = np.median(np.array(v), axis=0)
        print(f"{key} candidates in the sweep, {len(v)} calls: device us, median: fill {m[0]:.1f}, walk {m[1]:.1f}, gram (signed) {m[2]:.1f}, chain {m[3]:.1f}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        main()
