"""Timing of the duplicate-landmark queries on the joint graph: CholBatch.landmark_pair_mahalanobis on DupJoint's planted
list (tests/joint_landmark_pair_cases.py: two robots of 14 poses, 25 point pairs) and, on the C4 eight-robot batch (as
tools/batch_joint_compat_timing.py builds it) after one exact joint pass, on one full sweep of 128 cross-robot point pairs proposed by
landmark_pairs_within(cross_only=True); beside them get_landmark_pair_covariances on the same pairs and the search itself.  No number
is fixed in advance.  Wall times with the device synchronised around the timed region: the median (min - max) of 21 repetitions after
three warm-ups.

    timeout -k 10 900 python tools/joint_landmark_pair_timing.py > profiles/joint_landmark_pair_timing.txt

--summarise DIR: from a `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/joint_landmark_pair_timing.py` run (a run
of its own, no counters), the device time of each sweep of the test by part (fill, walk, signed gram, finish), medians per number of
pairs in the sweep.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, WARM = 21, 3


def series(torch, f):
    def timed():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    for _ in range(WARM):
        f()
    t = [timed() for _ in range(REPS)]
    return f"{np.median(t):8.3f} ms ({min(t):.3f} - {max(t):.3f})"


def dup_joint(torch, s):
    import joint_graphs as jg
    import joint_landmark_pair_cases as jp
    from slide_slam_amd.distributed import PassDriver, setup_local_shards
    dev = torch.device("cuda", 0)
    J = jp.DupJoint()
    shards, assoc = jg.build(J, lambda: s.SlideGraph(s.default_params(**jp.DUP_KW)))
    batch = s.CholBatch(J.R)
    for t, sh in enumerate(shards):
        sh.graph.join_chol_batch(batch, t)
    bufs, info = setup_local_shards(shards, None, device=dev, assoc=assoc)
    drv = PassDriver(shards, bufs, info["n_slots"], batch=batch, device=dev, arrow=True, sep_dim=info["sep_dim"], sep_prof=info.get("sep_prof"))
    drv.setup_ghosts(J.relmeas)
    drv.one_pass()
    torch.cuda.synchronize()
    gid = assoc[0]
    rows = np.array([(ra, int(np.flatnonzero(gid[ra][2] == ga)[0]), rb, int(np.flatnonzero(gid[rb][2] == gb)[0]))
                     for ra, ga, rb, gb, _, _ in J.dups["point"]], np.int64)
    sigma = jp.SIGMA["point"]
    out = batch.landmark_pair_mahalanobis(s.CLS_ELLIPSOID, rows, sigma)
    assert (out["status"] == 0).all()
    print(f"DupJoint: 2 robots of 14 poses, {len(rows)} planted point pairs ({int((rows[:, 0] != rows[:, 2]).sum())} across robots), one sweep")
    print(f"    landmark_pair_mahalanobis:      {series(torch, lambda: batch.landmark_pair_mahalanobis(s.CLS_ELLIPSOID, rows, sigma))}", flush=True)
    print(f"    get_landmark_pair_covariances:  {series(torch, lambda: batch.get_landmark_pair_covariances(s.CLS_ELLIPSOID, rows))}", flush=True)
    print(f"    landmark_pairs_within, 1.5 m:   {series(torch, lambda: batch.landmark_pairs_within(s.CLS_ELLIPSOID, 1.5, True))}", flush=True)
    for sh in shards:
        sh.graph.join_chol_batch(None)


def c4(torch, s):
    from slide_slam_amd.distributed import PassDriver, gpu_matcher, setup_local_shards
    from slide_slam_amd.replay import replay_single
    from slide_slam_amd.synth import SynthConfig, make_relmeas, make_robot_log, make_world
    dev = torch.device("cuda", 0)
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
    drv.one_pass()
    torch.cuda.synchronize()
    print(f"C4: {R} robots, poses {[gb.graph.stats()['n_pose'] for gb in shards]}, shared slots {info['n_slots']}, separator coordinates "
          f"{info['sep_dim']}, lambda coordinates {getattr(drv, 'lam_dim', 0)}")
    sigma = np.full(3, 0.05)
    radius, rows = 0.5, np.zeros((0, 4), np.int64)
    while len(rows) < 128 and radius < 64.0:          # grow the radius until the search proposes a full sweep of served cross pairs
        sa, ia, sb, ib, _ = batch.landmark_pairs_within(s.CLS_ELLIPSOID, radius, True)
        near = np.stack([sa, ia.astype(np.int64), sb, ib.astype(np.int64)], axis=1)
        st = batch.landmark_pair_mahalanobis(s.CLS_ELLIPSOID, near[:4096], sigma)["status"]
        rows = near[:4096][st == 0]
        n_near = len(near)
        radius *= 1.5
    radius /= 1.5
    print(f"    landmark_pairs_within(cross_only) at {radius:.2f} m: {n_near} pairs; {series(torch, lambda: batch.landmark_pairs_within(s.CLS_ELLIPSOID, radius, True))}",
          flush=True)
    if len(rows) < 128:
        print("    fewer than 128 served cross-robot pairs on this job: the sweep is not measured")
        return
    rows = rows[:128]
    print(f"    one sweep of 128 cross-robot point pairs ({int((rows[:, 0] != rows[:, 2]).sum())} with ends in two slots):")
    print(f"    landmark_pair_mahalanobis:      {series(torch, lambda: batch.landmark_pair_mahalanobis(s.CLS_ELLIPSOID, rows, sigma))}", flush=True)
    print(f"    get_landmark_pair_covariances (two sweeps of 64): {series(torch, lambda: batch.get_landmark_pair_covariances(s.CLS_ELLIPSOID, rows))}",
          flush=True)


def main():
    import torch
    torch.zeros(1, device=torch.device("cuda", 0))      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    print(f"landmark pairs on the joint graph; ms wall, median (min - max) of {REPS} after {WARM} warm-ups")
    dup_joint(torch, s)
    c4(torch, s)
    print("per-stage device times (fill, walk, gram, finish): from a kernel trace in a run of its own, --summarise")


def summarise(d):
    import csv
    import glob
    rows = list(csv.DictReader(open(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    grid = [k for k in rows[0] if "Grid_Size" in k][0]
    recs, cur = {}, None
    for r in rows:
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "k_joint_lm_pair_fill" in name:            # a sweep starts with its fill and ends with its finish
            cur = dict(key=int(r[grid]) // 64, fill=us, walk=0.0, gram=0.0, finish=0.0)
        elif cur is None:
            continue
        elif "k_gram_" in name:
            cur["gram"] += us
        elif "k_obs_gate_finish" in name or "k_joint_lm_pair_cov_finish" in name:
            cur["finish"] = us
            recs.setdefault((cur["key"], "cov" if "cov_finish" in name else "test"), []).append([cur[k] for k in ("fill", "walk", "gram", "finish")])
            cur = None
        else:
            cur["walk"] += us
    for key, v in sorted(recs.items()):
        m = np.median(np.array(v), axis=0)
        print(f"{key[0]} pairs in the sweep ({key[1]}), {len(v)} sweeps: device us, median: fill {m[0]:.1f}, walk {m[1]:.1f}, gram (signed) {m[2]:.1f}, "
              f"finish {m[3]:.1f}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        main()
