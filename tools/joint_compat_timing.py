"""Timing of SlideGraph.observation_joint_compatibility on the 625-pose C4shard robot graph
tools/observation_gate_timing.py uses: one group of 20 point candidates at the newest pose against its nearest landmarks (one frame's
hypothesis) beside observation_mahalanobis on the same 20 candidates, 6 such groups in one call, and one group of 128 points (384
rows: a whole sweep, the chain's longest run).  Each at prob = 0.99 and evaluate-only.  No number is fixed in advance.  Wall times
with the device synchronised around the timed region: the median (min - max) of 21 repetitions after three warm-ups.

    timeout -k 10 500 python tools/joint_compat_timing.py > profiles/joint_compat_timing.txt

--summarise DIR: from a `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/joint_compat_timing.py` run, the device
time of each call by part (fill, walk, gram, chain), medians per number of candidates in the sweep.
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
    cnt = b.counts()

    def point(p, l):
        st, x = G.get_pose12(0, p)
        assert st == 0
        R, t = x[:9].reshape(3, 3), x[9:12]
        q = R.T @ (G.get_landmark(2, l)[1] - t)
        return ("point", 0, p, l, q / np.linalg.norm(q), float(np.linalg.norm(q)))

    xyz, _ = b.landmark_table(2)
    st, x = G.get_pose12(0, P - 1)
    near = np.argsort(np.linalg.norm(xyz - x[9:12], axis=1))
    assert len(near) >= 128, len(near)
    frame = [point(P - 1, int(l)) for l in near[:20]]
    sweep = [point(P - 1, int(l)) for l in near[:128]]

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def series(f):
        for _ in range(WARM):
            out = f()
        assert (out["status"] == 0).all(), out["status"]
        t = [timed(f) for _ in range(REPS)]
        return f"{np.median(t):8.3f} ms ({min(t):.3f} - {max(t):.3f})", float(np.median(t)), out
    print(f"observation_joint_compatibility, {P} poses, {T} tile columns, {cnt['point']} points; ms wall, median (min - max) of {REPS} after "
          f"{WARM} warm-ups")
    tg, mg, _ = series(lambda: G.observation_mahalanobis(frame))
    print(f"(observation_mahalanobis, the same 20 points one by one) {tg}", flush=True)
    for name, groups in (("one group of 20 points at the newest pose", [frame]), ("6 such groups in one call", [frame] * 6),
                         ("one group of 128 points", [sweep])):
        for prob in (0.99, 0.0):
            tj, mj, out = series(lambda: G.observation_joint_compatibility(groups, prob=prob))
            assert (out["group_status"] == 0).all()
            tail = f"; ratio to the individual gate {mj / mg:.2f}" if groups[0] is frame and len(groups) == 1 else ""
            print(f"({name}, prob {prob}: {sum(len(g) for g in groups)} candidates, {3 * sum(len(g) for g in groups)} rows, accepted "
                  f"{out['group_count'].tolist()}) {tj}{tail}", flush=True)


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
        if "k_obs_joint_lin" in name:                 # a sweep starts with its fill and ends behind its chain launches
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
        print(f"{key} candidates in the sweep, {len(v)} calls: device us, median: fill {m[0]:.1f}, walk {m[1]:.1f}, gram {m[2]:.1f}, chain {m[3]:.1f}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        main()
