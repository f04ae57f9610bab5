"""Timing of the gate at the predicted pose on the 625-pose C4shard robot graph tools/observation_gate_timing.py uses.

1. SlideGraph.predicted_observation_mahalanobis for one frame's worth — 20 point candidates at the prediction behind the newest
   pose, against its nearest landmarks — beside observation_mahalanobis for the same landmarks AT the newest pose (the in-graph gate),
   and the same call with the walk forced to start at block column 0 (SLIDE_OBS_GATE_FULL_WALK=1): where the time goes.
2. The streaming frame: two back-ends replay the same log, one with the association gate on (prob 0.99, drop), one without; the
   last REPS frames of each are timed one by one (process_frame, the device synchronised around it).  Under the default sigmas
   (1 m / 1 rad, 400) the gate rejects nothing, so both take the same frames; the difference is the gate's cost.
3. bench.py --gpus 1: ms_per_step with the parent's library (SLIDE_LIB_VARIANT=<name>: _lib/<name>.so, a build of the parent
   commit) and with this one, alternating, each in a fresh process.  Skipped, and said so, when no such library is given.

No number is fixed in advance.  Wall times with the device synchronised around the timed region: the median (min - max) of 21
repetitions after three warm-ups.

    timeout -k 10 900 python tools/predicted_gate_timing.py [--parent-variant NAME] [--bench-pairs N] > profiles/predicted_gate_timing.txt
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 21, 3


def quat(R):
    """Rotation matrix -> (x, y, z, w)."""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def pose_of(p7):
    x, y, z, w = np.asarray(p7[3:], float) / np.linalg.norm(p7[3:])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R, np.asarray(p7[:3], float)


def bench_once(variant, steps, warmup):
    env = dict(os.environ)
    env.pop("SLIDE_LIB_VARIANT", None)
    if variant:
        env["SLIDE_LIB_VARIANT"] = variant
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-variant", default=None, help="name of a parent-commit build under slide_slam_amd/_lib/ (NAME.so)")
    ap.add_argument("--bench-pairs", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=200)
    ap.add_argument("--bench-warmup", type=int, default=20)
    args = ap.parse_args()
    if args.parent_variant:      # (before this process opens the device: the runs are children of their own, one at a time)
        print(f"== python bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}, the parent's library and this one alternating ==")
        both = {"parent": [], "this change": []}
        for _ in range(args.bench_pairs):
            both["parent"].append(bench_once(args.parent_variant, args.bench_steps, args.bench_warmup))
            both["this change"].append(bench_once(None, args.bench_steps, args.bench_warmup))
        for name, v in both.items():
            print(f"{name:12s}: ms_per_step " + ", ".join(f"{x:.5f}" for x in v), flush=True)
    else:
        print("== bench.py: no parent library given (--parent-variant), not measured ==", flush=True)

    import torch
    torch.zeros(1, device=torch.device("cuda", 0))      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from slide_slam_amd.replay import IDENT7
    from slide_slam_amd.synth import SynthConfig, frame_detections, make_robot_log, make_world
    cfg = SynthConfig.preset("C4shard")
    log = make_robot_log(cfg, make_world(cfg), 0)
    P = cfg.poses_per_robot

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def fmt(t):
        return f"{np.median(t):8.3f} ms ({min(t):.3f} - {max(t):.3f})"

    # ---- 2. the streaming frame, gate off and on (the last REPS frames of the replay; WARM frames before them untimed) ----------
    runs = {}
    for name, gate in (("gate off", None), ("gate on ", 0.99)):
        b = s.SlideBackend(s.default_params(), 1)
        if gate:
            b.set_association_gate(gate, "drop")
        prev = IDENT7.copy()
        t, ta = [], []
        for k in range(P):
            det = frame_detections(log, k)
            ms, r = timed(lambda: b.process_frame(0, log["rel7"][k], prev, det, 0))
            assert r["status"] == 0
            prev = r["pose7"].copy()
            if k >= P - REPS:
                t.append(ms); ta.append(1e3 * r["t_assoc"])
        runs[name] = (b, t, ta, prev)
    print(f"== the streaming frame (process_frame, C4shard robot 0, frames {P - REPS} .. {P - 1}; ms wall, median (min - max) of {REPS}) ==")
    for name, (b, t, ta, _) in runs.items():
        print(f"{name}: frame {fmt(t)}; of it association (with the gate, where on) {fmt(ta)}; gate_stats {b.gate_stats()}", flush=True)
    same = np.array_equal(runs["gate off"][3], runs["gate on "][3])
    print(f"the two replays end at the same pose bit for bit: {same}")

    # ---- 1. the call by itself ---------------------------------------------------------------------------------------------------
    b = runs["gate off"][0]
    G = b.graph
    T = len(G.tile_profile())
    cnt = b.counts()

    def pose(p):
        st, x = G.get_pose12(0, p)
        assert st == 0
        return x[:9].reshape(3, 3), x[9:12]

    Rk, tk = pose(P - 1)
    Rr, tr = pose_of(log["rel7"][P - 1])                 # (the last step again: a plausible next one)
    Rn, tn = Rk @ Rr, tk + Rk @ tr
    rel7 = np.concatenate([tr, quat(Rr)])
    est7 = np.concatenate([tn, quat(Rn)])
    xyz, _ = b.landmark_table(2)
    near = np.argsort(np.linalg.norm(xyz - tn, axis=1))[:20]

    def point(R, t, l):
        q = R.T @ (G.get_landmark(2, l)[1] - t)
        return ("point", 0, P - 1, l, q / np.linalg.norm(q), float(np.linalg.norm(q)))
    at_pred = [point(Rn, tn, int(l)) for l in near]
    at_pose = [point(Rk, tk, int(l)) for l in near]

    def series(f):
        for _ in range(WARM):
            out = f()
        assert (out["status"] == 0).all(), out["status"]
        t = [timed(f)[0] for _ in range(REPS)]
        return fmt(t), float(np.median(t))
    print(f"== the call by itself: 20 point candidates, {P} poses, {T} tile columns, {cnt['point']} points, {cnt['cube']} cubes, {cnt['cyl']} cylinders; "
          f"ms wall, median (min - max) of {REPS} after {WARM} warm-ups ==")
    tp, mp = series(lambda: G.predicted_observation_mahalanobis(0, P - 1, rel7, est7, at_pred))
    tg, mg = series(lambda: G.observation_mahalanobis(at_pose))
    print(f"predicted_observation_mahalanobis, from pose {P - 1}: {tp}")
    print(f"observation_mahalanobis at pose {P - 1}, the same landmarks: {tg}; the prediction takes {mp / mg:.2f} of it")
    os.environ["SLIDE_OBS_GATE_FULL_WALK"] = "1"
    tf, mf = series(lambda: G.predicted_observation_mahalanobis(0, P - 1, rel7, est7, at_pred))
    del os.environ["SLIDE_OBS_GATE_FULL_WALK"]
    print(f"the same call, the walk forced to start at block column 0 ({T} substitution launches): {tf}; the short walk takes {mp / mf:.2f} of it")
    one = [at_pred[0]]
    t1, m1 = series(lambda: G.predicted_observation_mahalanobis(0, P - 1, rel7, est7, one))
    t0, m0 = series(lambda: G.predicted_observation_mahalanobis(0, P - 1, rel7, est7, []))
    print(f"one candidate: {t1}; an empty list (the state checks and the call's own overhead): {t0}")
    print("(where the time goes: one linearise-and-fill launch, the substitution launches from the walk's first block column on, two gram "
          "launches, one finish launch and ONE read-back per class; the difference between 20 candidates and one is the width of the sweep, "
          "the rest is launch latency and the read-back's synchronise)")


if __name__ == "__main__":
    main()
