"""Timing of SlideGraph.observation_mahalanobis on the 625-pose C4shard robot graph tools/closure_gate_timing.py uses:
20 point candidates at the newest pose against its nearest landmarks (one frame's worth), 128 of them (one full sweep), and 1024
candidates of all three classes across the trajectory; beside each, closure_mahalanobis with the same number of COLUMNS of B (three per
point, nine per cube, seven per cylinder against six per closure).  For the first list also the walk forced to start at block column 0
(SLIDE_OBS_GATE_FULL_WALK=1): what the short walk saves.  No number is fixed in advance.  Wall times with the device synchronised
around the timed region: the median (min - max) of 21 repetitions after three warm-ups.

    timeout -k 10 500 python tools/observation_gate_timing.py > profiles/observation_gate_timing.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 21, 3


def quat(R):
    """Rotation matrix -> (x, y, z, w)."""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-3:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(max(1e-300, 1.0 + R[i, i] - R[j, j] - R[k, k])) * 2
    q = np.zeros(4)
    q[i], q[j], q[k], q[3] = s / 4, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return q


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
    cnt = b.counts()

    def pose(p):
        st, x = G.get_pose12(0, p)
        assert st == 0
        return x[:9].reshape(3, 3), x[9:12]

    def pose7(p):
        R, t = pose(p)
        return np.concatenate([t, quat(R)])

    def point(p, l):
        R, t = pose(p)
        q = R.T @ (G.get_landmark(2, l)[1] - t)
        return ("point", 0, p, l, q / np.linalg.norm(q), float(np.linalg.norm(q)))

    def cube(p, l):
        v = G.get_landmark(1, l)[1]
        return ("cube", 0, p, l, pose7(p), np.concatenate([v[9:12], quat(v[:9].reshape(3, 3))]), v[12:15])

    def cylinder(p, l):
        v = G.get_landmark(0, l)[1]
        return ("cylinder", 0, p, l, pose7(p), v[:3], v[3:6], float(v[6]))

    xyz, _ = b.landmark_table(2)
    near = np.argsort(np.linalg.norm(xyz - pose(P - 1)[1], axis=1))
    frame = [point(P - 1, int(l)) for l in near[:20]]
    sweep = [point(P - 1, int(near[i % len(near)])) for i in range(128)]
    mixed = []
    for i in range(1024):
        kind = ("point", "cube", "point", "cylinder")[i % 4]
        if kind == "cube" and cnt["cube"] > 0:
            mixed.append(cube(int(rng.integers(P)), int(rng.integers(cnt["cube"]))))
        elif kind == "cylinder" and cnt["cyl"] > 0:
            mixed.append(cylinder(int(rng.integers(P)), int(rng.integers(cnt["cyl"]))))
        else:
            mixed.append(point(int(rng.integers(P)), int(rng.integers(cnt["point"]))))

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
        return f"{np.median(t):8.3f} ms ({min(t):.3f} - {max(t):.3f})", float(np.median(t))
    print(f"observation_mahalanobis against closure_mahalanobis (the same number of columns), {P} poses, {T} tile columns, {cnt['point']} points, "
          f"{cnt['cube']} cubes, {cnt['cyl']} cylinders; ms wall, median (min - max) of {REPS} after {WARM} warm-ups")
    dims = {"point": 3, "cube": 9, "cylinder": 7}
    for name, cands in (("one frame: 20 points at the newest pose", frame), ("128 points at the newest pose", sweep),
                        ("1024 mixed across the trajectory", mixed)):
        cols = sum(dims[c[0]] for c in cands)
        ncl = (cols + 5) // 6
        ends = [(int(rng.integers(P // 2, P)), int(rng.integers(0, P // 2))) for _ in range(ncl)]
        closures = [(0, i, 0, j, IDENT7, sigma) for i, j in ends]
        tg, mg = series(lambda: G.observation_mahalanobis(cands))
        tc, mc = series(lambda: G.closure_mahalanobis(closures))
        print(f"({name}: {len(cands)} candidates, {cols} columns) gate {tg}; closure gate, {ncl} closures = {6 * ncl} columns, {tc}; ratio "
              f"{mg / mc:.2f}", flush=True)
        if cands is frame:
            os.environ["SLIDE_OBS_GATE_FULL_WALK"] = "1"
            tf, mf = series(lambda: G.observation_mahalanobis(cands))
            del os.environ["SLIDE_OBS_GATE_FULL_WALK"]
            print(f"    the same list, the walk forced to start at block column 0 ({T} substitution launches): {tf}; the short walk takes "
                  f"{mg / mf:.2f} of it (the candidates' pose {P - 1} lies in block column {6 * (P - 1) // 64} of {T}; the landmarks' first "
                  f"observers start the walk earlier)", flush=True)


if __name__ == "__main__":
    main()
