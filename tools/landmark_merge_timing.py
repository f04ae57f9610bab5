"""Timing of slide_graph_merge_landmarks on a 625-pose single-robot graph of C4shard's length with its split
landmarks planted: a chain of 625 key frames 1 m apart; every key frame k starts a point landmark k seen from k .. k + 3, and every
second one is SPLIT, the object mapped again as point 100000 + k from k + 4 .. k + 6 (the association lost its match); every fifth key
frame a cylinder seen from k .. k + 2.  The graph is built through the binding's add calls, so the same call list, with the dropped
keys renamed, is also the only alternative the graph offered before: destroy it, build it again rekeyed, gauss_newton(1).

Per pair count n (1, 16, 256 split point pairs, fuse = 1), on a fresh solved graph each time: wall ms of the merge_landmarks call
(device synchronised around it) and its parts from slide_graph_merge_timing (host restructure; upload; the fusion with its table
upload and read-back; k_lm_merge_fuse alone between two HIP events), wall ms of the solve() that follows (the full update), and of the
alternative, split into the replay of the call list through the binding (Python and ctypes: an upper bound on what a C++ caller
pays) and the gauss_newton(1) behind it.  Median (min - max) of REPS fresh graphs after one warm-up graph.  No number is fixed in
advance.

    timeout -k 10 500 python tools/landmark_merge_timing.py > profiles/landmark_merge_timing.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, P, SPLIT = 5, 625, 100000


def yaw7(t, yaw):
    return np.array([t[0], t[1], t[2], 0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)])


def plant(seed=0):
    """The graph as a list of (method, arguments) and the (keep, drop) rows of its split points."""
    rng = np.random.default_rng(seed)
    yaw = np.cumsum(rng.normal(0, 0.03, P))
    pos = np.zeros((P, 3))
    for k in range(1, P):
        pos[k] = pos[k - 1] + np.array([np.cos(yaw[k]), np.sin(yaw[k]), 0.0])
    calls = [("set_prior", (0, yaw7(pos[0], yaw[0])))]
    est = [yaw7(pos[0], yaw[0])]
    for k in range(1, P):
        c, s = np.cos(yaw[k - 1]), np.sin(yaw[k - 1])
        d = pos[k] - pos[k - 1]
        rel = yaw7([c * d[0] + s * d[1], -s * d[0] + c * d[1], 0.0], yaw[k] - yaw[k - 1])
        est.append(yaw7(pos[k] + rng.normal(0, 0.01, 3), yaw[k] + rng.normal(0, 0.002)))
        calls.append(("add_keypose_between", (0, k - 1, k, rel, est[k])))

    def bearing(k, xyz):
        c, s = np.cos(yaw[k]), np.sin(yaw[k])
        d = xyz - pos[k]
        q = np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1], d[2]])
        return q / np.linalg.norm(q), float(np.linalg.norm(q))

    rows = []
    ray = np.array([0.0, 0.05, 1.0]) / np.linalg.norm([0.0, 0.05, 1.0])
    for k in range(P):
        c, s = np.cos(yaw[k]), np.sin(yaw[k])
        off = np.array([6.0, rng.uniform(-3, 3), rng.uniform(-1, 2)])
        xyz = pos[k] + np.array([c * off[0] - s * off[1], s * off[0] + c * off[1], off[2]])
        for idx, obs in ((k, range(k, min(P, k + 4))), (SPLIT + k, range(k + 4, min(P, k + 7)) if k % 2 == 0 else ())):
            if len(obs) == 0:
                continue
            calls.append(("add_point_landmark", (idx, xyz + rng.normal(0, 0.02, 3))))
            for j in obs:
                calls.append(("add_range_bearing", (0, j, idx) + bearing(j, xyz + rng.normal(0, 0.005, 3))))
            if idx >= SPLIT and k + 7 <= P:      # (a whole copy: three factors)
                rows.append((k, idx))
        if k % 5 == 0:
            root = xyz + np.array([1.0, 1.0, 0.0])
            for n, j in enumerate(range(k, min(P, k + 3))):
                calls.append(("add_cylinder", (0, j, k, est[j], root + rng.normal(0, 0.005, 3), ray, 0.25, n > 0)))
    return calls, np.array(rows, np.uint64)


def build(s, calls, drop=None):
    """The call list into a fresh SlideGraph; drop: {dropped point key: kept key} renames on the way (the rekeyed rebuild)."""
    drop = drop or {}
    G = s.SlideGraph(s.default_params())
    for name, a in calls:
        if name == "add_point_landmark" and a[0] in drop:
            continue
        if name == "add_range_bearing" and a[2] in drop:
            a = a[:2] + (drop[a[2]],) + a[3:]
        getattr(G, name)(*a)
    return G


def main():
    import torch
    torch.zeros(1, device=torch.device("cuda", 0))      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    calls, rows = plant()

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def fmt(v):
        return f"{np.median(v):9.3f} ({min(v):.3f} - {max(v):.3f})"

    G = build(s, calls)
    assert G.gauss_newton(2) == 0
    st = G.stats()
    print(f"landmark merge, {st['n_pose']} poses, {len(G.tile_profile())} tile columns, {st['n_lm']} landmarks ({len(rows)} split points), "
          f"{st['n_factors']} factors, {len(calls)} add calls; ms, median (min - max) of {REPS} fresh graphs after one warm-up graph")
    del G
    for n in (1, 16, 256):
        pick = rows[np.linspace(0, len(rows) - 1, n).astype(int)]      # spread along the trajectory
        drop = {int(d): int(k) for k, d in pick}
        cols = {k: [] for k in ("call", "host", "upload", "fuse", "kernel", "update", "replay", "gn1")}
        for rep in range(REPS + 1):
            G = build(s, calls)
            assert G.gauss_newton(2) == 0
            t_call, res = wall(lambda: G.merge_landmarks(s.CLS_ELLIPSOID, pick, True))
            assert (res["status"] == 0).all() and (res["moved"] == 3).all()
            parts = G.merge_timing()
            t_upd, rc = wall(G.solve)
            assert rc == 0 and G.incremental_stats()["last_first_column"] == 0
            del G
            t_replay, R = wall(lambda: build(s, calls, drop))
            t_gn, rc = wall(lambda: R.gauss_newton(1))
            assert rc == 0
            del R
            if rep:      # (the first graph warms up)
                for k, v in zip(cols, (t_call, parts["host_ms"], parts["upload_ms"], parts["fuse_ms"], parts["fuse_kernel_ms"], t_upd, t_replay, t_gn)):
                    cols[k].append(v)
        print(f"{n:4d} pairs  merge_landmarks {fmt(cols['call'])}: host restructure {fmt(cols['host'])}, upload {fmt(cols['upload'])}, "
              f"fusion with read-back {fmt(cols['fuse'])}, k_lm_merge_fuse (HIP events) {fmt(cols['kernel'])}", flush=True)
        print(f"            the full update that follows (solve) {fmt(cols['update'])}", flush=True)
        print(f"            alternative: rebuild rekeyed through the binding {fmt(cols['replay'])} + gauss_newton(1) {fmt(cols['gn1'])}", flush=True)


if __name__ == "__main__":
    main()
