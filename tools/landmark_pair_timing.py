"""Timing of the duplicate-landmark queries on the 625-pose C4shard robot graph tools/observation_gate_timing.py uses:
SlideGraph.landmark_pair_mahalanobis on 42 and on 1000 in-profile point pairs (neighbours proposed by landmark_pairs_within that the
host sends down route 0), the same pairs forced down route 1 (SLIDE_LM_PAIR_SUBSTITUTE=1), get_landmark_pair_covariances on the 42,
the graph's own search, and pairs_within on a 5000-point map.  No number is fixed in advance.  Wall times with the device synchronised
around the timed region: the median (min - max) of 21 repetitions after three warm-ups.  The per-stage device times of route 1 (fill,
walk, gram, finish) need a kernel trace in a run of its own; they are not measured by this tool.

    timeout -k 10 500 python tools/landmark_pair_timing.py > profiles/landmark_pair_timing.txt
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
    P, T, cnt = cfg.poses_per_robot, len(G.tile_profile()), b.counts()
    sigma = np.full(3, 0.05)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def series(f):
        for _ in range(WARM):
            f()
        t = [timed(f) for _ in range(REPS)]
        return f"{np.median(t):8.3f} ms ({min(t):.3f} - {max(t):.3f})", float(np.median(t))

    print(f"landmark pairs, {P} poses, {T} tile columns, {cnt['point']} points, {cnt['cube']} cubes, {cnt['cyl']} cylinders; ms wall, median "
          f"(min - max) of {REPS} after {WARM} warm-ups")
    # neighbours: grow the radius until the search proposes enough pairs that the host serves on route 0
    radius, pairs0 = 1.0, np.zeros((0, 2), np.uint64)
    while len(pairs0) < 1000 and radius < 64.0:
        ia, ib, _ = G.landmark_pairs_within(s.CLS_ELLIPSOID, radius)
        near = np.stack([ia, ib], axis=1)
        res = G.landmark_pair_mahalanobis(s.CLS_ELLIPSOID, near, sigma)
        pairs0 = near[(res["status"] == 0) & (res["route"] == 0)]
        n_near, n_sub = len(near), int(((res["status"] == 0) & (res["route"] == 1)).sum())
        radius *= 1.5
    radius /= 1.5
    print(f"landmark_pairs_within at {radius:.2f} m: {n_near} pairs, {len(pairs0)} served on route 0, {n_sub} on route 1", flush=True)
    ts, _ = series(lambda: G.landmark_pairs_within(s.CLS_ELLIPSOID, radius))
    print(f"the graph's search at that radius ({cnt['point']} points, two calls: count, then emit with room): {ts}", flush=True)
    for n in (42, 1000):
        if len(pairs0) == 0:
            print(f"{n} pairs: no route-0 pair on this graph, not measured")
            continue
        pairs = pairs0[np.arange(n) % len(pairs0)]
        t0, m0 = series(lambda: G.landmark_pair_mahalanobis(s.CLS_ELLIPSOID, pairs, sigma))
        os.environ["SLIDE_LM_PAIR_SUBSTITUTE"] = "1"
        try:
            out = G.landmark_pair_mahalanobis(s.CLS_ELLIPSOID, pairs, sigma)
            assert (out["route"] == 1).all()
            t1, m1 = series(lambda: G.landmark_pair_mahalanobis(s.CLS_ELLIPSOID, pairs, sigma))
        finally:
            del os.environ["SLIDE_LM_PAIR_SUBSTITUTE"]
        print(f"{n} in-profile point pairs ({len(np.unique(pairs, axis=0))} distinct): route 0 {t0}; forced to route 1 ({(n + 127) // 128} sweeps) {t1}; "
              f"route 0 takes {m0 / m1:.4f} of it", flush=True)
        if n == 42:
            tc, _ = series(lambda: G.get_landmark_pair_covariances(s.CLS_ELLIPSOID, pairs))
            print(f"    get_landmark_pair_covariances on the same 42, route 0: {tc}", flush=True)
    rng = np.random.default_rng(0)
    xyz = rng.uniform(0.0, 1.0, (5000, 3)) * np.array([200.0, 200.0, 5.0])
    labels = rng.integers(0, 4, 5000).astype(np.int32)
    n5 = len(s.pairs_within(xyz, 0.75)[0])
    tp, _ = series(lambda: s.pairs_within(xyz, 0.75))
    tl, _ = series(lambda: s.pairs_within(xyz, 0.75, labels))
    print(f"pairs_within on a 5000-point map (200 x 200 x 5 m, radius 0.75 m, {n5} pairs; upload, count, emit, read-back, twice: the wrapper "
          f"counts first): {tp}; with labels {tl}")
    print("per-stage device times of route 1 (fill, walk, gram, finish): not measured (they need a kernel trace in a run of its own)")


if __name__ == "__main__":
    main()
