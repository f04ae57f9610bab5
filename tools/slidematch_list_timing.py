"""Timing of inter-robot SlideMatch place recognition over a list of robot pairs: one find_inter_loop_closures call
against a loop of find_inter_loop_closure calls over the same pairs (the path a caller had before), alternating in ONE process on one
GPU.  Wall times: the median of REPS repetitions after WARM warm-ups; the loop is measured a second time at the end, and the
difference of its two medians is the run-to-run spread the comparison is read against.

    timeout -k 10 900 python tools/slidematch_list_timing.py [A B C]

Workloads (forest parameters: ignore_dimension, 5 deg yaw steps, 0.5 m cells):
  A  7 pairs with a shared reference at the golden indoor maps' size (32 objects against 7 views of the 35-object map)
  B  7 pairs of the 792 / 554-object forest pair over its first two rings
  C  28 mixed pairs: all pairs of eight maps (indoor maps and views of them, a 60-object map, the forest pair), two rings
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, WARM = 7, 2


def _view(rng, m, yaw, shift):
    q = m[rng.permutation(len(m))].copy()
    c, s = np.cos(-yaw), np.sin(-yaw)
    xy = q[:, 1:3] - np.array(shift)
    q[:, 1] = c * xy[:, 0] - s * xy[:, 1]
    q[:, 2] = s * xy[:, 0] + c * xy[:, 1]
    q[:, 1:3] += rng.normal(0, 0.03, (len(q), 2))
    return np.ascontiguousarray(q)


def workloads():
    import place_cases as pc
    import slidematch_list_cases as lc
    rng = np.random.default_rng(2024)
    m0, m1 = lc.load_map("robot0Map_indoor.txt"), lc.load_map("robot1Map_indoor.txt")
    forest = pc.full_size_pair(2)
    base = dict(ignore_dimension=1, search_yaw_step_size=float(np.deg2rad(5.0)), search_xy_step_size=0.5)
    out = {}
    views = [m1] + [_view(rng, m1, rng.uniform(-3, 3), rng.uniform(-2, 2, 2)) for _ in range(6)]
    out["A"] = dict(what="7 pairs, shared 32-object reference, 35-object queries", maps=[m0] + views, pairs=[(0, k + 1) for k in range(7)], params=base)
    fq = [forest["qry7"]] + [_view(rng, forest["qry7"], rng.uniform(-0.2, 0.2), rng.uniform(-2, 2, 2)) for _ in range(6)]
    out["B"] = dict(what="7 pairs, 792-object reference, 554-object queries, 2 rings", maps=[forest["ref7"]] + fq, pairs=[(0, k + 1) for k in range(7)],
                    params=dict(base, max_rings=2))
    sixty = lc.mixed_list(1)["maps"][2]
    eight = [m0, m1, _view(rng, m0, 0.7, (1.0, -2.0)), _view(rng, m0, -1.1, (0.5, 1.5)), _view(rng, m1, 2.0, (-1.0, 0.5)), sixty, forest["ref7"], forest["qry7"]]
    out["C"] = dict(what="28 pairs: all pairs of eight maps (32 to 792 objects), 2 rings", maps=eight, pairs=[(i, j) for i in range(8) for j in range(i + 1, 8)],
                    params=dict(base, max_rings=2))
    return out


def main(names):
    import torch
    torch.zeros(1, device=torch.device("cuda", 0))      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    print(f"SlideMatch over a list of pairs: one list call against a loop of single calls, median of {REPS} after {WARM} warm-ups, ms wall")
    for name, w in workloads().items():
        if names and name not in names:
            continue
        gp = s.place_default_params(**w["params"])
        maps, pairs = w["maps"], w["pairs"]
        loop = lambda: [s.find_inter_loop_closure(maps[a], maps[b], gp) for a, b in pairs]        # noqa: E731
        lst = lambda: s.find_inter_loop_closures(maps, pairs, gp)                                  # noqa: E731

        def timed(f):
            t0 = time.perf_counter()
            f()
            return 1e3 * (time.perf_counter() - t0)
        for _ in range(WARM):
            one, many = loop(), lst()
        for o, m in zip(one, many):                      # the same answers before any time is taken
            assert o["found"] == m["found"] and o["inliers"] == m["inliers"] and (not o["found"] or np.array_equal(o["tf"], m["tf"]))
        t_loop, t_list = [], []
        for _ in range(REPS):
            t_loop.append(timed(loop))
            t_list.append(timed(lst))
        t_loop2 = [timed(loop) for _ in range(REPS)]
        ml, mb, ml2 = np.median(t_loop), np.median(t_list), np.median(t_loop2)
        spread = abs(ml - ml2)
        n = len(pairs)
        cand = sum(m["candidates"] for m in many)
        verdict = "faster than the loop by more than the spread" if ml - mb > spread else ("slower than the loop by more than the spread" if mb - ml > spread else "within the spread of the loop")
        print(f"({name}) {w['what']}: {cand} candidates, found {sum(m['found'] for m in many)} of {n}")
        print(f"    loop of single calls {ml:9.3f} ms ({min(t_loop):.3f} - {max(t_loop):.3f}); measured again {ml2:9.3f} ms: spread {spread:.3f} ms")
        print(f"    one list call        {mb:9.3f} ms ({min(t_list):.3f} - {max(t_list):.3f}); ratio {ml / mb:5.2f}: {verdict}")
        print(f"    per call, by construction: loop {2 * n} launches, {2 * n} blocking read-backs, {15 * n} device allocations and uploads; "
              f"list 2 launches, 1 read-back, 1 allocation, 1 upload", flush=True)


if __name__ == "__main__":
    main([a for a in sys.argv[1:] if not a.startswith("--")])
