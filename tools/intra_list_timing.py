"""Timing of one attempt of the same-robot loop-closure thread over a list of candidate key poses: one
intra_loop_closure_attempt call (submap extraction on the device + the list sweep) against the path a caller had before — per
candidate a numpy getkeyPoseSubmap + prepareLCInput (tests/intra_list_cases.py) and one find_intra_loop_closure call — alternating in
ONE process on one GPU.  Wall times with the device synchronised around the timed region: the median of REPS repetitions after WARM
warm-ups; the loop is measured a second time at the end, and the difference of its two medians is the run-to-run spread the
comparison is read against.

    timeout -k 10 900 python tools/intra_list_timing.py [1 8 64]

Workload: a 10 000-object map (half cylinders, a quarter cubes, a quarter ellipsoids) over 300 m x 300 m, 20 detections, radius 20 m,
the default intra window (4840 lattice poses per candidate); the candidates are the first 1, 8 and 64 entries of loop_candidate_list
around the last key pose."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, WARM = 21, 3


def main(counts):
    import torch
    torch.zeros(1, device=torch.device("cuda", 0))      # (torch initialises the device before the library's HIP runtime is loaded)
    import intra_list_cases as ic
    import slide_slam_amd as s
    case = ic.attempt_case(n_objects=10000, seed=2025, extent=150.0, n_pose=400, turns=2.05)
    tabs = ic.tables_args(case["tables"])
    gp = s.place_default_params(**case["params"])
    idx, n_all = s.loop_candidate_list(case["cloud"], 30.0, len(case["cloud"]) - 1, 30)
    assert n_all >= max(counts), (n_all, counts)
    print(f"intra loop closure over a list of candidates: one attempt call against a loop of numpy extraction + single call, "
          f"median of {REPS} after {WARM} warm-ups, ms wall; 10000-object map, 20 detections, radius 20 m, {n_all} candidates in range")

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    for n in counts:
        poses = ic.key_pose7(case["cloud"], idx[:n])

        def loop():
            out = []
            for k in range(n):
                sub = ic.submaps_reference(case["tables"], poses[k:k + 1, :3], case["radius"], case["max_dz"])["rows"]
                out.append(s.find_intra_loop_closure(case["meas"], sub, case["query_pose"], poses[k], gp))
            return out

        def attempt():
            return s.intra_loop_closure_attempt(*tabs, case["meas"], case["query_pose"], poses, case["radius"], gp, max_dz=case["max_dz"])

        def extract_only():
            return s.keypose_submaps(*tabs, poses[:, :3], case["radius"], case["max_dz"], capacity=10000 * n, with_src=False)
        for _ in range(WARM):
            one, many = loop(), attempt()
        for o, m in zip(one, many):                      # the same answers before any time is taken
            assert o["found"] == m["found"] and o["inliers"] == m["inliers"] and (not o["found"] or np.array_equal(o["tf"], m["tf"]))
        t_loop, t_list = [], []
        for _ in range(REPS):
            t_loop.append(timed(loop))
            t_list.append(timed(attempt))
        t_loop2 = [timed(loop) for _ in range(REPS)]
        t_ext = [timed(extract_only) for _ in range(REPS)]
        ml, mb, ml2, me = np.median(t_loop), np.median(t_list), np.median(t_loop2), np.median(t_ext)
        spread = abs(ml - ml2)
        verdict = "faster than the loop by more than the spread" if ml - mb > spread else ("slower than the loop by more than the spread" if mb - ml > spread else "within the spread of the loop")
        sizes = [m["submap_size"] for m in many]
        print(f"({n} candidates) submaps of {min(sizes)} to {max(sizes)} objects, found {sum(m['found'] for m in many)} of {n}")
        print(f"    loop: numpy extraction + single call {ml:9.3f} ms ({min(t_loop):.3f} - {max(t_loop):.3f}); measured again {ml2:9.3f} ms: spread {spread:.3f} ms")
        print(f"    one attempt call                     {mb:9.3f} ms ({min(t_list):.3f} - {max(t_list):.3f}); ratio {ml / mb:5.2f}: {verdict}")
        print(f"    of which keypose_submaps alone       {me:9.3f} ms ({min(t_ext):.3f} - {max(t_ext):.3f})")
        print(f"    per call, by construction: loop {2 * n} launches, {2 * n} blocking read-backs, {15 * n} device allocations and uploads; "
              f"attempt 5 launches, 3 blocking read-backs, the map tables uploaded once", flush=True)


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    main(args or [1, 8, 64])
