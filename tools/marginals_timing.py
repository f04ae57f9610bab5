"""Timing of the marginals and the information gain on the 625-pose robot graph of the C4shard world.

    python tools/marginals_timing.py                 # wall times (stream synchronised) + the factorisation's kernel profile
    rocprofv3 --kernel-trace -d DIR -o run -- python tools/marginals_timing.py
    python tools/marginals_timing.py --summarise DIR # device time per kernel of cov_kernels.hip from that trace (rocpd database)
"""
import glob
import os
import re
import sqlite3
import sys
import time
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = r"(k_sinv_prep|k_sinv_tile|k_sub_fwd|k_sub_bwd|k_lm_cov|k_pose_blocks|k_gram|k_lm_V|k_jt_scatter|k_chol_step)"


def summarise(d):
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    agg = defaultdict(lambda: [0, 0.0])
    for name, start, end in c.execute("select name, start, end from kernels"):
        m = re.search(KERNELS, name)
        if m:
            key = m.group(1) + ("<true>" if m.group(1) == "k_sinv_tile" and "ILb1" in name else "")
            agg[key][0] += 1
            agg[key][1] += (end - start) * 1e-6
    for k, (n, ms) in sorted(agg.items()):
        print(f"{k:18s} launches {n:6d}  total {ms:9.3f} ms  mean {1e3 * ms / n:8.2f} us")


def main():
    import numpy as np
    import torch
    torch.zeros(1, device="cuda:0")      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from slide_slam_amd.replay import IDENT7
    from slide_slam_amd.synth import SynthConfig, frame_detections, make_robot_log, make_world
    cfg = SynthConfig.preset("C4shard")
    log = make_robot_log(cfg, make_world(cfg), 0)
    b = s.SlideBackend(s.default_params(), 1)
    G = b.graph
    prev = IDENT7.copy()
    for k in range(cfg.poses_per_robot):
        prev = b.process_frame(0, log["rel7"][k], prev, frame_detections(log, k), 0)["pose7"].copy()
    print("block columns", len(G.tile_profile()))
    G.set_profiling(True)
    G.gauss_newton(1)
    print("factorisation (chol_step) ms:", G.get_profile()["chol_step"])
    G.set_profiling(False)
    P = cfg.poses_per_robot
    for rep in range(3):
        G.gauss_newton(1)
        t0 = time.perf_counter(); G.get_pose_covariances(0, np.arange(P)); t1 = time.perf_counter()
        G.get_pose_covariances(0, np.arange(P)); t2 = time.perf_counter()
        tr = G.marginal_traces(0); t3 = time.perf_counter()
        G.closure_info_gain(0, [600, 10], [20.0]); t4 = time.perf_counter()
        G.closure_info_gain(0, [600, 400, 200, 10], [20.0] * 3); t5 = time.perf_counter()
        G.closure_info_gain(0, list(range(624, -1, -9))[:65], [10.0] * 64); t6 = time.perf_counter()
        print(f"rep {rep}: {P} pose marginals incl. the selected inversion {1e3 * (t1 - t0):.2f} ms, again (cached) {1e3 * (t2 - t1):.2f} ms, "
              f"traces incl. {int(tr[3])} point landmarks {1e3 * (t3 - t2):.2f} ms, gain m=1 {1e3 * (t4 - t3):.2f} ms, "
              f"m=3 {1e3 * (t5 - t4):.2f} ms, m=64 {1e3 * (t6 - t5):.2f} ms")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        main()
