"""Timing of the observation loss.  Reported only; there is no target.

Printed in the order (b), (a); every run of (a) is printed as it ends.

(a) Loss off, the parent commit's library against this one: robot 0's 625-frame streaming build of C4shard (ms per frame: associate +
    add + update) and SlideGraph.gauss_newton(1) on the graph it leaves.  One process per run (a process loads one library), the two
    libraries alternating, 21 runs each after 3 warm-up runs, median with min and max.  The parent's library is expected as
    slide_slam_amd/_lib/parent.so (a build of the parent commit's sources, loaded through SLIDE_LIB_VARIANT=parent); without it this part
    prints NOT MEASURED.
(b) This library, loss off against Huber on all classes, alternating in one process: gauss_newton(1) wall time, and the device time of
    the `linearize` stage (the launch the loss is fused into) from get_profile.

    timeout -k 10 1100 python tools/observation_loss_timing.py > profiles/observation_loss_timing.txt
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM, PROF_ITERS = 21, 3, 20


def stream_build(s, cfg, log):
    from slide_slam_amd.replay import IDENT7
    from slide_slam_amd.synth import frame_detections
    import torch
    b = s.SlideBackend(s.default_params(), 1)
    prev = IDENT7.copy()
    dets = [frame_detections(log, k) for k in range(cfg.poses_per_robot)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(cfg.poses_per_robot):
        r = b.process_frame(0, log["rel7"][k], prev, dets[k], 0)
        assert r["status"] == 0
        prev = r["pose7"].copy()
    torch.cuda.synchronize()
    return b, 1e3 * (time.perf_counter() - t0) / cfg.poses_per_robot


def timed_gn(G):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    assert G.gauss_newton(1) == 0
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def setup():
    import torch
    torch.zeros(1, device=torch.device("cuda", 0))      # (torch initialises the device before the library's HIP runtime is loaded)
    import slide_slam_amd as s
    from slide_slam_amd.synth import SynthConfig, make_robot_log, make_world
    cfg = SynthConfig.preset("C4shard")
    return s, cfg, make_robot_log(cfg, make_world(cfg), 0)


def child():
    """One run: the second of two streaming builds (the first loads the kernels), then gauss_newton(1), median of 7 after 2."""
    s, cfg, log = setup()
    stream_build(s, cfg, log)
    b, ms_frame = stream_build(s, cfg, log)
    t = [timed_gn(b.graph) for _ in range(9)][2:]
    print(json.dumps({"ms_per_frame": ms_frame, "gn_ms": float(np.median(t))}), flush=True)


def fmt(v):
    return f"{np.median(v):8.4f} ms ({min(v):.4f} - {max(v):.4f})"


def against_parent():
    print(f"== loss off, the parent commit's library against this one; one process per run, alternating, {REPS} runs each after {WARM} warm-up runs ==")
    if not os.path.exists(os.path.join(ROOT, "slide_slam_amd", "_lib", "parent.so")):
        print("NOT MEASURED: slide_slam_amd/_lib/parent.so (a build of the parent commit) is not there")
        return
    res = {"parent": [], "new": []}
    for rep in range(WARM + REPS):
        for tag in ("parent", "new"):
            env = dict(os.environ)
            env.pop("SLIDE_LIB_VARIANT", None)
            if tag == "parent":
                env["SLIDE_LIB_VARIANT"] = "parent"
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=180)
            if r.returncode != 0:      # (nothing more is started on the device after a run that failed)
                print(f"run {rep} of {tag} ended with status {r.returncode}; stopping\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
                sys.exit(1)
            one = json.loads(r.stdout.strip().splitlines()[-1])
            print(f"run {rep:2d} {tag:6s} ms_per_frame {one['ms_per_frame']:.4f} gn_ms {one['gn_ms']:.4f}" + ("" if rep >= WARM else "  (warm-up)"), flush=True)
            if rep >= WARM:
                res[tag].append(one)
    for key, what in (("ms_per_frame", "streaming build, 625 frames, ms per frame"), ("gn_ms", "gauss_newton(1) on the graph it leaves")):
        print(what)
        for tag in ("parent", "new"):
            print(f"{tag:6s}: {fmt([x[key] for x in res[tag]])}")


def on_against_off():
    s, cfg, log = setup()
    b, _ = stream_build(s, cfg, log)
    G = b.graph
    t = {"off": [], "on": []}
    for rep in range(WARM + REPS):
        for tag in ("off", "on"):
            G.set_observation_loss("huber" if tag == "on" else None)
            timed_gn(G)                                # (the first step after a change of the loss re-captures the pass)
            ms = timed_gn(G)
            if rep >= WARM:
                t[tag].append(ms)
    st = G.stats()
    print("== this library, loss off against Huber (k = 1.345) on all classes, alternating in one process ==")
    print(f"gauss_newton(1), {st['n_pose']} poses, {st['n_factors'] - st['n_pose']} landmark factors, {len(G.tile_profile())} tile columns; ms wall, "
          f"median (min - max) of {REPS} after {WARM} warm-ups")
    for tag in ("off", "on"):
        print(f"loss {tag:3s}: {fmt(t[tag])}")
    G.set_profiling(True)
    for tag in ("off", "on"):
        G.set_observation_loss("huber" if tag == "on" else None)
        assert G.gauss_newton(1) == 0
        p0 = G.get_profile()["linearize"]
        for _ in range(PROF_ITERS):
            assert G.gauss_newton(1) == 0
        p1 = G.get_profile()["linearize"]
        n = p1["launches"] - p0["launches"]
        print(f"linearize, loss {tag:3s}: {1e3 * (p1['ms'] - p0['ms']) / n:.2f} us per launch over {n} launches (HIP events around the launch)")
    w = G.observation_weights()["weight"]
    print(f"weights of the last reweighted step: {int((w == 1.0).sum())} of {len(w)} at 1, {int((w < 0.1).sum())} below 0.1, smallest {w.min():.3e}\n", flush=True)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    elif "--on-off" in sys.argv:
        on_against_off()
    else:                         # (this process never opens the device: one process at a time does)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--on-off"], timeout=400)
        if r.returncode != 0:
            sys.exit(r.returncode)
        against_parent()
