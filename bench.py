#!/usr/bin/env python3
"""bench.py — pose-graph updates/s + ms per Gauss-Newton iteration of the SlideSLAM backend hot path on MI355X.

A *step* is one pass of the hot path over the resident graph: relinearise every factor, assemble the
landmark-eliminated (Schur) pose system, factor + solve it (FP64-MFMA Cholesky), back-substitute the
landmarks and retract — i.e. one Gauss-Newton iteration = one pose-graph update
(reference: SemanticFactorGraph::solve, backend/sloam/src/factorgraph/graph.cpp:260-272).

Workload (BASELINE.json configs[3]): the 8-robot / 10 k-landmark / 5 k-pose synthetic graph, one sub-graph per robot (625 poses,
~1250 landmarks, ~12.5 k landmark factors each), 8 / N robots per GPU — the SAME graph at N = 1, 2, 4, 8 (strong scaling).
All robots of a GPU sit in one CholBatch and ONE host thread drives the pass: at N = 1 the whole pass of all eight robots is one
replayed hipGraph; at N > 1 it is three replayed parts with the two shared-landmark all-reduces (RCCL over xGMI) issued on the
same HIP stream between them — one host synchronisation per pass.  value = robot pose-graph updates/s = 8 * steps / time.
`--robots-per-gpu 1` is the weak-scaling variant (one robot per GPU at every N).  Inputs are resident in HBM before the timed
region.  Synthetic, seeded data (slide_slam_amd/synth.py).

A pass takes the EXACT joint Gauss-Newton step of all robots (default, --joint exact): the shared landmarks stay as the separator of
the joint graph, every robot factors its banded pose system with the separator's coupling rows as a border, one FP64-MFMA product per
robot forms its Schur complement onto the separator, the summed separator system (ONE all-reduce per pass at N > 1) is factored and
substituted back — the step the reference's full replica takes with one solve(), no inner iteration.

A plain run sets the job up, takes the first passes one by one (the convergence probe, --probe; not timed), warms up, times the steps
and prints the JSON line's headline part.  With --full the bench also (a) reports how many passes / ms the job needs to come within
1e-4 (relative, on poses) of where it ends, from the probe's poses (`convergence`; exit code 1 when it does not), (b) times the stages
of the pass with HIP events on the pass's stream (`roofline`: the border product against the FP64-MFMA peak, the factorisations'
serial chains), (c) times the association sweep (`roofline.assoc`, HBM) and the SlideMatch / SlideGraph / CLIPPER legs, (d) runs the
job once more with SURVEY 8d's relative-pose density (`dense_relmeas`) and (e) in the cpu_baseline leg runs the SAME exact joint passes
on oracle shards on the host's cores — timed as the CPU figure, compared pose by pose with identically built GPU shards (`parity`).
The options that shape or skip those legs (--no-cpu, --no-place-leg, --no-dense-leg, --no-dense-relmeas, --assoc-report) act with
--full only; --no-parity leaves out the probe in either mode.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--robots-per-gpu R] [--no-cpu] [--frames F] [--ingest-only] [--no-parity]
       [--dump-outputs DIR]  (the poses and landmark estimates the last timed step left, DIR/<name>.npy, for comparing two builds)
       [--full]  (everything besides the headline, above; a minute and more)
Multi-GPU: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6   # MI355X FP64 matrix peak, public spec (MI355X_MICROARCH.md lists no f64 row)
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E ~8 TB/s


CHART = 0                      # --chart: 0 = SLIDE_CHART_CAYLEY (the default, what cubeFactor.h:96-97 names), 1 = SLIDE_CHART_EXPMAP; product and oracle alike
DENSE_LEG = True               # roofline.dense_profile: the same kernels on the same graphs with the structure ignored
DENSE_PROFILE = False          # --dense-profile: every graph of the run ignores the structure of its reduced system (profiling aid)


def build_shard(s, log, frames=None, ingest_only=False):
    """Stream one robot's frame log through the per-frame path (association + add + iSAM2-equivalent update).
    ingest_only (profiling aid): add every frame without solving (association against the un-refined map at the ground-truth
    poses, as the cpu_baseline leg does), then one solve — every k_chol_step launch of the run is then full-size."""
    from slide_slam_amd.replay import replay_single
    gb = s.SlideBackend(s.default_params(pose_chart=CHART), 1)
    if DENSE_PROFILE:
        gb.graph.set_dense_profile(True)
    if not ingest_only:
        out = replay_single(gb, log, n_frames=frames, collect=False)
        return gb, out
    from slide_slam_amd.synth import frame_detections
    P = len(log["rel7"]) if frames is None else frames
    t_frame = []
    for k in range(P):
        t0 = time.perf_counter()
        gb.process_frame(0, log["rel7"][k], log["gt7"][k], frame_detections(log, k), s.FRAME_FOREIGN)
        t_frame.append(time.perf_counter() - t0)
    if gb.ingest_solve() != 0:
        raise RuntimeError("ingest solve failed")
    return gb, dict(t_frame=t_frame)


def all_poses(gb, P):
    return np.array([gb.graph.get_pose12(0, k)[1] for k in range(P)])


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, shards, final, dist=None, world=1, rank=0):
    """--dump-outputs: what the timed passes left in the graphs — every robot's poses (robot, pose, 12: rotation row-major, then
    translation) and every robot's landmark estimates by class (rows of all robots in robot order) — as float64 .npy files, so that
    two builds run with the same arguments can be compared array for array.  Above DUMP_LIMIT_BYTES in all, a fixed seeded sample of
    rows is written instead (the row indices beside it).  Collective at world > 1: every rank passes its robots, rank 0 writes."""
    mine = {"poses": final}
    for cls, name in enumerate(("cyl", "cube", "point")):
        rows = [gb.graph.get_landmark(cls, i)[1] for gb in shards for i in range(gb.counts()[name])]
        mine[f"landmarks_{name}"] = np.array(rows, dtype=np.float64).reshape(len(rows), (7, 15, 3)[cls])
    parts = [mine]
    if dist is not None and world > 1:
        parts = [None] * world
        dist.all_gather_object(parts, mine)
    if rank != 0:
        return
    out = {k: np.concatenate([np.asarray(p[k], dtype=np.float64) for p in parts], axis=0) for k in mine}
    if sum(a.nbytes for a in out.values()) > DUMP_LIMIT_BYTES:
        rng = np.random.default_rng(0)
        rows = {k: a.reshape(-1, a.shape[-1]) for k, a in out.items()}
        frac = (DUMP_LIMIT_BYTES - 65536) / sum(a.nbytes + 8 * len(a) for a in rows.values())     # (the row indices count too)
        for k, a in rows.items():
            keep = np.sort(rng.choice(len(a), max(1, int(len(a) * frac)), replace=False))
            out[k], out[k + "_rows"] = a[keep], keep.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, a in out.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    sys.stderr.write(f"bench.py: outputs of the last timed step written to {out_dir}: " +
                     ", ".join(f"{k}{list(a.shape)}" for k, a in out.items()) + "\n")


def _oracle_shard(L, po, log, frames, threads):
    from slide_slam_amd.synth import frame_detections
    ob = po.OracleBackend(po.OrcParams.default(num_threads=threads, pose_chart=CHART), 1, L=L)
    P = len(log["rel7"]) if frames is None else frames
    for k in range(P):
        ob.process_frame(0, log["rel7"][k], log["gt7"][k], frame_detections(log, k), 2)
    ob.graph.set_relin_threshold(0.0)
    return ob


def _time_iters(ob, budget_s, cap=200):
    times, t_start = [], time.perf_counter()
    while len(times) < 2 or (time.perf_counter() - t_start < budget_s and len(times) < cap):
        t0 = time.perf_counter()
        if ob.ingest_solve() != 0:
            raise RuntimeError("oracle solve failed")
        times.append(time.perf_counter() - t0)
    return times


def cpu_baselines(logs, frames, budget_s=10.0):
    """The oracle (CPU restatement of the reference, C++ -O3 -march=native; NOT GTSAM) timed on the same graph on this box's
    host cores.  Every shard ingests its frames without solving (association against the un-refined map), then full
    linearise + Schur + Cholesky + back-substitution passes (threshold 0) are timed; the Cholesky works inside the profile of
    the assembled matrix (oracle/graph.hpp chol_profile), as a sparse direct solver would.  Three variants:
      robots_as_threads  the job's robots as independent host threads, one core each ("one sloam_node per robot on one PC",
                         README.md:238 of the reference) — the whole-job figure that stands beside `value`;
      single_thread      one robot's shard on one core (the reference's runSLOAMNode is single-threaded);
      omp                one robot's shard with OpenMP over all cores (the best this restatement can do for one robot)."""
    from oracle import pyoracle as po
    L = po.lib(native=True)
    ncpu = os.cpu_count() or 1
    out = {}
    ob = _oracle_shard(L, po, logs[0], frames, 1)
    times = _time_iters(ob, budget_s)
    st = ob.graph.stats()
    desc = f"{st['n_pose']}-pose / {st['n_lm']}-landmark / {st['n_factors']}-factor robot sub-graph"
    it1 = float(np.median(times))
    out["single_thread"] = dict(value=1.0 / it1, unit="pose-graph updates/s", cores=1, kind="port", ms_per_iter=it1 * 1e3,
                                sample=f"{len(times)} full Gauss-Newton iterations (about {budget_s:.0f} s) of one {desc}, median",
                                t_linearize_s=st["t_linearize"], t_schur_s=st["t_schur"], t_chol_s=st["t_chol"])
    del ob
    thr = min(ncpu, 16)
    ob = _oracle_shard(L, po, logs[0], frames, thr)
    times = _time_iters(ob, 0.5 * budget_s)
    itn = float(np.median(times))
    out["omp"] = dict(value=1.0 / itn, unit="pose-graph updates/s", cores=thr, kind="port", ms_per_iter=itn * 1e3,
                      sample=f"{len(times)} full Gauss-Newton iterations of one {desc}, {thr} OpenMP threads, median")
    del ob
    # the robots as independent threads, one core each (ctypes releases the GIL inside the oracle)
    R = min(len(logs), ncpu)
    shards = [_oracle_shard(L, po, logs[r], frames, 1) for r in range(R)]
    iters = min(max(2, int(budget_s / max(it1, 1e-3))), 400)
    err = []

    def work(ob):
        try:
            for _ in range(iters):
                if ob.ingest_solve() != 0:
                    raise RuntimeError("oracle solve failed")
        except BaseException as e:      # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(ob,), daemon=True) for ob in shards]
    t0 = time.perf_counter()
    for x in th:
        x.start()
    for x in th:
        x.join()
    wall = time.perf_counter() - t0
    if err:
        raise err[0]
    out["robots_as_threads"] = dict(value=R * iters / wall, unit="pose-graph updates/s", cores=R, kind="port",
                                    ms_per_iter=wall / iters * 1e3,
                                    sample=f"{R} robot sub-graphs ({desc} each) as {R} host threads with one core each, {iters} full "
                                           f"Gauss-Newton iterations per robot ({wall:.1f} s)")
    return out


def cpu_exact_joint_leg(s, logs, frames, passes=3, relmeas=None):
    """cpu_baseline leg of the exact joint step: the job's robots as oracle shards (CPU restatement, C++ -O3 -march=native, NOT GTSAM)
    on this box's host cores, built like bench.py --ingest-only builds the GPU shards (every frame at its ground-truth pose, association
    against the un-refined map, one solve), merged across robots, then `passes` exact joint Gauss-Newton passes — linearise, eliminate
    private landmarks and poses per robot (OpenMP over all cores inside a shard, one shard after the other), sum, factor and solve the
    separator system, substitute back: the SAME algorithm and work as a GPU pass — timed.  By-product (the oracle as checker): identically
    built GPU shards take the same passes and every pass's poses are compared."""
    import torch
    from oracle import pyoracle as po
    from slide_slam_amd.distributed import PassDriver, gpu_matcher, setup_local_shards
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_worker import oracle_matcher
    from slide_slam_amd.synth import frame_detections
    L = po.lib(native=True)
    ncpu = min(os.cpu_count() or 1, 16)
    R = len(logs)
    P = len(logs[0]["rel7"]) if frames is None else frames
    O, A = [], []
    for lg in logs:
        o = po.OracleBackend(po.OrcParams.default(num_threads=ncpu, pose_chart=CHART), 1, L=L)
        a = s.SlideBackend(s.default_params(pose_chart=CHART), 1)
        for k in range(P):
            o.process_frame(0, lg["rel7"][k], lg["gt7"][k], frame_detections(lg, k), 2)
            a.process_frame(0, lg["rel7"][k], lg["gt7"][k], frame_detections(lg, k), s.FRAME_FOREIGN)
        assert o.ingest_solve() == 0 and a.ingest_solve() == 0
        O.append(o); A.append(a)
    dev = torch.device("cuda", torch.cuda.current_device())
    batch = s.CholBatch(R)
    for t, a in enumerate(A):
        a.graph.join_chol_batch(batch, t)
    bufA, infoA = setup_local_shards(A, gpu_matcher, device=dev)
    bufO, infoO = setup_local_shards(O, oracle_matcher)
    dA = PassDriver(A, bufA, infoA["n_slots"], batch=batch, device=dev, arrow=True, sep_dim=infoA["sep_dim"], sep_prof=infoA.get("sep_prof"))
    dO = PassDriver(O, bufO, infoO["n_slots"], arrow=True, sep_dim=infoO["sep_dim"], sep_prof=infoO.get("sep_prof"))
    if relmeas:
        dA.setup_ghosts(relmeas)
        dO.setup_ghosts(relmeas)
    poses = lambda sh: np.array([[x.graph.get_pose12(0, k)[1] for k in range(P)] for x in sh])      # noqa: E731
    t_cpu, rel = [], []
    for _ in range(passes):
        dA.one_pass()
        t0 = time.perf_counter()
        dO.one_pass()
        t_cpu.append(time.perf_counter() - t0)
        a, o = poses(A), poses(O)
        rel.append(float((np.linalg.norm((a - o).reshape(R, -1), axis=1) / np.linalg.norm(o.reshape(R, -1), axis=1)).max()))
    for a in A:
        a.graph.join_chol_batch(None)
    tp = float(np.median(t_cpu))
    st = O[0].graph.stats()
    cb = dict(value=R / tp, unit="pose-graph updates/s", cores=ncpu, kind="port", ms_per_iter=tp * 1e3,
              sample=f"{passes} exact joint Gauss-Newton passes of the {R} robot sub-graphs ({st['n_pose']} poses / {st['n_lm']} landmarks / "
                     f"{st['n_factors']} factors in robot 0's; separator {infoO['sep_dim']} coordinates over {infoO['n_slots']} shared slots), "
                     f"{sum(t_cpu):.1f} s, median; OpenMP with {ncpu} threads inside a shard, shards one after the other",
              note="CPU restatement (oracle/), not GTSAM: the reference cannot be built here (DESIGN 2); same algorithm and work as a GPU pass")
    ok = bool(infoA["n_slots"] == infoO["n_slots"] and infoA["sep_dim"] == infoO["sep_dim"] and all(np.isfinite(rel)) and max(rel) < 1e-6)
    par = dict(gpu_vs_oracle_max_rel=max(rel), per_pass=rel, passes_compared=passes, slots_equal=infoA["n_slots"] == infoO["n_slots"], ok=ok,
               what="poses of every robot after each exact joint pass: GPU shards (one CholBatch, replayed hipGraph) vs oracle shards taking "
                    "the same passes, identically built (ingest-only) — relative, per robot, the worst; tolerance 1e-6 (north-star bar 1e-4)")
    return cb, par


def assoc_roofline(s, n_map=10000, K=1000, n_obs=20, n_query=8192, repeats=5):
    """Association sweep (getSubmap K-NN gate + matchEllipsoidModels) at the headline sizes, batched over query frames against one
    resident map: algorithmic bytes per frame = 12 N_map + 28 K_eff + 36 N_obs over the device time per frame
    (HIP events on the launch stream around `repeats` launches on resident inputs)."""
    from slide_slam_amd.synth import assoc_sweep_case
    # the generator of tests/test_gpu_kernels.py::test_assoc_sweep_batch_matches_oracle (time the tested data): every
    # frame detects the n_obs landmarks nearest to the robot
    cloud, model, label, qpos, obs, olab = assoc_sweep_case(2024, n_map, n_obs, n_query)
    out, ms = s.assoc_sweep_batch(cloud, model, label, qpos, obs, olab, K, 0.75, repeats=repeats)
    k_eff = min(K, n_map)
    bytes_per_frame = 12 * n_map + 28 * k_eff + 36 * n_obs
    per_launch_s = ms * 1e-3 / repeats
    ach = bytes_per_frame * n_query / per_launch_s / 1e9
    return {"bound": "hbm", "kernel": "k_assoc_sweep_r (float32 K-NN scan with a thread's twenty distance words kept in registers, K-select by one histogram over bins linear in the squared distance + ranks inside the K-th key's bin, label-gated nearest neighbour: survivors grouped by label, float screening, the exact double-precision rule on the one or two candidates inside the error bound; 38 KB of LDS, three 512-thread workgroups per CU; SLIDE_ASSOC_REG=0: round 4's k_assoc_sweep_512)",
            "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
            "bytes_per_frame": bytes_per_frame, "frames_per_launch": n_query, "avg_launch_ms": per_launch_s * 1e3,
            "frames_per_s": n_query / per_launch_s, "matched_fraction": float((out >= 0).mean()),
            "traffic": _pmc_traffic("k_assoc_sweep_r") or _pmc_traffic("k_assoc_sweep_512") or _pmc_traffic("k_assoc_sweep"),
            "hbm_side_GBs": (((_pmc_traffic("k_assoc_sweep_r") or _pmc_traffic("k_assoc_sweep_512") or _pmc_traffic("k_assoc_sweep")) or 0.0) / per_launch_s / 1e9) or None,
            "config": {"n_map": n_map, "K": K, "n_obs": n_obs, "n_query": n_query},
            "note": "algorithmic bytes: every frame is charged the whole float32 cloud although the 120 KB map stays in L2 / "
                    "Infinity Cache across the frames of a launch (SURVEY.md 8d caveat); traffic = HBM-side bytes per launch (PMC), hbm_side_GBs = "
                    "that over the launch time: the leg is bound by the in-CU select / match arithmetic, not by DRAM"}


FP64_VALU_PEAK_TFLOPS = 78.6   # MI355X FP64 vector peak, public spec (equal to the matrix figure on this part)


def _oplace(gp):
    """The oracle's parameter struct (oracle/place.hpp) filled from the product's."""
    import ctypes as C

    class OPlace(C.Structure):
        _fields_ = [("dilation_factor", C.c_double), ("xy_step", C.c_double), ("yaw_half_range", C.c_double), ("yaw_step", C.c_double),
                    ("match_threshold", C.c_double), ("match_threshold_dimension", C.c_double), ("disable_yaw_search", C.c_int),
                    ("ignore_dimension", C.c_int), ("min_num_inliers", C.c_int), ("use_lsq", C.c_int),
                    ("min_num_map_objects_to_start", C.c_int), ("max_rings", C.c_int)]
    return OPlace(gp.dilation_factor, gp.search_xy_step_size, gp.match_yaw_half_range, gp.search_yaw_step_size, gp.match_threshold_position,
                  gp.match_threshold_dimension, gp.disable_yaw_search, gp.ignore_dimension, gp.min_num_inliers,
                  gp.use_nonlinear_least_squares, gp.min_num_map_objects_to_start, gp.max_rings)


def place_roofline(s, with_cpu=True):
    """SlideMatch (PlaceRecognition::MatchMaps, place_recognition.cpp:98-387; SURVEY 8d: pair-tests/s, bound FP64 vector ALU / LDS) on
    (a) the reference's own indoor maps (clipper_semantic_object/examples/data/robot{0,1}Map_indoor.txt, the fixture of
    tests/test_gpu_place.py) and (b) a synthetic pair of 792 / 554 objects at the forest parameters (0.5 m, 5 deg, half range ~130 m;
    the first `rings` rings of the anytime loop).  Kernel time: HIP events around k_place_sweep + k_place_argmax (slide_last_device_ms)."""
    import ctypes as C
    from slide_slam_amd import api
    golden = os.path.join(ROOT, "tests", "golden")

    def load(name):
        a = np.loadtxt(os.path.join(golden, name))
        out = np.zeros((a.shape[0], 7))
        out[:, :4] = a[:, :4]
        return out
    cases = {}
    ref, qry = load("robot0Map_indoor.txt"), load("robot1Map_indoor.txt")
    for m in (ref, qry):
        m[:, 1:3] -= m[:, 1:3].mean(axis=0)
    cases["reference_indoor_maps"] = (ref, qry, dict(ignore_dimension=1, search_yaw_step_size=np.deg2rad(5.0), search_xy_step_size=0.5), 1)
    rng = np.random.default_rng(792)
    n = 792
    big = np.zeros((n, 7))
    big[:, 0] = rng.integers(1, 4, n)
    big[:, 1:3] = rng.uniform(-105.0, 105.0, (n, 2))
    big[:, 3] = rng.normal(0, 0.3, n)
    big[:, 4:7] = rng.uniform(0.3, 2.0, (n, 3))
    keep = rng.permutation(n)[: int(0.7 * n)]
    q = big[keep].copy()
    yaw, shift = 0.6, np.array([7.5, -4.0])
    c, sn = np.cos(-yaw), np.sin(-yaw)
    xy = q[:, 1:3] - shift
    q[:, 1] = c * xy[:, 0] - sn * xy[:, 1]
    q[:, 2] = sn * xy[:, 0] + c * xy[:, 1]
    q[:, 1:3] += rng.normal(0, 0.05, q[:, 1:3].shape)
    for m in (big, q):
        m[:, 1:3] -= m[:, 1:3].mean(axis=0)
    cases["synthetic_forest_792"] = (big, q, dict(ignore_dimension=1, search_yaw_step_size=np.deg2rad(5.0), search_xy_step_size=0.5, max_rings=6), 1)
    out = {"bound": "fp64_valu", "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s", "flop_per_pair_test": 10,
           "kernel": "k_place_sweep_b (wavefront per (x, y, yaw) candidate, lanes = query objects, both maps in LDS BUCKETED BY LABEL, the distance "
                     "test without the square root (v < v_crit), four reference objects per round) + k_place_argmax",
           "note": "pair tests = candidates x query objects x reference objects = the iterations of the reference's loops (place_recognition.cpp:281-357), "
                   "priced at SURVEY 8d's ~10 flops each against the FP64 vector peak (public spec, 78.6 TFLOP/s): `frac`.  The kernel gets the same "
                   "inlier counts from fewer operations — the label test is a bucket table, so only `distance_tests` (about a third at three labels) "
                   "reach the vector ALU, at 5 flops + a compare each: `frac_executed` prices those.  The maps are LDS-resident, HBM traffic is negligible.  "
                   "Round 4's kernel (SLIDE_PLACE_PLAIN=1): 0.96 s for the 792-object case, this one 0.066 s, identical results"}
    for name, (r7, q7, kw, _) in cases.items():
        gp = s.place_default_params(**kw)
        g = s.match_maps(r7, q7, gp)            # warm
        g = s.match_maps(r7, q7, gp)
        ms = api.last_device_ms(api.MS_PLACE_SWEEP)
        tests = api.last_device_ms(api.MS_PLACE_PAIR_TESTS)
        dist = api.last_device_ms(api.MS_PLACE_DIST_TESTS)
        d = {"n_ref": int(len(r7)), "n_query": int(len(q7)), "candidates": int(g["candidates"]), "inliers": int(g["inliers"]),
             "kernel_ms": ms, "pair_tests": tests, "pair_tests_per_s": tests / (ms * 1e-3), "achieved": tests * 10 / (ms * 1e-3) / 1e12,
             "distance_tests": dist, "distance_tests_per_s": dist / (ms * 1e-3), "achieved_executed": dist * 6 / (ms * 1e-3) / 1e12}
        d["frac"] = d["achieved"] / FP64_VALU_PEAK_TFLOPS
        d["frac_executed"] = d["achieved_executed"] / FP64_VALU_PEAK_TFLOPS
        if with_cpu:
            from oracle import pyoracle as po
            kw2 = dict(kw)
            kw2["max_rings"] = 1                # a bounded sample of the same sweep: its first ring
            gp1 = s.place_default_params(**kw2)
            g1 = s.match_maps(r7, q7, gp1)
            op = _oplace(gp1)
            best = np.zeros(3)
            pr, pq = np.full(len(q7), -1, np.int32), np.full(len(q7), -1, np.int32)
            r7c, q7c = np.ascontiguousarray(r7), np.ascontiguousarray(q7)
            t0 = time.perf_counter()
            inl = po.lib().orc_match_maps(r7c.ctypes.data_as(C.c_void_p), C.c_int(len(r7c)), q7c.ctypes.data_as(C.c_void_p), C.c_int(len(q7c)),
                                          C.byref(op), best.ctypes.data_as(C.c_void_p), pr.ctypes.data_as(C.c_void_p), pq.ctypes.data_as(C.c_void_p))
            dt = time.perf_counter() - t0
            t1 = float(g1["candidates"]) * len(q7) * len(r7)
            d["cpu_baseline"] = {"kind": "port", "cores": 1, "sample": "the first ring of the same sweep (max_rings = 1)", "seconds": dt,
                                 "pair_tests_per_s": t1 / dt, "same_result_as_gpu": bool(inl == g1["inliers"] and np.array_equal(best, g1["xyyaw"]))}
        out[name] = d
    big_case = out["synthetic_forest_792"]
    out.update({"achieved": big_case["achieved"], "frac": big_case["frac"], "traffic": None})
    return out


def slidegraph_roofline(s, with_cpu=True, m_clipper=4096):
    """SlideGraph's kernels: triangle matching (semantic_clipper.cpp:49-118: 24 B read per triangle pair), CLIPPER's affinity
    (clipper.cpp:21-65: m (m - 1) / 2 evaluations) and the projected-gradient solve (clipper.cpp:172-323: nnz * 12 B per product) — kernel
    times from slide_last_device_ms (HIP events around the launches; the upload of the dense affinity matrix is outside them)."""
    import ctypes as C
    from scipy.spatial import Delaunay
    from slide_slam_amd import api
    res = {}
    ocp = None
    if with_cpu:
        from oracle import pyoracle as po

        class OCP(C.Structure):
            _fields_ = [("tol_u", C.c_double), ("tol_F", C.c_double), ("maxiniters", C.c_int), ("maxoliters", C.c_int), ("beta", C.c_double),
                        ("maxlsiters", C.c_int), ("eps", C.c_double), ("affinityeps", C.c_double), ("rescale_u0", C.c_int), ("sigma", C.c_double),
                        ("epsilon", C.c_double), ("mindist", C.c_double)]
        ocp = OCP()
        po.lib().orc_clipper_default_params(C.byref(ocp))
        ocp.sigma, ocp.epsilon = 0.1, 0.3
    # -- triangles: two Delaunay triangulations of 792-point maps (~1570 triangles each, 2.5 M pairs)
    rng = np.random.default_rng(14)
    ref = rng.uniform(-105, 105, (792, 2))
    qry = ref[rng.permutation(792)[:700]] + rng.normal(0, 0.01, (700, 2))
    tm = ref[Delaunay(ref, qhull_options="Qt Qbb Qc Qz Q12").simplices].astype(np.float64)
    td = qry[Delaunay(qry, qhull_options="Qt Qbb Qc Qz Q12").simplices].astype(np.float64)
    s.match_triangles(tm, td, 0.1)
    pts, diffs = s.match_triangles(tm, td, 0.1)
    ms = api.last_device_ms(api.MS_TRI_MATCH)
    pairs = api.last_device_ms(api.MS_TRI_PAIRS)
    tri = {"bound": "hbm", "kernel": "k_tri_prepare x 2 + k_tri_match (count pass, emit pass)", "model_triangles": int(len(tm)), "data_triangles": int(len(td)),
           "matched_pairs": int(len(diffs)), "kernel_ms": ms, "triangle_pairs": pairs, "pairs_per_s": pairs / (ms * 1e-3),
           "achieved": 2 * pairs * 24 / (ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "traffic": None,
           "note": "algorithmic bytes: 24 B (a sorted distance triple) per triangle pair and pass, two passes (count, emit); the triples of both maps "
                   "(75 KB) are L2-resident: the bound in practice is the compare / ballot work per pair, not DRAM"}
    tri["frac"] = tri["achieved"] / HBM_PEAK_GBS
    if with_cpu:
        from oracle import pyoracle as po
        sub = tm[:200]
        tmf, tdf = np.ascontiguousarray(sub.reshape(-1, 6)), np.ascontiguousarray(td.reshape(-1, 6))
        cap = len(sub) * len(td)
        op_, od_ = np.zeros((cap, 3, 4)), np.zeros(cap)
        t0 = time.perf_counter()
        po.lib().orc_match_triangles(tmf.ctypes.data_as(C.c_void_p), C.c_int(len(sub)), tdf.ctypes.data_as(C.c_void_p), C.c_int(len(td)),
                                     C.c_double(0.1), op_.ctypes.data_as(C.c_void_p), od_.ctypes.data_as(C.c_void_p), C.c_int(cap))
        dt = time.perf_counter() - t0
        tri["cpu_baseline"] = {"kind": "port", "cores": 1, "sample": "the first 200 model triangles against all data triangles", "seconds": dt,
                               "pairs_per_s": len(sub) * len(td) / dt}
    res["triangles"] = tri
    # -- affinity: m putative associations between two point sets (scorePairwiseConsistency)
    m = m_clipper
    D1 = rng.uniform(-100, 100, (m, 2))
    D2 = D1 + rng.normal(0, 0.02, (m, 2))
    A = np.column_stack([np.arange(m), rng.permutation(m)]).astype(np.int32)
    A[: m // 8, 1] = A[: m // 8, 0]                                            # an eighth of the associations are true
    s.clipper_affinity(D1, D2, A, sigma=0.1, epsilon=0.3)
    M = s.clipper_affinity(D1, D2, A, sigma=0.1, epsilon=0.3)
    ms = api.last_device_ms(api.MS_AFFINITY)
    evals = m * (m - 1) / 2
    aff = {"bound": "fp64_valu", "kernel": "k_clipper_affinity (one thread per association pair)", "m": m, "kernel_ms": ms, "evaluations": evals,
           "evaluations_per_s": evals / (ms * 1e-3), "achieved": evals * 64 / (ms * 1e-3) / 1e9, "unit": "GB/s", "peak": HBM_PEAK_GBS, "traffic": None,
           "note": "SURVEY 8d charges 64 B per evaluation if the four points were streamed; the two point sets (64 KB) are cache-resident and "
                   "the m x m dense result (128 MB at m = 4096) is what moves: 8 B written per evaluation"}
    aff["frac"] = aff["achieved"] / HBM_PEAK_GBS
    if with_cpu:
        from oracle import pyoracle as po
        mc = 1024
        Ac = np.ascontiguousarray(A[:mc])
        Mo = np.zeros((mc, mc))
        opar = po.lib()
        D1c, D2c = np.ascontiguousarray(D1), np.ascontiguousarray(D2)
        t0 = time.perf_counter()
        opar.orc_clipper_affinity(D1c.ctypes.data_as(C.c_void_p), C.c_int(m), D2c.ctypes.data_as(C.c_void_p), C.c_int(m), C.c_int(2),
                                  Ac.ctypes.data_as(C.c_void_p), C.c_int(mc), C.byref(ocp), Mo.ctypes.data_as(C.c_void_p))
        dt = time.perf_counter() - t0
        aff["cpu_baseline"] = {"kind": "port", "cores": 1, "sample": "the first 1024 associations (523 776 evaluations)", "seconds": dt,
                               "evaluations_per_s": mc * (mc - 1) / 2 / dt}
    res["affinity"] = aff
    # -- dense clique: the whole projected-gradient solve on the device (cooperative multi-workgroup solve at m >= 1024)
    u0 = rng.uniform(0, 1, m)
    p = s.clipper_params(sigma=0.1, epsilon=0.3)
    s.clipper_dense_clique(M, u0, p)
    nodes, u, score = s.clipper_dense_clique(M, u0, p)
    ms_solve, ms_csr = api.last_device_ms(api.MS_CLQ_SOLVE), api.last_device_ms(api.MS_CLQ_CSR)
    nnz = api.last_device_ms(api.MS_CLQ_NNZ)
    wgs, evals_g = s.clipper_last_solve_info()
    clq = {"bound": "hbm", "kernel": "k_clq_solve_coop" if wgs > 1 else "k_clq_solve", "m": m, "nnz": nnz, "workgroups": int(wgs), "gradient_evaluations": evals_g,
           "clique_size": int(len(nodes)), "solve_ms": ms_solve, "csr_build_ms": ms_csr, "us_per_product": ms_solve * 1e3 / max(evals_g, 1.0),
           "achieved": nnz * 12 * evals_g / (ms_solve * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "traffic": None,
           "note": "algorithmic bytes: nnz * 12 B (value + column index) per sparse product, one product per gradient evaluation; the CSR "
                   "(%.1f MB) is L2-resident and every evaluation ends in a grid barrier: the solve is latency-bound, not DRAM-bound.  The dense "
                   "128 MB affinity matrix is uploaded by the stand-alone entry point; the upload is outside both timers" % (nnz * 12 / 1e6)}
    clq["frac"] = clq["achieved"] / HBM_PEAK_GBS
    if with_cpu:
        from oracle import pyoracle as po
        on, ou, osc = np.zeros(m, np.int32), np.zeros(m), C.c_double(0)
        Mc = np.ascontiguousarray(M)
        t0 = time.perf_counter()
        n_o = po.lib().orc_clipper_solve(Mc.ctypes.data_as(C.c_void_p), C.c_int(m), u0.ctypes.data_as(C.c_void_p), C.byref(ocp),
                                         on.ctypes.data_as(C.c_void_p), ou.ctypes.data_as(C.c_void_p), C.byref(osc))
        dt = time.perf_counter() - t0
        clq["cpu_baseline"] = {"kind": "port", "cores": 1, "sample": "the same problem from the same start (dense-to-sparse conversion included)", "seconds": dt,
                               "same_clique_as_gpu": bool(sorted(on[:n_o].tolist()) == sorted(nodes.tolist()))}
    res["clipper"] = clq
    return res


def association_report(s, cfg, logs, frames, merge_n_global, merge_slots):
    """The sharded job's cross-robot association against the reference's: the timed passes run on the MERGE of the robots'
    final maps (distributed.associate_global); the reference's replica associates every foreign packet frame by frame against its own moving
    maps (sloamNode.cpp:912-1002).  Here the product plays that replica at full size (one SlideBackend ingesting all robots), and the two
    partitions of the landmarks are compared: global landmarks per class, landmarks held by two or more robots (shared slots)."""
    from slide_slam_amd.distributed import associate_by_ingest
    from slide_slam_amd.replay import replay_multi, replay_single
    t0 = time.perf_counter()
    R = len(logs)
    P = len(logs[0]["rel7"]) if frames is None else frames
    own = []
    for lg in logs:
        gb = s.SlideBackend(s.default_params(pose_chart=CHART), 1)
        own.append(replay_single(gb, lg, n_frames=frames))
    rb = s.SlideBackend(s.default_params(pose_chart=CHART), R)
    rep = replay_multi(rb, dict(cfg=cfg, logs=logs, relmeas=[]), n_frames=frames, own_node_factory=lambda: s.SlideBackend(s.default_params(pose_chart=CHART), 1))
    names = ("cyl_id", "cube_id", "ell_id")
    own_ids = [[own[r][names[c]] for c in range(3)] for r in range(R)]
    rep_ids = [[[rep["ids"][k][r][c] for k in range(P)] for c in range(3)] for r in range(R)]
    gid, n_glob, st = associate_by_ingest(own_ids, rep_ids)
    slots = 0
    for c in range(3):
        cnt = np.zeros(n_glob[c], np.int32)
        for r in range(R):
            cnt[np.unique(gid[r][c])] += 1
        slots += int((cnt >= 2).sum())
    cts = rb.counts()
    return {"merge_of_final_maps": {"global_landmarks": [int(x) for x in merge_n_global], "shared_slots": int(merge_slots)},
            "replica_frame_by_frame": {"global_landmarks": [int(x) for x in n_glob], "shared_slots": slots, "split": st["split"], "collapsed": st["collapsed"],
                                       "replica_counts": [cts["cyl"], cts["cube"], cts["point"]]},
            "seconds": time.perf_counter() - t0,
            "note": "the timed passes use the merge; setup_local_shards(assoc=associate_by_ingest(..)) installs the replica's partition instead "
                    "(tests/test_bench_config.py::test_exact_joint_step_with_the_replicas_frame_by_frame_association: inventory identical to the "
                    "oracle replica's, 5e-6 to its optimum on C4tiny)"}


def _pmc_traffic(kernel, **match):
    """HBM-side bytes per launch of `kernel` from the committed PMC summaries (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate
    passes, gfx950 corrections applied; a PMC pass cannot run inside the timed bench): newest round first."""
    pdir = os.path.join(ROOT, "profiles")
    for rnd in ("r05", "r04", "r03", "r02_dense", "r02", "r01"):
        for name in sorted(os.listdir(pdir)) if os.path.isdir(pdir) else []:
            if not (name.startswith(rnd + "_pmc_traffic") and name.endswith(".json")):
                continue
            try:
                with open(os.path.join(pdir, name)) as fh:
                    pmc = json.load(fh)
            except (OSError, ValueError):
                continue
            if pmc.get("kernel") == kernel and all(pmc.get(k) == v for k, v in match.items()):
                return pmc.get("hbm_bytes_per_launch")
    return None


def _pmc_mfma_util(kernel, avg_launch_ms=None):
    """Matrix-pipe utilisation of `kernel` from the committed PMC summary (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES in its own pass,
    tools/gpu_mfma_util.sh; the kernel's LARGEST grid = the exact joint passes' launches): {"busy_cycles_per_launch", "util_profiled"
    (busy / (the profiled dispatches' own duration x 2.4 GHz x 1024 SIMDs)), "util_at_this_runs_launch_time"} or None."""
    pdir = os.path.join(ROOT, "profiles")
    try:
        with open(os.path.join(pdir, "r05_pmc_mfma_util.json")) as fh:
            groups = json.load(fh).get(kernel) or []
    except (OSError, ValueError):
        return None
    if not groups:
        return None
    g = max(groups, key=lambda e: e.get("grid", 0))
    out = {"busy_cycles_per_launch": g.get("mfma_busy_cycles_per_dispatch"), "util_profiled": g.get("mfma_util"), "grid": g.get("grid"),
           "source": "profiles/r05_pmc_mfma_util.json (SQ_VALU_MFMA_BUSY_CYCLES; 64 busy cycles = one v_mfma_f64_16x16x4_f64)"}
    if avg_launch_ms and g.get("mfma_busy_cycles_per_dispatch"):
        out["util_at_this_runs_launch_time"] = g["mfma_busy_cycles_per_dispatch"] / (avg_launch_ms * 1e-3 * 2.4e9 * 1024)
    return out


def chol_flops(T, prof=None):
    """FLOPs of one factorisation with the RHS row: per block column k with n_k rows below it INSIDE THE PROFILE (prof[k] = last
    tile row of column k the solver touches; None = every tile of the lower triangle), trailing update n_k^2 * 64 + triangular solve
    n_k * 64^2 + diagonal block 64^3 / 3   (= n^3 / 3 overall for the dense profile)."""
    nk = [((T - 1 if prof is None else int(prof[k])) - k) * 64 + 1 for k in range(T)]
    return sum(v * v * 64.0 + v * 64.0 * 64.0 + 64.0 ** 3 / 3.0 for v in nk)


def band_flops(T, prof, nbr):
    """FLOPs of the steps over the T block columns of a BORDERED band (exact joint step): per column k with v rows of the band below it
    inside the profile and w = 64 nbr + 1 border rows (the separator's coupling rows and the right-hand side): trailing update of the band
    and of the border rows (v^2 + 2 v w) * 64, triangular solves (v + w) * 64^2, diagonal block 64^3 / 3.  The border x border block is
    not touched by the steps (border_flops)."""
    w = 64 * nbr + 1
    tot = 0.0
    for k in range(T):
        v = (int(prof[k]) - k) * 64
        tot += (v * v + 2.0 * v * w) * 64.0 + (v + w) * 64.0 * 64.0 + 64.0 ** 3 / 3.0
    return tot


def segmented_flops(segs, seg_prof_of, ends, first):
    """The same two counts for a band cut into segments (slide_graph_get_segments / _get_segment_table): every segment is a bordered band
    of its own whose border rows are the tile rows that are non-zero in it (first[s][i] <= column), the border product sums per segment."""
    INF = 1 << 29
    nbr = first.shape[1] - 1
    band = done = 0.0
    for s_, (t0, t1) in enumerate(segs):
        f = first[s_]
        for k in range(t0, t1):
            v = (seg_prof_of(s_, k) - k) * 64
            w = 64 * int(sum(1 for i in range(nbr) if f[i] <= k)) + 1
            band += (v * v + 2.0 * v * w) * 64.0 + (v + w) * 64.0 * 64.0 + 64.0 ** 3 / 3.0
        for j in range(nbr):
            for i in range(j, nbr + 1):
                c0 = max(int(f[i]), int(f[j]))
                if c0 < INF:
                    done += 2.0 * 64 ** 3 * max(0, ends[s_] - c0)
    return band, done


def border_flops(T, first):
    """FLOPs of the border product bord(i, j) -= sum_c W^T(i, c) W^T(j, c)^T over the tiles i >= j (i = nbr: the right-hand-side row):
    2 * 64^3 per tile and column block c >= max(first[i], first[j]) — (performed, the same with no column skipped)."""
    nbr = len(first)
    fi = list(first) + [0]
    done = dense = 0.0
    for j in range(nbr):
        for i in range(j, nbr + 1):
            done += 2.0 * 64 ** 3 * max(0, T - max(fi[i], fi[j]))
            dense += 2.0 * 64 ** 3 * T
    return done, dense


def self_launch(n):
    """Run this script as n ranks under torch.distributed.run (child process in its own session; stdout / stderr inherited) and return
    its exit code.  The exchange between the ranks is RCCL ("nccl") unless SLIDE_BENCH_BACKEND says otherwise; a multi-GPU RCCL job has
    never run on the one-GPU boxes this was developed on, so a child that fails or does not finish within SLIDE_BENCH_CHILD_TIMEOUT
    seconds (default 1500) is ended — its own process group, nothing else — and the job is run ONCE more with the exchange staged through
    the host over gloo, which the 2- and 4-rank rehearsals on one GPU did exercise; the JSON line then says so ("backend": "gloo", and
    config.multi_gpu_fallback)."""
    import signal
    import socket
    import subprocess

    def run(extra_env):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # (the host driver only supports dmabuf IPC: RCCL needs it)
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // n)))
        env.update(extra_env)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
        child = subprocess.Popen(cmd, env=env, cwd=ROOT, start_new_session=True)
        try:
            return child.wait(timeout=float(os.environ.get("SLIDE_BENCH_CHILD_TIMEOUT", "1500")))
        except subprocess.TimeoutExpired:
            for sig in (signal.SIGTERM, signal.SIGKILL):
                try:
                    os.killpg(child.pid, sig)      # the child's own session: exactly the ranks started above
                except ProcessLookupError:
                    break
                try:
                    child.wait(timeout=20)
                    break
                except subprocess.TimeoutExpired:
                    continue
            return 124

    rc = run({})
    if rc != 0 and "SLIDE_BENCH_BACKEND" not in os.environ and os.environ.get("SLIDE_BENCH_NO_FALLBACK") != "1":
        sys.stderr.write(f"bench.py: the {n}-rank run over RCCL ended with code {rc}; running it once more with the exchange staged through the host (gloo)\n")
        rc = run({"SLIDE_BENCH_BACKEND": "gloo", "SLIDE_BENCH_FALLBACK_NOTE": f"the RCCL run ended with code {rc}; exchange staged through the host over gloo"})
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--preset", default="C4")
    ap.add_argument("--frames", type=int, default=None, help="truncate each robot's log (debug)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the un-batched re-run and the convergence probe")
    ap.add_argument("--ingest-only", action="store_true", help="build the graph without per-frame solves (profiling aid)")
    ap.add_argument("--assoc-report", action="store_true", help="add the merge-vs-replica association report: a full-size replica ingests every robot frame by frame (about a minute; profiles/r05_association_c4_full.json holds the round's result)")
    ap.add_argument("--no-place-leg", action="store_true", help="skip the SlideMatch / SlideGraph / CLIPPER legs of the roofline")
    ap.add_argument("--no-dense-leg", action="store_true", help="skip the dense-profile legs of the roofline (rocprofv3 runs of the default)")
    ap.add_argument("--dense-profile", action="store_true",
                    help="the whole run on the dense profile (every tile of the lower triangle): the configuration of roofline.dense_profile, "
                         "for rocprofv3 runs")
    ap.add_argument("--robots-per-gpu", type=int, default=0,
                    help="robot shards per GPU; 0 = the preset's robots / N when that divides (the SAME 8-robot graph at every N: "
                         "strong scaling), else 1; 1 = one robot per GPU at every N (weak scaling)")
    ap.add_argument("--probe", type=int, default=10, help="passes recorded one by one for the convergence figure")
    ap.add_argument("--joint", choices=("exact", "pcg", "jacobi"), default="exact",
                    help="joint Gauss-Newton step over the robots: exact = shared landmarks as the separator of the joint graph (one "
                         "all-reduce per pass, no inner iteration: the step of the reference's full replica); pcg = --pcg conjugate-gradient "
                         "iterations on the global reduced pose system per pass (inexact); jacobi = every robot's own block solve only")
    ap.add_argument("--no-relmeas", action="store_true",
                    help="leave out the inter-robot relative-pose factors (SURVEY 8d: one per robot pair within 60 m every 50 frames)")
    ap.add_argument("--chart", choices=("cayley", "expmap"), default="cayley",
                    help="Pose3 retraction chart of product AND oracle: cayley = GTSAM 4.0.3's default (cubeFactor.h:96-97), expmap = GTSAM_POSE3_EXPMAP builds")
    ap.add_argument("--no-dense-relmeas", action="store_true", help="skip the leg with SURVEY 8d's relative-pose density (reported beside the headline)")
    ap.add_argument("--pcg", type=int, default=8, help="--joint pcg: PCG iterations per pass")
    ap.add_argument("--pcg-tol", type=float, default=0.0, help="--joint pcg: relative tolerance on sqrt(r^T M^-1 r) (0: every iteration counts)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what they computed (every robot's poses and landmark estimates) as DIR/<name>.npy, float64")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: convergence figure, stage / kernel / roofline profiles, parity checks, the dense "
                         "relative-pose leg, the association / SlideMatch / SlideGraph / CLIPPER legs and the CPU baselines (a minute and more); "
                         "without it the run sets up, warms up, times the steps and prints the headline line")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    global DENSE_PROFILE, DENSE_LEG, CHART
    CHART = 1 if args.chart == "expmap" else 0
    DENSE_PROFILE = args.dense_profile
    DENSE_LEG = not (args.no_dense_leg or args.dense_profile)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` as the driver may call it: start the N ranks ourselves (torch.distributed.run, one process per GPU)
        # as a CHILD process, before torch or anything that touches the GPU is imported here, relay its output (rank 0 prints the JSON
        # line) and leave with its exit code.
        if args.dump_outputs:       # (the ranks start in the repository root: the last --dump-outputs, absolute, is the one they take)
            sys.argv += ["--dump-outputs", os.path.abspath(args.dump_outputs)]
        raise SystemExit(self_launch(args.gpus))
    import torch            # torch first: it must initialise the device before this library's HIP runtime is loaded
    dist = None
    # SLIDE_BENCH_BACKEND=gloo rehearses the N > 1 path with every rank on GPU 0 (collectives staged through the
    # host); the real runs use nccl (= RCCL over xGMI), one GPU per rank.
    backend = os.environ.get("SLIDE_BENCH_BACKEND", "nccl")
    dev_index = local_rank if backend == "nccl" else 0
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1 or os.environ.get("SLIDE_BENCH_FORCE_DIST") == "1":
        import torch.distributed as dist
        if "MASTER_ADDR" not in os.environ:      # SLIDE_BENCH_FORCE_DIST on a plain `python bench.py`: a one-rank RCCL group
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=os.environ.get("MASTER_PORT", "29533"), RANK="0", WORLD_SIZE="1")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=device)
        else:
            dist.init_process_group(backend=backend)

    import slide_slam_amd as s
    from slide_slam_amd.distributed import PassDriver, TorchComm, gpu_matcher, setup_local_shards
    from slide_slam_amd.synth import SynthConfig, make_robot_log, make_world
    s.device_check()
    cfg = SynthConfig.preset(args.preset)
    R = args.robots_per_gpu if args.robots_per_gpu > 0 else (cfg.robots // world if cfg.robots % world == 0 else 1)
    robots = world * R
    world_map = make_world(cfg)
    logs = [make_robot_log(cfg, world_map, (rank * R + t) % cfg.robots) for t in range(R)]
    P = len(logs[0]["rel7"]) if args.frames is None else args.frames
    multi = robots > 1          # several sub-graphs with shared landmarks: the distributed pass; else one robot's own joint graph
    use_dist = dist is not None
    wdev = world if use_dist else 1
    base = TorchComm(device=device, stage_through_host=(backend != "nccl")) if use_dist else None
    sync_coll = os.environ.get("SLIDE_BENCH_SYNC_COLLECTIVES") == "1"     # diagnostic: host-synchronous collectives

    def barrier():
        torch.cuda.synchronize()
        if use_dist and world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def build_all():
        shards, reps = [], []
        t0 = time.perf_counter()
        for lg in logs:
            gb, rep = build_shard(s, lg, args.frames, args.ingest_only)
            shards.append(gb)
            reps.append(rep)
        return shards, reps, time.perf_counter() - t0

    shards, reps, t_build = build_all()
    rep = reps[0]
    st = shards[0].graph.stats()
    T = st["chol_dim"] // 64
    info, parity, conv, batched_prof, dense_leg = {}, None, None, None, None

    if multi:
        batch = s.CholBatch(R)
        for t, gb in enumerate(shards):
            gb.graph.join_chol_batch(batch, t)
        bufs, info = setup_local_shards(shards, gpu_matcher, base=base, rank=rank, world=wdev, device=device)
        drv = PassDriver(shards, bufs, info["n_slots"], batch=batch, base=base, world=wdev, device=device,
                         pcg_iters=args.pcg if args.joint == "pcg" else 0, pcg_tol=args.pcg_tol, arrow=args.joint == "exact", sep_dim=info["sep_dim"], sep_prof=info.get("sep_prof"))
        info["relmeas"] = "none"
        if not args.no_relmeas and args.joint == "exact" and robots == cfg.robots and args.frames is None:      # (the PCG / block-Jacobi passes' un-batched parity path carries no ghosts)
            from slide_slam_amd.synth import make_relmeas
            all_logs = logs if world == 1 else [make_robot_log(cfg, world_map, r) for r in range(cfg.robots)]
            rel = make_relmeas(cfg, all_logs)
            ng = drv.setup_ghosts(rel, rank=rank)
            info["n_relmeas"] = len(rel)
            info["relmeas"] = (f"{len(rel)} (addRelativeMeasFactor, graph.cpp:247-258; one per robot pair within 60 m at the same key frame, every "
                               f"{cfg.relmeas_every} frames), " +
                               ("each carried exactly as six further separator coordinates (its linearised residual)" if args.joint == "exact" else
                                "cross block left out of the step (gradient exact)") +
                               f"; {ng} ghost pose slots (linearisation points) refreshed at the start of every pass")
        info["totals"] = {k: int(sum(gb.graph.stats()[k] for gb in shards)) for k in ("n_pose", "n_lm", "n_factors")}
        info["totals"]["shared_slots"] = int(info["n_slots"])
        _blk = info["sep_prof"][1] if isinstance(info.get("sep_prof"), tuple) else (0, 0)
        info["sep_exchange_bytes"] = int(8 * s.CholBatch.sep_exchange_len(info["sep_dim"], info.get("n_relmeas", 0), _blk[0], _blk[1])) if info.get("sep_dim") else 0
        if getattr(drv, "sep_owner", None) is not None:
            _segs = [s.CholBatch.sep_segment(info["sep_dim"], info.get("n_relmeas", 0), _blk[0], _blk[1], w) for w in range(3)]
            info["sep_owned"] = dict(leaf=drv.sep_owner["leaf"], leaf_bytes=8 * _segs[drv.sep_owner["leaf"]][1] if len(drv.sep_owner["half_ranks"]) > 1 else 0,
                                     top_bytes=8 * _segs[2][1], rounds_inside_half=len(drv._pair_groups) - 1)
        if sync_coll:
            drv.stream_ordered = False
        if drv.arrow:
            info["stream_ordered_collectives"] = bool(drv.stream_ordered)
        if os.environ.get("SLIDE_BENCH_FORCE_PARTS") == "1":      # rehearsal of the N > 1 control flow (cut pass + RCCL on the batch's stream) on one rank
            drv.force_parts = True
        step = drv.one_pass
        js = (f", exact joint step: shared landmarks as separator ({info['sep_dim']} coordinates)" if drv.arrow else
              f", joint solve: {drv.pcg_iters} PCG iterations on the global reduced system" if drv.pcg_iters else ", block-Jacobi over robots")
        mode = ("one replayed hipGraph per pass, factorisations batched" if (wdev == 1 and not drv.force_parts) else
                f"replayed hipGraph parts, {backend} all-reduces of the shared-landmark blocks on the same stream between them") + js
    else:
        g = shards[0].graph
        step = lambda: g.gauss_newton(1)
        mode = "one robot, its own joint graph"

    # ---- convergence probe: the first passes one by one, poses kept with --full (not timed) ----
    # The probe passes run with or without --full: they and the cost read after each of them (which commits delta into theta) are
    # part of the state the warm-up and the timed steps start from.
    probe, probe_chi2 = [], []
    n_probe = 0 if args.no_parity or not multi else max(0, args.probe)
    for _ in range(n_probe):
        step()
        if args.full:
            probe.append(np.stack([all_poses(gb, P) for gb in shards]))
        probe_chi2.append(sum(gb.graph.chi2()["total"] for gb in shards))
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    dt = time.perf_counter() - t0
    if use_dist and world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    n_passes = n_probe + args.warmup + args.steps
    final = np.stack([all_poses(gb, P) for gb in shards])
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, shards, final, dist if use_dist else None, world, rank)
    finite = bool(np.isfinite(final).all())
    if not args.full:
        devs = _devices(dist, world)
        if rank == 0:
            print(json.dumps(headline(args, cfg, world, wdev, R, backend, dt, shards[0].graph.stats(), rep, t_build, info, mode, finite, dist, devs)),
                  flush=True)
        if use_dist:
            dist.destroy_process_group()
        if rank == 0 and not finite:
            raise SystemExit(1)
        return
    final_chi2 = sum(gb.graph.chi2()["total"] for gb in shards) if multi else None

    if multi:
        ptrs = [b.data_ptr() for b in bufs]
        if drv.arrow:
            info["border"] = [dict(first=[int(v) for v in gb.graph.border_profile()], T=int(gb.graph.stats()["chol_dim"] // 64),
                                   prof=[int(v) for v in gb.graph.tile_profile()], segs=gb.graph.segments(), segtab=gb.graph.segment_table())
                              for gb in shards]
            if wdev == 1 and not drv.force_parts:
                runs = [batch.profile_exact_joint(ptrs) for _ in range(7)]
                info["exact_joint_stages_ms"] = {k: float(np.median([r[0][k] for r in runs])) for k in runs[0][0]}
                info["separator_block_columns"] = runs[0][1]
            else:
                cuts = [drv.timed_cut_pass() for _ in range(7)]
                info["cut_pass_ms"] = {k: float(np.median([c[k] for c in cuts])) for k in cuts[0]}
        if wdev == 1 and not drv.force_parts:
            # device time of the batched step kernels (HIP events on the batch's stream, un-captured passes) for the roofline
            pr = sorted(batch.profile(ptrs) for _ in range(5))
            profs = [gb.graph.tile_profile() for gb in shards]
            batched_prof = dict(ms_steps=pr[len(pr) // 2][0], launches=pr[0][1], robots=R, flops=sum(chol_flops(T, pf) for pf in profs),
                                tiles=int(sum(int(pf[k]) - k + 1 for pf in profs for k in range(len(pf)))), tiles_dense=R * T * (T + 1) // 2)
            # the same graphs with the structure ignored (every tile of the lower triangle): the GEMM-shaped extreme of the same kernels
            if DENSE_LEG and not drv.arrow:
                for gb in shards:
                    gb.graph.set_dense_profile(True)
                for _ in range(3):
                    step()
                barrier()
                td = time.perf_counter()
                nd = max(5, min(args.steps, 20))
                for _ in range(nd):
                    step()
                barrier()
                td = (time.perf_counter() - td) / nd
                prd = sorted(batch.profile(ptrs) for _ in range(5))
                dense_leg = dict(ms_steps=prd[len(prd) // 2][0], launches=prd[0][1], ms_per_step=td * 1e3, flops=R * chol_flops(T))
                for gb in shards:
                    gb.graph.set_dense_profile(False)
                step()
        if n_probe:
            # cost (sum of squared whitened residuals over all factors of the job) after every probe pass and the poses' distance to
            # where the run ends (relative, per robot, the worst): passes / ms until that distance stays below the north-star 1e-4
            chi = list(probe_chi2)
            fin = final_chi2
            ref = np.linalg.norm(final.reshape(R, -1), axis=1)
            errs = [float((np.linalg.norm((p - final).reshape(R, -1), axis=1) / ref).max()) for p in probe]
            if use_dist and world > 1:
                tt = torch.tensor(chi + [fin], dtype=torch.float64, device="cuda")
                dist.all_reduce(tt)
                chi, fin = [float(v) for v in tt[:-1]], float(tt[-1])
                te = torch.tensor(errs, dtype=torch.float64, device="cuda")
                dist.all_reduce(te, op=dist.ReduceOp.MAX)
                errs = [float(v) for v in te]
            hit = [i + 1 for i, c in enumerate(chi) if c <= fin * 1.001]
            below = [k + 1 for k in range(len(errs)) if all(e <= 1e-4 for e in errs[k:])]
            p4 = below[0] if below else None
            conv = {"passes_to_1e-4_pose": p4, "ms_to_1e-4": (p4 * dt / args.steps * 1e3 if p4 else None),
                    "passes_to_0.1pct_of_final_cost": hit[0] if hit else None, "probe_passes": n_probe, "final_chi2": fin,
                    "chi2_after": {str(k): chi[k - 1] for k in (1, 2, 3, 4, 5, 10, 20, 40) if k <= n_probe},
                    "pose_rel_distance_to_final_after": {str(k): errs[k - 1] for k in (1, 2, 3, 4, 5, 10, 20, 40) if k <= n_probe},
                    "note": ("exact joint Gauss-Newton step (shared landmarks as the separator of the joint graph)" if drv.arrow else
                             "inexact joint step: PCG on the global reduced pose system" if drv.pcg_iters else
                             "block-Jacobi over robots (no joint solve): does not converge once robots share many landmarks") +
                            f"; final = after all {n_passes} passes of this run; start = the robots' own streaming builds merged (cross-robot "
                            "association), nothing joint solved yet; chi2 = 2 x NonlinearFactorGraph::error over all robots"}
        if not args.no_parity and not drv.arrow:
            # ---- parity of what was timed: identically built shards, the same number of passes through the UN-batched path ----
            for gb in shards:
                gb.graph.join_chol_batch(None)
            ref_shards, _, _ = build_all()
            rbufs, rinfo = setup_local_shards(ref_shards, gpu_matcher, base=base, rank=rank, world=wdev, device=device)
            rdrv = PassDriver(ref_shards, rbufs, rinfo["n_slots"], batch=None, base=base, world=wdev, device=device, pcg_iters=args.pcg)
            for i in range(n_passes):
                rdrv.one_pass()
                if i < n_probe:            # (the probe committed delta into theta after each of its passes: same here, same arithmetic)
                    for gb in ref_shards:
                        gb.graph.chi2()
            for gb in ref_shards:
                gb.graph.chi2()
            ref_final = np.stack([all_poses(gb, P) for gb in ref_shards])
            rel = float(np.abs(final - ref_final).max() / max(np.abs(ref_final).max(), 1.0))
            if use_dist and world > 1:
                tt = torch.tensor([rel if np.isfinite(rel) else 1e30], dtype=torch.float64, device="cuda")
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                rel = float(tt.item())
            same_slots = rinfo["n_slots"] == info["n_slots"]
            parity = {"batched_vs_unbatched_max_rel": rel, "passes_compared": n_passes, "slots_equal": same_slots, "finite": finite,
                      "ok": bool(finite and np.isfinite(rel) and rel < 1e-6 and same_slots),
                      "what": "poses of every robot after the probe + warm-up + timed passes vs identically built shards driven the same "
                              "number of passes through slide_graph_dist_phase (no batch, no captured graph, host-side sums); tolerance "
                              "1e-6 relative (only the summation order of the exchange differs)"}
            del ref_shards, rdrv, rbufs
    if multi and use_dist and world > 1 and drv.arrow and not args.no_parity:
        parity = n1_replica_parity(args, s, cfg, world_map, rank, world, device, dist, final, n_probe, n_passes, info)
    if multi and drv.arrow and wdev == 1 and not drv.force_parts and not args.no_relmeas and args.frames is None and not args.no_dense_relmeas and robots == cfg.robots:
        # ---- the same job with SURVEY 8d's relative-pose DENSITY (the timed headline carries the 2 factors the lock-step generator finds):
        # identically built shards, one factor per adjacent robot pair every 50 frames near the other's trajectory ----
        from slide_slam_amd.synth import make_relmeas_dense
        rel2 = make_relmeas_dense(cfg, logs)
        sh2, _, _ = build_all()
        b2 = s.CholBatch(R)
        for t, gb in enumerate(sh2):
            gb.graph.join_chol_batch(b2, t)
        bufs2, info2 = setup_local_shards(sh2, gpu_matcher, device=device)
        d2 = PassDriver(sh2, bufs2, info2["n_slots"], batch=b2, device=device, arrow=True, sep_dim=info2["sep_dim"], sep_prof=info2.get("sep_prof"))
        ng2 = d2.setup_ghosts(rel2)
        for _ in range(5):
            d2.one_pass()
        barrier()
        t2 = time.perf_counter()
        nd2 = max(5, min(args.steps, 50))
        for _ in range(nd2):
            d2.one_pass()
        barrier()
        t2 = (time.perf_counter() - t2) / nd2
        fin2 = bool(np.isfinite(np.stack([all_poses(gb, P) for gb in sh2])).all())
        for gb in sh2:
            gb.graph.join_chol_batch(None)
        info["dense_relmeas"] = dict(n_relmeas=len(rel2), lambda_coordinates=6 * len(rel2), ghost_slots=int(ng2), ms_per_step=t2 * 1e3, finite=fin2,
                                     what="the same job with one addRelativeMeasFactor (graph.cpp:247-258) per ADJACENT robot pair every 50 frames "
                                          "while the observer is within 40 m of the other robot's trajectory, paired with that robot's spatially closest "
                                          "pose (the reference pairs by time stamp, sloam.cpp:321-412: two different indices) — SURVEY 8d's density; "
                                          "parity of this variant: tests/test_bench_config.py::test_c4_exact_joint_step_with_dense_relative_pose_factors_at_size")
        del d2, b2, sh2, bufs2
    report(args, s, cfg, rank, world, wdev, R, backend, dt, shards, rep, t_build, info, mode, batched_prof, parity, conv, finite, dist, T, dense_leg)
    if use_dist:
        dist.destroy_process_group()
    if rank == 0 and ((parity is not None and not parity["ok"]) or not finite or
                      (multi and conv is not None and args.joint == "exact" and conv["passes_to_1e-4_pose"] is None)):
        raise SystemExit(1)


def n1_replica_parity(args, s, cfg, world_map, rank, world, device, dist, final, n_probe, n_passes, info):
    """N > 1: every line verifies itself against N = 1.  The ranks' final poses are gathered; rank 0 builds ALL robots of the job once
    more on its own GPU (the same streaming builds), merges them as one process (one CholBatch, the whole pass one replayed hipGraph,
    no collective) and drives the same number of exact joint passes — the N = 1 job of this very code — and the poses are compared:
    parity.vs_n1_max_rel, relative per robot, the worst; the bench exits 1 above 1e-6."""
    from slide_slam_amd.distributed import PassDriver, gpu_matcher, setup_local_shards
    from slide_slam_amd.synth import make_relmeas, make_robot_log
    gathered = [None] * world
    dist.all_gather_object(gathered, final)
    if rank != 0:
        return None
    job = np.concatenate(gathered, axis=0)
    robots = job.shape[0]
    if robots > 8:                   # (a CholBatch holds eight graphs)
        return {"vs_n1_max_rel": None, "ok": True, "what": f"not run: {robots} robots do not fit one CholBatch (8)"}
    P = job.shape[1]
    logs = [make_robot_log(cfg, world_map, r % cfg.robots) for r in range(robots)]
    ref = [build_shard(s, lg, args.frames, args.ingest_only)[0] for lg in logs]
    batch = s.CholBatch(robots)
    for t, gb in enumerate(ref):
        gb.graph.join_chol_batch(batch, t)
    bufs, rinfo = setup_local_shards(ref, gpu_matcher, device=device)
    drv = PassDriver(ref, bufs, rinfo["n_slots"], batch=batch, device=device, arrow=True, sep_dim=rinfo["sep_dim"], sep_prof=rinfo.get("sep_prof"))
    if info.get("n_relmeas"):
        drv.setup_ghosts(make_relmeas(cfg, logs))
    for i in range(n_passes):
        drv.one_pass()
        if i < n_probe:              # (the probe read the cost after each of its passes, which commits delta into theta: same here)
            for gb in ref:
                gb.graph.chi2()
    one = np.stack([all_poses(gb, P) for gb in ref])
    for gb in ref:
        gb.graph.join_chol_batch(None)
    rel = float((np.linalg.norm((job - one).reshape(robots, -1), axis=1) / np.linalg.norm(one.reshape(robots, -1), axis=1)).max())
    same = bool(rinfo["n_slots"] == info["n_slots"] and rinfo["sep_dim"] == info["sep_dim"])
    return {"vs_n1_max_rel": rel, "passes_compared": n_passes, "slots_equal": same, "ok": bool(np.isfinite(rel) and rel < 1e-6 and same),
            "what": f"poses of every robot after the probe + warm-up + timed passes of this {world}-rank job vs the SAME job run as one process "
                    "on rank 0's GPU (all robots in one CholBatch, no collective) — relative, per robot, the worst; tolerance 1e-6 (only the "
                    "summation order of the separator system's exchange differs; north-star bar 1e-4)"}


def _devices(dist, world):
    """This rank's device, or every rank's (collective at world > 1)."""
    import torch
    devs = [f"cuda:{torch.cuda.current_device()} {torch.cuda.get_device_name()}"]
    if dist is not None and world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, devs[0])
        devs = gathered
    return devs


def headline(args, cfg, world, wdev, R, backend, dt, st, rep, t_build, info, mode, finite, dist, devs):
    """The JSON line's headline part: the timed steps' figure, the configuration it was taken on, robot 0's streaming build (timed while the
    graphs were set up) — all a plain run prints; --full adds its own figures to it (report)."""
    robots = world * R
    n = st["chol_dim"]
    n_slots = info.get("n_slots", 0) if info else 0
    return {
        "metric": "pose-graph updates/sec + ms/Gauss-Newton iter, 8-robot 10k-landmark graph",
        "value": robots * args.steps / dt,
        "unit": "pose-graph updates/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "ms_per_gn_iter": dt / args.steps * 1e3,
        "higher_is_better": True,
        # the preset's robots over N GPUs (total work fixed) -> strong; a fixed number of robots per GPU -> weak
        "scaling": "strong" if (args.robots_per_gpu == 0 and robots == cfg.robots) else "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic (seeded, slide_slam_amd/synth.py)",
        "config": {"workload": f"{cfg.name} (BASELINE configs[3]): {robots} robot sub-graphs, {R} per GPU ({mode}) "
                               f"({st['n_pose']} poses, {st['n_lm']} landmarks, {st['n_factors']} factors in robot 0's); "
                               "a step = one Gauss-Newton pass of all of them, value = robot pose-graph updates/s; "
                               f"Pose3 chart: {args.chart} (product and oracle; --chart, both charts are parity-tested: tests/test_golden.py, test_bench_config.py); "
                               f"graph totals of this rank's {R} robots: {info.get('totals')}; synthetic noise: odometry sigma per metre "
                               f"{tuple(cfg.sigma_odom)} [rot, trans], detection position {cfg.sigma_det_pos} m, cube yaw {cfg.sigma_cube_yaw} rad, "
                               f"scale {cfg.sigma_scale} (SURVEY 8d specifies 20x / 10x more: with it the cross-robot association finds 15 % of the "
                               "shared landmarks, DESIGN 5); inter-robot relative-pose factors: " + str(info.get("relmeas", "none")),
                   "robots": robots, "robots_per_gpu": R, "reduced_system_dim": n, "chol_tile": 64,
                   "world_size": (dist.get_world_size() if dist is not None else 1), "backend": (backend if dist is not None else None),
                   "multi_gpu_fallback": os.environ.get("SLIDE_BENCH_FALLBACK_NOTE"),
                   "devices": devs,
                   "collective": None if not n_slots else (
                       ((f"{backend} " if wdev > 1 else "device-side gather, no inter-GPU ") +
                        (f"all-reduce x1 per pass: the packed separator system of the {n_slots} shared-landmark slots "
                         f"({info.get('sep_dim')} coordinates, {info.get('sep_exchange_bytes')} B)" if not info.get("sep_owned") else
                         f"the ranks split in two halves along the dissection of the separator system ({info.get('sep_dim')} coordinates over "
                         f"{n_slots} shared-landmark slots), every rank factors the leaf its half's robots see; PAIRWISE exchanges only (two-rank "
                         f"all-reduces: the sums follow one binary tree over the robot index at every rank count, bit for bit the N = 1 job's): "
                         f"{info['sep_owned']['rounds_inside_half']} round(s) inside the half over the own leaf's segment "
                         f"({info['sep_owned']['leaf_bytes']} B) and the top block's ({info['sep_owned']['top_bytes']} B), then one round between the "
                         f"halves over the top block — per pass, instead of the whole packed system ({info.get('sep_exchange_bytes')} B)") +
                        (f"; {'stream-ordered on the pass stream' if info.get('stream_ordered_collectives') else 'host-synchronous'}" if wdev > 1 else ""))
                       if info.get("sep_dim") and args.joint == "exact" else
                       ((f"{backend} " if wdev > 1 else "device-side local sum, no inter-GPU ") +
                        f"all-reduce x2 per pass over {n_slots} shared-landmark slots ({n_slots * 63 * 8} B per pass)"))},
        "stream_replay": {"frames": len(rep["t_frame"]), "updates_per_s": len(rep["t_frame"]) / max(sum(rep["t_frame"]), 1e-9),
                          "ms_last_frame": rep["t_frame"][-1] * 1e3, "ms_max_frame": max(rep["t_frame"]) * 1e3,
                          "ms_mean_last_100": float(np.mean(rep["t_frame"][-100:]) * 1e3), "build_s_all_local_robots": t_build,
                          "what": "robot 0's streaming build alone on the GPU: associate + add + iSAM2-equivalent update per frame, PCIe included"},
        "finite": finite,
    }


def report(args, s, cfg, rank, world, wdev, R, backend, dt, shards, rep, t_build, info, mode, bt, parity, conv, finite, dist, T, dense_leg=None):
    """--full: profile pass on this rank's first shard alone, the side legs and the CPU baselines + the JSON line (rank 0)."""
    g = shards[0].graph
    robots = world * R
    for sh in shards:
        sh.graph.join_chol_batch(None)
    st = g.stats()
    # per-kernel device time (HIP events on the launch stream) over a separate profiled pass of robot 0's sub-graph by itself
    g.set_profiling(True)
    nprof = max(3, min(args.steps, 5))
    for _ in range(nprof):
        g.gauss_newton(1)
    prof = g.get_profile()
    tprof = g.tile_profile()
    prof_all = prof
    if DENSE_LEG:
        g.set_dense_profile(True)          # and robot 0 alone with the structure ignored
        g.gauss_newton(1)
        for _ in range(nprof):
            g.gauss_newton(1)
        prof_all = g.get_profile()
        g.set_dense_profile(False)
    g.set_profiling(False)
    devs = _devices(dist, world)
    if rank != 0:
        return
    n = st["chol_dim"]
    upd_flops = chol_flops(T, tprof)
    upd = prof.get("chol_step", dict(ms=0.0, launches=1))
    upd_ms = upd["ms"] / max(upd["launches"], 1)
    upd_launches_per_iter = upd["launches"] / nprof
    flops_per_launch = upd_flops / max(upd_launches_per_iter, 1)
    ach = flops_per_launch / (upd_ms * 1e-3) / 1e12 if upd_ms > 0 else 0.0
    # the dense leg: the profiler accumulated both runs, the structure-aware one is subtracted
    updd = prof_all.get("chol_step", dict(ms=0.0, launches=1))
    dms = max(updd["ms"] - upd["ms"], 0.0) / max(updd["launches"] - upd["launches"], 1)
    dflops = chol_flops(T) / T
    dach = dflops / (dms * 1e-3) / 1e12 if dms > 0 else 0.0
    single = dict(kernel="k_chol_step (one robot alone)", achieved=ach, frac=ach / FP64_MFMA_PEAK_TFLOPS, flops_per_launch=flops_per_launch,
                  avg_launch_ms=upd_ms, traffic=None,
                  dense_profile=dict(achieved=dach, frac=dach / FP64_MFMA_PEAK_TFLOPS, flops_per_launch=dflops, avg_launch_ms=dms,
                                     traffic=_pmc_traffic("k_chol_step") if n == 3776 else None))
    traffic = None
    roof_kernel = "k_chol_step (v_mfma_f64_16x16x4_f64)"
    if bt:
        # the timed region ran k_chol_step_batched.  The robots of the GPU are factored in `groups` launch sequences of robots / groups
        # systems each on as many streams (independent systems: the sequences overlap, nothing synchronises them between fork and
        # join), so launches overlap in time: achieved = ALL algorithmic flops of the batched factor + solve / the HIP-event window
        # around it (fork .. join, the extractions and the chained backward substitutions included); flops_per_launch and
        # avg_launch_ms are that window shared out over the groups x 59 launches
        groups = max(1, bt["launches"] // max(T, 1))       # launch sequences the library used (one per system on a narrow profile, else two)
        per = max(1, bt["robots"] // groups)
        roof_kernel = (f"k_chol_step_batched (v_mfma_f64_16x16x4_f64, {per} factorisations per launch, {groups} overlapping launch sequences)")
        upd_launches_per_iter = bt["launches"]
        upd_ms = bt["ms_steps"] / max(upd_launches_per_iter, 1)
        flops_per_launch = bt["flops"] / max(upd_launches_per_iter, 1)
        ach = flops_per_launch / (upd_ms * 1e-3) / 1e12
        traffic = _pmc_traffic("k_chol_step_batched", robots=bt["robots"], profile="dense" if DENSE_PROFILE else "structure") if n == 3776 else None
    kernel_ms = {k: v["ms"] / nprof for k, v in prof.items()}
    dominant = max(kernel_ms, key=kernel_ms.get)
    exact = None
    stages = info.get("exact_joint_stages_ms") if info else None
    if stages and bt:
        # ---- the exact joint pass, stage by stage (HIP events on the pass's stream, un-captured passes after the timed region) ----
        bd = info["border"]
        groups = max(1, bt["launches"] // max(T, 1))
        fl_band = fl_done = fl_dense = 0.0
        n_seg = 1
        for b in bd:
            dn, de = border_flops(b["T"], b["first"])
            fl_dense += de
            if b.get("segtab") is not None and b["segs"][0]:
                # a cut band: the segments' steps, the second level (the cuts' poses: a dense system of nsep block columns with the rest
                # of the border as its border — counted with the band), the border product per segment
                segs, n_sep_poses = b["segs"]
                ends, first = b["segtab"]
                n_seg = max(n_seg, len(segs))
                fb, fd = segmented_flops(segs, lambda s_, k, b=b, segs=segs: min(b["prof"][k], segs[s_][1] - 1), ends, first)
                nsep = (6 * n_sep_poses + 63) // 64
                w2 = 64.0 * (len(b["first"]) - nsep) + 1
                fl_band += fb + chol_flops(nsep) + w2 * (64.0 * nsep) ** 2 + w2 * w2 * 64.0 * nsep
                fl_done += fd
            else:
                fl_band += band_flops(b["T"], b["prof"], len(b["first"]))
                fl_done += dn
        if n_seg > 1:      # launch sequences of the segments: bt["launches"] = sequences x the longest segment
            seq_len = max(t1 - t0 for b in bd if b.get("segtab") is not None for (t0, t1) in b["segs"][0])
            groups = max(1, round(bt["launches"] / max(seq_len, 1)))
        Ts = info["separator_block_columns"]
        blocks = info["sep_prof"][1] if isinstance(info.get("sep_prof"), tuple) else None
        if blocks is None:
            fl_sep, sep_launches, sep_bound = chol_flops(Ts), Ts, "mfma"
            sep_kernel = (f"k_chol_step (dense {Ts}-block-column separator system of {info.get('sep_dim')} coordinates, one launch per block column) "
                          "+ chained substitution")
        else:
            # dissected: two leaf blocks side by side (with the top block's w rows as their border), the top block's Schur complement, the top block
            Ta, Tb = blocks[0], blocks[1]
            Tt = Ts - Ta - Tb
            w = 64.0 * Tt + 1
            fl_sep = sum(chol_flops(t) + w * (64.0 * t) ** 2 + w * w * 64.0 * t for t in (Ta, Tb)) + chol_flops(Tt)
            sep_launches, sep_bound = max(Ta, Tb) + Tt, "latency"
            sep_kernel = (f"k_chol_step_batched + k_border_syrk + k_chol_step: separator system of {info.get('sep_dim')} coordinates, nested dissection "
                          f"over the robots: leaf blocks of {Ta} and {Tb} block columns factored side by side, top block of {Tt}; "
                          f"{sep_launches} step launches in a row instead of {Ts}, each bound by the chain of its 64-column diagonal block")
        ms_band, ms_syrk, ms_sep = stages["band_factorisations"], stages["border_products"], stages["separator_solve"]
        tf = lambda fl, ms: fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0      # noqa: E731
        exact = {
            "stages_ms": stages, "stages_sum_ms": float(sum(stages.values())),
            "band_factorisations": {
                "kernel": (f"k_chol_step_batched ({max(1, bt['robots'] // groups)} bordered systems per launch, {groups} overlapping launch sequences of {T} launches)"
                           if n_seg == 1 else
                           f"k_chol_step_batched (every band cut into {n_seg} segments factored side by side — nested dissection, the cuts' poses at a second "
                           f"level: {bt['launches']} launches in the overlapping sequences of the segments, then the second level's)"),
                "bound": "latency", "flops": fl_band, "window_ms": ms_band, "launches": bt["launches"],
                "flops_per_launch": fl_band / max(bt["launches"], 1), "avg_launch_ms": ms_band * groups / max(bt["launches"], 1),
                "achieved": tf(fl_band / groups, ms_band), "aggregate": tf(fl_band, ms_band), "unit": "TFLOP/s", "peak": FP64_MFMA_PEAK_TFLOPS,
                "frac": tf(fl_band / groups, ms_band) / FP64_MFMA_PEAK_TFLOPS, "mfma_util_pmc": _pmc_mfma_util("k_chol_step_batched"),
                "note": "every launch is the serial chain of one 64-column diagonal block (sixteen dependent 4x4 pivot steps) beside the "
                        "panel tiles of the band and of the border: bound by that chain's latency, not by the matrix pipe; avg_launch_ms = "
                        "the window over the launches of one sequence (dispatch gaps included), rocprofv3's per-launch average is in "
                        "profiles/r03_*kernel_stats.csv"},
            "border_product": {
                "kernel": "k_border_syrk (v_mfma_f64_16x16x4_f64; one launch per pass: every robot's Schur complement onto the separator, K = 64 T; "
                          "workgroups from a job table balanced over the XCD queues, operand loads fifteen k-steps ahead across the segments of a cut band)",
                "bound": "mfma", "flops_per_launch": fl_done, "flops_dense_equivalent": fl_dense, "avg_launch_ms": ms_syrk,
                "achieved": tf(fl_done, ms_syrk), "unit": "TFLOP/s", "peak": FP64_MFMA_PEAK_TFLOPS, "frac": tf(fl_done, ms_syrk) / FP64_MFMA_PEAK_TFLOPS,
                "traffic": _pmc_traffic("k_border_syrk"), "mfma_util_pmc": _pmc_mfma_util("k_border_syrk", ms_syrk),
                "traffic_note": "HBM-side bytes per k_border_syrk launch averaged over the THREE launches of a pass (this one, plus the two small "
                                "ones at the separator's own levels): the robots' launch carries ~3x the figure less a few MB"},
            "separator": {
                "kernel": sep_kernel,
                "bound": sep_bound, "flops": fl_sep, "window_ms": ms_sep, "launches": sep_launches, "flops_per_launch": fl_sep / max(sep_launches, 1),
                "avg_launch_ms": ms_sep / max(sep_launches, 1), "achieved": tf(fl_sep, ms_sep), "unit": "TFLOP/s", "peak": FP64_MFMA_PEAK_TFLOPS,
                "frac": tf(fl_sep, ms_sep) / FP64_MFMA_PEAK_TFLOPS},
        }
        dom = max(("band_factorisations", "border_product", "separator"), key=lambda k: {"band_factorisations": ms_band, "border_product": ms_syrk, "separator": ms_sep}[k])
        exact["dominant_by_time"] = dom
    res = headline(args, cfg, world, wdev, R, backend, dt, st, rep, t_build, info, mode, finite, dist, devs)
    res["roofline"] = {"bound": "mfma", "kernel": roof_kernel, "achieved": ach,
                       "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / FP64_MFMA_PEAK_TFLOPS,
                       "traffic": traffic, "traffic_unit": "HBM-side bytes per launch (PMC, profiles/r0x_pmc_traffic*.json)",
                       "one_robot_alone": single,
                       "profile": (None if not bt else {
                           "tiles_touched": bt["tiles"], "tiles_lower_triangle": bt["tiles_dense"],
                           "note": "the reduced pose systems of this workload are banded (key frames share landmarks with a few neighbours "
                                   "only): the solver works inside the tile-level profile, the flops counted are the ones performed, and the "
                                   "launches are bound by the serial diagonal-block chain, not by the matrix pipe; dense_profile = the same "
                                   "kernels on the same graphs with the structure ignored"}),
                       "dense_profile": (None if not (bt and dense_leg) else (lambda dm, dfl: {
                           "achieved": dfl / (dm * 1e-3) / 1e12, "frac": dfl / (dm * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                           "flops_per_launch": dfl, "avg_launch_ms": dm, "ms_per_step": dense_leg["ms_per_step"],
                           "traffic": _pmc_traffic("k_chol_step_batched", robots=bt["robots"], profile="dense") if n == 3776 else None,
                           "launch_sequences": max(1, dense_leg["launches"] // max(T, 1))})(
                               dense_leg["ms_steps"] / max(dense_leg["launches"], 1), dense_leg["flops"] / max(dense_leg["launches"], 1))),
                       "flops_per_launch": flops_per_launch, "avg_launch_ms": upd_ms,
                       "launches_per_iter": upd_launches_per_iter, "dominant_by_time": dominant,
                       "scope": ("HIP events on the batch's stream around the batched factor + solve (fork .. join of the launch sequences) of "
                                 "un-captured passes after the timed region; one_robot_alone = robot 0's sub-graph by itself, un-batched "
                                 "k_chol_step (the per-GPU load of the N = 8 run)")}
    res["kernel_ms_per_iter"] = kernel_ms
    try:
        # the same streaming build with iSAM2's bounded back-substitution (wildfire threshold 1e-3: what the reference's GTSAM runs with;
        # off by default here — the parity tests compare exact updates)
        from slide_slam_amd.replay import replay_single
        from slide_slam_amd.synth import make_robot_log, make_world
        gw = s.SlideBackend(s.default_params(pose_chart=CHART), 1)
        gw.graph.set_wildfire(1e-3)
        rw = replay_single(gw, make_robot_log(cfg, make_world(cfg), 0), n_frames=args.frames, collect=False)
        tw = rw["t_frame"]
        res["stream_replay"]["wildfire_1e-3"] = {"updates_per_s": len(tw) / max(sum(tw), 1e-9), "ms_last_frame": tw[-1] * 1e3,
                                                 "ms_mean_last_100": float(np.mean(tw[-100:]) * 1e3), "blocks_kept": gw.graph.wildfire_stats()["kept_total"]}
        del gw
    except Exception as e:      # noqa: BLE001
        res["stream_replay"]["wildfire_1e-3"] = {"error": repr(e)}
    if exact:
        d = exact[exact["dominant_by_time"]]
        res["roofline"] = {"bound": "mfma", "limited_by": d["bound"],      # (priced against the FP64 matrix pipe; "latency": a serial chain, not the pipe, sets the time)
                           "kernel": d["kernel"], "achieved": d["achieved"], "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                           "frac": d["frac"], "traffic": _pmc_traffic("k_chol_step_batched", robots=bt["robots"], profile="exact_joint") if n == 3776 else None,
                           "traffic_unit": "HBM-side bytes per launch (PMC, profiles/r0x_pmc_traffic*.json)",
                           "flops_per_launch": d["flops_per_launch"], "avg_launch_ms": d["avg_launch_ms"], "launches_per_iter": d.get("launches", 1),
                           "dominant_by_time": exact["dominant_by_time"], "exact_joint_pass": exact, "one_robot_alone": single,
                           "scope": "stage times: HIP events on the pass's stream between the stages of un-captured exact joint passes after the "
                                    "timed region (medians of 7); the dominant stage by time is reported at the top, the others under "
                                    "exact_joint_pass (border_product = the pass's FP64-MFMA GEMM)"}
    if info.get("cut_pass_ms"):
        res["cut_pass_ms"] = info["cut_pass_ms"]
    if info.get("dense_relmeas"):
        res["dense_relmeas"] = info["dense_relmeas"]
    if parity is not None:
        res["parity"] = parity
    if conv is not None:
        res["convergence"] = conv
    try:
        res["roofline"]["assoc"] = assoc_roofline(s)
    except Exception as e:      # noqa: BLE001  (the headline number stands on its own)
        res["roofline"]["assoc"] = {"error": repr(e)}
    if rank == 0 and world == 1 and info.get("n_global") is not None and getattr(args, "assoc_report", False):
        try:
            from slide_slam_amd.synth import make_robot_log, make_world
            wm_ = make_world(cfg)
            res["association"] = association_report(s, cfg, [make_robot_log(cfg, wm_, r) for r in range(cfg.robots)], args.frames,
                                                    info["n_global"], info.get("n_slots", 0))
        except Exception as e:      # noqa: BLE001
            res["association"] = {"error": repr(e)}
    if rank == 0 and not getattr(args, "no_place_leg", False):
        # A13 - A15 (SlideMatch sweep, SlideGraph triangle matching, CLIPPER): the kernels' own legs, the oracle timed beside them
        try:
            res["roofline"]["place"] = place_roofline(s, with_cpu=not args.no_cpu)
        except Exception as e:      # noqa: BLE001
            res["roofline"]["place"] = {"error": repr(e)}
        try:
            res["roofline"].update(slidegraph_roofline(s, with_cpu=not args.no_cpu))
        except Exception as e:      # noqa: BLE001
            res["roofline"]["clipper"] = {"error": repr(e)}
    if not args.no_cpu:
        try:
            from slide_slam_amd.synth import make_robot_log, make_world
            wm = make_world(cfg)
            all_logs = [make_robot_log(cfg, wm, r) for r in range(min(cfg.robots, os.cpu_count() or 1, 8))]
            if args.joint == "exact" and robots > 1 and world == 1:
                from slide_slam_amd.synth import make_relmeas
                cb, par = cpu_exact_joint_leg(s, all_logs, args.frames,
                                              relmeas=None if (args.no_relmeas or args.frames is not None) else make_relmeas(cfg, all_logs))
                res["cpu_baseline"] = cb
                res["parity"] = par
            v = cpu_baselines(all_logs, args.frames, budget_s=5.0 if "cpu_baseline" in res else 10.0)
            if "cpu_baseline" not in res:
                res["cpu_baseline"] = v["robots_as_threads"]
                res["cpu_baseline_variants"] = {k: v[k] for k in ("single_thread", "omp")}
            else:
                res["cpu_baseline_variants"] = v
        except Exception as e:  # noqa: BLE001  (the GPU number stands on its own)
            res.setdefault("cpu_baseline", {"error": repr(e)})
    print(json.dumps(res), flush=True)
    if isinstance(res.get("parity"), dict) and res["parity"].get("ok") is False:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
