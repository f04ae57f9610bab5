"""The C-ABI library loads on a GPU-less host and exports every symbol include/slide_gpu.h declares;
compute entry points fail loudly (no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest

import slide_slam_amd as s
from slide_slam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions(name="slide_gpu.h"):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(slide_[a-z0-9_]+)\s*\(", txt)))


def test_every_declared_symbol_is_exported():
    L = s.lib()
    declared = _header_functions()
    assert len(declared) >= 40
    missing = [f for f in declared if not hasattr(L, f)]
    assert not missing, missing
    assert sorted(api.EXPORTS) == declared
    wire_declared = _header_functions("slide_wire.h")                 # include/slide_wire.h: wire codec + bag reader (host code)
    assert len(wire_declared) == 14
    assert not [f for f in wire_declared if not hasattr(L, f)]


def test_default_params_mirror_reference_defaults():
    p = s.default_params()
    assert p.relinearize_threshold == 0.1 and p.noise_floor == 0.01            # graph.cpp:17, graph.h:125
    assert list(p.noise_model_prior_first_pose_vec) == [1e-6] * 6              # graphWrapper.cpp:31
    assert list(p.noise_model_odom_vec) == [0.1] * 6 and list(p.noise_model_cube_vec) == [0.1] * 9
    assert p.cylinder_sigma == 400.0 and p.bearing_range_sigma == 1.0          # graphWrapper.cpp:60,63
    assert (p.cylinder_match_thresh, p.cuboid_match_thresh, p.ellipsoid_match_thresh) == (2.0, 2.0, 0.75)
    assert (p.knn_cylinder, p.knn_cube, p.knn_ellipsoid) == (50, 30, 1000)
    pp = s.place_default_params()
    assert pp.search_xy_step_size == 0.5 and pp.min_num_inliers == 5 and pp.dilation_factor == 1.2


def test_host_logic_closest_stamp():
    """GetIndexClosestPoseMstPair (sloam.cpp:428-440) is host logic: usable without a device."""
    assert s.closest_stamp([5, 15, 12], [0, 0, 0], 13, 500000000) == (1, 1.5)
    assert s.closest_stamp([], [], 10, 0)[0] == -1


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(s.SlideError):
        s.device_check()
    with pytest.raises(s.SlideError):
        s.SlideGraph(s.default_params())
    with pytest.raises(s.SlideError):
        s.dense_spd_solve(np.eye(4), np.ones(4))
    with pytest.raises(s.SlideError):
        s.submap_knn(np.zeros((4, 3), np.float32), np.zeros(3), 2)


def test_bench_self_launch_fails_loudly_without_a_gpu():
    """`python bench.py --gpus 2` (how the driver starts the multi-GPU bench) launches the ranks itself under torch.distributed.run; a
    failed RCCL run is repeated ONCE with the exchange staged through the host, and a job that cannot run — no GPU here — ends with a
    non-zero exit code and no JSON line, never with a number from some other path."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the 2-rank bench would run (covered by tests/test_bench_config.py on the GPU box)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("SLIDE_BENCH_BACKEND", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"], env=env, cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "running it once more with the exchange staged through the host" in r.stderr
    assert not any(line.startswith("{") for line in r.stdout.splitlines())


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "slide_slam_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "pyoracle" not in txt and "liboracle" not in txt and '#include "../oracle' not in txt, f


def test_find_relative_meas_match_host_logic():
    """sloam_test.cpp:59-205 through the product's entry point (pure host bookkeeping: runs without a GPU) and against the
    oracle on random schedules."""
    import slide_slam_amd as s
    from slide_slam_amd.api import SlideError
    import pytest
    f = s.find_relative_meas_match
    assert len(f([[], []], [0, 0], 0, [])[0]) == 0
    with pytest.raises(SlideError):
        f([[], []], [0, 0], 0, [((0, 0), 0, False)])                 # robotIndex == host -> the reference throws
    with pytest.raises(SlideError):
        f([[], []], [0, 0], 0, [((0, 0), 1, True)])                  # onlyUseOdom -> the reference throws
    m, left = f([[(5, 0)], [(5, 0)]], [1, 1], 0, [((5, 0), 1, False)])
    assert len(m) == 1 and tuple(m[0][2:]) == (0, 0) and len(left) == 0
    m, left = f([[(5, 0), (7, 0)], [(5, 0), (7, 0)]], [2, 2], 0, [((5, 0), 1, False), ((7, 1000), 1, False)])
    assert len(m) == 2 and tuple(m[0][2:]) == (0, 0) and tuple(m[1][2:]) == (1, 1) and len(left) == 0
    m, left = f([[(5, 0), (7, 0), (9, 8000000)], [(5, 0), (7, 0), (10, 2000000)]], [3, 3], 0, [((10, 0), 1, False)])
    assert len(m) == 0 and len(left) == 1                            # > 1 ms -> kept, not matched
    m, left = f([[(4, 0)], [(4, 0)]], [1, 1], 0, [((2, 0), 1, False)])
    assert len(m) == 0 and len(left) == 0                            # stale -> pruned
    # random schedules against the oracle
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_oracle_pins import _find
    rng = np.random.default_rng(0)
    for _ in range(50):
        packets = [[(int(t), int(rng.integers(0, 3)) * 400000) for t in np.sort(rng.integers(0, 30, rng.integers(0, 12)))] for _ in range(3)]
        counters = [int(rng.integers(0, len(pk) + 1)) for pk in packets]
        pending = [((int(rng.integers(0, 30)), int(rng.integers(0, 3)) * 400000), int(rng.integers(1, 3)), False) for _ in range(rng.integers(0, 8))]
        m, left = f(packets, counters, 0, pending)
        n, mo, nleft = _find(packets, counters, 0, pending)
        assert n == len(m) and np.array_equal(mo, m) and nleft == len(left)


def test_delaunay_equals_qhull():
    """the triangle SET equals qhull's (scipy wraps qhull; the reference's options, observation.cpp:25-26)."""
    from scipy.spatial import Delaunay
    for seed in range(12):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(3, 600))
        pts = rng.uniform(-80, 80, (n, 2))
        if seed % 4 == 0:
            pts = np.round(pts) + rng.normal(0, 1e-3, (n, 2))      # near-lattice: long thin triangles, near-cocircular quadruples
        mine = [tuple(t) for t in s.delaunay_2d(pts)]
        ref = sorted(tuple(sorted(int(v) for v in simplex)) for simplex in Delaunay(pts, qhull_options="Qt Qbb Qc Qz Q12").simplices)
        assert mine == ref
    assert len(s.delaunay_2d(np.zeros((2, 2)))) == 0
    assert len(s.delaunay_2d(np.array([[0.0, 0], [1, 1], [2, 2], [3, 3]]))) == 0     # collinear


def _pick_both(odom, obs, rel, latest, now, tol, mind):
    """product + oracle on the same queues; they must agree, the tuple is returned"""
    import ctypes as C
    from oracle import pyoracle as po
    got = s.pick_next_measurement(odom, obs, rel, latest, now, tol, mind)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    def st(lst):
        a = np.array([[x[0], x[1]] for x in lst] + [[0, 0]], np.int64)
        return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])
    os_, on_ = st([o[0] for o in odom]); bs, bn = st(obs); rs, rn = st(rel)
    op = np.ascontiguousarray(np.array([o[1] for o in odom] + [[0, 0, 0, 0, 0, 0, 1.0]], np.float64))
    out = np.zeros(4, np.int32)
    po.lib().orc_pick_next_measurement(P(os_), P(on_), P(op), C.c_int(len(odom)), P(bs), P(bn), C.c_int(len(obs)), P(rs), P(rn),
                                       C.c_int(len(rel)), C.c_int64(latest[0][0]), C.c_int64(latest[0][1]),
                                       P(np.ascontiguousarray(latest[1], dtype=np.float64)), C.c_double(now), C.c_double(tol),
                                       C.c_float(mind), P(out))
    assert got == tuple(int(v) for v in out)
    return got


def test_pick_next_measurement_reference_scenarios():
    """src/test/input_test.cpp:92-149, every expectation in order (queue sizes / fronts via the returned pop counts)."""
    I = [0, 0, 0, 0, 0, 0, 1.0]
    one = [1.0, 0, 0, 0, 0, 0, 1.0]
    latest0 = ((0, 0), I)
    odom1, obs1, rel1 = [((1, 0), one)], [(1, 0)], [(1, 0)]
    odom10, obs10, rel10 = [((10, 0), one)], [(10, 0)], [(10, 0)]
    assert _pick_both([], [], [], latest0, 1000.0, 3.0, 0.5)[0] == 0
    assert _pick_both(odom1, [], [], latest0, 1000.0, 3.0, 0.5)[0] == 1
    assert _pick_both([], obs1, [], latest0, 1000.0, 3.0, 0.5)[0] == 2
    assert _pick_both([], [], rel1, latest0, 1000.0, 3.0, 0.5)[0] == 3
    assert _pick_both([], obs1, rel10, latest0, 1000.0, 3.0, 0.5)[0] == 2
    assert _pick_both([], obs10, rel1, latest0, 1000.0, 3.0, 0.5)[0] == 3
    large = [((i, 0), one) for i in range(100)]
    m, po_, _, _ = _pick_both(large, [], [], latest0, 76.0, 3.0, 0.5)
    assert m == 1 and len(large) - po_ == 27 and large[po_][0][0] == 73
    large = large[po_:]
    m, po_, _, _ = _pick_both(large, [], [], latest0, 76.0, 3.0, 1.5)
    assert m == 0 and po_ == 0 and len(large) == 27 and large[0][0][0] == 73
    assert _pick_both(odom1, obs10, rel10, latest0, 10.0, 8.0, 0.5)[0] == 1
    assert _pick_both(odom1, obs1, rel10, latest0, 10.0, 8.0, 0.5)[0] == 2
    assert _pick_both(odom1, obs10, rel1, latest0, 10.0, 8.0, 0.5)[0] == 3
    q_odom = [((i, 0), one) for i in range(12)]
    q_obs = [(i, 0) for i in range(12)]
    q_rel = [(i, 0) for i in range(12)]
    m, a, b, c = _pick_both(q_odom, q_obs, q_rel, ((10, 0), I), 12.0, 3.0, 0.5)
    assert m == 0 and 12 - a == 2 and 12 - b == 2 and 12 - c == 2 and q_odom[a][0][0] == 10


def test_in_loop_closure_region_matches_oracle():
    import ctypes as C
    from oracle import pyoracle as po
    rng = np.random.default_rng(4)
    hits = 0
    for _ in range(200):
        n = int(rng.integers(0, 120))
        cloud = np.cumsum(rng.normal(0, 1.5, (n, 3)), axis=0).astype(np.float32)
        cloud[:, 2] *= 0.2
        q = cloud[-1].astype(np.float64) + rng.normal(0, 2.0, 3) if n else rng.normal(0, 1, 3)
        got = s.in_loop_closure_region(cloud, q, 10.0, 2.0, 30)
        c32 = np.ascontiguousarray(cloud.reshape(-1) if n else np.zeros(3, np.float32))
        ref = po.lib().orc_in_loop_closure_region(c32.ctypes.data_as(C.c_void_p), C.c_int(n), np.ascontiguousarray(q).ctypes.data_as(C.c_void_p),
                                                  C.c_double(10.0), C.c_double(2.0), C.c_uint64(30))
        assert got == bool(ref)
        hits += int(got)
    assert 10 < hits < 190


def test_loop_candidate_idx_matches_oracle():
    """CylinderMapManager::getLoopCandidateIdx (cylinderMapManager.cpp:160-184): product (host code) vs the oracle's
    sort-then-scan restatement, incl. the < 50 poses gate, the 'older than' rule, exact distance ties (by index) and the
    reference's size_t wrap-around for an index above pose_idx."""
    import ctypes as C
    from oracle import pyoracle as po
    rng = np.random.default_rng(12)

    def oracle(cloud, max_dist, pose_idx, at_least):
        cand = C.c_uint64(0)
        c32 = np.ascontiguousarray(cloud.reshape(-1))
        ok = po.lib().orc_loop_candidate_idx(c32.ctypes.data_as(C.c_void_p), C.c_int(len(cloud)), C.c_double(max_dist),
                                             C.c_uint64(pose_idx), C.c_uint64(at_least), C.byref(cand))
        return int(cand.value) if ok else None
    found = 0
    for trial in range(300):
        n = int(rng.integers(40, 400))
        # a loopy walk, so that old poses come back into range
        t = np.linspace(0, rng.uniform(2, 9), n)
        cloud = np.column_stack([20 * np.cos(t), 20 * np.sin(t), 0.1 * t]).astype(np.float32)
        cloud += rng.normal(0, 0.3, cloud.shape).astype(np.float32)
        if trial % 7 == 0:
            cloud[n // 3] = cloud[n // 4]          # exactly equidistant neighbours
        pose_idx = n - 1 if trial % 3 else int(rng.integers(0, n))
        got = s.loop_candidate_idx(cloud, 5.0, pose_idx, 30)
        assert got == oracle(cloud, 5.0, pose_idx, 30), (trial, n, pose_idx)
        if n < 50:
            assert got is None
        found += got is not None
    assert 30 < found < 290
    # size_t wrap-around: from pose 10 of 60, pose 11 (a LATER pose, 0.1 m away) qualifies in the reference
    line = np.column_stack([0.1 * np.arange(60), np.zeros(60), np.zeros(60)]).astype(np.float32)
    assert s.loop_candidate_idx(line, 0.15, 10, 30) == 11 == oracle(line, 0.15, 10, 30)
    with pytest.raises(s.SlideError):
        s.loop_candidate_idx(line, 1.0, 60, 30)


def test_merge_refuses_unknown_keys_loudly():
    """a factor on a key that is in neither the graph nor the pending values is refused with an error (isam->update throws
    there), not dropped silently.  Host logic up to the upload, which needs a device: without one the call fails earlier with
    SLIDE_ERR_HIP, so only the symbol / counter plumbing is checked here; the behaviour itself is tested under -m gpu."""
    assert "slide_graph_rejected_count" in s.api.EXPORTS


def _build_adaptor_check(tmp_path):
    import subprocess
    exe = str(tmp_path / "adaptor_check")
    lib_dir = os.path.dirname(s.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "adaptor_compile_check.cpp"),
                        "-o", exe, "-L" + lib_dir, "-lslide_gpu", "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_cpp_adaptor_compiles_and_links(tmp_path):
    """include/slide_sloam_adaptor.hpp: the S1 / S2 classes with the reference's method names (graph.h:70-121, graphWrapper.h:82-134)
    compile warning-free as C++17 and link against libslide_gpu.so; executed on the GPU box by tests/test_host_entry_points_gpu.py."""
    import subprocess
    exe = _build_adaptor_check(tmp_path)
    assert subprocess.run([exe]).returncode == 0          # no argument: link check only


def test_pointer_keeps_its_converted_array():
    """api._p(api._d(list)) converts into a temporary nothing else holds: the pointer must keep it alive for the call, or two such
    arguments of one call (add_keypose_between's rel and est) can share freed memory and read the second's contents."""
    import gc
    from slide_slam_amd import api
    a = api._p(api._d([1.0, 2, 3, 4, 5, 6, 7]))
    b = api._p(api._d([10.0, 20, 30, 40, 50, 60, 70]))
    gc.collect()
    assert a.value != b.value
    ra = np.ctypeslib.as_array((ctypes.c_double * 7).from_address(a.value))
    rb = np.ctypeslib.as_array((ctypes.c_double * 7).from_address(b.value))
    assert np.array_equal(ra, np.arange(1, 8)) and np.array_equal(rb, 10 * np.arange(1, 8))
