"""slide_find_inter_loop_closures on the GPU: every pair of a list equals the single call (slide_find_inter_loop_closure) bit for bit,
its winner is the numpy reference's first-of-maximum (tests/slidematch_list_cases.py), and the oracle's findInterLoopClosure agrees —
whatever else is in the list, wherever the pair stands in it and however many workgroups it was given."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_cases as pc  # noqa: E402
import slidematch_list_cases as lc  # noqa: E402

from oracle import pyoracle as po  # noqa: E402
from slide_slam_amd.api import SLIDE_ERR_CAPACITY as CAPACITY  # noqa: E402

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class OPlace(C.Structure):                     # the oracle's parameter block (tests/test_gpu_place.py)
    _fields_ = [("dilation_factor", C.c_double), ("xy_step", C.c_double), ("yaw_half_range", C.c_double),
                ("yaw_step", C.c_double), ("match_threshold", C.c_double), ("match_threshold_dimension", C.c_double),
                ("disable_yaw_search", C.c_int), ("ignore_dimension", C.c_int), ("min_num_inliers", C.c_int),
                ("use_lsq", C.c_int), ("min_num_map_objects_to_start", C.c_int), ("max_rings", C.c_int)]


def _params(gpu, case):
    return gpu.place_default_params(**case["params"])


def _single(gpu, case, gp):
    """the single call per DISTINCT pair of the case"""
    return {(a, b): gpu.find_inter_loop_closure(case["maps"][a], case["maps"][b], gp) for a, b in set(case["pairs"])}


def _same_as_single(r, one):
    """found, inliers, xyzyaw and tf bit for bit; a pair that is not found has the identity (the single call leaves its tf alone)"""
    assert r["found"] == one["found"] and r["inliers"] == one["inliers"], (r, one)
    if one["found"]:
        assert np.array_equal(r["tf"], one["tf"]) and np.array_equal(r["xyzyaw"], one["xyzyaw"])
    else:
        assert np.array_equal(r["tf"], np.eye(4)) and np.array_equal(r["xyzyaw"], np.zeros(4))


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("found", "tf", "inliers", "xyzyaw", "status", "best_index", "candidates"))


@pytest.mark.parametrize("ig", [0, 1])
def test_mixed_list_three_ways(gpu, ig):
    case = lc.mixed_list(ig)
    gp = _params(gpu, case)
    res = gpu.find_inter_loop_closures(case["maps"], case["pairs"], gp)
    one = _single(gpu, case, gp)
    ref = lc.list_reference(case)
    op = OPlace(gp.dilation_factor, gp.search_xy_step_size, gp.match_yaw_half_range, gp.search_yaw_step_size, gp.match_threshold_position,
                gp.match_threshold_dimension, gp.disable_yaw_search, gp.ignore_dimension, gp.min_num_inliers, gp.use_nonlinear_least_squares,
                gp.min_num_map_objects_to_start, gp.max_rings)
    n_found = 0
    for k, (a, b) in enumerate(case["pairs"]):
        r = res[k]
        print(f"pair {k} {(a, b)}: found {r['found']} inliers {r['inliers']} best {r['best_index']} of {r['candidates']}")
        assert r["status"] == 0
        _same_as_single(r, one[(a, b)])                                                     # 1. the single call, bit for bit
        assert r["best_index"] == ref[k]["best_index"] and r["candidates"] == ref[k]["candidates"]      # 2. the numpy reference
        assert r["inliers"] == ref[k]["max_count"]
        A, B = np.ascontiguousarray(case["maps"][a]), np.ascontiguousarray(case["maps"][b])
        tf, inl, xyz = np.zeros(16), C.c_int(0), np.zeros(4)                                   # 3. the oracle
        ok = po.lib().orc_find_transformation(_p(A), C.c_int(len(A)), _p(B), C.c_int(len(B)), C.byref(op), _p(tf), C.byref(inl), _p(xyz))
        assert r["inliers"] == inl.value and r["found"] == bool(ok)
        if ok:
            n_found += 1
            print(f"   |xyzyaw - oracle| {np.abs(r['xyzyaw'] - xyz).max():.3e}  |tf - oracle| {np.abs(r['tf'].ravel() - tf).max():.3e}")
            assert np.allclose(r["xyzyaw"], xyz, atol=1e-9) and np.allclose(r["tf"].ravel(), tf, atol=1e-9)
    assert n_found >= case["edges"]["found_at_least"]


def test_ties_take_the_first_of_the_maximum(gpu):
    seen = []
    for name, case in lc.tie_lists().items():
        gp = _params(gpu, case)
        res = gpu.find_inter_loop_closures(case["maps"], case["pairs"], gp)
        ref = lc.list_reference(case)
        for k, r in enumerate(res):
            assert r["status"] == 0 and r["best_index"] == ref[k]["best_index"] and r["candidates"] == ref[k]["candidates"], (name, k)
            assert r["inliers"] == ref[k]["max_count"]
        for k in case["tie_at"]:
            assert res[k]["inliers"] == 1 and res[k]["best_index"] == lc.tie_edges(ref[k])["first"]
            seen.append(res[k])
    assert len(seen) == 5 and all(_same_bits(seen[0], r) for r in seen[1:])


@pytest.mark.parametrize("ig", [0, 1])
def test_chunks_of_64_65_128_query_objects(gpu, ig):
    case = lc.chunk_list(ig)
    gp = _params(gpu, case)
    res = gpu.find_inter_loop_closures(case["maps"], case["pairs"], gp)
    one = _single(gpu, case, gp)
    ref = lc.list_reference(case)
    for k, (a, b) in enumerate(case["pairs"]):
        assert res[k]["status"] == 0 and res[k]["best_index"] == ref[k]["best_index"] and res[k]["candidates"] == ref[k]["candidates"], k
        assert res[k]["inliers"] == ref[k]["max_count"]
        _same_as_single(res[k], one[(a, b)])


@pytest.mark.parametrize("ig", [0, 1])
def test_statuses_in_one_list(gpu, ig):
    case = lc.status_list(ig)
    x = case["expect"]
    gp = _params(gpu, case)
    res = gpu.find_inter_loop_closures(case["maps"], case["pairs"], gp)
    ref = lc.list_reference(case)
    for k in x["gated"]:
        r = res[k]
        assert (r["found"], r["status"], r["inliers"], r["best_index"], r["candidates"]) == (False, 0, 0, -1, 0), k
        assert np.array_equal(r["tf"], np.eye(4)) and np.array_equal(r["xyzyaw"], np.zeros(4))
    for k in x["empty_lattice"]:
        r = res[k]
        a, b = case["pairs"][k]
        one = gpu.find_inter_loop_closure(case["maps"][a], case["maps"][b], gp)
        assert (r["found"], r["status"], r["best_index"], r["candidates"]) == (False, 0, -1, 0) and r["inliers"] == one["inliers"]
        assert np.array_equal(r["tf"], np.eye(4)) and np.array_equal(r["xyzyaw"], np.zeros(4))
    for k in x["capacity"]:
        r = res[k]
        assert r["status"] == CAPACITY and r["found"] is False and r["inliers"] == 0 and r["best_index"] == -1
        assert r["candidates"] == ref[k]["candidates"]
        assert np.array_equal(r["tf"], np.eye(4)) and np.array_equal(r["xyzyaw"], np.zeros(4))
        a, b = case["pairs"][k]
        with pytest.raises(Exception):                                     # the single call's 150 KiB rule
            gpu.find_inter_loop_closure(case["maps"][a], case["maps"][b], gp)
    # the live pairs around them — the one at capacity (a 150 KiB image beside images of a few hundred bytes) included — are what
    # they are alone, and what the reference says
    for k in x["live"]:
        a, b = case["pairs"][k]
        r = res[k]
        assert r["status"] == 0 and r["best_index"] == ref[k]["best_index"] and r["candidates"] == ref[k]["candidates"], k
        assert r["inliers"] == ref[k]["max_count"]
        _same_as_single(r, gpu.find_inter_loop_closure(case["maps"][a], case["maps"][b], gp))
        alone = gpu.find_inter_loop_closures([case["maps"][a], case["maps"][b]], [(0, 1)], gp)[0]
        assert _same_bits(r, alone), k
    for k in x["at_capacity"]:
        assert res[k]["found"]


def test_permuting_the_pairs_permutes_the_outputs(gpu):
    case = lc.mixed_list(0)
    gp = _params(gpu, case)
    res = gpu.find_inter_loop_closures(case["maps"], case["pairs"], gp)
    perm = np.random.default_rng(3).permutation(len(case["pairs"]))
    assert not np.array_equal(perm, np.arange(len(perm)))
    res_p = gpu.find_inter_loop_closures(case["maps"], [case["pairs"][i] for i in perm], gp)
    for j, i in enumerate(perm):
        assert _same_bits(res_p[j], res[i]), (j, i)


def test_full_size_pair_twice_in_a_list(gpu):
    case = lc.full_size_list()
    gp = _params(gpu, case)
    res = gpu.find_inter_loop_closures(case["maps"], case["pairs"], gp)
    one = _single(gpu, case, gp)
    for k, (a, b) in enumerate(case["pairs"]):
        assert res[k]["status"] == 0
        _same_as_single(res[k], one[(a, b)])
    assert res[0]["candidates"] > 2 * 2048 * 4 and res[0]["inliers"] > 0          # every wave of the launch takes more than one candidate
    assert _same_bits(res[0], res[2])
    # the same winner as the single sweep of the centred maps reports
    r, q = lc.centre(case["maps"][0])[0], lc.centre(case["maps"][1])[0]
    sweep = gpu.match_maps_sweep(r, q, gp)
    assert sweep["best_index"] == res[0]["best_index"] and sweep["candidates"] == res[0]["candidates"]
    assert pc.first_argmax(sweep["inliers"]) == res[0]["best_index"]
