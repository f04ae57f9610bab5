"""PlaceRecognition::findInterLoopClosureWithClipper (place_recognition.cpp:541-629) for one pair of maps and for a list of pairs:
what is decided on the host — the exports, the reference's defaults, the whole-call refusals, the empty list, the object-count gate and
the (0, 0) filter — is reached without a device."""
import ctypes as C
import os

import numpy as np

import slide_slam_amd as s
from slide_slam_amd import api

INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _map(n, seed, zeros=0, x_only_zero=0):
    """n + zeros + x_only_zero rows: `zeros` of them at x = y = 0 (dropped), `x_only_zero` with x = 0 alone (kept)"""
    rng = np.random.default_rng(seed)
    m = np.zeros((n + zeros + x_only_zero, 7))
    m[:, 0] = 1
    m[:, 1:3] = rng.uniform(1.0, 30.0, (len(m), 2))
    m[:, 3] = rng.uniform(-1, 1, len(m))          # z and the dimensions play no part in the filter
    m[:zeros, 1:3] = 0.0
    m[zeros:zeros + x_only_zero, 1] = 0.0
    return m[rng.permutation(len(m))]


def _raw(maps, pairs, n_pairs=None, n_maps=None, off=None, null=(), u0=None, n_u0=None):
    """the list form through ctypes with every argument under the test's control; outputs start as sentinels"""
    flat = np.ascontiguousarray(np.concatenate(maps, axis=0))
    if off is None:
        off = np.concatenate([[0], np.cumsum([len(m) for m in maps])])
    off = np.ascontiguousarray(off, dtype=np.int32)
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    k = max(len(pr), 1)
    tf = np.full((k, 16), 7.0); counts = np.full((k, 4), 7, np.int32); found = np.full(k, 7, np.int32); status = np.full(k, 7, np.int32)
    args = dict(maps7=_p(flat), map_off=_p(off), pairs=_p(pr), tf=_p(tf), counts=_p(counts), found=_p(found), status=_p(status))
    for name in null:
        args[name] = None
    p = s.slidegraph_params()
    rc = s.lib().slide_find_inter_loop_closures_clipper(args["maps7"], args["map_off"], C.c_int(len(maps) if n_maps is None else n_maps), args["pairs"],
                                                        C.c_int(len(pr) if n_pairs is None else n_pairs), C.byref(p), u0, n_u0, args["tf"],
                                                        args["counts"], args["found"], args["status"])
    return rc, tf, counts, found, status


def _untouched(tf, counts, found, status):
    return (tf == 7.0).all() and (counts == 7).all() and (found == 7).all() and (status == 7).all()


def test_new_declarations_are_exported():
    L = s.lib()
    for name in ("slide_slidegraph_default_params", "slide_find_inter_loop_closure_clipper", "slide_find_inter_loop_closures_clipper"):
        assert hasattr(L, name) and name in api.EXPORTS
    header = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    assert "slide_slidegraph_params_t" in header and "place_recognition.cpp:541-629" in header and "sloamNode.cpp:587-694" in header
    for f in ("slidegraph_params", "find_inter_loop_closure_clipper", "find_inter_loop_closures_clipper"):
        assert callable(getattr(s, f))


def test_defaults_are_the_references():
    p = s.slidegraph_params()                        # place_recognition.cpp:65-75
    assert (p.sigma, p.epsilon, p.num_inliers_threshold, p.matching_threshold, p.min_num_map_objects_to_start) == (0.1, 0.1, 10, 0.1, 20)
    q = s.slidegraph_params(sigma=0.05, num_inliers_threshold=4)
    assert (q.sigma, q.epsilon, q.num_inliers_threshold) == (0.05, 0.1, 4)


def test_whole_call_refusals_write_nothing():
    a, b = _map(19, 1), _map(19, 2)          # (below the gate: a call that were NOT refused would still need no device)
    ok = _raw([a, b], [(0, 1)])
    assert ok[0] == api.SLIDE_OK and not _untouched(*ok[1:])
    cases = {
        "n_pairs < 0": dict(n_pairs=-1),
        "n_maps < 0": dict(n_maps=-1),
        "pairs NULL": dict(null=("pairs",)),
        "map_off NULL": dict(null=("map_off",)),
        "maps7 NULL": dict(null=("maps7",)),
        "tf NULL": dict(null=("tf",)),
        "counts NULL": dict(null=("counts",)),
        "found NULL": dict(null=("found",)),
        "decreasing map_off": dict(off=[0, 30, 19]),
        "negative map_off": dict(off=[-1, 19, 38]),
    }
    for what, kw in cases.items():
        rc, *outs = _raw([a, b], [(0, 1)], **kw)
        assert rc == INVALID and _untouched(*outs), what
    for bad in ((0, 2), (2, 0), (-1, 1), (0, -1)):
        rc, *outs = _raw([a, b], [(0, 1), bad])
        assert rc == INVALID and _untouched(*outs), bad
    ptrs = (C.c_void_p * 1)(a.ctypes.data)              # a u0[k] whose length nothing states
    rc, *outs = _raw([a, b], [(0, 1)], u0=ptrs, n_u0=None)
    assert rc == INVALID and _untouched(*outs)
    # status alone may be NULL
    rc, tf, counts, found, _ = _raw([a, b], [(0, 1)], null=("status",))
    assert rc == api.SLIDE_OK and found[0] == 0 and list(counts[0]) == [19, 19, 0, 0]


def test_empty_list_is_ok_without_a_device():
    rc, *outs = _raw([_map(25, 3)], [], n_pairs=0)
    assert rc == api.SLIDE_OK and _untouched(*outs)
    rc = s.lib().slide_find_inter_loop_closures_clipper(None, None, C.c_int(0), None, C.c_int(0), None, None, None, None, None, None, None)
    assert rc == api.SLIDE_OK
    assert s.find_inter_loop_closures_clipper([_map(25, 3)], []) == []


def test_gate_is_decided_on_the_host():
    """19 kept objects on both sides (:618, default 20): found 0, identity, counts {19, 19, 0, 0} — here, where no device exists."""
    a, b = _map(19, 4, zeros=3), _map(19, 5, zeros=1)
    r = s.find_inter_loop_closure_clipper(a, b)
    assert r["found"] is False and np.array_equal(r["tf"], np.eye(4))
    assert (r["n_ref_used"], r["n_qry_used"], r["n_putative"], r["n_inliers"]) == (19, 19, 0, 0)
    many = s.find_inter_loop_closures_clipper([a, b], [(0, 1), (1, 0), (0, 0)])
    assert len(many) == 3
    for m in many:
        assert m["status"] == 0 and not m["found"] and np.array_equal(m["tf"], np.eye(4))
        assert (m["n_ref_used"], m["n_qry_used"], m["n_putative"], m["n_inliers"]) == (19, 19, 0, 0)
    # one side below the gate is enough: the large side is not even triangulated
    r = s.find_inter_loop_closure_clipper(_map(40, 6), b)
    assert not r["found"] and (r["n_ref_used"], r["n_qry_used"]) == (40, 19)
    # the gate is the caller's parameter
    r = s.find_inter_loop_closure_clipper(a, b, s.slidegraph_params(min_num_map_objects_to_start=25))
    assert not r["found"] and (r["n_ref_used"], r["n_qry_used"]) == (19, 19)


def test_zero_rows_are_filtered_and_x_zero_alone_is_kept():
    a = _map(10, 7, zeros=4, x_only_zero=3)              # 17 rows, 13 kept
    y_only = _map(12, 8)
    y_only[:2, 2] = 0.0                                  # y = 0 alone: kept as well (:584 tests both coordinates)
    r = s.find_inter_loop_closure_clipper(a, y_only)
    assert (r["n_ref_used"], r["n_qry_used"]) == (13, 12) and not r["found"]
    r = s.find_inter_loop_closure_clipper(np.zeros((0, 7)), np.zeros((5, 7)))
    assert (r["n_ref_used"], r["n_qry_used"]) == (0, 0) and not r["found"]


def test_single_call_refuses_bad_arguments():
    a = _map(19, 9)
    tf = np.zeros(16); counts = np.zeros(4, np.int32); found = C.c_int(0)
    f = s.lib().slide_find_inter_loop_closure_clipper
    assert f(_p(a), C.c_int(-1), _p(a), C.c_int(19), None, None, C.c_int(0), _p(tf), _p(counts), C.byref(found)) == INVALID
    assert f(None, C.c_int(19), _p(a), C.c_int(19), None, None, C.c_int(0), _p(tf), _p(counts), C.byref(found)) == INVALID
    assert f(_p(a), C.c_int(19), _p(a), C.c_int(19), None, None, C.c_int(0), _p(tf), None, C.byref(found)) == INVALID
    assert f(_p(a), C.c_int(19), _p(a), C.c_int(19), None, None, C.c_int(0), _p(tf), _p(counts), C.byref(found)) == api.SLIDE_OK      # NULL params: the defaults
    assert list(counts) == [19, 19, 0, 0] and found.value == 0 and np.array_equal(tf.reshape(4, 4), np.eye(4))
