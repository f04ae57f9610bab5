"""The list form of SlideMatch (slide_find_inter_loop_closures) without a device: every edge a list of tests/slidematch_list_cases.py
claims is asserted on the numpy reference's own counts, and what the call decides on the host — the export, the whole-call refusals,
the empty list, the pairs that the gates stop — is reached through api.py and ctypes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_cases as pc  # noqa: E402
import slidematch_list_cases as lc  # noqa: E402

import slide_slam_amd as s  # noqa: E402
from slide_slam_amd import api  # noqa: E402

INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the cases' claims, on the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ig", [0, 1])
def test_mixed_list_is_what_it_claims(ig):
    case = lc.mixed_list(ig)
    e = case["edges"]
    assert [len(m) for m in case["maps"]] == e["sizes"] and len(case["pairs"]) == e["n_pairs"]
    assert sum(1 for a, _ in case["pairs"] if a == 0) == e["pairs_with_reference_0"]
    assert (0, 1) in case["pairs"] and (1, 0) in case["pairs"] and any(a == b for a, b in case["pairs"])
    assert np.any(case["maps"][2][:, 4:7] != 0) and not np.any(case["maps"][0][:, 4:7])
    ref = lc.list_reference(case)
    assert all(not r["gated"] and r["candidates"] > 1000 and r["best_index"] >= 0 for r in ref)
    assert sum(r["max_count"] >= case["params"]["min_num_inliers"] for r in ref) >= e["found_at_least"]
    # the lattices differ between the pairs (their half ranges come from both maps), so the pairs have different numbers of candidates
    assert len({r["candidates"] for r in ref}) >= 3
    # a repeated pair is the same pair: same reference
    assert ref[0]["best_index"] == ref[6]["best_index"] and ref[0]["best_index"] != ref[1]["best_index"]


def test_tie_case_has_equal_maxima_far_apart():
    for name, case in lc.tie_lists().items():
        ref = lc.list_reference(case)
        for k in case["tie_at"]:
            got = lc.tie_edges(ref[k])
            for key, want in case["edges"].items():
                assert got[key] == want, (name, key, got)
            assert ref[k]["best_index"] == got["first"] and got["n_tied"] >= 16
    heavy = lc.list_reference(lc.tie_lists()["between_heavy"])
    # "heavy": many times the tie pair's candidates x distance tests, so the tie pair's share of workgroups shrinks to a few
    assert heavy[0]["candidates"] * 64 * 16 > 100 * heavy[1]["candidates"]


@pytest.mark.parametrize("ig", [0, 1])
def test_chunk_cases_have_64_65_128_query_objects(ig):
    case = lc.chunk_list(ig)
    assert [len(case["maps"][b]) for _, b in case["pairs"]] == case["edges"]["nq"] == [64, 65, 128]
    ref = lc.list_reference(case)
    for r, (a, b) in zip(ref, case["pairs"]):
        assert r["candidates"] > 0 and r["max_count"] > 0 and len(np.unique(r["counts"])) > 2
        L = pc.bucket_layout(lc.centre(case["maps"][a])[0], lc.centre(case["maps"][b])[0])
        assert len(L["chunks"]) == (len(case["maps"][b]) + 63) // 64


@pytest.mark.parametrize("ig", [0, 1])
def test_status_list_is_what_it_claims(ig):
    case = lc.status_list(ig)
    e, x = case["edges"], case["expect"]
    assert e["capacity_nr"] == pc.bucketed_max_nr(3, ig) and len(case["maps"][0]) == e["capacity_nr"] and len(case["maps"][2]) == e["capacity_nr"] + 1
    assert np.array_equal(case["maps"][2][:-1], case["maps"][0])                    # the same map with one object more
    assert e["image_bytes_at"] <= pc.LDS_BYTES < e["image_bytes_over"]             # one object over the 150 KiB rule
    assert e["image_bytes_at"] > 100 * lc.lds_image_bytes(5, 3, ig)                # beside images of a few hundred bytes
    ref = lc.list_reference(case)
    assert sorted(x["gated"] + x["empty_lattice"] + x["capacity"] + x["live"]) == list(range(len(case["pairs"])))
    for k, r in enumerate(ref):
        assert r["gated"] == (k in x["gated"]), k
    for k in x["empty_lattice"]:
        assert ref[k]["lat"]["n"] == 0 and ref[k]["candidates"] == 0 and ref[k]["best_index"] == -1
    for k in x["live"] + x["capacity"]:
        assert ref[k]["candidates"] > 0
    for k in x["at_capacity"] + x["capacity"]:
        assert ref[k]["candidates"] == 49                                          # place_cases.capacity_case's lattice
    assert set(x["at_capacity"]) <= set(x["live"])
    for k in x["at_capacity"]:
        assert ref[k]["max_count"] >= case["params"]["min_num_inliers"]            # the pair at capacity is found


# ---- the host side of the call -----------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _raw(maps, pairs, n_pairs=None, n_maps=None, off=None, null=(), params=None):
    """the list form through ctypes with every argument under the test's control; outputs start as sentinels"""
    flat = np.ascontiguousarray(np.concatenate(maps, axis=0))
    if off is None:
        off = np.concatenate([[0], np.cumsum([len(m) for m in maps])])
    off = np.ascontiguousarray(off, dtype=np.int32)
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    k = max(len(pr), 1)
    out = dict(tf=np.full((k, 16), 7.0), inliers=np.full(k, 7, np.int32), xyzyaw=np.full((k, 4), 7.0), found=np.full(k, 7, np.int32),
               best_index=np.full(k, 7, np.int64), candidates=np.full(k, 7, np.int64), status=np.full(k, 7, np.int32))
    args = dict(maps7=_p(flat), map_off=_p(off), pairs=_p(pr), **{n: _p(a) for n, a in out.items()})
    for name in null:
        args[name] = None
    p = params or s.place_default_params()
    rc = s.lib().slide_find_inter_loop_closures(args["maps7"], args["map_off"], C.c_int(len(maps) if n_maps is None else n_maps), args["pairs"],
                                                C.c_int(len(pr) if n_pairs is None else n_pairs), C.byref(p), args["tf"], args["inliers"],
                                                args["xyzyaw"], args["found"], args["best_index"], args["candidates"], args["status"])
    return rc, out


def _untouched(out):
    return all((a == 7).all() for a in out.values())


def _small(n, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((n, 7))
    m[:, 0] = 1
    m[:, 1:3] = rng.uniform(-5, 5, (n, 2))
    return m


def test_declaration_is_exported_and_documented():
    assert hasattr(s.lib(), "slide_find_inter_loop_closures") and "slide_find_inter_loop_closures" in api.EXPORTS
    assert callable(s.find_inter_loop_closures)
    header = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    at = header.index("int slide_find_inter_loop_closures(")
    comment = header[header.rindex("/*", 0, at):at]
    assert "sloamNode.cpp:600-694" in comment and "place_recognition.cpp:498-538" in comment and "SLIDE_PLACE_PLAIN" in comment


def test_whole_call_refusals_write_nothing():
    a, b = _small(2, 1), _small(2, 2)
    gate = s.place_default_params(min_num_map_objects_to_start=3)      # (a call that were NOT refused would need no device)
    rc, out = _raw([a, b], [(0, 1)], params=gate)
    assert rc == api.SLIDE_OK and not _untouched(out)
    cases = {
        "n_pairs < 0": dict(n_pairs=-1),
        "n_maps < 0": dict(n_maps=-1),
        "pairs NULL": dict(null=("pairs",)),
        "map_off NULL": dict(null=("map_off",)),
        "maps7 NULL": dict(null=("maps7",)),
        "tf NULL": dict(null=("tf",)),
        "inliers NULL": dict(null=("inliers",)),
        "found NULL": dict(null=("found",)),
        "decreasing map_off": dict(off=[0, 3, 2]),
        "negative map_off": dict(off=[-1, 2, 4]),
    }
    for what, kw in cases.items():
        rc, out = _raw([a, b], [(0, 1)], params=gate, **kw)
        assert rc == INVALID and _untouched(out), what
    for bad in ((0, 2), (2, 0), (-1, 1), (0, -1)):
        rc, out = _raw([a, b], [(0, 1), bad], params=gate)
        assert rc == INVALID and _untouched(out), bad
    # best_index, n_candidates, xyzyaw4n and status may be NULL
    rc, out = _raw([a, b], [(0, 1)], params=gate, null=("best_index", "candidates", "xyzyaw", "status"))
    assert rc == api.SLIDE_OK and out["found"][0] == 0 and out["inliers"][0] == 0 and np.array_equal(out["tf"][0].reshape(4, 4), np.eye(4))
    assert all((out[n] == 7).all() for n in ("best_index", "candidates", "xyzyaw", "status"))
    with pytest.raises(Exception):
        s.find_inter_loop_closures([a, b], [(0, 2)], gate)


def test_empty_list_is_ok_without_a_device():
    rc, out = _raw([_small(4, 3)], [], n_pairs=0)
    assert rc == api.SLIDE_OK and _untouched(out)
    rc = s.lib().slide_find_inter_loop_closures(None, None, C.c_int(0), None, C.c_int(0), None, None, None, None, None, None, None, None)
    assert rc == api.SLIDE_OK
    assert s.find_inter_loop_closures([_small(4, 3)], [], s.place_default_params()) == []


def test_gated_pairs_never_reach_the_device():
    """min_num_map_objects_to_start and empty maps are decided on the host: here, where no device exists, such a list is answered."""
    maps = [_small(2, 4), _small(5, 5), np.zeros((0, 7))]
    res = s.find_inter_loop_closures(maps, [(0, 1), (1, 0), (1, 2), (2, 1), (2, 2)], s.place_default_params(min_num_map_objects_to_start=3))
    assert len(res) == 5
    for r in res:
        assert set(r) == {"found", "tf", "inliers", "xyzyaw", "status", "best_index", "candidates"}
        assert r["found"] is False and r["status"] == 0 and r["inliers"] == 0 and r["best_index"] == -1 and r["candidates"] == 0
        assert np.array_equal(r["tf"], np.eye(4)) and np.array_equal(r["xyzyaw"], np.zeros(4))
    # the default gate (1) still stops an empty map
    res = s.find_inter_loop_closures(maps, [(1, 2), (2, 1)], s.place_default_params())
    assert [r["found"] for r in res] == [False, False] and [r["status"] for r in res] == [0, 0]
