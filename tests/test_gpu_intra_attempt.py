"""slide_intra_loop_closure_attempt on the GPU: one attempt of SLOAMNode::intraLoopClosureThread_ over a list of candidate key poses
equals slide_keypose_submaps followed by slide_find_intra_loop_closures bit for bit, and with the list cut to the one candidate
getLoopCandidateIdx returns it is the reference's own attempt: numpy extraction plus the existing single call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intra_list_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("found", "tf", "inliers", "xyzyaw", "status", "best_index", "candidates")


@pytest.fixture(scope="module")
def attempt(gpu):
    case = ic.attempt_case()
    idx, n = gpu.loop_candidate_list(case["cloud"], 12.0, len(case["cloud"]) - 1, 30)
    assert n >= 8 and idx[0] == gpu.loop_candidate_idx(case["cloud"], 12.0, len(case["cloud"]) - 1, 30)
    # every candidate, then the first again and a key pose far above the map (an empty submap)
    poses = np.concatenate([ic.key_pose7(case["cloud"], idx), ic.key_pose7(case["cloud"], idx[:1]), [[0.1, 0.2, 50.3, 0, 0, 0, 1.0]]])
    gp = gpu.place_default_params(**case["params"])
    return case, gp, idx, poses


def test_attempt_equals_the_two_calls(gpu, attempt):
    case, gp, idx, poses = attempt
    tabs = ic.tables_args(case["tables"])
    got = gpu.intra_loop_closure_attempt(*tabs, case["meas"], case["query_pose"], poses, case["radius"], gp, max_dz=case["max_dz"])
    sub = gpu.keypose_submaps(*tabs, poses[:, :3], case["radius"], case["max_dz"])
    off = sub["sub_off"]
    two = gpu.find_intra_loop_closures(case["meas"], case["query_pose"], [sub["rows"][off[k]:off[k + 1]] for k in range(len(poses))], poses, gp)
    assert len(got) == len(two) == len(poses)
    print("submap sizes", [r["submap_size"] for r in got], "found", [r["found"] for r in got], "inliers", [r["inliers"] for r in got])
    assert [r["submap_size"] for r in got] == list(np.diff(off))
    for a, b in zip(got, two):
        assert all(np.array_equal(a[k], b[k]) for k in KEYS)
    assert got[-1]["submap_size"] == 0 and not got[-1]["found"] and got[-1]["candidates"] == 0
    assert all(np.array_equal(got[0][k], got[len(idx)][k]) for k in KEYS)
    assert sum(r["found"] for r in got) >= 2 and min(r["submap_size"] for r in got[:-1]) > 20


def test_first_candidate_alone_is_the_reference_s_attempt(gpu, attempt):
    case, gp, idx, poses = attempt
    first = gpu.loop_candidate_idx(case["cloud"], 12.0, len(case["cloud"]) - 1, 30)
    pose = ic.key_pose7(case["cloud"], [first])
    got = gpu.intra_loop_closure_attempt(*ic.tables_args(case["tables"]), case["meas"], case["query_pose"], pose, case["radius"], gp, max_dz=case["max_dz"])[0]
    ref = ic.submaps_reference(case["tables"], pose[:, :3], case["radius"], case["max_dz"])
    away = np.logical_and(np.abs(ref["dist"] - case["radius"]) > ic.MARGIN, np.abs(ref["dzs"] - case["max_dz"]) > ic.MARGIN)
    assert away.all()                                                       # a condition of the case: no object on a threshold
    one = gpu.find_intra_loop_closure(case["meas"], ref["rows"], case["query_pose"], pose[0], gp)
    assert got["submap_size"] == len(ref["rows"]) and got["found"] == one["found"] and got["inliers"] == one["inliers"]
    assert one["found"] and np.array_equal(got["tf"], one["tf"]) and np.array_equal(got["xyzyaw"], one["xyzyaw"])
