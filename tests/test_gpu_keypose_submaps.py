"""slide_keypose_submaps on the GPU: the submaps around a list of key poses (getkeyPoseSubmap of the three map managers +
prepareLCInput) equal the numpy restatement of tests/intra_list_cases.py exactly — offsets, source indices and rows — at class sizes
that straddle the kernel's chunk (256) and wave (64) edges, with objects exactly on both thresholds and poses that are no float32."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import intra_list_cases as ic  # noqa: E402

from slide_slam_amd.api import SLIDE_ERR_CAPACITY as CAPACITY  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(gpu, case, poses=None, **kw):
    poses = case["poses"] if poses is None else poses
    return gpu.keypose_submaps(*ic.tables_args(case["tables"]), poses, case["radius"], case["max_dz"], **kw)


@pytest.mark.parametrize("i", range(10))
def test_submaps_equal_the_numpy_restatement(gpu, i):
    case = ic.submap_cases()[i]
    ref = case["ref"]
    got = _run(gpu, case)
    print(f"case {i} sizes {case['edges']['sizes']}: {got['n_rows']} rows over {len(case['poses'])} poses, boundaries {case['edges']['boundaries']}")
    assert got["status"] == 0 and got["n_rows"] == ref["sub_off"][-1]
    assert np.array_equal(got["sub_off"], ref["sub_off"])
    assert np.array_equal(got["src_idx"], ref["src_idx"])
    assert np.array_equal(got["rows"], ref["rows"])
    off = got["sub_off"]
    assert off[3] == off[2]                                                     # the far pose: an empty segment
    a, b = slice(off[1], off[2]), slice(off[32], off[33])                       # the same pose listed twice
    assert np.array_equal(got["rows"][a], got["rows"][b]) and np.array_equal(got["src_idx"][a], got["src_idx"][b])
    if sum(case["edges"]["sizes"]):
        assert off[2] > off[1]
    else:
        assert got["n_rows"] == 0 and not off.any()


@pytest.mark.parametrize("i", [2, 5, 8])
def test_one_pose_alone_has_the_bits_it_has_in_the_list(gpu, i):
    case = ic.submap_cases()[i]
    many = _run(gpu, case)
    for k in (0, 1, 2, 17):
        one = _run(gpu, case, poses=case["poses"][k:k + 1])
        seg = slice(many["sub_off"][k], many["sub_off"][k + 1])
        assert one["status"] == 0 and one["n_rows"] == seg.stop - seg.start
        assert np.array_equal(one["rows"], many["rows"][seg]) and np.array_equal(one["src_idx"], many["src_idx"][seg])


def test_capacity_one_short(gpu):
    case = ic.submap_cases()[8]
    ref = case["ref"]
    n = int(ref["sub_off"][-1])
    assert n > 1
    got = _run(gpu, case, capacity=n - 1)
    assert got["status"] == CAPACITY and got["n_rows"] == n and np.array_equal(got["sub_off"], ref["sub_off"]) and len(got["rows"]) == 0
    exact = _run(gpu, case, capacity=n)
    assert exact["status"] == 0 and np.array_equal(exact["rows"], ref["rows"])
    no_src = _run(gpu, case, with_src=False)                                    # src_idx may be NULL
    assert no_src["status"] == 0 and no_src["src_idx"] is None and np.array_equal(no_src["rows"], ref["rows"])


def test_max_dz_is_a_parameter(gpu):
    case = dict(ic.submap_cases()[5])
    case["max_dz"] = 0.75
    ref = ic.submaps_reference(case["tables"], case["poses"][3:], case["radius"], 0.75)
    away = np.abs(ref["dzs"] - 0.75) > ic.MARGIN
    assert away.all() and ref["sub_off"][-1] < ic.submap_cases()[5]["ref"]["sub_off"][-1]
    got = _run(gpu, case, poses=case["poses"][3:])
    assert np.array_equal(got["sub_off"], ref["sub_off"]) and np.array_equal(got["src_idx"], ref["src_idx"]) and np.array_equal(got["rows"], ref["rows"])
