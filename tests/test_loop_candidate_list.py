"""slide_loop_candidate_list (host bookkeeping): every key pose that passes getLoopCandidateIdx's test
(cylinderMapManager.cpp:160-184), in slide_loop_candidate_idx's order."""
import numpy as np
import pytest

import slide_slam_amd as s


def _numpy_list(cloud, max_dist, pose_idx, at_least):
    """filter and sort in float32, operation by operation as the library's sibling does; a later pose wraps around (size_t)"""
    n = len(cloud)
    if n < 50:
        return np.zeros(0, np.int64)
    c = cloud.astype(np.float32)
    d = c - c[pose_idx]
    d2 = (d[:, 0] * d[:, 0]).astype(np.float32)
    d2 = (d2 + d[:, 1] * d[:, 1]).astype(np.float32)
    d2 = (d2 + d[:, 2] * d[:, 2]).astype(np.float32)
    idx = np.arange(n, dtype=np.uint64)
    age = np.uint64(pose_idx) - idx                      # wraps for idx > pose_idx
    ok = (d2 < np.float32(max_dist * max_dist)) & (idx != np.uint64(pose_idx)) & (age > np.uint64(at_least))
    keep = np.nonzero(ok)[0]
    return keep[np.lexsort((keep, d2[keep]))].astype(np.int64)


def _clouds():
    rng = np.random.default_rng(21)
    for trial in range(200):
        n = int(rng.integers(30, 300))                   # some below the 50-pose gate
        t = np.linspace(0, rng.uniform(2, 9), n)
        cloud = np.column_stack([20 * np.cos(t), 20 * np.sin(t), 0.1 * t]).astype(np.float32)
        cloud += rng.normal(0, 0.3, cloud.shape).astype(np.float32)
        if trial % 5 == 0:
            cloud[n // 3] = cloud[n // 4]                # exactly equidistant neighbours
            cloud[n // 5] = cloud[n // 4]
        pose_idx = n - 1 if trial % 3 else int(rng.integers(0, n))
        yield trial, cloud, pose_idx


def test_entry_zero_is_loop_candidate_idx_and_the_list_is_numpy_s():
    with np.errstate(over="ignore"):
        seen = dict(short=0, ties=0, several=0, none=0)
        for trial, cloud, pose_idx in _clouds():
            got, n_found = s.loop_candidate_list(cloud, 5.0, pose_idx, 30)
            want = _numpy_list(cloud, 5.0, pose_idx, 30)
            first = s.loop_candidate_idx(cloud, 5.0, pose_idx, 30)
            assert n_found == len(want) == len(got) and np.array_equal(got, want), (trial, len(cloud), pose_idx)
            assert (first is None) == (n_found == 0) and (first is None or first == got[0]), trial
            seen["short"] += len(cloud) < 50
            seen["none"] += n_found == 0
            seen["several"] += n_found > 3
            if n_found > 1:
                d2 = ((cloud[got] - cloud[pose_idx]).astype(np.float32) ** 2).sum(axis=1)
                seen["ties"] += bool((np.diff(d2) == 0).any())
    assert seen["short"] > 5 and seen["ties"] > 3 and seen["several"] > 30 and seen["none"] > 10, seen


def test_cap_truncates_and_n_found_stays_the_full_count():
    for trial, cloud, pose_idx in _clouds():
        full, n = s.loop_candidate_list(cloud, 5.0, pose_idx, 30)
        if n >= 4:
            for cap in (0, 1, n - 1, n, n + 5):
                got, n_found = s.loop_candidate_list(cloud, 5.0, pose_idx, 30, cap=cap)
                assert n_found == n and np.array_equal(got, full[:cap])
            break
    else:
        pytest.fail("no cloud with four candidates")
    line = np.column_stack([0.1 * np.arange(60), np.zeros(60), np.zeros(60)]).astype(np.float32)
    got, n = s.loop_candidate_list(line, 0.35, 10, 30)       # size_t wrap-around: LATER poses qualify, nearest first
    assert list(got) == [11, 12, 13] and n == 3
    with pytest.raises(s.SlideError):
        s.loop_candidate_list(line, 1.0, 60, 30)
    assert "slide_loop_candidate_list" in s.api.EXPORTS
