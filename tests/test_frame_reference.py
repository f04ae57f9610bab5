"""The frame cases of tests/frame_cases.py and their plain numpy reference, proven on the CPU against the oracle before a GPU sees
them (tests/test_gpu_frame_assoc.py): per frame and per detection the reference's match position, map index and the counts equal
OracleBackend's outside the margin rule, and no detection of a case that was not built to tie falls under the margin."""
import numpy as np
import pytest

import frame_cases as fc
from oracle import pyoracle as po


def _oracle(case):
    ob = po.OracleBackend(po.OrcParams.default(), case.n_robots)
    if case.knn != fc.K_DEFAULT:
        ob.set_knn(*case.knn)
    return ob


def test_oracle_knn_defaults_unchanged():
    """orc_backend_set_knn is an addition: a backend nobody touched still gates with the reference's 50 / 30 / 1000."""
    ob = po.OracleBackend(po.OrcParams.default(), 1)
    assert ob.knn() == (50, 30, 1000) == fc.K_DEFAULT
    ob.set_knn(1, 2, 3)
    assert ob.knn() == (1, 2, 3)
    assert po.OracleBackend(po.OrcParams.default(), 1).knn() == (50, 30, 1000)
    p = po.OrcParams.default()
    assert (p.cyl_thresh, p.cube_thresh, p.ell_thresh) == tuple(fc.THRESH[c] for c in fc.CLS)


def test_default_world_keeps_its_spacing():
    """The margin rule holds by construction: the closest pair of a class is farther apart than the class's threshold plus any noise."""
    w = fc.make_world(11, 120, 80, 1500)
    for c in fc.CLS:
        p = w[c]["pos"]
        d = np.linalg.norm(p[:, None, :2] - p[None, :, :2], axis=2)
        d[np.diag_indices(len(p))] = np.inf
        assert d.min() >= fc.SPACING[c] - 2 * fc.JITTER[c] > fc.THRESH[c] + 0.2, (c, d.min())


@pytest.mark.parametrize("name", list(fc.FOREIGN_CASES))
def test_numpy_reference_equals_oracle(name):
    case = fc.get_case(name)
    res, under = fc.check_against_numpy(_oracle(case), case)
    assert all(r["status"] == 0 for r in res)
    assert under == [], f"{name}: detections under the margin outside the named ties: {under}"
    n_frames = sum(1 for o in case.ops if o["op"] == "frame")
    assert len(res) == n_frames
    if name == "ties":
        for k in (1, 2):
            for c in fc.CLS:
                assert list(res[k][c + "_id"]) == case.expect_id[c], (k, c, res[k][c + "_id"])
                assert (res[k][c + "_match"] >= 0).all()
        # the rank counts only the keys below the winner: the coincident landmark of the other label lies in front of ellipsoid 10
        assert res[1]["ell_match"][3] == res[1]["ell_match"][4] + 1
    if name == "ties_many":
        for k in (1, 2):
            for c in fc.CLS:
                assert list(res[k][c + "_id"]) == case.expect_id and res[k][c + "_match"][3] == 3, (k, c, res[k][c + "_id"], res[k][c + "_match"])
    if name == "gate_tie":
        for k in (1, 2):
            for c in fc.CLS:
                assert list(res[k][c + "_id"]) == case.expect_id[k - 1] and list(res[k][c + "_match"]) == case.expect_match, (k, c)


def test_counted_frames_reach_what_they_are_for():
    """The detection-count cases really contain matches behind a selecting gate, new landmarks, unknown labels and non-trivial ranks."""
    case = fc.get_case("det_counts_40_65_100")
    res = fc.run_case(_oracle(case), case)
    r = res[1]
    assert [len(r[c + "_id"]) for c in fc.CLS] == [40, 65, 100]
    for c, K in zip(fc.CLS, fc.K_DEFAULT):
        m = r[c + "_match"]
        assert (m >= 0).sum() >= 10 and (m == -1).sum() >= 3, (c, m)
        assert m.max() < K and m.max() >= 20, (c, m.max())
    assert (r["cube_match"] >= 0).sum() < 65 - 3                      # cubes behind the K = 30 gate
    for c, n in (("cyl", 120), ("ell", 1500)):                        # landmarks that frame 1 created are matched in frame 2
        assert (res[2][c + "_match"][res[2][c + "_id"] >= n] >= 0).any(), (c, res[2][c + "_id"], res[2][c + "_match"])
    # (cubes have no label gate: an unknown label creates nothing; their new landmarks are matched where the gate does not select)
    case = fc.get_case("knn_K128_n127")
    res = fc.run_case(_oracle(case), case)
    for c in fc.CLS:
        assert (res[2][c + "_match"][res[2][c + "_id"] >= 127] >= 0).any(), (c, res[2][c + "_id"], res[2][c + "_match"])


@pytest.mark.parametrize("name", list(fc.HOST_CASES))
def test_host_cases_run_on_the_oracle(name):
    case = fc.get_case(name)
    ob = _oracle(case)
    ranks_off, seen = [], {}

    def before(k, op, prev):
        # the pose estimate and the models the matcher will see: where a match's rank (cloud order) is not its model-distance order
        if op["mode"] == fc.FRAME_FOREIGN or name != "host_rank":
            return
        seen["maps"], seen["pose"] = fc.read_new_models(ob, fc.empty_maps()), _compose(prev, op["rel7"])

    def after(k, op, r):
        if op["op"] != "frame" or op["mode"] == fc.FRAME_FOREIGN or name != "host_rank" or k == 0:
            return
        ranks_off.append(fc.ranks_off_distance_order(seen["maps"], seen["pose"], r))

    res = fc.run_case(ob, case, before, after)
    assert all(r["status"] == 0 for r in res)
    first = res[0]
    for c in fc.CLS:
        assert (first[c + "_match"] == -1).all() and np.array_equal(first[c + "_id"], np.arange(len(first[c + "_id"])))
    last = res[-1]
    assert sum(int((last[c + "_match"] >= 0).sum()) for c in fc.CLS) >= 20
    if name == "host_rank":
        assert sum(ranks_off) >= 3, ranks_off
    if name == "multi_robot":
        grown = [res[k]["counts"]["point"] for k in (0, 1, 2, 3)]
        assert grown == sorted(grown) and grown[3] > grown[0]


def _compose(a7, b7):
    Ra, ta = fc.pose7_Rt(a7)
    Rb, tb = fc.pose7_Rt(b7)
    return fc.pose7(Ra @ Rb, Ra @ tb + ta)
