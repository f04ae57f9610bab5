"""Selecting the mutually consistent subset of a list of loop closures (slide_closure_consistency_csr,
slide_select_consistent_closures, slide_graph_select_closures): what can be checked without a device — the symbols and the header's
words, the defaults, every whole-call refusal (reached on the host, outputs untouched), canonicalisation and grouping on hand-written
closures, the case generators' own checks and the symmetry rule of the restatement (tests/closure_cases.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import slide_slam_amd as s

import closure_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["slide_closure_consistency_csr", "slide_select_consistent_closures", "slide_graph_select_closures"]
I7 = [0.0, 0, 0, 0, 0, 0, 1]


def test_new_symbols_declared_exported_and_documented():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = s.lib()
    for f in NEW + ["slide_closure_canonicalize"]:
        assert re.search(r"\bint\s+" + f + r"\s*\(", code), f
        assert hasattr(L, f), f
        assert f in s.api.EXPORTS
    assert re.search(r"\bvoid\s+slide_closure_default_params\s*\(", code) and "slide_closure_default_params" in s.api.EXPORTS
    # the header says what the reference does instead, and what a closure means
    comments = " ".join(re.findall(r"/\*.*?\*/", txt, flags=re.S))
    assert "sloamNode.cpp:448-476" in comments and "graphWrapper.cpp:55" in comments
    assert "X_from^-1 X_to" in comments and "[rot(3), trans(3)]" in comments
    for f in ("closure_params", "closure_consistency_csr", "select_consistent_closures", "closure_canonicalize"):
        assert callable(getattr(s, f))
    assert callable(s.SlideGraph.select_closures)
    adaptor = open(os.path.join(ROOT, "include", "slide_sloam_adaptor.hpp")).read()
    assert "selectConsistentClosures" in adaptor


def test_defaults():
    p = s.closure_params()
    assert p.gate ** 2 == pytest.approx(16.81) and p.sigma == p.gate / 2
    assert p.affinityeps == 1e-4 and p.min_set == 1 and list(p.odom_sigma6) == [0.1] * 6
    assert (cc.GATE, cc.SIGMA, cc.AFFINITYEPS) == (p.gate, p.sigma, p.affinityeps)


def _raw_select(L, fr, fi, tr, ti, rel, sg, fp, tp, p, keep, ng):
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return s.lib().slide_select_consistent_closures(C.c_int(L), P(fr), P(fi), P(tr), P(ti), P(rel), P(sg), P(fp), P(tp),
                                                    C.byref(p) if p is not None else None, None, None, P(keep), None, None, None, None,
                                                    C.byref(ng) if ng is not None else None, None, None, None, None, C.c_longlong(0), None)


def test_whole_call_refusals_need_no_device_and_write_nothing():
    """Three closures of one group would reach the device; every refusal below comes back SLIDE_ERR_INVALID first, with keep and
    n_groups as they were."""
    good = dict(fr=np.zeros(3, np.int32), fi=np.array([40, 41, 42], np.uint64), tr=np.zeros(3, np.int32), ti=np.array([1, 2, 3], np.uint64),
                rel=np.tile(I7, (3, 1)), sg=np.full((3, 6), 0.1), fp=np.tile(I7, (3, 1)), tp=np.tile(I7, (3, 1)))

    def refused(L=3, p=None, ng_null=False, **change):
        a = {k: v.copy() for k, v in good.items()}
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                v(a[k])
        keep, ng = np.full(3, 77, np.int32), C.c_int(55)
        rc = _raw_select(L, a["fr"], a["fi"], a["tr"], a["ti"], a["rel"], a["sg"], a["fp"], a["tp"], p, keep, None if ng_null else ng)
        assert rc == -1, (change, rc)                                  # SLIDE_ERR_INVALID
        assert "closure selection" in s.api.last_error()
        assert keep.tolist() == [77] * 3 and ng.value == 55

    for name in good:
        refused(**{name: None})                                        # every needed pointer
    refused(ng_null=True)
    refused(L=-1)

    def put(i, j, v):
        def f(a):
            a[i, j] = v
        return f
    refused(rel=put(1, 0, np.nan))
    refused(rel=put(2, 6, np.inf))
    refused(fp=put(0, 2, np.nan))
    refused(tp=put(0, 2, -np.inf))
    refused(sg=put(1, 3, np.nan))
    refused(sg=put(1, 3, 0.0))                                          # a sigma <= 0
    refused(sg=put(2, 0, -0.1))

    def zero_quat(a):
        a[0, 3:] = 0.0
    refused(rel=zero_quat)

    def robot(a):
        a[1] = 13
    refused(fr=robot)
    for kw in (dict(gate=0.0), dict(gate=-1.0), dict(sigma=0.0), dict(sigma=float("nan")), dict(affinityeps=-1.0), dict(min_set=-1),
               dict(odom_sigma6=[0.1, 0.1, 0.0, 0.1, 0.1, 0.1])):
        refused(p=s.closure_params(**kw))
    # the same decisions in the other two calls
    rowptr, nnz = np.full(4, 9, np.int32), C.c_longlong(5)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = good["sg"].copy(); bad[0, 0] = 0.0
    rc = s.lib().slide_closure_consistency_csr(P(good["fp"]), P(good["tp"]), P(good["rel"]), P(bad), P(good["fi"]), P(good["ti"]), C.c_int(3), None,
                                               P(rowptr), None, None, C.c_longlong(0), C.byref(nnz))
    assert rc == -1 and rowptr.tolist() == [9] * 4 and nnz.value == 5
    keep, ng = np.full(3, 77, np.int32), C.c_int(55)
    rc = s.lib().slide_graph_select_closures(None, C.c_int(3), P(good["fr"]), P(good["fi"]), P(good["tr"]), P(good["ti"]), P(good["rel"]), P(good["sg"]),
                                             None, None, P(keep), None, None, None, None, C.byref(ng))
    assert rc == -1 and keep.tolist() == [77] * 3 and ng.value == 55


def test_lone_closures_and_empty_lists_are_answered_on_the_host():
    """A group of one closure never reaches the device: a list of lone closures is answered on a machine without one."""
    out = s.select_consistent_closures([], np.zeros((0, 7)), np.zeros((0, 7)))
    assert len(out["keep"]) == 0 and len(out["score"]) == 0
    cl = [(2, 7, 1, 3, I7, 0.1), (0, 1, 0, 9, I7, 0.1), (0, 5, 2, 6, I7, 0.1)]
    out = s.select_consistent_closures(cl, np.tile(I7, (3, 1)), np.tile(I7, (3, 1)))
    assert out["group"].tolist() == [2, 0, 1]                          # (1, 2) after the flip, (0, 0), (0, 2)
    assert out["keep"].tolist() == [True] * 3 and out["n_selected"].tolist() == [1] * 3 and out["score"].tolist() == [1.0] * 3
    out = s.select_consistent_closures(cl, np.tile(I7, (3, 1)), np.tile(I7, (3, 1)), params=s.closure_params(min_set=2))
    assert out["keep"].tolist() == [False] * 3 and out["n_selected"].tolist() == [1] * 3
    rowptr, col, val = s.closure_consistency_csr([I7], [I7], [I7], [[0.1] * 6], [4], [1])
    assert rowptr.tolist() == [0, 0] and len(col) == 0 and len(val) == 0


def test_canonicalisation_and_grouping():
    q = np.array([0.1, -0.2, 0.3, 0.9])
    q /= np.linalg.norm(q)
    rel = np.concatenate([[1.0, -2.0, 0.5], q])
    R, t = cc._pose(rel, np.float64)
    inv = cc.p7((R.T, -(R.T @ t)))
    shift = [1.0, 2.0, 3.0, 0, 0, 0, 1]
    cl = [(1, 50, 0, 3, rel, 0.1),          # 0: inter, flipped
          (0, 3, 1, 50, inv, 0.1),          # 1: its unflipped twin
          (0, 40, 0, 2, rel, 0.1),          # 2: same robot, late -> early
          (0, 2, 0, 40, inv, 0.1),          # 3: same robot, early -> late: not reordered
          (2, 9, 2, 1, rel, 0.1),           # 4: another robot
          (2, 5, 0, 6, shift, 0.1),         # 5: (0, 2) after the flip; identity rotation: the inverse is exact
          (1, 8, 1, 0, rel, 0.1)]           # 6
    o = s.closure_canonicalize(cl)
    assert o["flipped"].tolist() == [1, 0, 0, 0, 0, 1, 0]
    assert o["from_robot"].tolist() == [0, 0, 0, 0, 2, 0, 1] and o["to_robot"].tolist() == [1, 1, 0, 0, 2, 2, 1]
    assert o["from_idx"].tolist() == [3, 3, 40, 2, 9, 6, 8] and o["to_idx"].tolist() == [50, 50, 2, 40, 1, 5, 0]
    # groups by ascending (from_robot, to_robot): (0,0) (0,1) (0,2) (1,1) (2,2); rows stable within a group
    assert o["n_groups"] == 5 and o["group"].tolist() == [1, 1, 0, 0, 4, 2, 3]
    assert o["order"].tolist() == [2, 3, 0, 1, 6, 4, 5]
    # an untouched closure keeps its bits; the flipped one equals its twin (the twin's rel went through one more quaternion round
    # trip on the way in: a few ulp), exactly so where the inverse is exact
    for k in (1, 2, 3, 4, 6):
        assert np.array_equal(o["rel7"][k], np.asarray(cl[k][4], float))
    assert np.abs(o["rel7"][0] - o["rel7"][1]).max() < 1e-15
    assert o["rel7"][5].tolist() == [-1.0, -2.0, -3.0, 0, 0, 0, 1]
    # a permuted list: the same groups, each closure in its group
    perm = [4, 6, 0, 5, 3, 1, 2]
    o2 = s.closure_canonicalize([cl[k] for k in perm])
    assert o2["n_groups"] == 5 and o2["group"].tolist() == [o["group"][k] for k in perm]


def test_generators_hold_their_own_conditions():
    """Building a case runs its three self-checks (no d at the gate, no score at affinityeps, the oracle's CLIPPER selects exactly the
    planted set on the restatement's matrix)."""
    for inter in (False, True):
        c = cc.planted_case(1, inter=inter)
        t = c.truth
        assert t.sum() == 8 and len(c) == 12
        tt = c.d[np.ix_(t, t)][~np.eye(8, dtype=bool)]
        assert tt.max() < cc.GATE / 2 and c.d[np.ix_(t, ~t)].min() > 2 * cc.GATE and c.d[np.ix_(~t, ~t)][~np.eye(4, dtype=bool)].min() > 2 * cc.GATE
    for L in cc.CSR_SHAPES:
        c = cc.csr_case(L, inter=L in (5, 64))
        assert len(c) == L
        if L >= 63:              # distances on both sides of the gate
            off = ~np.eye(L, dtype=bool)
            assert (c.d[off] < cc.GATE).any() and (c.d[off] > cc.GATE).any()


def test_restatement_is_symmetric_only_with_the_smaller_index_first():
    c = cc.csr_case(5, inter=True)
    assert np.array_equal(c.M, c.M.T) and np.array_equal(c.d, c.d.T)
    d2, _ = cc.restate(*c.arrays(), smaller_first=False)
    assert not np.array_equal(d2, d2.T)
    assert np.array_equal(np.triu(d2), np.triu(c.d))                    # above the diagonal the two rules are one evaluation
