"""The duplicate-landmark queries (slide_graph_landmark_pair_mahalanobis / _get_landmark_pair_covariances / slide_pairs_within /
slide_graph_landmark_pairs_within): what can be checked without a device — the symbols and the header's words, the Python and adaptor
names, and the argument refusals, which are decided on the host before the graph handle or the device is looked at.  No graph handle
can be made without a device, so the refusals are provoked with a NULL handle (test_closure_gate_host.py's pattern): a call whose
arguments are good is refused FOR the handle, a call with a bad argument for that argument, whatever the handle — slide_last_error
says which.  The case generator's own assertions (tests/landmark_pair_cases.py) and its numpy restatement of the device's Schur route
run here too.  Everything that needs the factor is in test_gpu_landmark_pairs.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import slide_slam_amd as s

import landmark_pair_cases as lp
import observation_gate_cases as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["slide_graph_landmark_pair_mahalanobis", "slide_graph_get_landmark_pair_covariances", "slide_pairs_within",
       "slide_graph_landmark_pairs_within"]
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
INVALID = -1


def test_new_symbols_declared_exported_and_documented():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = s.lib()
    for f in NEW:
        assert re.search(r"\bint\s+" + f + r"\s*\(", code), f
        assert hasattr(L, f), f
        assert f in s.api.EXPORTS
    comments = " ".join(re.findall(r"/\*.*?\*/", txt, flags=re.S))
    doc = comments[comments.index("Duplicate landmarks"):]
    assert "jointMarginalCovariance" in doc and "selected inverse" in doc and "forward substitution" in doc
    assert "Cubes are refused" in doc and "SLIDE_LM_PAIR_SUBSTITUTE" in doc
    for name in ("landmark_pairs_within", "landmark_pair_mahalanobis", "get_landmark_pair_covariances", "duplicate_landmarks"):
        assert callable(getattr(s.SlideGraph, name)), name
    assert callable(s.pairs_within) and callable(s.api.pairs_within)
    adaptor = open(os.path.join(ROOT, "include", "slide_sloam_adaptor.hpp")).read()
    assert "landmarkPairMahalanobis" in adaptor and "jointLandmarkCovariance" in adaptor and "findDuplicateLandmarks" in adaptor


def _arrays(good, change):
    a = {k: (None if v is None else v.copy()) for k, v in good.items()}
    for k, v in change.items():
        if v is None:
            a[k] = None
        else:
            v(a[k])
    return a


def test_pair_test_argument_refusals_come_before_the_graph_and_write_nothing():
    good = dict(cls=np.array([2, 0, 2], np.int32), ia=np.array([0, 6, 3], np.uint64), ib=np.array([100, 106, 103], np.uint64),
                s3=np.full(3, 0.05), s7=np.full(7, 0.02))

    def refused(why, n=3, d2_null=False, **change):
        a = _arrays(good, change)
        d2, dof, Cm, r = np.full(3, 77.0), np.full(3, 77, np.int32), np.full((3, 81), 77.0), np.full((3, 9), 77.0)
        route, st = np.full(3, 77, np.int32), np.full(3, 77, np.int32)
        rc = s.lib().slide_graph_landmark_pair_mahalanobis(None, C.c_int(n), P(a["cls"]), P(a["ia"]), P(a["ib"]), P(a["s3"]), P(a["s7"]),
                                                           None if d2_null else P(d2), P(dof), P(Cm), P(r), P(route), P(st))
        assert rc == INVALID, (change, rc)
        err = s.api.last_error()
        assert "landmark_pair_mahalanobis" in err and why in err, (change, err)
        assert (d2 == 77).all() and (dof == 77).all() and (Cm == 77).all() and (r == 77).all() and (route == 77).all() and (st == 77).all()

    def put(i, v):
        def f(a):
            a[i] = v
        return f
    refused("the graph is NULL")                                        # good arguments: only the handle is wrong
    for name in good:
        refused("pointer is NULL", **{name: None})
    refused("pointer is NULL", d2_null=True)
    refused("n < 0", n=-1)
    refused("neither SLIDE_CLS_ELLIPSOID nor SLIDE_CLS_CYLINDER", cls=put(1, 1))      # a cube
    refused("neither SLIDE_CLS_ELLIPSOID nor SLIDE_CLS_CYLINDER", cls=put(2, 7))
    refused("neither SLIDE_CLS_ELLIPSOID nor SLIDE_CLS_CYLINDER", cls=put(0, -1))
    for bad in (0.0, -0.05, np.nan, np.inf):
        refused("sigma that is non-finite or <= 0", s3=put(1, bad))
        refused("sigma that is non-finite or <= 0", s7=put(6, bad))


def test_pair_covariance_argument_refusals_come_before_the_graph_and_write_nothing():
    good = dict(cls=np.array([2, 1], np.int32), ia=np.array([0, 3], np.uint64), ib=np.array([100, 9], np.uint64))

    def refused(why, n=2, out_null=False, **change):
        a = _arrays(good, change)
        out, route, st = np.full((2, 324), 77.0), np.full(2, 77, np.int32), np.full(2, 77, np.int32)
        rc = s.lib().slide_graph_get_landmark_pair_covariances(None, C.c_int(n), P(a["cls"]), P(a["ia"]), P(a["ib"]),
                                                               None if out_null else P(out), P(route), P(st))
        assert rc == INVALID, (change, rc)
        err = s.api.last_error()
        assert "get_landmark_pair_covariances" in err and why in err, (change, err)
        assert (out == 77).all() and (route == 77).all() and (st == 77).all()

    def cls3(a):
        a[1] = 3
    refused("the graph is NULL")                                        # (a cube pair among them: every class is served)
    for name in good:
        refused("pointer is NULL", **{name: None})
    refused("pointer is NULL", out_null=True)
    refused("n < 0", n=-1)
    refused("not a landmark class", cls=cls3)


def test_search_argument_refusals_write_nothing():
    xyz = np.zeros((4, 3))

    def refused(why, n=4, radius=1.0, cap=8, xyz_null=False, null=()):
        oi, oj, dist, tot = np.full(8, 77, np.int32), np.full(8, 77, np.int32), np.full(8, 77.0), np.full(1, 77, np.int64)
        outs = {"i": oi, "j": oj, "d": dist, "n": tot}
        ptr = {k: (None if k in null else P(v)) for k, v in outs.items()}
        rc = s.lib().slide_pairs_within(None if xyz_null else P(xyz), None, C.c_int(n), C.c_double(radius), C.c_int64(cap), ptr["i"], ptr["j"],
                                        ptr["d"], ptr["n"])
        assert rc == INVALID, (why, rc)
        err = s.api.last_error()
        assert "pairs_within" in err and why in err, err
        assert (oi == 77).all() and (oj == 77).all() and (dist == 77).all() and (tot == 77).all()

    refused("n < 0", n=-1)
    refused("cap < 0", cap=-1)
    refused("pointer is NULL", xyz_null=True)
    for k in "ijdn":
        refused("pointer is NULL", null=(k,))
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused("radius that is non-finite or <= 0", radius=bad)


def test_graph_search_argument_refusals_come_before_the_graph_and_write_nothing():
    sel = np.array([0, 3, 6], np.uint64)

    def refused(why, cls=2, radius=0.75, n_sel=3, cap=8, null=()):
        ia, ib, dist, tot = np.full(8, 77, np.uint64), np.full(8, 77, np.uint64), np.full(8, 77.0), np.full(1, 77, np.int64)
        outs = {"a": ia, "b": ib, "d": dist, "n": tot}
        ptr = {k: (None if k in null else P(v)) for k, v in outs.items()}
        rc = s.lib().slide_graph_landmark_pairs_within(None, C.c_int(cls), C.c_double(radius), C.c_int(n_sel), P(sel), None, C.c_int64(cap),
                                                       ptr["a"], ptr["b"], ptr["d"], ptr["n"])
        assert rc == INVALID, (why, rc)
        err = s.api.last_error()
        assert "landmark_pairs_within" in err and why in err, err
        assert (ia == 77).all() and (ib == 77).all() and (dist == 77).all() and (tot == 77).all()

    refused("the graph is NULL")
    refused("not a landmark class", cls=3)
    refused("n < 0", n_sel=-1)
    refused("cap < 0", cap=-1)
    for k in "abdn":
        refused("pointer is NULL", null=(k,))
    for bad in (0.0, -0.5, np.nan, np.inf):
        refused("radius that is non-finite or <= 0", radius=bad)


@pytest.mark.parametrize("chart", [0, 1])
def test_generator_holds_its_own_conditions(chart):
    """dup40 asserts on itself under d2_ref alone (landmark_pair_cases.planted): every true pair below 0.25 of the 0.99 quantile of its
    D, every distinct pair above 1.5 of it — while the true revisit pair lies as far apart as the distinct pairs do."""
    c = lp.case("dup40", chart)
    for kind, n_true, n_all in (("point", 13, 37), ("cylinder", 6, 18)):
        pairs, flags, d2, dist = lp.planted(c, kind)
        assert len(pairs) == n_all and flags.sum() == n_true
        print(f"[lm-pairs] chart {chart} {kind}: true d2 <= {d2[flags].max():.3g} at <= {dist[flags].max():.3g} m, distinct d2 >= "
              f"{d2[~flags].min():.3g} at {dist[~flags].min():.3g} .. {dist[~flags].max():.3g} m")
    pairs, flags, d2, dist = lp.planted(c, "point")
    k = int(np.flatnonzero((pairs == np.array(lp.REVISIT, np.uint64)).all(axis=1))[0])
    assert flags[k] and dist[k] > 0.8 * dist[~flags].min()      # (distance cannot tell the revisit from a distinct object)


@pytest.mark.parametrize("chart", [0, 1])
def test_schur_route_restated_in_numpy_equals_the_reference(chart):
    """C by the device's route — Hinv, F = E Hinv, B over the reduced pose system — against C_ref off the dense inverse."""
    c = lp.case("dup40", chart)
    for kind in ("point", "cylinder"):
        pairs, _, _, _ = lp.planted(c, kind)
        _, Cs, _ = lp.ref_pairs(c, kind, pairs, c.cpu_values)
        for (a, b), C_ref in zip(pairs, Cs):
            Cm = lp.schur_form(c, kind, a, b)
            err = float(np.abs(Cm - C_ref).max() / np.abs(C_ref).max())
            assert err <= og.gate_bound(c, C_ref), (kind, a, b, err)
