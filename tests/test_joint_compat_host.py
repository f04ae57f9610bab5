"""The joint-compatibility test of landmark observations (slide_graph_observation_joint_compatibility, slide_chi2_quantile): what can
be checked without a device — the symbols and the header's words, the quantile against scipy, the argument refusals (decided on the
host before the graph handle or the device is looked at, provoked with a NULL handle as test_observation_gate_host.py provokes them),
the route the device takes against the dense reference, and the planted scenarios' figures under the reference alone
(tests/joint_compat_cases.py).  Everything that needs the factor is in test_gpu_joint_compat.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.stats import chi2

import slide_slam_amd as s

import joint_compat_cases as jc
import observation_gate_cases as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "slide_graph_observation_joint_compatibility"
I7 = [0.0, 0, 0, 0, 0, 0, 1]
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
CYL, CUBE, POINT = 0, 1, 2


def test_symbols_declared_exported_and_documented():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in (NAME, "slide_chi2_quantile"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code)
        assert hasattr(s.lib(), name) and name in s.api.EXPORTS
    comments = re.sub(r"[\s*]+", " ", " ".join(re.findall(r"/\*.*?\*/", txt, flags=re.S)))
    for words in ("Neira and Tardos", "X = C_iS L_S^-T", "prob == 0: evaluate only", "SLIDE_ERR_CAPACITY when the served rows exceed",
                  "boost::math::quantile"):
        assert words in comments, words
    assert callable(s.SlideGraph.observation_joint_compatibility) and callable(s.chi2_quantile)
    adaptor = open(os.path.join(ROOT, "include", "slide_sloam_adaptor.hpp")).read()
    assert "observationJointCompatibility" in adaptor and NAME in adaptor


# ---- the quantile -----------------------------------------------------------------------------------------------------------------
def test_quantile_known_values():
    assert [round(s.chi2_quantile(0.99, d), 3) for d in (3, 7, 9)] == [11.345, 18.475, 21.666]
    assert round(s.chi2_quantile(0.99, 6), 2) == 16.81
    assert {d: round(s.chi2_quantile(0.99, d), 3) for d in (3, 7, 9)} == s.OBSERVATION_GATE_CHI2_99


def test_quantile_against_scipy():
    """Newton on the regularised incomplete gamma function against scipy.stats.chi2.ppf, dof 1 .. 384: 1e-12 relative (a textbook
    routine reaches 1e-14, so two decades are left)."""
    dof = np.arange(1, 385)
    worst = 0.0
    for prob in (0.9, 0.95, 0.99, 0.999):
        got = np.array([s.chi2_quantile(prob, int(d)) for d in dof])
        err = np.abs(got / chi2.ppf(prob, dof) - 1)
        print(f"[joint-compat] quantile prob {prob}: largest relative error {err.max():.2e} at dof {dof[err.argmax()]}")
        worst = max(worst, float(err.max()))
    assert worst <= 1e-12


@pytest.mark.parametrize("prob,dof", [(0.0, 3), (-0.1, 3), (1.0, 3), (1.5, 3), (float("nan"), 3), (0.99, 0), (0.99, -2)])
def test_quantile_refusals(prob, dof):
    q = C.c_double(77.0)
    assert s.lib().slide_chi2_quantile(C.c_double(prob), C.c_int(dof), C.byref(q)) == -1
    assert q.value == 77.0 and "chi2_quantile" in s.api.last_error()
    with pytest.raises(s.SlideError):
        s.chi2_quantile(prob, dof)


# ---- the argument refusals --------------------------------------------------------------------------------------------------------
def _good():
    meas = np.zeros((3, 17))
    meas[0, :4] = [1.0, 0.0, 0.0, 5.0]
    meas[1, :7], meas[1, 7:14], meas[1, 14:17] = I7, [4.0, 1, 0, 0, 0, 0, 1], [1.0, 2.0, 0.5]
    meas[2, :7], meas[2, 7:10], meas[2, 10:13], meas[2, 13] = I7, [3.0, 1, 0], [0.0, 0, 1], 0.3
    return dict(ptr=np.array([0, 2, 3], np.int32), robot=np.zeros(3, np.int32), pidx=np.array([7, 8, 9], np.uint64),
                cls=np.array([POINT, CUBE, CYL], np.int32), lidx=np.array([0, 3, 6], np.uint64), meas=meas)


OUTS = ("accepted", "d2_single", "d2_joint", "dof_joint", "status", "group_d2", "group_dof", "group_count", "group_status")


def test_argument_refusals_come_before_the_graph_and_write_nothing():
    def refused(why, n_groups=2, prob=0.99, null_out=None, **change):
        a = _good()
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                v(a[k])
        o = {k: np.full(3, 77.0) if k in ("d2_single", "d2_joint", "group_d2") else np.full(3, 77, np.int32) for k in OUTS}
        rc = getattr(s.lib(), NAME)(None, C.c_int(n_groups), P(a["ptr"]), P(a["robot"]), P(a["pidx"]), P(a["cls"]), P(a["lidx"]), P(a["meas"]),
                                    C.c_double(prob), *[None if k == null_out else P(o[k]) for k in OUTS])
        assert rc == -1, (change, rc)                                  # SLIDE_ERR_INVALID
        err = s.api.last_error()
        assert "observation_joint_compatibility" in err and why in err, (change, err)
        assert all((v == 77).all() for v in o.values())

    def put(i, j, v):
        def f(a):
            a[i, j] = v
        return f

    def put1(i, v):
        def f(a):
            a[i] = v
        return f

    def zero(i, lo, hi):
        def f(a):
            a[i, lo:hi] = 0.0
        return f
    refused("the graph is NULL")                                        # good arguments: only the handle is wrong
    refused("the graph is NULL", prob=0.0)                              # (evaluate only is a good argument)
    for name in _good():
        refused("pointer is NULL", **{name: None})
    for name in OUTS:
        refused("pointer is NULL", null_out=name)
    refused("n_groups < 0", n_groups=-1)
    refused("does not start at 0", ptr=put1(0, 1))
    refused("decreases", ptr=put1(1, 4))
    for prob in (-0.5, 1.0, 1.5, float("nan"), float("inf")):
        refused("prob", prob=prob)
    refused("robot outside", robot=put1(1, 13))
    refused("class", cls=put1(0, 3))
    refused("non-finite", meas=put(0, 3, np.nan))
    refused("zero quaternion", meas=zero(1, 3, 7))
    refused("zero quaternion", meas=zero(2, 3, 7))
    refused("zero bearing", meas=zero(0, 0, 3))
    refused("range <= 0", meas=put(0, 3, 0.0))
    refused("zero ray", meas=zero(2, 10, 13))


# ---- the reference against itself -------------------------------------------------------------------------------------------------
MIXED = [("point", 39, 36), ("point", 39, 33), ("cylinder", 38, 36), ("cube", 39, 39), ("point", 20, 0), ("cube", 4, 3), ("cylinder", 7, 6)]


@pytest.mark.parametrize("chart", [0, 1])
def test_schur_route_equals_the_dense_reference(chart):
    """Block (i, j) = [i == j] (I + Al_i H_ll^-1 Al_i^T) + B_i^T S^-1 B_j, the route the kernels take, equals the stacked
    I + A Sig A^T — cross blocks between different landmarks included — on chain40 to 1e-9 relative to max |C_ref|."""
    c = og.case("chain40", chart)
    group = jc.noisy_group(c, c.cpu_values, MIXED, seed=1)
    _, C_ref, _ = jc.stacked_ref(c, group, c.cpu_values)
    err = float(np.abs(jc.schur_route(c, group, c.cpu_values) - C_ref).max() / np.abs(C_ref).max())
    off_diag = C_ref[:3, 3:6]
    print(f"[joint-compat] chain40 chart {chart}: Schur route against the dense inverse {err:.2e}; a cross block's largest entry "
          f"{np.abs(off_diag).max():.3g}")
    assert err <= 1e-9
    assert np.abs(off_diag).max() > 1e-3          # (the cross blocks are not small: two points seen from one pose)


def test_rule_by_bordering_equals_the_stacked_solve():
    """The bordered form the device runs (X = C_iS L_S^-T, D = C_ii - X X^T = G G^T, y_i = G^-1 (r_i - X y_S)) gives the stacked d2 of
    ref_rule's dense solves."""
    c = og.case("chain40", 0)
    r, Cm, off = jc.stacked_ref(c, jc.noisy_group(c, c.cpu_values, MIXED, seed=2), c.cpu_values)
    want = jc.ref_rule(r, Cm, off, 0.0)
    L, y = np.zeros((0, 0)), np.zeros(0)
    for i in range(len(off) - 1):
        rows = np.arange(off[i], off[i + 1])
        X = np.linalg.solve(L, Cm[np.ix_(rows, np.arange(off[i]))].T).T if len(y) else np.zeros((len(rows), 0))
        G = np.linalg.cholesky(Cm[np.ix_(rows, rows)] - X @ X.T)
        y = np.concatenate([y, np.linalg.solve(G, r[rows] - X @ y)])
        L = np.block([[L, np.zeros((L.shape[0], len(rows)))], [X, G]])
        assert abs(y @ y - want["d2_joint"][i]) <= 1e-10 * want["d2_joint"][i]


def test_planted_scenarios_under_the_reference():
    """planted40, chart 0, at the reference's own estimate: six point candidates from pose 39 whose ranges are moved by +/- s
    sqrt(C_ii[2][2]).  s = 2.5: all six pass alone at 11.345, the stacked d2 is 53.26 against 34.81, the greedy rule keeps 0, 2, 4, 5
    and rejects 1 and 3 (18.37 > 16.81, 26.58 > 21.67).  s = 3: 3 fails alone (13.09), 1 and 5 jointly (26.48 > 16.81, 30.16 > 26.22),
    0, 2 and 4 are kept (20.31 < 21.67).  Unit noise: 14.14 stacked, at most 4.18 alone, all kept."""
    c = og.case("planted40", 0)
    v = c.cpu_values
    a = jc.ref_group(c, jc.planted_moved(c, v, 2.5), v, 0.99)
    assert np.round(a["d2_single"], 2).tolist() == [5.21, 7.22, 5.82, 9.69, 6.83, 6.51] and (a["d2_single"] < 11.345).all()
    assert round(jc.ref_group(c, jc.planted_moved(c, v, 2.5), v, 0.0)["group_d2"], 2) == 53.26
    assert round(float(chi2.ppf(0.99, 18)), 2) == 34.81
    assert a["accepted"].tolist() == [True, False, True, False, True, True]
    assert round(a["d2_joint"][1], 2) == 18.37 and round(a["d2_joint"][3], 2) == 26.58
    assert a["group_count"] == 4 and a["group_dof"] == 12
    b = jc.ref_group(c, jc.planted_moved(c, v, 3.0), v, 0.99)
    assert b["accepted"].tolist() == [True, False, True, False, True, False]
    assert round(b["d2_single"][3], 2) == 13.09 and round(b["d2_joint"][1], 2) == 26.48 and round(b["d2_joint"][5], 2) == 30.16
    assert round(b["d2_joint"][4], 2) == 20.31 and round(float(chi2.ppf(0.99, 12)), 2) == 26.22
    t = jc.ref_group(c, jc.planted_true(c), v, 0.99)
    assert t["accepted"].all() and round(t["group_d2"], 2) == 14.14 and round(t["d2_single"].max(), 2) == 4.18
    assert min(a["margin"], b["margin"], t["margin"]) >= 6e-2
    print(f"[joint-compat] planted margins {a['margin']:.3f} {b['margin']:.3f} {t['margin']:.3f}; cond(C) {np.linalg.cond(a['C']):.1f}")
