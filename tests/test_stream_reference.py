"""The streaming referee (tests/stream_graphs.py) judged against the oracle's own solve() before it judges the kernels
(test_gpu_stream_step.py): every case of the GPU file, run on an OracleGraph that solves each update itself.  Per update:

  - the Tracker, fed the oracle's read-backs, reproduces the oracle's theta (its export after the solve) to rounding, and its count
    of relinearised variables is the oracle's n_relin;
  - the oracle's estimate is theta (+) dx_ref within gn_reference's bound (Run.solve: check_step);

and each case shows here that it triggers the event it exists for."""
import numpy as np
import pytest

import stream_graphs as sg
from oracle import pyoracle as po

VLEN = {po.V_POSE: 12, po.V_POINT: 3, po.V_CUBE: 15, po.V_CYL: 7}      # (the rest of a variable's 15 doubles is not its value)
NOTHING = 1 << 30


def run(chart, case, *a, **kw):
    S, R = sg.oracle_stream(chart, 60, **kw)
    marks = case(S, R, *a)
    for n, u in enumerate(R.updates):
        assert u.n_relin == u.oracle_relin, (n, u)
        for k, t in enumerate(u.ref.vtype):
            m = VLEN[int(t)]
            th, mine = u.oracle_theta[k, :m], u.values[k, :m]
            assert np.abs(th - mine).max() <= 1e-13 * max(1.0, np.abs(th).max()), (n, k, th, mine)
    return S, R, marks


@pytest.mark.parametrize("chart", [0, 1])
def test_plain(chart):
    _, R, _ = run(chart, sg.case_plain)
    T = [u.T for u in R.updates]
    assert T[0] == 1 and max(T) == 5 and sum(t <= 2 for t in T) == 21
    assert sum(u.n_relin > 0 for u in R.updates) > 40           # (new poses and landmarks keep relinearising)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("cls", ["point", "cube", "cyl"])
def test_reobserve(chart, cls):
    _, _, marks = run(chart, sg.case_reobserve, cls)
    for f, u in marks.items():
        assert u.pmin_fac == f and u.pmin <= f, (f, u)          # (the re-observed landmark's first observer)
        assert u.pmin == f or f == 42, (f, u)                   # (pose 42: the newest poses' relinearisation reaches 41)


@pytest.mark.parametrize("chart", [0, 1])
def test_late_observation(chart):
    _, _, m = run(chart, sg.case_late)
    late, after = m["late"], m["after"]
    assert late.pmin_fac == 25                                  # (the late observer)
    assert m["key"] in after.moved and after.pmin_rel == 25      # (the landmark relinearises: from its NEW first observer on)


@pytest.mark.parametrize("chart", [0, 1])
def test_loop(chart):
    _, _, marks = run(chart, sg.case_loop)
    assert sorted(marks) == [0, 10, 11, 21, 44]
    for i, u in marks.items():
        assert u.pmin <= u.pmin_fac <= i, (i, u)
        assert u.pmin == i or i == 44, (i, u)                   # (pose 44: the newest pose's landmarks reach 43)


@pytest.mark.parametrize("chart", [0, 1])
def test_drift_correction(chart):
    _, _, m = run(chart, sg.case_drift, yaw_bias=0.02)
    corr, nxt = m["correction"], m["next"]
    assert corr.pmin_fac == 0
    assert nxt.n_relin > 30 and m["lm"] in nxt.moved and sg.var_key("pose", m["pose"]) in nxt.moved
    assert any(sg.var_key("pose", k) in nxt.moved for k in range(1, 10))      # (old poses relinearised)
    assert nxt.pmin_rel < nxt.pmin_fac                          # (the dirty column comes from the relinearisation: the prediction)


@pytest.mark.parametrize("chart", [0, 1])
def test_repeat(chart):
    _, _, m = run(chart, sg.case_repeat)
    assert all(u.pmin_fac == NOTHING for u in m["small"] + m["big"])
    assert m["small"][0].pmin_rel < NOTHING                              # (a dirty column from relinearisation alone)
    assert m["small"][-1].pmin == NOTHING and m["small"][-1].T == 3      # (nothing dirty: the substitutions are repeated)
    assert m["big"][0].n_relin > 0 and m["big"][0].T == 5                # (relinearisation inside the repeated update)
