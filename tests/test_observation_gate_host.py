"""The individual-compatibility gate of landmark observations (slide_graph_observation_mahalanobis): what can be checked without a
device — the symbol and the header's words, the Python and adaptor methods, and the argument refusals, which are decided on the host
before the graph handle or the device is looked at.  No graph handle can be made without a device, so the refusals are provoked with
a NULL handle, as test_closure_gate_host.py provokes them: a call whose arguments are good is refused FOR the handle, a call with a
bad argument for that argument, whatever the handle — slide_last_error says which.  The numpy reference of
tests/observation_gate_cases.py is checked against itself here too: the Schur form the device follows against the dense inverse, the
measurement conventions of the three add calls, and the planted generator's own conditions.  Everything that needs the factor is in
test_gpu_observation_gate.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import slide_slam_amd as s

import observation_gate_cases as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "slide_graph_observation_mahalanobis"
I7 = [0.0, 0, 0, 0, 0, 0, 1]
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
CYL, CUBE, POINT = 0, 1, 2


def test_symbol_declared_exported_and_documented():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", code)
    assert hasattr(s.lib(), NAME) and NAME in s.api.EXPORTS
    comments = re.sub(r"[\s*]+", " ", " ".join(re.findall(r"/\*.*?\*/", txt, flags=re.S)))
    for words in ("11.345", "18.475", "21.666", "sloam.cpp:73-203", "no threshold is applied", "No counterpart in the reference",
                  "jointMarginalCovariance({X(i), L(j)})", "LAST LINEARISATION POINT", "CURRENT ESTIMATE", "The graph is only read"):
        assert words in comments, words
    assert callable(s.SlideGraph.observation_mahalanobis)
    assert s.OBSERVATION_GATE_CHI2_99 == {3: 11.345, 7: 18.475, 9: 21.666} == og.QUANTILE
    adaptor = open(os.path.join(ROOT, "include", "slide_sloam_adaptor.hpp")).read()
    assert "observationMahalanobis" in adaptor and NAME in adaptor


def _good():
    meas = np.zeros((3, 17))
    meas[0, :4] = [1.0, 0.0, 0.0, 5.0]                                          # point: bearing, range
    meas[1, :7], meas[1, 7:14], meas[1, 14:17] = I7, [4.0, 1, 0, 0, 0, 0, 1], [1.0, 2.0, 0.5]   # cube: pose7, cube7, scale
    meas[2, :7], meas[2, 7:10], meas[2, 10:13], meas[2, 13] = I7, [3.0, 1, 0], [0.0, 0, 1], 0.3  # cylinder: pose7, root, ray, radius
    return dict(robot=np.zeros(3, np.int32), pidx=np.array([7, 8, 9], np.uint64), cls=np.array([POINT, CUBE, CYL], np.int32),
                lidx=np.array([0, 3, 6], np.uint64), meas=meas)


def test_argument_refusals_come_before_the_graph_and_write_nothing():
    def refused(why, n=3, d2_null=False, **change):
        a = _good()
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                v(a[k])
        d2, dof, Cm, r, st = np.full(3, 77.0), np.full(3, 77, np.int32), np.full((3, 81), 77.0), np.full((3, 9), 77.0), np.full(3, 77, np.int32)
        rc = getattr(s.lib(), NAME)(None, C.c_int(n), P(a["robot"]), P(a["pidx"]), P(a["cls"]), P(a["lidx"]), P(a["meas"]),
                                    None if d2_null else P(d2), P(dof), P(Cm), P(r), P(st))
        assert rc == -1, (change, rc)                                  # SLIDE_ERR_INVALID
        err = s.api.last_error()
        assert "observation_mahalanobis" in err and why in err, (change, err)
        assert (d2 == 77).all() and (dof == 77).all() and (Cm == 77).all() and (r == 77).all() and (st == 77).all()

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
    for name in _good():
        refused("pointer is NULL", **{name: None})
    refused("pointer is NULL", d2_null=True)
    refused("n < 0", n=-1)
    refused("robot outside", robot=put1(1, 13))
    refused("robot outside", robot=put1(2, -1))
    refused("class", cls=put1(0, 3))
    refused("class", cls=put1(2, -1))
    refused("non-finite", meas=put(0, 3, np.nan))
    refused("non-finite", meas=put(1, 16, np.inf))
    refused("non-finite", meas=put(2, 15, np.nan))                      # (the padding is read too: it must be zero, so finite)
    refused("zero quaternion", meas=zero(1, 3, 7))                      # the cube candidate's pose
    refused("zero quaternion", meas=zero(1, 10, 14))                    # ... its cube
    refused("zero quaternion", meas=zero(2, 3, 7))                      # the cylinder candidate's pose
    refused("zero bearing", meas=zero(0, 0, 3))
    refused("range <= 0", meas=put(0, 3, 0.0))
    refused("range <= 0", meas=put(0, 3, -1.0))
    refused("zero ray", meas=zero(2, 10, 13))


def test_generators_hold_their_own_conditions():
    """The planted list asserts on itself under d2_ref alone (observation_gate_cases.planted_list): every true candidate below 0.75 of
    its class's quantile, every false one above twice it."""
    for chart in (0, 1):
        c = og.case("planted40", chart)
        cands, flags, d2, dof = og.planted_list(c)
        assert len(cands) == 3 * (9 + 4 + 5) and flags.sum() == 2 * (9 + 4 + 5)
        for m in (3, 7, 9):
            sel = dof == m
            print(f"[obs-gate-cases] chart {chart} dof {m}: true max {d2[sel & flags].max():.2f} ({d2[sel & flags].max() / og.QUANTILE[m]:.2f} of "
                  f"the quantile), false min {d2[sel & ~flags].min():.1f}")


@pytest.mark.parametrize("chart", [0, 1])
def test_schur_form_equals_the_dense_reference(chart):
    """C = I + Al H_ll^-1 Al^T + B^T S^-1 B with B = P_p^T Ap^T - sum_f P_{p_f}^T F_f Al^T, F = E H_ll^-1 (the route the kernels take)
    equals I + A Sig[sel, sel] A^T on chain40 to 1e-9 relative: the sign and the orientation of F the kernel must follow."""
    c = og.case("chain40", chart)
    cands = og.perturbed_list(c, c.cpu_values)
    _, _, Cs, _ = og.ref_gate(c, cands, c.cpu_values)
    worst = max(float(np.abs(og.schur_form(c, cand, c.cpu_values) - Cs[k]).max() / np.abs(Cs[k]).max()) for k, cand in enumerate(cands))
    print(f"[obs-gate-cases] chain40 chart {chart}: Schur form against the dense inverse {worst:.2e} over {len(cands)} candidates")
    assert worst <= 1e-9


@pytest.mark.parametrize("kind,pose,lm", [("point", 7, 0), ("point", 1, 0), ("cylinder", 13, 6), ("cylinder", 7, 6), ("cube", 12, 3), ("cube", 4, 3)])
def test_noise_free_candidate_has_zero_residual(kind, pose, lm):
    """A candidate measured without noise at the reference estimate's own geometry: |r| < 1e-9 and d2_ref < 1e-15 — the measurement
    conventions of the three add calls (the bearing's frame, pose_world^-1 cube_world, the cylinder's projection) as add_rules states
    them; a measurement of another landmark is far from zero."""
    c = og.case("chain40", 1)
    cand = og.at_estimate(c, c.cpu_values, kind, 0, pose, lm, np.zeros(og.KIND[kind][3]))
    rs, _, _, d2 = og.ref_gate(c, [cand], c.cpu_values)
    assert np.abs(rs[0]).max() < 1e-9 and d2[0] < 1e-15, (rs[0], d2[0])
    other = cand[:3] + (lm + 12,) + cand[4:]
    assert np.abs(og.ref_gate(c, [other], c.cpu_values)[0][0]).max() > 1e-3      # (a cylinder's sigma is 400 here: metres give 1e-2)
