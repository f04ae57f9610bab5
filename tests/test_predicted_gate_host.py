"""The observation gate at a predicted pose (slide_graph_predicted_observation_mahalanobis) and the back-end's association gate
(slide_backend_set_association_gate / slide_backend_gate_stats): what can be checked without a device — the symbols and the header's
words, the Python and adaptor methods, the argument refusals (decided on the host before the graph handle or the device is looked
at, provoked with a NULL handle as test_observation_gate_host.py provokes them), and the numpy reference of
tests/predicted_gate_cases.py against itself: the device's route (pred_block_form, the closed form of the augmented marginal on the
unchanged reduced system) against the dense inverse of the augmented H, and the planted generator's own conditions.  Everything that
needs the factor is in test_gpu_predicted_gate.py and test_gpu_backend_gate.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import slide_slam_amd as s

import observation_gate_cases as og
import predicted_gate_cases as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "slide_graph_predicted_observation_mahalanobis"
I7 = [0.0, 0, 0, 0, 0, 0, 1]
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
CYL, CUBE, POINT = 0, 1, 2


def test_symbols_declared_exported_and_documented():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in (NAME, "slide_backend_set_association_gate", "slide_backend_gate_stats"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(s.lib(), name) and name in s.api.EXPORTS, name
    for define in ("SLIDE_GATE_DROP 0", "SLIDE_GATE_NEW 1", "SLIDE_MATCH_GATED (-2)"):
        assert "#define " + define in code, define
    comments = re.sub(r"[\s*]+", " ", " ".join(re.findall(r"/\*.*?\*/", txt, flags=re.S)))
    for words in ("PREDICTED pose", "Ad(X_n^-1 X_k)", "Sig(n, n) = Ad Sig(k, k) Ad^T + diag(s^2)", "Ap diag(s^2) Ap^T", "P_k^T (Ap Ad)^T",
                  "noise_model_odom_vec x max(|t_rel|, noise_floor)", "the Between's residual does not enter",
                  "no add, no factorisation and no change to the graph", "as an EKF gates at the predicted state"):
        assert words in comments, words
    assert callable(s.SlideGraph.predicted_observation_mahalanobis)
    assert callable(s.SlideBackend.set_association_gate) and callable(s.SlideBackend.gate_stats)
    assert s.MATCH_GATED == -2 and (s.GATE_DROP, s.GATE_NEW) == (0, 1)
    adaptor = open(os.path.join(ROOT, "include", "slide_sloam_adaptor.hpp")).read()
    for word in ("predictedObservationMahalanobis", "setAssociationGate", NAME, "slide_backend_set_association_gate"):
        assert word in adaptor, word


def _good():
    meas = np.zeros((3, 17))
    meas[0, :4] = [1.0, 0.0, 0.0, 5.0]
    meas[1, :7], meas[1, 7:14], meas[1, 14:17] = I7, [4.0, 1, 0, 0, 0, 0, 1], [1.0, 2.0, 0.5]
    meas[2, :7], meas[2, 7:10], meas[2, 10:13], meas[2, 13] = I7, [3.0, 1, 0], [0.0, 0, 1], 0.3
    return dict(rel=np.array([1.0, 0, 0, 0, 0, 0, 1]), est=np.array([8.0, 0, 0, 0, 0, 0, 1]), cls=np.array([POINT, CUBE, CYL], np.int32),
                lidx=np.array([0, 3, 6], np.uint64), meas=meas)


def test_argument_refusals_come_before_the_graph_and_write_nothing():
    def refused(why, n=3, robot=0, d2_null=False, **change):
        a = _good()
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                v(a[k])
        d2, dof, Cm, r, st = np.full(3, 77.0), np.full(3, 77, np.int32), np.full((3, 81), 77.0), np.full((3, 9), 77.0), np.full(3, 77, np.int32)
        rc = getattr(s.lib(), NAME)(None, C.c_int(robot), C.c_uint64(7), P(a["rel"]), P(a["est"]), C.c_int(n), P(a["cls"]), P(a["lidx"]),
                                    P(a["meas"]), None if d2_null else P(d2), P(dof), P(Cm), P(r), P(st))
        assert rc == -1, (change, rc)                                  # SLIDE_ERR_INVALID
        err = s.api.last_error()
        assert "predicted_observation_mahalanobis" in err and why in err, (change, err)
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

    def zero1(lo, hi):
        def f(a):
            a[lo:hi] = 0.0
        return f
    refused("the graph is NULL")                                        # good arguments: only the handle is wrong
    for name in _good():
        refused("pointer is NULL", **{name: None})
    refused("pointer is NULL", d2_null=True)
    refused("n < 0", n=-1)
    refused("robot outside", robot=13)
    refused("robot outside", robot=-1)
    refused("class", cls=put1(0, 3))
    refused("non-finite", meas=put(0, 3, np.nan))
    refused("non-finite", meas=put(2, 15, np.inf))
    refused("zero quaternion", meas=zero(1, 3, 7))
    refused("zero quaternion", meas=zero(2, 3, 7))
    refused("zero bearing", meas=zero(0, 0, 3))
    refused("range <= 0", meas=put(0, 3, 0.0))
    refused("zero ray", meas=zero(2, 10, 13))
    # the step's and the prediction's own
    refused("non-finite", rel=put1(0, np.nan))
    refused("non-finite", est=put1(6, np.inf))
    refused("zero quaternion", rel=zero1(3, 7))
    refused("zero quaternion", est=zero1(3, 7))
    refused("the graph is NULL", n=0)                                   # (an empty list still needs a graph)


def test_backend_gate_refusals_without_a_backend():
    L = s.lib()
    assert L.slide_backend_set_association_gate(None, C.c_double(0.99), C.c_int(0)) == -1
    assert "set_association_gate" in s.api.last_error()
    out = np.full(4, 77, np.int64)
    assert L.slide_backend_gate_stats(None, P(out)) == -1 and (out == 77).all()


def test_generator_holds_its_own_conditions():
    """The planted list asserts on itself under d2_ref alone (predicted_gate_cases.planted): every true candidate below 0.75 of its
    class's 0.99 quantile, every false one above 1.5 of it."""
    for chart in (0, 1):
        c = og.case("planted40", chart)
        _, _, cands, flags, d2, dof = pg.planted(c)
        assert len(cands) == 2 * (5 + 2 + 3) and flags.sum() == 5 + 2 + 3
        for m in (3, 7, 9):
            sel = dof == m
            print(f"[pred-gate-cases] chart {chart} dof {m}: true max {d2[sel & flags].max():.2f} ({d2[sel & flags].max() / pg.QUANTILE[m]:.2f} of "
                  f"the quantile), false min {d2[sel & ~flags].min():.1f} ({d2[sel & ~flags].min() / pg.QUANTILE[m]:.2f})")


@pytest.mark.parametrize("name", ["chain40", "planted40"])
@pytest.mark.parametrize("chart", [0, 1])
def test_block_form_equals_the_dense_augmented_reference(name, chart):
    """C = I + Al H_ll^-1 Al^T + Ap diag(s^2) Ap^T + B^T S^-1 B with B = P_k^T (Ap Ad)^T - sum_f P_{p_f}^T F_f Al^T, on the UNCHANGED
    reduced system, equals I + A Sig_aug[sel, sel] A^T from the dense inverse of the augmented H within block_form's 1e-9 relative, for
    the three classes, from the first, a middle and the newest pose."""
    c = og.case(name, chart)
    vals = c.cpu_values
    worst, n = 0.0, 0
    for k in pg.FROMS[name]:
        rel7, est7 = pg.predict(vals, 0, k, pg.STEP, np.array([0.01, -0.02, 0.015, 0.05, -0.04, 0.02]))
        cands = pg.perturbed_list(c, vals, k, est7, pg.LANDMARKS[name], seed=3 + k)
        _, Cs, _ = pg.ref_gate(c, 0, k, rel7, est7, cands, vals)
        for i, cand in enumerate(cands):
            Cb = pg.pred_block_form(c, 0, k, rel7, est7, cand, vals)
            worst = max(worst, float(np.abs(Cb - Cs[i]).max() / np.abs(Cs[i]).max()))
            n += 1
    print(f"[pred-gate-cases] {name} chart {chart}: block form against the dense augmented inverse {worst:.2e} over {n} candidates")
    assert {x[0] for x in pg.LANDMARKS[name]} == {"point", "cube", "cylinder"}
    assert worst <= 1e-9


def test_the_between_jacobian_of_the_new_pose_is_the_whitening():
    """H_T of the oracle's Between equals diag(1 / s) exactly, and H_F = -diag(1 / s) Ad(X_n^-1 X_k) to rounding: what the closed form
    of the augmented marginal rests on."""
    c = og.case("chain40", 1)
    vals = c.cpu_values
    rel7, est7 = pg.predict(vals, 0, 20, pg.STEP, np.array([0.01, -0.02, 0.015, 0.05, -0.04, 0.02]))
    sg = pg.between_sigmas(pg.odom_sigma(c), rel7)
    HF, HT = pg.between_jacobians(1, vals.pose12(0, 20), pg.pose12_of(est7), rel7, sg)
    assert np.array_equal(HT, np.diag(1.0 / sg))
    import closure_cases as cc
    import closure_gate_cases as cg
    Ad = pg.adjoint(cc._mul(cc._inv(cc._pose(est7, np.float64)), cg.pose_of(vals.pose12(0, 20))))
    assert np.abs(HF + np.diag(1.0 / sg) @ Ad).max() <= 1e-12 * np.abs(HF).max()
