"""The individual-compatibility gate of landmark observations on the JOINT graph (slide_chol_batch_observation_mahalanobis): what can
be checked without a device — the symbol and the header's words, the Python methods, and the argument refusals, which are the
single-graph call's own and are decided on the host before the batch handle or the device is looked at (provoked with a NULL handle,
as test_observation_gate_host.py provokes them).  The numpy side of tests/joint_observation_gate_cases.py is checked against itself
here too: the block form the device follows (private landmarks eliminated, shared ones kept as separator rows, the lambda rows counted
with D = -I) against the dense inverse of the joint H, and the planted generator's own conditions.  Everything that needs the factor is
in test_gpu_joint_observation_gate.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import slide_slam_amd as s

import joint_graphs as jg
import joint_observation_gate_cases as jo
from test_observation_gate_host import _good

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "slide_chol_batch_observation_mahalanobis"
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731


def test_symbol_declared_exported_and_documented():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", code)
    assert m
    args = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert args == ["b", "n", "pose_slot", "pose_idx", "lm_slot", "cls", "lm_idx", "meas17", "d2", "dof", "C81", "r9", "status"], args
    assert hasattr(s.lib(), NAME) and NAME in s.api.EXPORTS
    comments = re.sub(r"[\s*]+", " ", " ".join(re.findall(r"/\*.*?\*/", txt, flags=re.S)))
    for words in ("lm_slot == NULL means the pose's slot", "W^T D W", "G0 = 0", "separator variable", "No counterpart in the reference",
                  "neither a factor nor a shared slot", "the cached joint Sigma is neither used nor touched"):
        assert words in comments, words
    assert callable(s.CholBatch.observation_mahalanobis)
    from slide_slam_amd.distributed import PassDriver
    assert callable(PassDriver.observation_mahalanobis)


def test_argument_refusals_come_before_the_batch_and_write_nothing():
    """Every refusal of the single-graph call in its own words, lm_slot given and NULL; lm_slot itself is checked like pose_slot."""
    def refused(why, n=3, d2_null=False, lm_slot="same", **change):
        a = _good()
        a["lslot"] = None if lm_slot is None else a["robot"].copy()
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                v(a[k])
        d2, dof, Cm, r, st = np.full(3, 77.0), np.full(3, 77, np.int32), np.full((3, 81), 77.0), np.full((3, 9), 77.0), np.full(3, 77, np.int32)
        rc = getattr(s.lib(), NAME)(None, C.c_int(n), P(a["robot"]), P(a["pidx"]), P(a["lslot"]), P(a["cls"]), P(a["lidx"]), P(a["meas"]),
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
    for lm_slot in ("same", None):
        refused("the batch is NULL", lm_slot=lm_slot)                   # good arguments: only the handle is wrong
        for name in _good():
            refused("pointer is NULL", lm_slot=lm_slot, **{name: None})
        refused("pointer is NULL", d2_null=True, lm_slot=lm_slot)
        refused("n < 0", n=-1, lm_slot=lm_slot)
        refused("robot outside", lm_slot=lm_slot, robot=put1(1, 13))
        refused("robot outside", lm_slot=lm_slot, robot=put1(2, -1))
        refused("class", lm_slot=lm_slot, cls=put1(0, 3))
        refused("class", lm_slot=lm_slot, cls=put1(2, -1))
        refused("non-finite", lm_slot=lm_slot, meas=put(0, 3, np.nan))
        refused("non-finite", lm_slot=lm_slot, meas=put(1, 16, np.inf))
        refused("non-finite", lm_slot=lm_slot, meas=put(2, 15, np.nan))
        refused("zero quaternion", lm_slot=lm_slot, meas=zero(1, 3, 7))
        refused("zero quaternion", lm_slot=lm_slot, meas=zero(1, 10, 14))
        refused("zero quaternion", lm_slot=lm_slot, meas=zero(2, 3, 7))
        refused("zero bearing", lm_slot=lm_slot, meas=zero(0, 0, 3))
        refused("range <= 0", lm_slot=lm_slot, meas=put(0, 3, 0.0))
        refused("range <= 0", lm_slot=lm_slot, meas=put(0, 3, -1.0))
        refused("zero ray", lm_slot=lm_slot, meas=zero(2, 10, 13))
    refused("robot outside", lslot=put1(0, 13))
    refused("robot outside", lslot=put1(2, -1))


def test_python_tuples_take_an_optional_landmark_slot():
    """_observation_arrays: the trailing lm_slot of a CholBatch candidate; without it the landmark's slot is the pose's."""
    arrays = s.api._observation_arrays
    cands = [("point", 1, 7, 2, [1.0, 0, 0], 5.0), ("point", 1, 7, 2, [1.0, 0, 0], 5.0, 0),
             ("cylinder", 0, 3, 4, [0.0, 0, 0, 0, 0, 0, 1], [3.0, 1, 0], [0.0, 0, 1], 0.3, 1),
             ("cube", 1, 3, 4, [0.0, 0, 0, 0, 0, 0, 1], [4.0, 1, 0, 0, 0, 0, 1], [1.0, 2.0, 0.5])]
    n, k, slot, pidx, cls, lidx, meas, lslot = arrays(cands, True)
    assert n == 4 and slot.tolist() == [1, 1, 0, 1] and lslot.tolist() == [1, 0, 1, 1] and cls.tolist() == [2, 2, 0, 1]
    assert np.array_equal(meas[0], meas[1]) and meas[2, 13] == 0.3 and meas[3, 16] == 0.5
    with pytest.raises(s.api.SlideError, match="measurement values"):
        arrays(cands[1:2], False)                                       # (a single graph's candidate carries no slot of its own)
    assert arrays([], True)[0] == 0


def _four(c, vals):
    """A private landmark from its own robot and from the other (cross-robot), a shared landmark — per class the case holds."""
    rows = [x for x in jo.named_pairs(c) if x[5] in ("not an observer", "observer", "cross-robot, private", "shared, own replica",
                                                      "shared, other replica", "cross-robot, shared")]
    return [jo.at_estimate(c, vals, k, sl, p, l, 0.7 * np.ones(jo.KIND[k][3]), ls) for k, sl, p, ls, l, _ in rows], [x[5] for x in rows]


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("name", ["shared_mix", "relmeas"])
def test_block_form_equals_the_dense_reference(name, chart):
    """C = I + G0 + W^T D W on the joint system (private landmarks eliminated with their factors' poses in the LANDMARK's robot, shared
    ones as rows of K with G0 = 0 and no factor sum, lambda rows counted negatively) equals I + A Sig[sel, sel] A^T to 1e-9 relative:
    a private landmark from its own robot, a private landmark cross-robot, a shared landmark, and all of them on a job with lambda
    rows.  The two mistakes the form guards against are shown to matter: the lambda rows counted positively, and a shared landmark
    treated as eliminated."""
    J = jg.shared_mix_case(2) if name == "shared_mix" else jg.relmeas_case(R=2, n_rel=3, P=14)
    c = jo.JointObsCase(J, chart)
    Y = jo.joint_system(c)
    assert Y["n_lam"] == (18 if name == "relmeas" else 0)
    cands, notes = _four(c, c.cpu_values)
    assert {"not an observer", "cross-robot, private", "shared, own replica", "cross-robot, shared"} <= set(notes)
    _, _, Cs, _ = jo.ref_gate(c, cands, c.cpu_values)
    worst = wrong_sign = 0.0
    for k, cand in enumerate(cands):
        top = float(np.abs(Cs[k]).max())
        worst = max(worst, float(np.abs(jo.block_form(c, cand, c.cpu_values) - Cs[k]).max() / top))
        wrong_sign = max(wrong_sign, float(np.abs(jo.block_form(c, cand, c.cpu_values, lambda_sign=1.0) - Cs[k]).max() / top))
    print(f"[joint-obs-gate-cases] {name} chart {chart}: block form against the dense inverse {worst:.2e} over {len(cands)} candidates"
          f" (lambda rows counted positively: {wrong_sign:.2e})")
    assert worst <= 1e-9
    if name == "relmeas":
        assert wrong_sign > 1e-6
    # the two names of a shared landmark are one variable of the reference
    a, b = notes.index("shared, own replica"), notes.index("shared, other replica")
    assert np.array_equal(c.sel(cands[a]), c.sel(cands[b])) and np.array_equal(Cs[a], Cs[b])


def test_generators_hold_their_own_conditions():
    """The planted list asserts on itself under d2_ref alone (joint_observation_gate_cases.planted_list): every true candidate below
    0.75 of its class's quantile, every false one above twice it; cross-robot candidates on both sides."""
    for chart in (0, 1):
        c = jo.planted_case(chart)
        cands, flags, d2, dof = jo.planted_list(c)
        cross = np.array([jo.split(x)[1] != x[1] for x in cands])
        assert len(cands) == 3 * len(c.J.lms) and flags.sum() == 2 * len(c.J.lms)
        assert (cross & flags).sum() >= 4 and (cross & ~flags).sum() >= 4
        for m in (3, 7, 9):
            sel = dof == m
            print(f"[joint-obs-gate-cases] chart {chart} dof {m}: true max {d2[sel & flags].max():.2f} ({d2[sel & flags].max() / jo.QUANTILE[m]:.2f} "
                  f"of the quantile), false min {d2[sel & ~flags].min():.1f} ({d2[sel & ~flags].min() / jo.QUANTILE[m]:.1f})")
