"""The joint-compatibility test of landmark observations on the JOINT graph (slide_chol_batch_observation_joint_compatibility): what
can be checked without a device — the symbol and the header's words, the Python methods, the argument refusals (the single-graph
call's group and probability checks and the candidates' own, decided on the host before the batch handle or the device is looked at,
provoked with a NULL handle), the route the device takes in numpy (tests/batch_joint_compat_cases.block_route: block_form's pieces
stacked, the lambda rows counted negatively) against the dense inverse of the joint H, and the decision generators' conditions under
the reference alone.  Everything that needs the factor is in test_gpu_batch_joint_compat.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import slide_slam_amd as s

import batch_joint_compat_cases as bj
import joint_graphs as jg
import joint_observation_gate_cases as jo
from test_joint_compat_host import OUTS, _good

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "slide_chol_batch_observation_joint_compatibility"
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731


def test_symbol_declared_exported_and_documented():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", code)
    assert m
    args = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert args == ["b", "n_groups", "group_ptr", "pose_slot", "pose_idx", "lm_slot", "cls", "lm_idx", "meas17", "prob", "accepted", "d2_single",
                    "d2_joint", "dof_joint", "status", "group_d2", "group_dof", "group_count", "group_status"], args
    assert hasattr(s.lib(), NAME) and NAME in s.api.EXPORTS
    comments = re.sub(r"[\s*]+", " ", " ".join(re.findall(r"/\*.*?\*/", txt, flags=re.S)))
    for words in ("slide_graph_observation_joint_compatibility on the JOINT graph", "[i == j] (I + G0_i) + W_i^T D W_j",
                  "may not be named twice in a group", "two replicas are one landmark and give the same bits",
                  "the cached joint Sigma is neither used nor touched"):
        assert words in comments, words
    assert callable(s.CholBatch.observation_joint_compatibility)
    from slide_slam_amd.distributed import PassDriver
    assert callable(PassDriver.observation_joint_compatibility)


def test_argument_refusals_come_before_the_batch_and_write_nothing():
    """The single-graph call's refusals under this call's name, lm_slot given and NULL; lm_slot itself is checked like pose_slot."""
    def refused(why, n_groups=2, prob=0.99, null_out=None, lm_slot="same", **change):
        a = _good()
        a["lslot"] = None if lm_slot is None else a["robot"].copy()
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                v(a[k])
        o = {k: np.full(3, 77.0) if k in ("d2_single", "d2_joint", "group_d2") else np.full(3, 77, np.int32) for k in OUTS}
        rc = getattr(s.lib(), NAME)(None, C.c_int(n_groups), P(a["ptr"]), P(a["robot"]), P(a["pidx"]), P(a["lslot"]), P(a["cls"]), P(a["lidx"]),
                                    P(a["meas"]), C.c_double(prob), *[None if k == null_out else P(o[k]) for k in OUTS])
        assert rc == -1, (change, rc)                                  # SLIDE_ERR_INVALID
        err = s.api.last_error()
        assert "chol_batch_observation_joint_compatibility" in err and why in err, (change, err)
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
    for lm_slot in ("same", None):
        refused("the batch is NULL", lm_slot=lm_slot)                   # good arguments: only the handle is wrong
        refused("the batch is NULL", prob=0.0, lm_slot=lm_slot)         # (evaluate only is a good argument)
        for name in _good():
            refused("pointer is NULL", lm_slot=lm_slot, **{name: None})
        for name in OUTS:
            refused("pointer is NULL", null_out=name, lm_slot=lm_slot)
        refused("n_groups < 0", n_groups=-1, lm_slot=lm_slot)
        refused("does not start at 0", ptr=put1(0, 1), lm_slot=lm_slot)
        refused("decreases", ptr=put1(1, 4), lm_slot=lm_slot)
        for prob in (-0.5, 1.0, 1.5, float("nan"), float("inf")):
            refused("prob", prob=prob, lm_slot=lm_slot)
        refused("robot outside", robot=put1(1, 13), lm_slot=lm_slot)
        refused("class", cls=put1(0, 3), lm_slot=lm_slot)
        refused("class", cls=put1(2, -1), lm_slot=lm_slot)
        refused("non-finite", meas=put(0, 3, np.nan), lm_slot=lm_slot)
        refused("non-finite", meas=put(1, 16, np.inf), lm_slot=lm_slot)
        refused("zero quaternion", meas=zero(1, 3, 7), lm_slot=lm_slot)
        refused("zero bearing", meas=zero(0, 0, 3), lm_slot=lm_slot)
        refused("range <= 0", meas=put(0, 3, 0.0), lm_slot=lm_slot)
        refused("zero ray", meas=zero(2, 10, 13), lm_slot=lm_slot)
    refused("robot outside", lslot=put1(0, 13))
    refused("robot outside", lslot=put1(2, -1))


# ---- the route against the dense reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("name", ["shared_mix", "relmeas"])
def test_block_route_equals_the_dense_reference(name, chart):
    """Block (i, j) = [i == j] (I + G0_i) + W_i^T D W_j on the joint system equals the stacked I + A Sig[u, u] A^T to 1e-9 relative to
    max |C_ref|, for every evaluate-only group: private landmarks from the landmark's own robot, private landmarks named cross-robot
    and shared landmarks mixed in one group, and one shared landmark named by two robots' poses through different replicas (the two
    candidates share columns of A there; the swapped names are the same variables).  With the lambda rows counted positively the
    route is visibly off on the job that has them."""
    J = jg.shared_mix_case(2) if name == "shared_mix" else jg.relmeas_case(R=2, n_rel=3, P=14)
    c = jo.JointObsCase(J, chart)
    assert jo.joint_system(c)["n_lam"] == (18 if name == "relmeas" else 0)
    v = c.cpu_values
    groups = bj.eval_groups(c, v)
    worst = 0.0
    for gname, grp in groups.items():
        _, C_ref, off = bj.stacked_ref(c, grp, v)
        top = float(np.abs(C_ref).max())
        err = float(np.abs(bj.block_route(c, grp, v) - C_ref).max() / top)
        wrong = float(np.abs(bj.block_route(c, grp, v, lambda_sign=1.0) - C_ref).max() / top)
        print(f"[batch-joint-compat] {name} chart {chart} {gname}: {len(grp)} candidates, {off[-1]} rows, route against the dense inverse "
              f"{err:.2e} (lambda rows counted positively: {wrong:.2e})")
        assert err <= 1e-9, (gname, err)
        if name == "relmeas":
            assert wrong > 1e-4, (gname, wrong)
        worst = max(worst, err)
    six = groups["6 at one pose"]
    kinds = {(len(c.robots_of(jo.split(x)[1], x[0], x[3])) > 1, bj.is_cross(x)) for x in six}
    assert {(False, False), (False, True)} <= kinds and any(sh for sh, _ in kinds), kinds
    # one candidate alone: the stacked route is the individual gate's block form (the same terms added in another order)
    one = groups["mixed"][:1]
    assert np.allclose(bj.block_route(c, one, v), jo.block_form(c, one[0], v), rtol=1e-13, atol=0)
    # the shared landmark named twice: a genuine cross block between the two candidates, and the swapped names are the same matrix
    t, sw = groups["shared twice"], groups["shared twice, swapped"]
    _, Ct, off = bj.stacked_ref(c, t, v)
    assert np.abs(Ct[off[0]:off[1], off[2]:off[3]]).max() > 1e-3
    assert np.array_equal(Ct, bj.stacked_ref(c, sw, v)[1])
    print(f"[batch-joint-compat] {name} chart {chart}: largest error {worst:.2e}")


# ---- the decision generators --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart", [0, 1])
def test_planted_hypotheses_under_the_reference(chart):
    """PlantedJoint under the joint gate's parameters, at the reference's own estimate: the true hypothesis (six points from robot 0's
    last pose, four of them cross-robot or shared) is accepted whole at 0.99; moved by +/- PLANTED_S sqrt(C_ii[2][2]) every candidate
    passes alone and the stacked set fails; every comparison stands MARGIN from its quantile."""
    c = jo.planted_case(chart)
    v = c.cpu_values
    true = bj.planted_true(c)
    far = [bj.is_cross(x) or len(c.robots_of(jo.split(x)[1], x[0], x[3])) > 1 for x in true]
    assert len(true) == 6 and sum(far) >= 3
    t = bj.ref_group(c, true, v, 0.99)
    assert t["accepted"].all() and t["group_count"] == 6 and t["margin"] >= bj.MARGIN
    moved = bj.planted_moved(c, v)
    m = bj.ref_group(c, moved, v, 0.99)
    q3 = s.chi2_quantile(0.99, 3)
    assert (m["d2_single"] < q3).all() and m["group_count"] < 6 and m["margin"] >= bj.MARGIN
    whole = bj.ref_group(c, moved, v, 0.0)["group_d2"]
    assert whole > s.chi2_quantile(0.99, 18)
    print(f"[batch-joint-compat] planted chart {chart}: true d2 {t['group_d2']:.2f} (alone at most {t['d2_single'].max():.2f}), margin "
          f"{t['margin']:.3f}; moved by {bj.PLANTED_S}: alone {np.round(m['d2_single'], 2).tolist()}, stacked {whole:.2f} against "
          f"{s.chi2_quantile(0.99, 18):.2f}, kept {m['accepted'].astype(int).tolist()}, d2_joint {np.round(m['d2_joint'], 2).tolist()}, margin "
          f"{m['margin']:.3f}")


def test_many_points_joint_holds_what_the_large_groups_need():
    """The two-robot sibling of many_points_graph: at least 129 distinct points, private ones of both robots and shared ones among the
    first 33."""
    J = bj.many_points_joint()
    pts = [(g, sorted({r for r, _ in obs})) for cls, g, _, obs in J.lms if cls == 2]
    assert len(pts) >= 129
    first = [r for _, r in pts[:33]]
    assert [0] in first and [1] in first and any(len(r) > 1 for r in first)
