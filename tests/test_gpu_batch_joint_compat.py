"""The joint-compatibility test of landmark observations on the JOINT multi-robot graph, on the device
(slide_chol_batch_observation_joint_compatibility: k_joint_obs_joint_lin, one walk of the forward half of the joint substitution per
sweep, the lower tiles of every group's signed gram, k_joint_compat_chain) against the stacked dense reference and the rule in numpy
of tests/batch_joint_compat_cases.py, evaluated at the poses and landmarks read back from the device after the pass.

Per case: test_gpu_joint_observation_gate.GateRun (the reference at the values the pass linearises at, one exact joint pass).
Tolerances: the single-graph test's.  d2_single, d2_joint and group_d2 relative to the reference within tol x cond(C), floor 1e-12, C
the stacked reference matrix of the set tested at that step and tol dense_inverse's tolerance for the case; accepted, dof_joint,
group_dof, group_count and the statuses are exact; every decision test's generator has asserted that each comparison stands 1e-3 from
its quantile.  The independence and read-only checks are bit for bit.  SLIDE_ERR_NOT_SPD is not covered, as in the neighbours: C is I
plus a positive semi-definite matrix and has no non-positive pivot for finite input.

Measured on the device (largest error as a share of its bound): see DESIGN.md section 7, the joint-compatibility paragraph of the
joint graph."""
import ctypes as C

import numpy as np
import pytest

import batch_joint_compat_cases as bj
import joint_closure_gate_cases as jcg
import joint_graphs as jg
import joint_observation_gate_cases as jo
import observation_loss_cases as oc
import robust_cases as rc
from test_gpu_joint_marginals import dense_inverse
from test_gpu_joint_observation_gate import GateRun, sync
from test_gpu_joint_step import Run

pytestmark = pytest.mark.gpu

MISSING, INVALID, NOT_SPD, CAPACITY = 1, -1, -2, -3
FIELDS = ("accepted", "d2_single", "d2_joint", "dof_joint", "status")
GROUP_FIELDS = ("group_d2", "group_dof", "group_count", "group_status")


def bound(c, cond):
    return max(c.tol * cond, 1e-12)


def check_group(c, cands, out, g, vals, prob, tag):
    """Group g of `out` against the reference of its served candidates (status 0), exact where it must be.  -> the reference."""
    a, b = out["group_ptr"][g], out["group_ptr"][g + 1]
    assert b - a == len(cands) and out["group_status"][g] == 0
    on = [k for k in range(len(cands)) if out["status"][a + k] == 0]
    ref = bj.ref_group(c, [cands[k] for k in on], vals, prob)
    worst = 0.0
    for i, k in enumerate(on):
        e1 = abs(out["d2_single"][a + k] - ref["d2_single"][i]) / ref["d2_single"][i]
        ej = abs(out["d2_joint"][a + k] - ref["d2_joint"][i]) / ref["d2_joint"][i]
        b1, bj_ = bound(c, ref["cond_single"][i]), bound(c, ref["cond_joint"][i])
        print(f"[batch-joint-compat] {tag} candidate {k}: d2_single err {e1:.2e} (bound {b1:.2e}), d2_joint err {ej:.2e} (bound {bj_:.2e})")
        assert e1 <= b1 and ej <= bj_, (tag, k, e1, b1, ej, bj_)
        assert out["accepted"][a + k] == ref["accepted"][i] and out["dof_joint"][a + k] == ref["dof_joint"][i], (tag, k)
        worst = max(worst, e1 / b1, ej / bj_)
    assert out["group_dof"][g] == ref["group_dof"] and out["group_count"][g] == ref["group_count"]
    if ref["group_count"]:
        last = int(np.flatnonzero(ref["accepted"])[-1])
        eg = abs(out["group_d2"][g] - ref["group_d2"]) / ref["group_d2"]
        assert eg <= bound(c, ref["cond_joint"][last]), (tag, eg)
    else:
        assert out["group_d2"][g] == 0
    print(f"[batch-joint-compat] {tag}: {len(on)} candidates, {ref['group_dof']} rows accepted, group d2 {out['group_d2'][g]:.6g} ref "
          f"{ref['group_d2']:.6g}, largest error / bound {worst:.2e}")
    return ref


def same_group(x, gx, y, gy, what):
    ax, bx, ay, by = x["group_ptr"][gx], x["group_ptr"][gx + 1], y["group_ptr"][gy], y["group_ptr"][gy + 1]
    for f in FIELDS:
        assert np.array_equal(x[f][ax:bx], y[f][ay:by]), (what, f)
    for f in GROUP_FIELDS:
        assert x[f][gx] == y[f][gy], (what, f)


def case_of(name):
    """(the Joint, what the pass must show): the unsigned path (no lambda rows) and the signed one (18 lambda coordinates)."""
    if name == "shared_mix":
        J = jg.shared_mix_case(2)

        def ev(r):
            assert r.info["n_slots"] > 0 and r.drv.arrow and not J.relmeas and getattr(r.drv, "lam_dim", 0) == 0
    else:
        J = jg.relmeas_case(R=2, n_rel=3, P=14)

        def ev(r):
            assert r.drv.lam_dim == 18
    return J, ev


# ---- against the reference ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,chart", [("shared_mix", 0), ("shared_mix", 1), ("relmeas", 0)])
def test_evaluate_only_against_the_stacked_reference(gpu, name, chart):
    """prob = 0 on a job without lambda rows (the unsigned gram, both charts) and on one with them (the signed gram), each against
    its own reference: two and six candidates from one pose, a mixed-class group and its permutation, candidates at poses of two
    robots, robot 0's pose against landmarks only robot 1 holds, and a shared landmark named twice through two replicas — bit for bit
    the group with the replicas' names swapped."""
    J, ev = case_of(name)
    g = GateRun(gpu, J, chart, ev)
    try:
        groups = bj.eval_groups(g.c, g.vals)
        names = list(groups)
        out = g.batch.observation_joint_compatibility(list(groups.values()), prob=0.0)
        assert (out["status"] == 0).all() and out["accepted"].all() and (out["group_status"] == 0).all()
        refs = {n: check_group(g.c, groups[n], out, i, g.vals, 0.0, f"{name} chart {chart} {n}") for i, n in enumerate(names)}
        assert out["group_count"].tolist() == [len(groups[n]) for n in names]
        assert out["group_dof"].tolist() == [sum(bj.rows_of(groups[n])) for n in names]
        m, p = names.index("mixed"), names.index("mixed, permuted")
        assert abs(out["group_d2"][p] - out["group_d2"][m]) <= 2 * bound(g.c, refs["mixed"]["cond_joint"][-1]) * out["group_d2"][m]
        a, b = out["group_ptr"][m], out["group_ptr"][m + 1]
        assert (np.diff(out["d2_joint"][a:b]) >= 0).all()                   # (a prefix sequence grows)
        same_group(out, names.index("shared twice"), out, names.index("shared twice, swapped"), "replicas swapped")
        same_group(g.r.drv.observation_joint_compatibility([groups["mixed"]], prob=0.0), 0, out, m, "driver")
    finally:
        g.close()


@pytest.mark.parametrize("name", ["shared_mix", "relmeas"])
def test_one_candidate_per_group_equals_the_individual_gate(gpu, name):
    J, ev = case_of(name)
    g = GateRun(gpu, J, 0, ev)
    try:
        groups = bj.eval_groups(g.c, g.vals)
        cands = groups["6 at one pose"] + groups["mixed"] + groups["cross-robot"] + groups["shared twice"]
        out = g.batch.observation_joint_compatibility([[x] for x in cands], prob=0.0)
        alone = g.batch.observation_mahalanobis(cands)
        assert (out["status"] == 0).all() and out["accepted"].all() and out["dof_joint"].tolist() == bj.rows_of(cands)
        assert np.array_equal(out["d2_single"], out["d2_joint"]) and np.array_equal(out["group_d2"], out["d2_joint"])
        for k, cand in enumerate(cands):
            ref = check_group(g.c, [cand], out, k, g.vals, 0.0, f"{name} one {cand[0]}")
            assert abs(out["d2_single"][k] - alone["d2"][k]) <= bound(g.c, ref["cond_single"][0]) * alone["d2"][k]
    finally:
        g.close()


@pytest.mark.parametrize("chart", [0, 1])
def test_selection_on_the_planted_hypotheses(gpu, chart):
    """PlantedJoint under the joint gate's parameters at prob = 0.99, at the device's own estimate: the true hypothesis from robot 0's
    last pose (four of six cross-robot or shared) is kept whole; with the ranges moved by +/- 2.5 sqrt(C_ii[2][2]) every candidate
    passes alone, the stacked set fails and the rule keeps the reference's subset.  The reference's comparisons stand 1e-3 from their
    quantiles (ref_group asserts it)."""
    J = jo.PlantedJoint()
    g = GateRun(gpu, J, chart, okw=jo.PLANTED_OKW, kw=jo.PLANTED_KW)
    try:
        true, moved = bj.planted_true(g.c), bj.planted_moved(g.c, g.vals)
        out = g.batch.observation_joint_compatibility([true, moved], prob=0.99)
        assert (out["status"] == 0).all()
        t = check_group(g.c, true, out, 0, g.vals, 0.99, f"planted chart {chart} true")
        m = check_group(g.c, moved, out, 1, g.vals, 0.99, f"planted chart {chart} moved")
        assert t["accepted"].all() and out["group_count"][0] == 6
        assert (out["d2_single"][6:] < gpu.chi2_quantile(0.99, 3)).all() and out["group_count"][1] < 6
        assert out["accepted"][6:].tolist() == m["accepted"].tolist()
        ev = g.batch.observation_joint_compatibility([moved], prob=0.0)
        assert ev["group_d2"][0] > gpu.chi2_quantile(0.99, 18) and ev["accepted"].all()
    finally:
        g.close()


# ---- properties ---------------------------------------------------------------------------------------------------------------------

def test_groups_do_not_depend_on_their_neighbours(gpu):
    """The evaluate-only groups and three frames' worth of matches onto the whole joint map (more than 96 rows each), on the job with
    lambda rows: more than two sweeps' columns.  Every group is bit for bit what the call gives for it alone, first in the list and
    last, under evaluate-only and under a selection that rejects some candidates."""
    J, ev = case_of("relmeas")
    g = GateRun(gpu, J, 0, ev)
    try:
        b, c, v = g.batch, g.c, g.vals
        groups = list(bj.eval_groups(c, v).values())
        groups[1:1] = [bj.all_from(c, v, 0, J.sizes[0] - 1, 300)]
        groups += [bj.all_from(c, v, 1, J.sizes[1] - 1, 301), bj.all_from(c, v, 0, 5, 302), bj.all_from(c, v, 1, 2, 303)]
        rows = [sum(bj.rows_of(x)) for x in groups]

        def sweeps(rs):                                                     # (the call's packing: whole groups, in order, 384 columns)
            n, used = 1, 0
            for x in rs:
                n, used = (n + 1, x) if used + x > 384 else (n, used + x)
            return n
        assert sweeps(rows) >= 2 and sweeps(rows[::-1]) >= 2 and max(rows) > 96, rows
        for prob in (0.0, 0.2):
            full = b.observation_joint_compatibility(groups, prob=prob)
            assert (full["group_status"] == 0).all() and (full["status"] == 0).all()
            back = b.observation_joint_compatibility(groups[::-1], prob=prob)
            for i, grp in enumerate(groups):
                same_group(b.observation_joint_compatibility([grp], prob=prob), 0, full, i, ("alone", i, prob))
                same_group(back, len(groups) - 1 - i, full, i, ("reversed", i, prob))
            if prob:
                lens = np.array([len(x) for x in groups])
                assert (full["group_count"] < lens).any() and full["group_count"].any()          # (the selection does select)
                print(f"[batch-joint-compat] selection at {prob}: accepted {full['group_count'].tolist()} of {lens.tolist()}; rows {rows}")
    finally:
        g.close()


def test_past_the_lds_boundary_and_capacity(gpu):
    """Two robots with 134 points: groups of 99 rows (33 points) and 97 rows (30 points and a cylinder), the first that leave LDS,
    against the reference; 129 distinct points (387 rows): SLIDE_ERR_CAPACITY with zeros, the neighbours served."""
    J = bj.many_points_joint()
    g = GateRun(gpu, J, 0)
    try:
        c, v = g.c, g.vals
        g99, g97, g387, g6 = bj.many_group(c, v, 33, 41), bj.many_group(c, v, 30, 42, cyl=True), bj.many_group(c, v, 129, 43), bj.many_group(c, v, 2, 44)
        assert sum(bj.is_cross(x) for x in g99) >= 8 and any(len(c.robots_of(jo.split(x)[1], x[0], x[3])) > 1 for x in g99)
        out = g.batch.observation_joint_compatibility([g99, g387, g97, g6], prob=0.0)
        assert out["group_status"].tolist() == [0, CAPACITY, 0, 0]
        assert out["group_dof"].tolist() == [99, 0, 97, 6] and out["group_count"].tolist() == [33, 0, 31, 2]
        a, b = out["group_ptr"][1], out["group_ptr"][2]
        assert out["group_d2"][1] == 0 and (out["status"][a:b] == 0).all()
        for f in ("accepted", "d2_single", "d2_joint", "dof_joint"):
            assert not out[f][a:b].any(), f
        for i, grp, name in ((0, g99, "99 rows"), (2, g97, "97 rows"), (3, g6, "6 rows")):
            check_group(c, grp, out, i, v, 0.0, name)
    finally:
        g.close()


def test_statuses_inside_a_group(gpu):
    """A private landmark named twice: SLIDE_ERR_INVALID for the group, zeros, the neighbours served (a shared one twice is served:
    test_evaluate_only_against_the_stacked_reference).  A missing slot, pose or landmark: skipped, the others have the values of the
    group without it, bit for bit."""
    J, ev = case_of("shared_mix")
    g = GateRun(gpu, J, 0, ev)
    try:
        b = g.batch
        grp = bj.eval_groups(g.c, g.vals)["mixed"]
        priv = next(k for k, x in enumerate(grp) if len(g.c.robots_of(jo.split(x)[1], x[0], x[3])) == 1 and x[0] == "point")
        twice = grp[:3] + [grp[priv]] + grp[3:]
        pt = grp[priv]
        n = jo.NARGS["point"]
        holes = [grp[0], ("point", 0, J.sizes[0] + 5) + pt[3:], grp[1], ("point", 0, 3, 999) + pt[4:n], grp[2], ("point", 2, 3) + pt[3:n], grp[3],
                 ("point", 0, 3) + pt[3:n] + (2,), grp[4]]
        out = b.observation_joint_compatibility([grp, twice, holes], prob=0.0)
        assert out["group_status"].tolist() == [0, INVALID, 0]
        a, e = out["group_ptr"][1], out["group_ptr"][2]
        assert out["group_d2"][1] == 0 and out["group_dof"][1] == 0 and out["group_count"][1] == 0 and (out["status"][a:e] == 0).all()
        for f in ("accepted", "d2_single", "d2_joint", "dof_joint"):
            assert not out[f][a:e].any(), f
        h = out["group_ptr"][2]
        assert out["status"][h:].tolist() == [0, MISSING, 0, MISSING, 0, MISSING, 0, MISSING, 0]
        keep = h + np.array([0, 2, 4, 6, 8])
        for f in FIELDS:
            assert np.array_equal(out[f][keep], out[f][:5]), f
            assert not out[f][h + np.array([1, 3, 5, 7])].any() or f == "status", f
        for f in ("group_d2", "group_dof", "group_count"):
            assert out[f][2] == out[f][0], f
        check_group(g.c, grp, out, 0, g.vals, 0.0, "mixed")
        none = b.observation_joint_compatibility([[holes[1]], []], prob=0.99)
        assert none["status"].tolist() == [MISSING] and none["group_status"].tolist() == [0, 0] and not none["group_dof"].any()
        empty = b.observation_joint_compatibility([])
        assert len(empty["accepted"]) == 0 and len(empty["group_d2"]) == 0
        with pytest.raises(gpu.SlideError, match="SLIDE_ERR_INVALID"):              # (an argument refusal on a live batch)
            b.observation_joint_compatibility([grp], 1.0)
    finally:
        g.close()


def test_queries_leave_the_batch_as_it_was(gpu):
    """get_pose_covariances, observation_mahalanobis, closure_mahalanobis and the next pass of a batch that served joint-compatibility
    queries are bit for bit those of a batch that never did."""
    J, _ = case_of("relmeas")

    def state(run, cands):
        vals = jo.shard_values(run.shards)
        cov = [run.batch.get_pose_covariances(s, np.arange(J.sizes[s])) for s in range(J.R)]
        gate = run.batch.closure_mahalanobis(jcg.perturbed_list(J, vals.pose12))
        obs = run.batch.observation_mahalanobis(cands)
        return cov, gate, obs

    g = GateRun(gpu, J)
    try:
        groups = list(bj.eval_groups(g.c, g.vals).values()) + [bj.all_from(g.c, g.vals, 0, J.sizes[0] - 1, 300, 2.0)]
        flat = [x for grp in groups for x in grp]
        for prob in (0.0, 0.99):
            assert (g.batch.observation_joint_compatibility(groups, prob=prob)["group_status"] == 0).all()
        st1 = state(g.r, flat)
        assert (g.batch.observation_joint_compatibility(groups, prob=0.5)["group_status"] == 0).all()      # (with the joint Sigma cached now)
        g.r.drv.one_pass()
        sync()
        with_q = g.r.values()
    finally:
        g.close()
    r2 = Run(gpu, J, 0)
    try:
        r2.drv.one_pass()
        sync()
        st2 = state(r2, flat)
        r2.drv.one_pass()
        sync()
        for a, b in zip(st1[0], st2[0]):
            assert np.array_equal(a, b)
        for f in ("d2", "C", "r"):
            assert np.array_equal(st1[1][f], st2[1][f]), f
            assert np.array_equal(st1[2][f], st2[2][f]), f
        assert np.array_equal(with_q, r2.values())
    finally:
        r2.close()


def test_noise_is_the_base_noise_under_an_observation_loss(gpu):
    """Under a batch Huber observation loss the call is served against the reweighted joint H (the reference is built from the factors
    scaled by the loss's weights at the point the pass linearises, as test_gpu_joint_observation_gate.py builds it); the candidates'
    own noise is the base noise."""
    import joint_observation_loss_cases as jl
    J = jl.kinds_case()
    okw, kw = oc.params(0)
    seen = {}

    def prepare(r):
        r.drv.set_observation_loss("huber")

    def case(r):
        ref, vals = r.ref, r.values()
        sel = oc.selected(ref)
        _, _, w, _, _ = oc.obs_step(ref, vals, rc.HUBER, 0.0, sel)
        assert (w[sel] < 0.9).sum() >= 3                                  # the loss does reweight this graph
        seen["plain"] = dense_inverse(ref, vals)[0]
        base = ref.fsig
        ref.fsig = base / np.sqrt(w)[:, None]
        try:
            return jo.JointObsCase(J, 0, ref=ref, vals=vals, params=okw)
        finally:
            ref.fsig = base
    kw = {k: v for k, v in kw.items() if k != "pose_chart"}
    g = GateRun(gpu, J, 0, okw=dict(bearing_sigma=oc.SIGMA, cyl_sigma=oc.SIGMA), kw=kw, prepare=prepare, case=case)
    try:
        grp = bj.some_group(g.c, g.vals)
        out = g.batch.observation_joint_compatibility([grp], prob=0.0)
        assert (out["status"] == 0).all()
        check_group(g.c, grp, out, 0, g.vals, 0.0, "huber")
        g.c.Sig = seen["plain"]                                           # the same group against the unweighted H differs
        assert abs(bj.ref_group(g.c, grp, g.vals, 0.0)["group_d2"] / out["group_d2"][0] - 1) > 1e-3
    finally:
        g.close()


def test_whole_call_refusals(gpu):
    """joint_state's refusals: before a pass, after a graph changed, in PCG mode; nothing is written.  The driver's method raises as
    _joint_ok() does when the batch does not run exact passes."""
    J = jg.shared_mix_case(2)
    P0 = J.sizes[0]
    I7 = np.array([1.0, 0, 0, 0, 0, 0, 1])
    cand = ("point", 0, 3, 0, [1.0, 0.0, 0.0], 5.0, 1)

    def raw(b):
        L = gpu.lib()
        P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        n, k, slot, pidx, cls, lidx, meas, lslot = gpu.api._observation_arrays([cand], True)
        ptr = np.array([0, 1], np.int32)
        outs = [np.full(1, 77, np.int32), np.full(1, 77.0), np.full(1, 77.0), np.full(1, 77, np.int32), np.full(1, 77, np.int32), np.full(1, 77.0),
                np.full(1, 77, np.int32), np.full(1, 77, np.int32), np.full(1, 77, np.int32)]
        rc_ = L.slide_chol_batch_observation_joint_compatibility(C.c_void_p(b.h), C.c_int(1), P(ptr), P(slot), P(pidx), P(lslot), P(cls), P(lidx),
                                                                 P(meas), C.c_double(0.99), *[P(o) for o in outs])
        return rc_, all((a == 77).all() for a in outs)

    r = Run(gpu, J, 0)
    try:
        with pytest.raises(gpu.SlideError, match="no whole exact joint pass"):
            r.batch.observation_joint_compatibility([[cand]])
        assert raw(r.batch) == (-1, True)
        r.drv.one_pass()
        sync()
        assert raw(r.batch) == (0, False)
        G = r.shards[0].graph
        st, v = G.get_pose12(0, P0 - 1)
        est = np.concatenate([v[9:12] + np.array([1.0, 0.0, 0.0]), [0.0, 0.0, 0.0, 1.0]])
        G.add_keypose_between(0, P0 - 1, P0, I7, est)
        with pytest.raises(gpu.SlideError, match="changed since the last exact joint pass"):
            r.batch.observation_joint_compatibility([[cand]])
        assert raw(r.batch) == (-1, True)
    finally:
        r.close()
    rp = Run(gpu, J, 0, pcg_iters=20, pcg_tol=1e-10)
    try:
        rp.drv.one_pass()
        sync()
        with pytest.raises(gpu.SlideError, match="does not run exact joint passes"):
            rp.batch.observation_joint_compatibility([[cand]])
        assert raw(rp.batch) == (-1, True)
        with pytest.raises(ValueError):
            rp.drv.observation_joint_compatibility([[cand]])
    finally:
        rp.close()
