"""The joint-compatibility test of landmark observations on the device (slide_graph_observation_joint_compatibility: one forward
substitution per sweep on the resident factor, k_obs_joint_lin, the lower tiles of every group's whole gram, k_joint_compat_chain)
against the dense reference and the rule in numpy of tests/joint_compat_cases.py, evaluated at the poses and landmarks read back
from the device.

Tolerances.  d2_single, d2_joint and group_d2: relative to the reference within tol x cond(C), floor 1e-12 (observation_gate_cases'
gate_bound), C the stacked reference matrix of the set tested at that step.  accepted, dof_joint, group_dof, group_count and the
statuses are exact; every decision test's generator has asserted that each comparison stands 1e-3 from its quantile.  The independence
checks are bit for bit."""
import numpy as np
import pytest

import joint_compat_cases as jc
import observation_gate_cases as og
import observation_loss_cases as oc
import robust_cases as rc
from gn_reference import EPS, Reference
from oracle import pyoracle as po
from test_gpu_marginals import _raises

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
    ref = jc.ref_group(c, [cands[k] for k in on], vals, prob)
    worst = 0.0
    for i, k in enumerate(on):
        e1 = abs(out["d2_single"][a + k] - ref["d2_single"][i]) / ref["d2_single"][i]
        ej = abs(out["d2_joint"][a + k] - ref["d2_joint"][i]) / ref["d2_joint"][i]
        b1, bj = bound(c, ref["cond_single"][i]), bound(c, ref["cond_joint"][i])
        assert e1 <= b1 and ej <= bj, (tag, k, e1, b1, ej, bj)
        assert out["accepted"][a + k] == ref["accepted"][i] and out["dof_joint"][a + k] == ref["dof_joint"][i], (tag, k)
        worst = max(worst, e1 / b1, ej / bj)
    assert out["group_dof"][g] == ref["group_dof"] and out["group_count"][g] == ref["group_count"]
    if ref["group_count"]:
        last = int(np.flatnonzero(ref["accepted"])[-1])
        eg = abs(out["group_d2"][g] - ref["group_d2"]) / ref["group_d2"]
        assert eg <= bound(c, ref["cond_joint"][last]), (tag, eg)
    else:
        assert out["group_d2"][g] == 0
    print(f"[joint-compat] {tag}: {len(on)} candidates, {ref['group_dof']} rows accepted, group d2 {out['group_d2'][g]:.6g} ref {ref['group_d2']:.6g}, "
          f"largest error / bound {worst:.2e}")
    return ref


def same_group(x, gx, y, gy, what):
    ax, bx, ay, by = x["group_ptr"][gx], x["group_ptr"][gx + 1], y["group_ptr"][gy], y["group_ptr"][gy + 1]
    for f in FIELDS:
        assert np.array_equal(x[f][ax:bx], y[f][ay:by]), (what, f)
    for f in GROUP_FIELDS:
        assert x[f][gx] == y[f][gy], (what, f)


def points(lms, pose):
    return [("point", pose, l) for l in lms]


# (kind, pose, landmark) of chain40's groups: landmark k is seen from poses k .. k + 3, points every third pose, cylinders at even and
# cubes at odd multiples of three
CHAIN_GROUPS = {
    "2 points at one pose": points((36, 33), 39),
    "6 points at one pose": points((24, 27, 30, 33, 36, 39), 39),
    "points at different poses": [("point", 39, 36), ("point", 20, 0), ("point", 7, 3), ("point", 30, 21)],
    "mixed": [("point", 39, 36), ("cylinder", 38, 30), ("point", 39, 33), ("cube", 39, 39), ("point", 38, 27)],
}


@pytest.mark.parametrize("chart", [0, 1])
def test_one_candidate_per_class_equals_the_individual_gate(gpu, chart):
    c = og.case("chain40", chart)
    G, _ = og.device_graph(gpu, "chain40", chart)
    vals = og.device_values(G)
    cands = jc.noisy_group(c, vals, [("point", 39, 36), ("cylinder", 13, 6), ("cube", 12, 3)], seed=11)
    out = G.observation_joint_compatibility([[x] for x in cands], prob=0.0)
    alone = G.observation_mahalanobis(cands)
    assert (out["status"] == 0).all() and out["accepted"].all() and out["dof_joint"].tolist() == [3, 7, 9]
    assert np.array_equal(out["d2_single"], out["d2_joint"]) and np.array_equal(out["group_d2"], out["d2_joint"])
    for k, cand in enumerate(cands):
        ref = check_group(c, [cand], out, k, vals, 0.0, f"chart {chart} one {cand[0]}")
        assert abs(out["d2_single"][k] - alone["d2"][k]) <= bound(c, ref["cond_single"][0]) * alone["d2"][k]


@pytest.mark.parametrize("chart", [0, 1])
def test_evaluate_only_against_the_stacked_reference(gpu, chart):
    """prob = 0: d2_joint is the prefix sequence of the stacked test and group_d2 the joint compatibility of the whole hypothesis.  A
    permuted group has the same group_d2 within the bound and another prefix sequence."""
    c = og.case("chain40", chart)
    G, _ = og.device_graph(gpu, "chain40", chart)
    vals = og.device_values(G)
    groups = [jc.noisy_group(c, vals, t, seed=20 + i) for i, t in enumerate(CHAIN_GROUPS.values())]
    perm = [4, 2, 0, 3, 1]
    groups.append([groups[3][k] for k in perm])
    out = G.observation_joint_compatibility(groups, prob=0.0)
    assert (out["status"] == 0).all() and out["accepted"].all() and (out["group_status"] == 0).all()
    refs = [check_group(c, grp, out, g, vals, 0.0, f"chart {chart} {name}") for g, (grp, name) in
            enumerate(zip(groups, list(CHAIN_GROUPS) + ["mixed, permuted"]))]
    assert out["group_dof"].tolist() == [6, 18, 12, 25, 25] and out["group_count"].tolist() == [2, 6, 4, 5, 5]
    a, b = out["group_ptr"][3], out["group_ptr"][4]
    assert abs(out["group_d2"][4] - out["group_d2"][3]) <= 2 * bound(c, refs[3]["cond_joint"][-1]) * out["group_d2"][3]
    assert not np.allclose(out["d2_joint"][a:b][perm], out["d2_joint"][b:b + 5], rtol=1e-3)
    assert (np.diff(out["d2_joint"][a:b]) >= 0).all()                      # (a prefix sequence grows)


def many(gpu):
    c = og.case("lc_many_points", 0)
    G, _ = og.device_graph(gpu, "lc_many_points", 0)
    return c, G, og.device_values(G)


def test_lds_boundary_and_capacity(gpu):
    """Groups of 96 rows (the last factored in LDS), 97 and 99 (the first in the work buffer) and exactly 384 (one whole sweep), then
    385 and more: SLIDE_ERR_CAPACITY with zeros, the neighbours served."""
    c, G, vals = many(gpu)
    pts = lambda n, seed: jc.noisy_group(c, vals, [("point", l % 12, 1 + l) for l in range(n)], seed=seed)
    cyl = jc.noisy_group(c, vals, [("cylinder", 5, 0)], seed=40)
    g96, g99, g97, g384 = pts(32, 41), pts(33, 42), pts(30, 43) + cyl, pts(128, 44)
    g387, g391 = pts(129, 45), pts(128, 46) + cyl
    out = G.observation_joint_compatibility([g96, g387, g99, g97, g391, g384], prob=0.0)
    assert out["group_status"].tolist() == [0, CAPACITY, 0, 0, CAPACITY, 0]
    assert out["group_dof"].tolist() == [96, 0, 99, 97, 0, 384] and out["group_count"].tolist() == [32, 0, 33, 31, 0, 128]
    for g in (1, 4):
        a, b = out["group_ptr"][g], out["group_ptr"][g + 1]
        assert out["group_d2"][g] == 0 and (out["status"][a:b] == 0).all()
        for f in ("accepted", "d2_single", "d2_joint", "dof_joint"):
            assert not out[f][a:b].any(), (g, f)
    for g, grp, name in ((0, g96, "96 rows"), (2, g99, "99 rows"), (3, g97, "97 rows"), (5, g384, "384 rows")):
        check_group(c, grp, out, g, vals, 0.0, name)


def test_statuses_inside_a_group(gpu):
    """A landmark named twice: SLIDE_ERR_INVALID for the group, zeros, the neighbours served.  A missing pose or landmark: skipped, the
    others have the values of the group without it, bit for bit."""
    c = og.case("chain40", 0)
    G, _ = og.device_graph(gpu, "chain40", 0)
    vals = og.device_values(G)
    grp = jc.noisy_group(c, vals, CHAIN_GROUPS["mixed"], seed=50)
    twice = grp[:3] + [grp[0]] + grp[3:]
    holes = [grp[0], ("point", 0, 99, 36) + grp[0][4:], grp[1], ("cube", 0, 39, 4) + grp[3][4:], grp[2], grp[3], ("cylinder", 1, 38, 30) + grp[1][4:],
             grp[4]]
    out = G.observation_joint_compatibility([grp, twice, holes], prob=0.0)
    assert out["group_status"].tolist() == [0, INVALID, 0]
    a, b = out["group_ptr"][1], out["group_ptr"][2]
    assert out["group_d2"][1] == 0 and out["group_dof"][1] == 0 and out["group_count"][1] == 0 and (out["status"][a:b] == 0).all()
    for f in ("accepted", "d2_single", "d2_joint", "dof_joint"):
        assert not out[f][a:b].any(), f
    h = out["group_ptr"][2]
    assert out["status"][h:].tolist() == [0, MISSING, 0, MISSING, 0, 0, MISSING, 0]
    keep = h + np.array([0, 2, 4, 5, 7])
    for f in FIELDS:
        assert np.array_equal(out[f][keep], out[f][:5]), f
        assert not out[f][h + np.array([1, 3, 6])].any() or f == "status", f
    for f in ("group_d2", "group_dof", "group_count"):
        assert out[f][2] == out[f][0], f
    check_group(c, grp, out, 0, vals, 0.0, "mixed")
    # a group of missing candidates only, and no groups at all
    none = G.observation_joint_compatibility([[holes[1]], []], prob=0.99)
    assert none["status"].tolist() == [MISSING] and none["group_status"].tolist() == [0, 0] and not none["group_dof"].any()
    empty = G.observation_joint_compatibility([])
    assert len(empty["accepted"]) == 0 and len(empty["group_d2"]) == 0
    _raises("SLIDE_ERR_INVALID", G.observation_joint_compatibility, [grp], 1.0)


def test_groups_do_not_depend_on_their_neighbours(gpu):
    """Groups of 18, 99, 97, 18, 192, 6, 300 and 60 rows in one call: three sweeps.  Every group is bit for bit what the call gives for it
    alone, first in the list and last, under evaluate-only and under the selection."""
    c, G, vals = many(gpu)
    pts = lambda n, seed, at=None: jc.noisy_group(c, vals, [("point", (l % 12) if at is None else at, 1 + l) for l in range(n)], seed=seed, scale=3.0)
    cyl = jc.noisy_group(c, vals, [("cylinder", 5, 0)], seed=60)
    groups = [pts(6, 61, at=11), pts(33, 62), pts(30, 63) + cyl, pts(6, 64), pts(64, 65), pts(2, 66), pts(100, 68), pts(20, 67, at=11)]
    for prob in (0.0, 0.2):
        full = G.observation_joint_compatibility(groups, prob=prob)
        assert (full["group_status"] == 0).all() and (full["status"] == 0).all()
        back = G.observation_joint_compatibility(groups[::-1], prob=prob)
        for g, grp in enumerate(groups):
            same_group(G.observation_joint_compatibility([grp], prob=prob), 0, full, g, ("alone", g, prob))
            same_group(back, len(groups) - 1 - g, full, g, ("reversed", g, prob))
        if prob:
            lens = np.array([len(g) for g in groups])
            assert (full["group_count"] < lens).any() and full["group_count"].any()          # (the selection does select)
            print(f"[joint-compat] selection at {prob}: accepted {full['group_count'].tolist()} of {[len(g) for g in groups]}")


@pytest.mark.parametrize("chart", [0, 1])
def test_selection_on_the_planted_scenarios(gpu, chart):
    """planted40 at prob = 0.99, at the device's own estimate: six ranges moved by +/- 2.5 and +/- 3 sqrt(C_ii[2][2]) (each passes alone
    at 2.5; the rule rejects what no single pose error explains), the all-true group (kept whole) and a group whose first candidate
    fails alone (rejected, the rest kept).  The decisions are the reference's, which stand 1e-3 from every quantile."""
    c = og.case("planted40", chart)
    G, _ = og.device_graph(gpu, "planted40", chart)
    vals = og.device_values(G)
    groups = {"moved 2.5": jc.planted_moved(c, vals, 2.5), "moved 3": jc.planted_moved(c, vals, 3.0), "true": jc.planted_true(c),
              "first fails": jc.planted_moved(c, vals, 5.0, only=(0,))}
    out = G.observation_joint_compatibility(list(groups.values()), prob=0.99)
    assert (out["status"] == 0).all()
    refs = {name: check_group(c, grp, out, g, vals, 0.99, f"chart {chart} {name}") for g, (name, grp) in enumerate(groups.items())}
    if chart == 0:
        assert refs["moved 2.5"]["accepted"].tolist() == [True, False, True, False, True, True]
        assert refs["moved 3"]["accepted"].tolist() == [True, False, True, False, True, False]
    assert (out["d2_single"][:6] < gpu.chi2_quantile(0.99, 3)).all() and out["group_count"][0] < 6
    assert refs["true"]["accepted"].all() and out["group_count"][2] == 6
    assert refs["first fails"]["accepted"].tolist() == [False] + [True] * 5 and out["d2_single"][18] > gpu.chi2_quantile(0.99, 3)
    ev = G.observation_joint_compatibility([groups["moved 2.5"]], prob=0.0)
    assert ev["group_d2"][0] > gpu.chi2_quantile(0.99, 18) and ev["accepted"].all()


def test_the_graph_is_only_read(gpu):
    A, _ = og.device_graph(gpu, "chain40", 0, solve=False)
    B, _ = og.device_graph(gpu, "chain40", 0, solve=False)
    c = og.case("chain40", 0)
    some = [[("point", 0, 7, 0, [1.0, 0.0, 0.0], 5.0)]]
    _raises("SLIDE_ERR_INVALID", A.observation_joint_compatibility, some)          # before the first solve
    for g in (A, B):
        g.set_incremental(True)
        assert g.gauss_newton(1) == 0
    vals = og.device_values(A)
    groups = [jc.noisy_group(c, vals, t, seed=70 + i) for i, t in enumerate(CHAIN_GROUPS.values())]
    flat = [x for grp in groups for x in grp]
    for prob in (0.0, 0.99):
        assert (A.observation_joint_compatibility(groups, prob=prob)["group_status"] == 0).all()
    ga, gb = A.observation_mahalanobis(flat), B.observation_mahalanobis(flat)
    for f in ("d2", "C", "r"):
        assert np.array_equal(ga[f], gb[f]), f
    assert np.array_equal(A.get_pose_covariances(0, range(40)), B.get_pose_covariances(0, range(40)))
    for g in (A, B):
        assert g.gauss_newton(1) == 0
    for p in range(40):
        assert np.array_equal(A.get_pose12(0, p)[1], B.get_pose12(0, p)[1]), p
    A.add_range_bearing(0, 7, 0, [1.0, 0.0, 0.0], 5.0)                            # a factor added and merged, not yet solved
    A.tile_profile()
    _raises("SLIDE_ERR_INVALID", A.observation_joint_compatibility, groups)


def test_noise_is_the_base_noise_under_an_observation_loss(gpu):
    """With a Huber observation loss set the call is served against the reweighted H (test_gpu_observation_gate.py's construction);
    the candidates' own noise is the base noise."""
    sig = oc.mixed_cube_sigmas(0)
    okw, kw = oc.params(0)
    ogr = po.OracleGraph(okw)
    oc.mixed_graph(ogr, sig)
    G = gpu.SlideGraph(gpu.default_params(**kw))
    oc.mixed_graph(G, sig)
    G.set_observation_loss("huber")
    assert G.gauss_newton(1) == 0
    ref = Reference(ogr, 0)
    sel = oc.selected(ref)
    _, H, w, _, _ = oc.obs_step(ref, ref.values, rc.HUBER, 0.0, sel)
    assert (w[sel] < 0.9).sum() >= 3
    ref.delta = 1.00001e-6
    _, H2, _, _, _ = oc.obs_step(ref, ref.values, rc.HUBER, 0.0, sel)
    ref.delta = 1e-6
    wj = np.sqrt(np.diag(H))
    Sig = np.linalg.inv(H)
    kappa = float(np.linalg.cond(H / np.outer(wj, wj)))
    nd = float(np.abs((np.linalg.inv(H2) - Sig) * np.outer(wj, wj)).max() / np.abs(Sig * np.outer(wj, wj)).max())

    class Case:
        chart, bearing_sigma, cyl_sigma, cube_vec = 0, oc.SIGMA, oc.SIGMA, np.full(9, 0.1)
        tol = 8 * H.shape[0] * EPS * kappa + 10 * nd

        def sel(self, kind, robot, pose_idx, lm_idx):
            vp, vl = ref.pose_var(robot, pose_idx), ref.lm_var(og.KIND[kind][2], lm_idx)
            return np.concatenate([np.arange(ref.off[vp], ref.off[vp + 1]), np.arange(ref.off[vl], ref.off[vl + 1])])
    c = Case()
    c.ref, c.Sig = ref, Sig
    vals = og.device_values(G)
    rng = np.random.default_rng(6)
    grp = [og.at_estimate(c, vals, kind, 0, p, l, rng.normal(0, 1, og.KIND[kind][3])) for kind, p, l in
           (("point", 5, 0), ("point", 3, 2), ("cube", 6, 2), ("cylinder", 1, 0), ("cylinder", 9, 4))]
    out = G.observation_joint_compatibility([grp], prob=0.0)
    assert (out["status"] == 0).all()
    check_group(c, grp, out, 0, vals, 0.0, "huber")
    _, Hu = ref.step()
    c.Sig = np.linalg.inv(Hu)
    assert abs(jc.ref_group(c, grp, vals, 0.0)["group_d2"] / out["group_d2"][0] - 1) > 1e-3      # (the weights did enter Sigma)
