"""The individual-compatibility gate of landmark observations on the device (slide_graph_observation_mahalanobis: one forward
substitution per sweep on the resident factor, obs_gate_kernels.hip's k_obs_gate_lin / k_obs_gate_finish, cov_kernels.hip's
k_gram_blocks) against the dense reference of tests/observation_gate_cases.py: Sigma the dense inverse of the full unreduced H, r and
A = [Ap | Al] from the oracle's orc_linearize at the poses and landmarks read back with get_pose12 / get_landmark,
d2_ref = r^T (I + A Sig A^T)^-1 r in numpy.

Tolerances.  d2: tol x cond(C_ref), floor 1e-12, relative to d2_ref, tol the dense inverse's (8 n eps kappa_s + the central-difference
floor: test_gpu_closure_gate.py's bound); C and r entry-wise by the same figure against the largest entry of C_ref (at least 1: C holds
the identity, r is whitened).  The independence checks are bit for bit."""
import os

import numpy as np
import pytest

import observation_gate_cases as og
import observation_loss_cases as oc
import robust_cases as rc
from gn_reference import EPS, Reference
from oracle import pyoracle as po
from test_gpu_marginals import _raises

pytestmark = pytest.mark.gpu

MISSING = 1


def check_gate(c, cands, out, vals, tag):
    rs, _, Cs, d2 = og.ref_gate(c, cands, vals)
    assert (out["status"] == 0).all(), out["status"]
    worst = 0.0
    for k, cand in enumerate(cands):
        m = og.KIND[cand[0]][3]
        assert out["dof"][k] == m
        bound = og.gate_bound(c, Cs[k])
        top = float(np.abs(Cs[k]).max())
        e_d = abs(out["d2"][k] - d2[k]) / d2[k]
        e_C = float(np.abs(out["C"][k][:m, :m] - Cs[k]).max() / top)
        e_r = float(np.abs(out["r"][k][:m] - rs[k]).max() / top)
        print(f"[obs-gate] {tag} {cand[0]} pose {cand[2]} landmark {cand[3]}: d2 {out['d2'][k]:.6g} ref {d2[k]:.6g} err {e_d:.2e}, C {e_C:.2e}, "
              f"r {e_r:.2e} (bound {bound:.2e})")
        assert max(e_d, e_C, e_r) <= bound, (k, e_d, e_C, e_r, bound)
        assert not out["C"][k][m:].any() and not out["C"][k][:, m:].any() and not out["r"][k][m:].any()
        worst = max(worst, max(e_d, e_C, e_r) / bound)
    return d2, worst


@pytest.mark.parametrize("name,chart", [("chain40", 0), ("chain40", 1), ("lc_cylinder", 0), ("lc_cube", 0), ("lc_point", 1)])
def test_gate_vs_reference(gpu, name, chart):
    """Candidates measured at the estimate's own geometry moved by 0.5 x, 2 x and 6 x their sigmas: a pose that already observes the
    landmark and one that does not, the first and the last pose, a landmark with one observer, the same (pose, landmark) twice; a
    landmark seen from every pose of the graph."""
    c = og.case(name, chart)
    G, _ = og.device_graph(gpu, name, chart)
    if name == "chain40":
        assert len(G.tile_profile()) == 4
    vals = og.device_values(G)
    cands = og.perturbed_list(c, vals)
    out = G.observation_mahalanobis(cands)
    d2, worst = check_gate(c, cands, out, vals, f"{name} chart {chart}")
    assert np.array_equal(out["C"], np.transpose(out["C"], (0, 2, 1)))
    print(f"[obs-gate] {name} chart {chart}: largest error / bound {worst:.3e}; d2_ref from {d2.min():.3g} to {d2.max():.3g}")


@pytest.mark.parametrize("chart", [0, 1])
def test_unperturbed_candidate_has_zero_residual(gpu, chart):
    G, _ = og.device_graph(gpu, "chain40", chart)
    c = og.case("chain40", chart)
    vals = og.device_values(G)
    cands = [og.at_estimate(c, vals, kind, 0, p, l, np.zeros(og.KIND[kind][3])) for kind, p, l in
             (("point", 7, 0), ("point", 1, 0), ("cylinder", 13, 6), ("cylinder", 7, 6), ("cube", 12, 3), ("cube", 4, 3))]
    out = G.observation_mahalanobis(cands)
    assert (out["status"] == 0).all()
    assert np.abs(out["r"]).max() < 1e-9 and out["d2"].max() < 1e-15, (out["r"], out["d2"])


@pytest.mark.parametrize("chart", [0, 1])
def test_planted_true_and_false_matches(gpu, chart):
    """planted40: the generator has asserted under d2_ref alone that the true candidates lie below 0.75 of their class's quantile and
    the false ones above twice it; the device puts each on the same side of the quantile, at its own estimate."""
    c = og.case("planted40", chart)
    cands, flags, _, dof = og.planted_list(c)
    G, _ = og.device_graph(gpu, "planted40", chart)
    out = G.observation_mahalanobis(cands)
    assert (out["status"] == 0).all() and (out["dof"] == dof).all()
    q = np.array([gpu.OBSERVATION_GATE_CHI2_99[int(d)] for d in out["dof"]])
    for m in (3, 7, 9):
        s = dof == m
        print(f"[obs-gate] planted chart {chart} dof {m}: true max {out['d2'][s & flags].max():.2f}, false min {out['d2'][s & ~flags].min():.1f} "
              f"(quantile {gpu.OBSERVATION_GATE_CHI2_99[m]})")
    assert ((out["d2"] < q) == flags).all(), (out["d2"], q, flags)
    check_gate(c, cands, out, og.device_values(G), f"planted40 chart {chart}")


def _same(a, b, ka, kb, what):
    for f in ("d2", "C", "r", "dof"):
        assert np.array_equal(a[f][ka], b[f][kb]), (what, f, ka, kb)


def test_candidates_do_not_depend_on_their_neighbours(gpu):
    """129 points, 43 cubes and 55 cylinders (one more than a sweep holds of each), repeating candidates where the graph has fewer
    distinct ones: d2, C and r of a candidate are bit for bit what the call gives for it alone, in its class's list, in a permuted list
    and in a mixed-class list.  A tail candidate (pose >= 30, landmark first seen at pose >= 27: its sweep starts at block column 2 or
    later) gives the same bits alone, beside a candidate at pose 0 and with the walk forced to start at column 0: the short walk changes
    nothing."""
    G, _ = og.device_graph(gpu, "chain40", 1)
    c = og.case("chain40", 1)
    vals = og.device_values(G)
    rng = np.random.default_rng(9)
    lists = {}
    for kind, count in (("point", 129), ("cube", 43), ("cylinder", 55)):
        m = og.KIND[kind][3]
        ids = [k for k in range(0, 40, 3) if kind == "point" or (k % 2 == 0) == (kind == "cylinder")]
        scale = 0.5 if kind == "point" else 1.5           # (a point's sigma is 1 m under the defaults: its range stays positive)
        base = [og.at_estimate(c, vals, kind, 0, int(rng.integers(40)), int(rng.choice(ids)), rng.normal(0, scale, m)) for _ in range(24)]
        lists[kind] = [base[i % 24] for i in range(count)]
    fulls = {}
    for kind, cl in lists.items():
        full = fulls[kind] = G.observation_mahalanobis(cl)
        assert (full["status"] == 0).all() and (full["d2"] > 0).all()
        for k in list(range(24)) + [len(cl) - 1]:                                # every distinct candidate alone, and the second sweep's
            _same(G.observation_mahalanobis([cl[k]]), full, 0, k, kind)
        _same(full, full, 24, 0, kind)                                           # exact duplicates
        perm = rng.permutation(len(cl))
        sh = G.observation_mahalanobis([cl[k] for k in perm])
        for f in ("d2", "C", "r"):
            assert np.array_equal(sh[f], full[f][perm]), (kind, f)
        assert np.array_equal(full["C"], np.transpose(full["C"], (0, 2, 1)))
    mixed = [lists[kind][i] for i in range(20) for kind in ("cube", "point", "cylinder")]
    mx = G.observation_mahalanobis(mixed)
    for i in range(20):
        for n, kind in enumerate(("cube", "point", "cylinder")):
            _same(fulls[kind], mx, i, 3 * i + n, "mixed " + kind)
    # the short walk: tail candidates alone (their sweep starts at block column >= 2) and beside a candidate at pose 0 (column 0)
    head = {kind: og.at_estimate(c, vals, kind, 0, 0, l, rng.normal(0, 1, og.KIND[kind][3])) for kind, l in
            (("point", 0), ("cylinder", 0), ("cube", 3))}
    for kind, p, l in (("point", 39, 36), ("point", 31, 30), ("cylinder", 38, 36), ("cylinder", 33, 30), ("cube", 39, 39), ("cube", 30, 27)):
        assert p >= 30 and l >= 27 and (6 * min(p, l)) // 64 >= 2
        tail = og.at_estimate(c, vals, kind, 0, p, l, rng.normal(0, 1, og.KIND[kind][3]))
        alone = G.observation_mahalanobis([tail])
        both = G.observation_mahalanobis([head[kind], tail])
        assert alone["status"][0] == 0 and alone["d2"][0] > 0
        _same(alone, both, 0, 1, ("tail", kind, p, l))
        os.environ["SLIDE_OBS_GATE_FULL_WALK"] = "1"                             # the library's measurement aid: every sweep walks from column 0
        try:
            forced = G.observation_mahalanobis([tail])
        finally:
            del os.environ["SLIDE_OBS_GATE_FULL_WALK"]
        _same(alone, forced, 0, 0, ("tail, full walk", kind, p, l))


def test_statuses_refusals_and_the_graph_is_left_as_it_was(gpu):
    A, _ = og.device_graph(gpu, "chain40", 0, solve=False)
    B, _ = og.device_graph(gpu, "chain40", 0, solve=False)
    c = og.case("chain40", 0)
    some = [("point", 0, 7, 0, [1.0, 0.0, 0.0], 5.0)]
    _raises("SLIDE_ERR_INVALID", A.observation_mahalanobis, some)                # before the first solve
    for g in (A, B):
        g.set_incremental(True)
        assert g.gauss_newton(1) == 0
    vals = og.device_values(A)
    rng = np.random.default_rng(4)
    cands = [og.at_estimate(c, vals, kind, 0, p, l, rng.normal(0, 1, og.KIND[kind][3])) for kind, p, l in
             (("point", 7, 0), ("cube", 12, 3), ("cylinder", 13, 6), ("point", 39, 39))]
    closures = [(0, 35, 0, 1, [0.0, 0, 0, 0, 0, 0, 1], [0.01] * 3 + [0.05] * 3), (0, 20, 0, 3, [1.0, 0, 0, 0, 0, 0, 1], [0.01] * 3 + [0.05] * 3)]
    gate_b = B.closure_mahalanobis(closures)
    good = A.observation_mahalanobis(cands)
    assert (good["status"] == 0).all() and good["dof"].tolist() == [3, 9, 7, 3]
    # an unknown pose and an unknown landmark: their own status and zeros, the neighbours served
    mixed = cands[:2] + [("point", 0, 99, 0) + cands[0][4:], ("cube", 0, 12, 4) + cands[1][4:], ("cylinder", 1, 13, 6) + cands[2][4:]] + cands[2:]
    out = A.observation_mahalanobis(mixed)
    assert out["status"].tolist() == [0, 0, MISSING, MISSING, MISSING, 0, 0]
    assert out["dof"].tolist() == [3, 9, 3, 9, 7, 7, 3]
    for k in (2, 3, 4):
        assert out["d2"][k] == 0 and not out["C"][k].any() and not out["r"][k].any()
    for f in ("d2", "C", "r"):
        assert np.array_equal(out[f][[0, 1, 5, 6]], good[f]), f
    # the empty list, and an argument refusal on a live graph
    empty = A.observation_mahalanobis([])
    assert len(empty["d2"]) == 0 and empty["C"].shape == (0, 9, 9)
    _raises("SLIDE_ERR_INVALID", A.observation_mahalanobis, [("point", 0, 7, 0, [0.0, 0.0, 0.0], 5.0)])
    _raises("SLIDE_ERR_INVALID", A.observation_mahalanobis, [("point", 13, 7, 0, [1.0, 0.0, 0.0], 5.0)])
    # the graph is only read: marginals, the closure gate and the next step's poses are those of a graph never queried
    assert np.array_equal(A.get_pose_covariances(0, range(40)), B.get_pose_covariances(0, range(40)))
    gate_a = A.closure_mahalanobis(closures)
    for f in ("d2", "C", "r"):
        assert np.array_equal(gate_a[f], gate_b[f]), f
    for g in (A, B):
        assert g.gauss_newton(1) == 0
    for p in range(40):
        assert np.array_equal(A.get_pose12(0, p)[1], B.get_pose12(0, p)[1]), p
    assert A.observation_mahalanobis(cands)["status"].tolist() == [0, 0, 0, 0]
    # a factor added and merged, not yet solved: whole-call refusal
    A.add_range_bearing(0, 7, 0, [1.0, 0.0, 0.0], 5.0)
    A.tile_profile()
    _raises("SLIDE_ERR_INVALID", A.observation_mahalanobis, cands)
    # a graph joined to a CholBatch
    batch = gpu.CholBatch(1)
    B.join_chol_batch(batch, 0)
    _raises("SLIDE_ERR_INVALID", B.observation_mahalanobis, cands)
    B.join_chol_batch(None)


def test_gate_noise_is_the_base_noise_under_an_observation_loss(gpu):
    """With an observation loss set the call is served; H is the reweighted system (the reference is built from the factors scaled by
    the loss's weights at the linearisation point, observation_loss_cases.obs_step), the candidate's own noise is the base noise and
    C's identity is unscaled."""
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
    assert (w[sel] < 0.9).sum() >= 3                                      # the loss does reweight this graph
    ref.delta = 1.00001e-6
    _, H2, _, _, _ = oc.obs_step(ref, ref.values, rc.HUBER, 0.0, sel)
    ref.delta = 1e-6
    wj = np.sqrt(np.diag(H))
    Sig = np.linalg.inv(H)
    kappa = float(np.linalg.cond(H / np.outer(wj, wj)))
    nd = float(np.abs((np.linalg.inv(H2) - Sig) * np.outer(wj, wj)).max() / np.abs(Sig * np.outer(wj, wj)).max())

    class Case:                                                            # what ref_gate reads of a case
        chart, bearing_sigma, cyl_sigma, cube_vec = 0, oc.SIGMA, oc.SIGMA, np.full(9, 0.1)
        tol = 8 * H.shape[0] * EPS * kappa + 10 * nd

        def sel(self, kind, robot, pose_idx, lm_idx):
            vp, vl = ref.pose_var(robot, pose_idx), ref.lm_var(og.KIND[kind][2], lm_idx)
            return np.concatenate([np.arange(ref.off[vp], ref.off[vp + 1]), np.arange(ref.off[vl], ref.off[vl + 1])])
    c = Case()
    c.ref, c.Sig = ref, Sig
    vals = og.device_values(G)
    rng = np.random.default_rng(6)
    cands = [og.at_estimate(c, vals, kind, 0, p, l, rng.normal(0, 1, og.KIND[kind][3])) for kind, p, l in
             (("point", 5, 0), ("point", 3, 2), ("cube", 6, 2), ("cylinder", 1, 0), ("cylinder", 9, 4))]
    out = G.observation_mahalanobis(cands)
    check_gate(c, cands, out, vals, "huber")
    # the same candidates against the unweighted H differ: the weights did enter Sigma
    _, Hu = ref.step()
    c.Sig = np.linalg.inv(Hu)
    _, _, _, d2u = og.ref_gate(c, cands, vals)
    assert np.abs(d2u / out["d2"] - 1).max() > 1e-3
