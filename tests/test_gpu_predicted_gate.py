"""The observation gate at a PREDICTED pose on the device (slide_graph_predicted_observation_mahalanobis: obs_gate_kernels.hip's
k_obs_gate_lin_pred, then the observation gate's own forward substitution, gram and k_obs_gate_finish) against the dense reference of
tests/predicted_gate_cases.py: the AUGMENTED H — the graph's full unreduced H plus the new pose and its Between factor, the oracle's
Between Jacobians at the poses read back with get_pose12 — inverted densely, r and A = [Ap | Al] from the oracle's orc_linearize at the
predicted pose and the landmark read back with get_landmark, d2_ref = r^T (I + A Sig_aug A^T)^-1 r in numpy.

Tolerances.  observation_gate_cases.gate_bound as it stands: tol x cond(C_ref), floor 1e-12, relative to d2_ref; C and r entry-wise by
the same figure against the largest entry of C_ref.  The independence checks are bit for bit.

Measured on an MI355X, largest error / gate_bound over each graph's three from poses, chart 0 | chart 1: chain40 2.1e-3 | 1.4e-3,
lc_point 4.6e-6 | 4.5e-6, lc_cube 3.5e-2 | 1.3e-2, lc_cylinder 1.0e-2 | 1.6e-2, planted40 7.8e-3 | 6.3e-3.  Planted, as fractions of
the class's 0.99 quantile: true at most 0.69 (points), 0.20 (cylinders), 0.27 (cubes); false at least 46, 162, 2.25 (DESIGN.md 7,
"The gate at the predicted pose")."""
import numpy as np
import pytest

import observation_gate_cases as og
import observation_loss_cases as oc
import predicted_gate_cases as pg
import robust_cases as rc
from gn_reference import EPS, Reference
from oracle import pyoracle as po
from test_gpu_marginals import _raises

pytestmark = pytest.mark.gpu

MISSING = 1
XI = np.array([0.01, -0.02, 0.015, 0.05, -0.04, 0.02])      # the odometry noise of the predictions that are not drawn


def check_gate(c, frm, rel7, est7, cands, out, vals, tag, odom=None):
    rs, Cs, d2 = pg.ref_gate(c, 0, frm, rel7, est7, cands, vals, odom)
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
        print(f"[pred-gate] {tag} from {frm} {cand[0]} {cand[3]}: d2 {out['d2'][k]:.6g} ref {d2[k]:.6g} err {e_d:.2e}, C {e_C:.2e}, r {e_r:.2e} "
              f"(bound {bound:.2e})")
        assert max(e_d, e_C, e_r) <= bound, (k, e_d, e_C, e_r, bound)
        assert not out["C"][k][m:].any() and not out["C"][k][:, m:].any() and not out["r"][k][m:].any()
        worst = max(worst, max(e_d, e_C, e_r) / bound)
    return d2, worst


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("name", ["chain40", "lc_point", "lc_cube", "lc_cylinder", "planted40"])
def test_gate_vs_augmented_reference(gpu, name, chart):
    """From the first, a middle and the newest pose: candidates of the three classes measured from the predicted pose at the
    landmarks' own estimates moved by 0.5 x, 2 x and 6 x their sigmas — landmarks the from pose observes and ones it does not, a
    landmark with ONE observer (chain40's point 39 and cube 39: from pose 39 is that observer, poses 0 and 20 are not), a landmark
    seen from every pose (lc_*)."""
    c = og.case(name, chart)
    G, _ = og.device_graph(gpu, name, chart)
    vals = og.device_values(G)
    worst = 0.0
    for frm in pg.FROMS[name]:
        rel7, est7 = pg.predict(vals, 0, frm, pg.STEP, XI)
        cands = pg.perturbed_list(c, vals, frm, est7, pg.LANDMARKS[name], seed=3 + frm)
        out = G.predicted_observation_mahalanobis(0, frm, rel7, est7, cands)
        _, w = check_gate(c, frm, rel7, est7, cands, out, vals, f"{name} chart {chart}")
        assert np.array_equal(out["C"], np.transpose(out["C"], (0, 2, 1)))
        worst = max(worst, w)
    print(f"[pred-gate] {name} chart {chart}: largest error / bound {worst:.3e}")


@pytest.mark.parametrize("chart", [0, 1])
def test_prediction_at_an_existing_pose_differs_from_the_in_graph_gate_by_the_odometry_term(gpu, chart):
    """A prediction that coincides with the from pose (rel = identity) has Ad = I: its C is the in-graph gate's C at that pose plus
    Ap diag(s^2) Ap^T, s = odom x noise_floor — both calls on one graph, compared to 1e-9 of the largest entry."""
    c = og.case("chain40", chart)
    G, _ = og.device_graph(gpu, "chain40", chart)
    vals = og.device_values(G)
    ident = (np.eye(3), np.zeros(3))
    rel7, est7 = pg.predict(vals, 0, 20, ident)
    cands = pg.perturbed_list(c, vals, 20, est7, [("point", 18), ("cylinder", 18), ("cube", 21)], seed=8)
    a = G.observation_mahalanobis(cands)
    b = G.predicted_observation_mahalanobis(0, 20, rel7, est7, cands)
    s2 = pg.between_sigmas(pg.odom_sigma(c), rel7) ** 2
    for k, cand in enumerate(cands):
        m = og.KIND[cand[0]][3]
        _, Ap, _ = og.linearize(c, cand, pg.at_prediction(vals, est7))
        want = a["C"][k][:m, :m] + Ap @ np.diag(s2) @ Ap.T
        assert np.abs(b["C"][k][:m, :m] - want).max() <= 1e-9 * np.abs(want).max()
        assert np.abs(b["r"][k] - a["r"][k]).max() <= 1e-9 * max(1.0, np.abs(a["r"][k]).max())


@pytest.mark.parametrize("chart", [0, 1])
def test_planted_true_and_false_matches(gpu, chart):
    """planted40: the generator has asserted under d2_ref alone that the true candidates lie below 0.75 of their class's 0.99 quantile
    and the false ones above 1.5 of it; the device puts each on the same side of the quantile, at its own estimate of pose 39 and of
    the landmarks, and meets the reference there."""
    c = og.case("planted40", chart)
    G, _ = og.device_graph(gpu, "planted40", chart)
    vals = og.device_values(G)
    rel7, est7, cands, flags, _, dof = pg.planted(c, vals)
    out = G.predicted_observation_mahalanobis(0, 39, rel7, est7, cands)
    assert (out["status"] == 0).all() and (out["dof"] == dof).all()
    q = np.array([gpu.chi2_quantile(0.99, int(d)) for d in out["dof"]])
    for m in (3, 7, 9):
        s = dof == m
        print(f"[pred-gate] planted chart {chart} dof {m}: true max {out['d2'][s & flags].max():.2f} ({out['d2'][s & flags].max() / q[s][0]:.2f} "
              f"of the quantile), false min {out['d2'][s & ~flags].min():.1f} ({out['d2'][s & ~flags].min() / q[s][0]:.2f})")
    assert ((out["d2"] < q) == flags).all(), (out["d2"], q, flags)
    check_gate(c, 39, rel7, est7, cands, out, vals, f"planted40 chart {chart}")


def _same(a, b, ka, kb, what):
    for f in ("d2", "C", "r", "dof"):
        assert np.array_equal(a[f][ka], b[f][kb]), (what, f, ka, kb)


def test_candidates_do_not_depend_on_their_neighbours(gpu):
    """129 points, 43 cubes and 55 cylinders (one more than a sweep holds of each), repeating candidates where the graph has fewer
    distinct ones: d2, C and r of a candidate are bit for bit what the call gives for it alone, in its class's list, in a permuted
    list and in a mixed-class list; C is symmetric bit for bit.  A candidate whose landmark is first seen late (its sweep's walk
    starts at block column >= 2 from pose 39) gives the same bits beside one whose landmark is first seen at pose 0."""
    G, _ = og.device_graph(gpu, "chain40", 1)
    c = og.case("chain40", 1)
    vals = og.device_values(G)
    rng = np.random.default_rng(9)
    frm = 20
    rel7, est7 = pg.predict(vals, 0, frm, pg.STEP, XI)
    X = pg.cc._pose(est7, np.float64)
    call = lambda cl: G.predicted_observation_mahalanobis(0, frm, rel7, est7, cl)
    lists = {}
    for kind, count in (("point", 129), ("cube", 43), ("cylinder", 55)):
        m = og.KIND[kind][3]
        ids = [k for k in range(0, 40, 3) if kind == "point" or (k % 2 == 0) == (kind == "cylinder")]
        scale = 0.5 if kind == "point" else 1.5
        base = []
        for _ in range(24):
            l = int(rng.choice(ids))
            base.append(og.observe(c, kind, 0, frm, l, X, og.lm_value(kind, vals.lm(kind, l)), rng.normal(0, scale, m)))
        lists[kind] = [base[i % 24] for i in range(count)]
    fulls = {}
    for kind, cl in lists.items():
        full = fulls[kind] = call(cl)
        assert (full["status"] == 0).all() and (full["d2"] > 0).all()
        for k in list(range(24)) + [len(cl) - 1]:                                # every distinct candidate alone, and the second sweep's
            _same(call([cl[k]]), full, 0, k, kind)
        _same(full, full, 24, 0, kind)
        perm = rng.permutation(len(cl))
        sh = call([cl[k] for k in perm])
        for f in ("d2", "C", "r"):
            assert np.array_equal(sh[f], full[f][perm]), (kind, f)
        assert np.array_equal(full["C"], np.transpose(full["C"], (0, 2, 1)))
    mixed = [lists[kind][i] for i in range(20) for kind in ("cube", "point", "cylinder")]
    mx = call(mixed)
    for i in range(20):
        for n, kind in enumerate(("cube", "point", "cylinder")):
            _same(fulls[kind], mx, i, 3 * i + n, "mixed " + kind)
    # the short walk from the newest pose
    rel39, est39 = pg.predict(vals, 0, 39, pg.STEP, XI)
    X39 = pg.cc._pose(est39, np.float64)
    for kind, l_tail, l_head in (("point", 36, 0), ("cylinder", 36, 0), ("cube", 39, 3)):
        mk = lambda l: og.observe(c, kind, 0, 39, l, X39, og.lm_value(kind, vals.lm(kind, l)), rng.normal(0, 0.5, og.KIND[kind][3]))
        assert (6 * min(39, l_tail)) // 64 >= 2
        tail, head = mk(l_tail), mk(l_head)
        alone = G.predicted_observation_mahalanobis(0, 39, rel39, est39, [tail])
        both = G.predicted_observation_mahalanobis(0, 39, rel39, est39, [head, tail])
        assert alone["status"][0] == 0 and alone["d2"][0] > 0
        _same(alone, both, 0, 1, ("tail", kind))


def test_statuses_refusals_and_the_graph_is_left_as_it_was(gpu):
    A, _ = og.device_graph(gpu, "chain40", 0, solve=False)
    B, _ = og.device_graph(gpu, "chain40", 0, solve=False)
    c = og.case("chain40", 0)
    I7 = [0.0, 0, 0, 0, 0, 0, 1]
    some = [("point", 0, 0, 0, [1.0, 0.0, 0.0], 5.0)]
    # before the first solve: a from pose the graph will never hold is SLIDE_MISSING (that check comes first); one it was given
    # is refused either as not uploaded yet (SLIDE_MISSING) or for the missing factorisation (SLIDE_ERR_INVALID)
    _raises("SLIDE_MISSING", A.predicted_observation_mahalanobis, 0, 99, I7, I7, some)
    _raises("SLIDE_", A.predicted_observation_mahalanobis, 0, 7, I7, I7, some)
    for g in (A, B):
        g.set_incremental(True)
        assert g.gauss_newton(1) == 0
    vals = og.device_values(A)
    rel7, est7 = pg.predict(vals, 0, 39, pg.STEP, XI)
    cands = pg.perturbed_list(c, vals, 39, est7, [("point", 0), ("cube", 3), ("cylinder", 6), ("point", 39)], seed=4)
    call = lambda g, cl, frm=39: g.predicted_observation_mahalanobis(0, frm, rel7, est7, cl)
    closures = [(0, 35, 0, 1, I7, [0.01] * 3 + [0.05] * 3), (0, 20, 0, 3, [1.0, 0, 0, 0, 0, 0, 1], [0.01] * 3 + [0.05] * 3)]
    in_graph = [og.at_estimate(c, vals, kind, 0, p, l, np.full(og.KIND[kind][3], 0.3)) for kind, p, l in (("point", 7, 0), ("cube", 12, 3))]
    gate_b, obs_b = B.closure_mahalanobis(closures), B.observation_mahalanobis(in_graph)
    good = call(A, cands)
    assert (good["status"] == 0).all() and good["dof"].tolist() == [3, 9, 7, 3]
    # an unknown landmark: its own status and zeros, the neighbours served; the tuple's robot and pose fields are ignored
    mixed = cands[:2] + [("cube", 0, 39, 4) + cands[1][4:], ("point", 0, 39, 1) + cands[0][4:]] + cands[2:]
    mixed[0] = ("point", 5, 999, 0) + cands[0][4:]
    out = call(A, mixed)
    assert out["status"].tolist() == [0, 0, MISSING, MISSING, 0, 0]
    assert out["dof"].tolist() == [3, 9, 9, 3, 7, 3]
    for k in (2, 3):
        assert out["d2"][k] == 0 and not out["C"][k].any() and not out["r"][k].any()
    for f in ("d2", "C", "r"):
        assert np.array_equal(out[f][[0, 1, 4, 5]], good[f]), f
    # a from pose the graph does not hold, of this robot and of another
    _raises("SLIDE_MISSING", call, A, cands, 40)
    _raises("SLIDE_MISSING", A.predicted_observation_mahalanobis, 1, 39, rel7, est7, cands)
    # the empty list, and argument refusals on a live graph
    empty = call(A, [])
    assert len(empty["d2"]) == 0 and empty["C"].shape == (0, 9, 9)
    _raises("SLIDE_ERR_INVALID", call, A, [("point", 0, 39, 0, [0.0, 0.0, 0.0], 5.0)])
    _raises("SLIDE_ERR_INVALID", A.predicted_observation_mahalanobis, 13, 39, rel7, est7, cands)
    _raises("SLIDE_ERR_INVALID", A.predicted_observation_mahalanobis, 0, 39, [0.0] * 7, est7, cands)
    _raises("SLIDE_ERR_INVALID", A.predicted_observation_mahalanobis, 0, 39, rel7, [np.nan] + list(est7[1:]), cands)
    # the graph is only read: marginals, the two in-graph gates and the next step's poses are those of a graph never queried
    assert np.array_equal(A.get_pose_covariances(0, range(40)), B.get_pose_covariances(0, range(40)))
    gate_a, obs_a = A.closure_mahalanobis(closures), A.observation_mahalanobis(in_graph)
    for f in ("d2", "C", "r"):
        assert np.array_equal(gate_a[f], gate_b[f]), f
        assert np.array_equal(obs_a[f], obs_b[f]), f
    for g in (A, B):
        assert g.gauss_newton(1) == 0
    for p in range(40):
        assert np.array_equal(A.get_pose12(0, p)[1], B.get_pose12(0, p)[1]), p
    assert A.get_pose12(0, 40)[0] == MISSING
    assert call(A, cands)["status"].tolist() == [0, 0, 0, 0]
    # a factor added and merged, not yet solved: whole-call refusal
    A.add_range_bearing(0, 7, 0, [1.0, 0.0, 0.0], 5.0)
    A.tile_profile()
    _raises("SLIDE_ERR_INVALID", call, A, cands)
    # a graph joined to a CholBatch
    batch = gpu.CholBatch(1)
    B.join_chol_batch(batch, 0)
    _raises("SLIDE_ERR_INVALID", call, B, cands)
    B.join_chol_batch(None)


def test_gate_noise_is_the_base_noise_under_an_observation_loss(gpu):
    """With a Huber observation loss set the call is served; H is the reweighted system (the reference's H is built from the factors
    scaled by the loss's weights at the linearisation point, observation_loss_cases.obs_step, and then augmented), the candidate's own
    noise and the Between's are the base noise."""
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

    class Case:                                                            # what ref_gate reads of a case
        chart, bearing_sigma, cyl_sigma, cube_vec = 0, oc.SIGMA, oc.SIGMA, np.full(9, 0.1)
        tol = 8 * H.shape[0] * EPS * kappa + 10 * nd
    c = Case()
    c.ref, c.H = ref, H
    odom = np.array(list(okw.odom_sigma))
    vals = og.device_values(G)
    frm = 11                                                               # (the chain's newest pose)
    rel7, est7 = pg.predict(vals, 0, frm, pg.STEP, XI)
    cands = pg.perturbed_list(c, vals, frm, est7, [("point", 0), ("point", 2), ("cube", 2), ("cylinder", 0), ("cylinder", 4)], seed=6)
    out = G.predicted_observation_mahalanobis(0, frm, rel7, est7, cands)
    check_gate(c, frm, rel7, est7, cands, out, vals, "huber", odom)
    # the same candidates against the unweighted H differ: the weights did enter
    _, c.H = ref.step()
    _, _, d2u = pg.ref_gate(c, 0, frm, rel7, est7, cands, vals, odom)
    assert np.abs(d2u / out["d2"] - 1).max() > 1e-3
