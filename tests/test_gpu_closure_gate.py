"""The individual-compatibility gate of loop closures and the joint marginal of pose pairs on the device
(slide_graph_closure_mahalanobis / slide_graph_get_pose_pair_covariances: one forward substitution per sweep on the resident factor,
closure_kernels.hip's k_closure_gate_lin / k_closure_gate_finish, cov_kernels.hip's k_gram_blocks) against the dense reference of
tests/closure_gate_cases.py: Sigma the dense inverse of the full unreduced H, r and A from the oracle's orc_linearize at the poses
read back with get_pose12, d2_ref = r^T (I + A Sig_pp A^T)^-1 r in numpy.

Tolerances.  A pair block: every entry, Jacobi-scaled as test_gpu_marginals.check_marginals scales, within that test's `tol`
(8 n eps kappa_s + the central-difference floor).  d2: tol x cond(C_ref), floor 1e-12, relative to d2_ref; C and r entry-wise by the
same figure against their largest entry.  Two routes to one block (pair block against get_pose_covariances, (a, b) against (b, a)):
1e-9 relative, the project's figure.  The independence checks are bit for bit."""
import numpy as np
import pytest

import closure_cases as cc
import closure_gate_cases as gc
from test_gpu_marginals import _raises

pytestmark = pytest.mark.gpu

MISSING, INVALID = 1, -1
GRAPHS3 = ["chain40", "loop36", "two_robots"]


def dev_pose12(G):
    def f(robot, idx):
        st, p = G.get_pose12(robot, idx)
        assert st == 0
        return p
    return f


def swap_blocks(b):
    return np.block([[b[6:, 6:], b[6:, :6]], [b[:6, 6:], b[:6, :6]]])


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("name", GRAPHS3)
def test_pair_covariance_vs_dense_inverse(gpu, chart, name):
    c = gc.case(name, chart)
    G, _ = gc.device_graph(gpu, name, chart)
    if name == "chain40":
        assert len(G.tile_profile()) == 4                                # first and last block columns differ
    pairs = gc.PAIRS[name]
    got, st = G.get_pose_pair_covariances(pairs)
    assert got.shape == (len(pairs), 12, 12) and (st == 0).all(), st
    worst = worst_diag = worst_swap = 0.0
    for k, (ra, ia, rb, ib) in enumerate(pairs):
        want, w = c.pair_sigma(ra, ia, rb, ib)
        worst = max(worst, float(np.abs((got[k] - want) * np.outer(w, w)).max() / c.scale))
        assert np.array_equal(got[k], got[k].T)
        da, db = G.get_pose_covariances(ra, [ia])[0], G.get_pose_covariances(rb, [ib])[0]
        worst_diag = max(worst_diag, float(np.abs(got[k][:6, :6] - da).max() / np.abs(da).max()),
                         float(np.abs(got[k][6:, 6:] - db).max() / np.abs(db).max()))
        if (rb, ib, ra, ia) in pairs:
            other = got[pairs.index((rb, ib, ra, ia))]
            worst_swap = max(worst_swap, float(np.abs(swap_blocks(other) - got[k]).max() / np.abs(got[k]).max()))
    print(f"[pair-cov] {name} chart {chart}: vs dense inverse {worst:.3e} (tol {c.tol:.2e}, kappa {c.kappa:.2e}), diagonal blocks vs "
          f"get_pose_covariances {worst_diag:.2e}, (b, a) vs (a, b) {worst_swap:.2e}")
    assert worst <= c.tol, (worst, c.tol, c.kappa)
    assert worst_diag <= 1e-9 and worst_swap <= 1e-9, (worst_diag, worst_swap)
    assert sum((p[2], p[3], p[0], p[1]) in pairs for p in pairs) >= 2


def check_gate(c, closures, out, pose12, tag):
    r, _, Cm, d2 = gc.ref_gate(c, closures, pose12)
    assert (out["status"] == 0).all(), out["status"]
    worst = 0.0
    for k in range(len(closures)):
        bound = gc.gate_bound(c, Cm[k])
        e_d = abs(out["d2"][k] - d2[k]) / d2[k]
        e_C = float(np.abs(out["C"][k] - Cm[k]).max() / np.abs(Cm[k]).max())
        e_r = float(np.abs(out["r"][k] - r[k]).max() / np.abs(r[k]).max())
        print(f"[gate] {tag} closure {k}: d2 {out['d2'][k]:.6g} ref {d2[k]:.6g} err {e_d:.2e}, C {e_C:.2e}, r {e_r:.2e} (bound {bound:.2e})")
        assert max(e_d, e_C, e_r) <= bound, (k, e_d, e_C, e_r, bound)
        worst = max(worst, max(e_d, e_C, e_r) / bound)
    return d2, worst


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("name", GRAPHS3)
def test_gate_vs_reference(gpu, chart, name):
    """Closures measured at the estimate's own relative pose times a fixed-seed tangent vector of 0.5 x, 2 x and 10 x their sigmas,
    the sigmas varied per closure; ends far apart, neighbours, both senses, two robots."""
    c = gc.case(name, chart)
    G, _ = gc.device_graph(gpu, name, chart)
    pose12 = dev_pose12(G)
    closures = gc.perturbed_list(name, pose12)
    assert len(closures) == 18 and len({tuple(x[5]) for x in closures}) == 18
    out = G.closure_mahalanobis(closures)
    d2, worst = check_gate(c, closures, out, pose12, f"{name} chart {chart}")
    assert np.array_equal(out["C"], np.transpose(out["C"], (0, 2, 1)))
    print(f"[gate] {name} chart {chart}: largest error / bound {worst:.3e}; d2_ref from {d2.min():.3g} to {d2.max():.3g}")


@pytest.mark.parametrize("chart", [0, 1])
def test_unperturbed_closure_has_zero_residual(gpu, chart):
    """rel7 exactly the estimate's X_from^-1 X_to: |r| < 1e-9 and d2 < 1e-15 — a wrong from / to sense or a missing inverse fails
    here (the swapped twin of the same closure is far outside the gate)."""
    G, _ = gc.device_graph(gpu, "two_robots", chart)
    pose12 = dev_pose12(G)
    ends = [(0, 23, 0, 1), (0, 20, 1, 2), (1, 15, 0, 0), (0, 6, 0, 5)]
    closures = [gc.measured(pose12, *e, np.zeros(6)) for e in ends]
    out = G.closure_mahalanobis(closures)
    assert (out["status"] == 0).all()
    assert np.abs(out["r"]).max() < 1e-9 and out["d2"].max() < 1e-15, (out["r"], out["d2"])
    swapped = [(x[2], x[3], x[0], x[1], x[4], x[5]) for x in closures[:3]]
    assert G.closure_mahalanobis(swapped)["d2"].min() > 100.0


@pytest.mark.parametrize("chart", [0, 1])
def test_planted_true_and_false_closures(gpu, chart):
    """noisy40: the generator has asserted under d2_ref alone that the true closures lie below 16.81 / 2 and the false ones above
    4 x 16.81; the device ranks each on the same side of 16.81 — at its own estimate, and within the bound of d2_ref there."""
    c = gc.case("noisy40", chart)
    closures, flags, d2_cpu = gc.planted_list(c)
    G, _ = gc.device_graph(gpu, "noisy40", chart)
    out = G.closure_mahalanobis(closures)
    assert (out["status"] == 0).all()
    assert ((out["d2"] < gc.GATE2) == flags).all(), (out["d2"], flags)
    check_gate(c, closures, out, dev_pose12(G), f"noisy40 planted chart {chart}")
    print(f"[gate] planted chart {chart}: true max {out['d2'][flags].max():.2f}, false min {out['d2'][~flags].min():.1f}")


def test_candidates_do_not_depend_on_their_neighbours(gpu):
    """65 candidates (a second sweep of one) with duplicates, two candidates sharing a pose, and one whose from is another's to: d2, C
    and r of candidate k are bit for bit what the call gives for it alone, first, last, and in a permuted list.  The same for 33 pairs."""
    G, _ = gc.device_graph(gpu, "chain40", 1)
    pose12 = dev_pose12(G)
    rng = np.random.default_rng(9)
    ends = []
    while len(ends) < 61:
        i, j = int(rng.integers(40)), int(rng.integers(40))
        if i != j:
            ends.append((0, i, 0, j))
    ends += [ends[0], ends[7], (0, ends[3][1], 0, 38 if ends[3][1] != 38 else 37), (0, ends[5][3], 0, ends[5][1])]
    closures = [gc.measured(pose12, *e, rng.normal(0, 1, 6) * cc.CLOSURE_SIGMA6 * 2, cc.CLOSURE_SIGMA6 * rng.uniform(0.5, 2.0, 6)) for e in ends]
    closures[61], closures[62] = closures[0], closures[7]                      # exact duplicates
    assert len(closures) == 65
    full = G.closure_mahalanobis(closures)
    assert (full["status"] == 0).all() and (full["d2"] > 0).all()
    for k in (0, 64, 63, 17):
        one = G.closure_mahalanobis([closures[k]])
        for f in ("d2", "C", "r"):
            assert np.array_equal(one[f][0], full[f][k]), (k, f)
    assert np.array_equal(full["d2"][61], full["d2"][0]) and np.array_equal(full["C"][62], full["C"][7])
    perm = rng.permutation(65)
    sh = G.closure_mahalanobis([closures[k] for k in perm])
    for f in ("d2", "C", "r"):
        assert np.array_equal(sh[f], full[f][perm]), f
    # pairs: 33 cross the sweep boundary of 32
    pairs = [(e[0], e[1], e[2], e[3]) for e in ends[:33]]
    pf, st = G.get_pose_pair_covariances(pairs)
    assert (st == 0).all()
    for k in (0, 32, 11):
        assert np.array_equal(G.get_pose_pair_covariances([pairs[k]])[0][0], pf[k]), k
    pp = rng.permutation(33)
    assert np.array_equal(G.get_pose_pair_covariances([pairs[k] for k in pp])[0], pf[pp])


def test_statuses_refusals_and_the_graph_is_left_as_it_was(gpu):
    A, _ = gc.device_graph(gpu, "loop36", 0, solve=False)
    B, _ = gc.device_graph(gpu, "loop36", 0, solve=False)
    I7 = [0.0, 0, 0, 0, 0, 0, 1]
    some = [(0, 30, 0, 2, I7, cc.CLOSURE_SIGMA6)]
    _raises("SLIDE_ERR_INVALID", A.closure_mahalanobis, some)                   # before the first solve
    _raises("SLIDE_ERR_INVALID", A.get_pose_pair_covariances, [(0, 1, 0, 2)])
    for g in (A, B):
        g.set_incremental(True)
        assert g.gauss_newton(1) == 0
    pose12 = dev_pose12(A)
    rng = np.random.default_rng(4)
    closures = [gc.measured(pose12, 0, i, 0, j, rng.normal(0, 1, 6) * cc.CLOSURE_SIGMA6) for i, j in ((35, 1), (20, 3), (30, 12), (9, 27))]
    good = A.closure_mahalanobis(closures)
    assert (good["status"] == 0).all()
    # an unknown pose and from == to: their own status and zeros, the others unaffected
    mixed = closures[:2] + [(0, 99, 0, 1, closures[0][4], cc.CLOSURE_SIGMA6), (0, 7, 0, 7, closures[0][4], cc.CLOSURE_SIGMA6),
                            (1, 0, 0, 1, closures[0][4], cc.CLOSURE_SIGMA6)] + closures[2:]
    out = A.closure_mahalanobis(mixed)
    assert out["status"].tolist() == [0, 0, MISSING, INVALID, MISSING, 0, 0]
    for k in (2, 3, 4):
        assert out["d2"][k] == 0 and not out["C"][k].any() and not out["r"][k].any()
    keep = [0, 1, 5, 6]
    for f in ("d2", "C", "r"):
        assert np.array_equal(out[f][keep], good[f]), f
    pc, st = A.get_pose_pair_covariances([(0, 1, 0, 2), (0, 1, 0, 99), (0, 4, 0, 4), (0, 2, 0, 1)])
    assert st.tolist() == [0, MISSING, INVALID, 0] and not pc[1].any() and not pc[2].any() and pc[0].any()
    # the empty list, and the refusals of the arguments on a live graph
    assert len(A.closure_mahalanobis([])["d2"]) == 0 and A.get_pose_pair_covariances([])[0].shape == (0, 12, 12)
    _raises("SLIDE_ERR_INVALID", A.closure_mahalanobis, [(0, 30, 0, 2, I7, [0.1, 0.1, 0.0, 0.1, 0.1, 0.1])])
    _raises("SLIDE_ERR_INVALID", A.closure_mahalanobis, [(0, 30, 0, 2, [0.0] * 7, cc.CLOSURE_SIGMA6)])
    _raises("SLIDE_ERR_INVALID", A.closure_mahalanobis, [(0, 30, 13, 2, I7, cc.CLOSURE_SIGMA6)])
    _raises("SLIDE_ERR_INVALID", A.closure_mahalanobis, [(0, 30, 0, 2, [np.nan, 0, 0, 0, 0, 0, 1], cc.CLOSURE_SIGMA6)])
    _raises("SLIDE_ERR_INVALID", A.get_pose_pair_covariances, [(0, 1, -1, 2)])
    # nothing moved: marginals and poses equal bit for bit those of a graph never queried, before and after the next solve
    for p in (0, 17, 35):
        assert np.array_equal(A.get_pose_covariance(0, p)[1], B.get_pose_covariance(0, p)[1])
    assert np.array_equal(A.get_pose_covariances(0, range(36)), B.get_pose_covariances(0, range(36)))
    for p in range(36):
        assert np.array_equal(A.get_pose12(0, p)[1], B.get_pose12(0, p)[1]), p
    # a following select_closures, and add_loop_closure + solve, behave as on the graph never queried
    sa, sb = A.select_closures(closures), B.select_closures(closures)
    assert sa["keep"].tolist() == sb["keep"].tolist() and np.array_equal(sa["score"], sb["score"])
    for g in (A, B):
        c0 = closures[0]
        g.add_loop_closure(c0[4], c0[1], c0[0], c0[3], c0[2])
    # a factor added and merged, not yet solved: whole-call refusal, nothing written
    A.tile_profile()
    _raises("SLIDE_ERR_INVALID", A.closure_mahalanobis, closures)
    _raises("SLIDE_ERR_INVALID", A.get_pose_pair_covariances, [(0, 1, 0, 2)])
    for g in (A, B):
        assert g.gauss_newton(1) == 0
    for p in range(36):
        assert np.array_equal(A.get_pose12(0, p)[1], B.get_pose12(0, p)[1]), p
    assert np.array_equal(A.get_pose_covariances(0, [7])[0], B.get_pose_covariances(0, [7])[0])
    assert np.array_equal(A.closure_mahalanobis(closures[1:])["d2"], B.closure_mahalanobis(closures[1:])["d2"])
    A.chi2()
    _raises("SLIDE_ERR_INVALID", A.closure_mahalanobis, closures)                # chi2() retires the factor it reads
    B.set_ghosts([0], [0])                                                      # a shard of a distributed solve
    _raises("SLIDE_ERR_INVALID", B.closure_mahalanobis, closures)
    _raises("SLIDE_ERR_INVALID", B.get_pose_pair_covariances, [(0, 1, 0, 2)])


def test_gate_with_select_closures(gpu):
    """One list through both calls on noisy40 (expmap chart, as the selection's graph test): eight true closures, one isolated false
    one, three false ones that agree with each other.  The generator has asserted on the CPU what d2_ref and the restatement of the
    consistency score say; on the device the gate's verdicts match d2_ref's.  Documented, not asserted as policy: what selection
    alone keeps, and what gate followed by selection leaves."""
    c = gc.case("noisy40", 1)
    G, _ = gc.device_graph(gpu, "noisy40", 1)
    closures, kinds, _ = gc.aliased_list(c, dev_pose12(G))
    _, _, _, d2_ref = gc.ref_gate(c, closures, dev_pose12(G))
    out = G.closure_mahalanobis(closures)
    assert (out["status"] == 0).all()
    passed = out["d2"] < gc.GATE2
    assert (passed == (d2_ref < gc.GATE2)).all() and (passed == (kinds == 0)).all(), (out["d2"], d2_ref, kinds)
    sel = G.select_closures(closures)
    assert (sel["status"] == 0).all()
    gated = [closures[k] for k in np.nonzero(passed)[0]]
    sel2 = G.select_closures(gated, params=gpu.closure_params(min_set=2))
    left = np.nonzero(passed)[0][sel2["keep"]]
    alone = G.select_closures([closures[k] for k in np.nonzero(kinds != 0)[0]], params=gpu.closure_params(min_set=2))
    print(f"[gate+select] kinds {kinds.tolist()} (0 true, 1 isolated false, 2 aliased false)\n"
          f"  gate d2 {np.round(out['d2'], 2).tolist()}\n  selection alone keeps {np.nonzero(sel['keep'])[0].tolist()}; of the four false "
          f"closures alone it keeps {alone['keep'].tolist()} (the aliased ones form a clique of their own)\n"
          f"  gate, then selection (min_set 2) leaves {left.tolist()}: {'exactly' if set(left) == set(np.nonzero(kinds == 0)[0]) else 'a subset of'} the true ones")
    assert set(left.tolist()) <= set(np.nonzero(kinds == 0)[0].tolist())
