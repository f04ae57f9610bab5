"""The duplicate-landmark queries on the device (slide_graph_landmark_pair_mahalanobis / _get_landmark_pair_covariances: route 0 on the
selected inverse, cov_kernels.hip's k_lm_pair_direct / k_lm_pair_cov; route 1 through the forward substitution, obs_gate_kernels.hip's
k_lm_pair_fill; slide_pairs_within / slide_graph_landmark_pairs_within: pairs_kernels.hip) against the dense reference of
tests/landmark_pair_cases.py: Sigma the dense inverse of the full unreduced H, d from the landmarks read back with get_landmark.

Tolerances.  d2: tol x cond(C_ref), floor 1e-12 (observation_gate_cases.gate_bound), relative to d2_ref; C and r entry-wise by the same
figure against the largest entry of C_ref, as test_gpu_observation_gate.check_gate.  Covariance blocks: the Jacobi-scaled bound of
test_gpu_marginals.check_marginals (|got - ref| scaled by diag(H)^1/2, relative to the largest scaled entry of inv(H), at most tol).
The independence checks are bit for bit.

A sweep of route 1 holds SLIDE_INFO_GAIN_SWEEP_COLS / D = 128 point pairs or 54 cylinder pairs (384 columns); the independence test
runs one more than that, and the 43 / 19 pairs (one more than 128 / 3, 128 / 7) its specification names."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gn_graphs as gg
import landmark_pair_cases as lp
import observation_gate_cases as og
from test_gpu_marginals import _raises

pytestmark = pytest.mark.gpu

MISSING, INVALID = 1, -1
HERE = os.path.dirname(os.path.abspath(__file__))
_GRAPHS = {}


def device(gpu, name, chart):
    """One solved device graph per (name, chart) for the whole module: the queries only read it."""
    if (name, chart) not in _GRAPHS:
        _GRAPHS[name, chart] = lp.device_graph(gpu, name, chart)
    return _GRAPHS[name, chart]


def check_pairs(c, kind, pairs, out, vals, tag):
    rs, Cs, d2 = lp.ref_pairs(c, kind, pairs, vals)
    D = lp.DIM[kind]
    assert (out["status"] == 0).all(), out["status"]
    worst = 0.0
    for k, (a, b) in enumerate(pairs):
        assert out["dof"][k] == D
        bound = og.gate_bound(c, Cs[k])
        top = float(np.abs(Cs[k]).max())
        e_d = abs(out["d2"][k] - d2[k]) / d2[k]
        e_C = float(np.abs(out["C"][k][:D, :D] - Cs[k]).max() / top)
        e_r = float(np.abs(out["r"][k][:D] - rs[k]).max() / top)
        print(f"[lm-pairs] {tag} {kind} {a} / {b} route {out['route'][k]}: d2 {out['d2'][k]:.6g} ref {d2[k]:.6g} err {e_d:.2e}, C {e_C:.2e}, "
              f"r {e_r:.2e} (bound {bound:.2e})")
        assert max(e_d, e_C, e_r) <= bound, (k, e_d, e_C, e_r, bound)
        assert not out["C"][k][D:].any() and not out["C"][k][:, D:].any() and not out["r"][k][D:].any()
        worst = max(worst, max(e_d, e_C, e_r) / bound)
    assert np.array_equal(out["C"], np.transpose(out["C"], (0, 2, 1)))      # symmetric bit for bit
    return d2, worst


@pytest.mark.parametrize("chart", [0, 1])
def test_pairs_vs_reference_decisions_and_routes(gpu, chart):
    """Every dup40 pair of both classes against the reference at the values read back; the decision at the 0.99 quantile equals the
    planted flag; both routes occur and the revisit pair, whose observers lie 35 poses apart, takes the substitution."""
    c = lp.case("dup40", chart)
    G, _ = device(gpu, "dup40", chart)
    prof = G.tile_profile()
    print(f"[lm-pairs] chart {chart}: tile profile {list(prof)}")
    vals = og.device_values(G)
    routes = {}
    for kind in ("point", "cylinder"):
        pairs, flags, _, _ = lp.planted(c, kind, vals)
        out = G.landmark_pair_mahalanobis(lp.CLS[kind], pairs, lp.SIGMA[kind])
        d2, worst = check_pairs(c, kind, pairs, out, vals, f"chart {chart}")
        assert np.array_equal(out["d2"] <= og.QUANTILE[lp.DIM[kind]], flags)
        assert np.array_equal(out["d2"] <= gpu.chi2_quantile(0.99, lp.DIM[kind]), flags)
        routes[kind] = out["route"]
        print(f"[lm-pairs] chart {chart} {kind}: largest error / bound {worst:.3e}; routes {np.bincount(out['route'], minlength=2)}")
        if kind == "point":
            k = int(np.flatnonzero((pairs == np.array(lp.REVISIT, np.uint64)).all(axis=1))[0])
            assert out["route"][k] == 1 and flags[k]
    assert set(routes["point"].tolist()) == {0, 1}
    assert (routes["cylinder"] == 0).all()          # (re-initialised within three poses: inside the band)


@pytest.mark.parametrize("chart", [0, 1])
def test_routes_agree(gpu, chart, tmp_path):
    """Every pair again in a fresh child process under SLIDE_LM_PAIR_SUBSTITUTE=1: all of them take route 1 there, and each agrees with
    the reference — and so with route 0 here — within the same bound; so do the joint marginals of the two routes."""
    c = lp.case("dup40", chart)
    G, _ = device(gpu, "dup40", chart)
    vals = og.device_values(G)
    path = str(tmp_path / "forced.npz")
    env = dict(os.environ, SLIDE_LM_PAIR_SUBSTITUTE="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "landmark_pair_child.py"), str(chart), path], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    F = np.load(path)
    scale = np.abs(c.Sig * np.outer(c.w, c.w)).max()
    n0 = 0
    for kind in ("point", "cylinder"):
        pairs, _, _, _ = lp.planted(c, kind, vals)
        D = lp.DIM[kind]
        here = G.landmark_pair_mahalanobis(lp.CLS[kind], pairs, lp.SIGMA[kind])
        lm = np.array([np.concatenate([vals.lm(kind, int(a)), vals.lm(kind, int(b))]) for a, b in pairs])
        assert np.array_equal(lm, F[f"{kind}_lm"])                      # the child stands where this process stands
        forced = {f: F[f"{kind}_{f}"] for f in ("d2", "C", "r", "route", "status")}
        forced["dof"] = np.full(len(pairs), D)
        assert (forced["route"] == 1).all()
        check_pairs(c, kind, pairs, forced, vals, f"chart {chart} forced")
        _, Cs, d2 = lp.ref_pairs(c, kind, pairs, vals)
        cov_here, st, route = G.get_landmark_pair_covariances(lp.CLS[kind], pairs)
        assert (st == 0).all() and np.array_equal(route, here["route"]) and (F[f"{kind}_cov_route"] == 1).all()
        for k, (a, b) in enumerate(pairs):
            if here["route"][k] != 0:
                continue
            n0 += 1
            bound = og.gate_bound(c, Cs[k])
            assert abs(here["d2"][k] - forced["d2"][k]) / d2[k] <= bound
            assert np.abs(here["C"][k] - forced["C"][k]).max() / np.abs(Cs[k]).max() <= bound
            sel = np.concatenate([lp.cols(c, kind, int(a)), lp.cols(c, kind, int(b))])
            ws = np.outer(c.w[sel], c.w[sel])
            assert np.abs((cov_here[k] - F[f"{kind}_cov"][k]) * ws).max() / scale <= c.tol
    assert n0 >= 30


def check_covs(c, G, kind, pairs, tag):
    """The joint marginals against the dense blocks (Jacobi-scaled); the diagonal blocks against get_landmark_covariances."""
    cls, D = lp.CLS[kind], lp.DIM[kind]
    cov, st, route = G.get_landmark_pair_covariances(cls, pairs)
    assert cov.shape == (len(pairs), 2 * D, 2 * D) and (st == 0).all()
    scale = np.abs(c.Sig * np.outer(c.w, c.w)).max()
    worst = 0.0
    for k, (a, b) in enumerate(pairs):
        sel = np.concatenate([lp.cols(c, kind, int(a)), lp.cols(c, kind, int(b))])
        ws = np.outer(c.w[sel], c.w[sel])
        worst = max(worst, float(np.abs((cov[k] - c.Sig[np.ix_(sel, sel)]) * ws).max() / scale))
        single = G.get_landmark_covariances(cls, [int(a), int(b)])
        assert np.abs((cov[k][:D, :D] - single[0]) * ws[:D, :D]).max() / scale <= c.tol
        assert np.abs((cov[k][D:, D:] - single[1]) * ws[D:, D:]).max() / scale <= c.tol
        assert np.abs((cov[k][:D, D:] - cov[k][D:, :D].T) * ws[:D, D:]).max() / scale <= c.tol
    print(f"[lm-pairs] {tag} {kind}: joint marginals, largest scaled error {worst:.3e} (tol {c.tol:.3e}), routes {np.bincount(route, minlength=2)}")
    assert worst <= c.tol, (worst, c.tol)
    return cov, route


@pytest.mark.parametrize("chart", [0, 1])
def test_pair_covariances_dup40(gpu, chart):
    """dup40's pairs of both classes, both routes: against the dense blocks; Sig_d rebuilt from the four blocks reproduces the C of
    the test within the gate's bound."""
    c = lp.case("dup40", chart)
    G, _ = device(gpu, "dup40", chart)
    vals = og.device_values(G)
    for kind in ("point", "cylinder"):
        pairs, _, _, _ = lp.planted(c, kind, vals)
        D, sg = lp.DIM[kind], lp.SIGMA[kind]
        cov, route = check_covs(c, G, kind, pairs, f"dup40 chart {chart}")
        out = G.landmark_pair_mahalanobis(lp.CLS[kind], pairs, sg)
        assert np.array_equal(route, out["route"])
        _, Cs, _ = lp.ref_pairs(c, kind, pairs, vals)
        for k in range(len(pairs)):
            Sd = cov[k][:D, :D] + cov[k][D:, D:] - cov[k][:D, D:] - cov[k][D:, :D]
            Cm = np.eye(D) + Sd / np.outer(sg, sg)
            assert np.abs(Cm - out["C"][k][:D, :D]).max() / np.abs(Cs[k]).max() <= og.gate_bound(c, Cs[k])


def test_pair_covariances_with_cubes(gpu):
    """planted40 (a point, and a cylinder or a cube, every third pose, four observers each): pairs of every class, near and across
    the profile.  lc_cube holds ONE cube and one point, so all it can name is a landmark paired with itself: its own status."""
    c = og.case("planted40", 0)
    G, _ = device(gpu, "planted40", 0)
    seen = set()
    for kind, pairs in (("cube", [(3, 9), (9, 15), (3, 39), (27, 33)]), ("cylinder", [(0, 6), (6, 36), (12, 18)]),
                        ("point", [(0, 3), (3, 36), (21, 24), (24, 21)])):
        _, route = check_covs(c, G, kind, np.array(pairs, np.uint64), "planted40")
        seen |= set(route.tolist())
    assert seen == {0, 1}
    _raises("SLIDE_ERR_INVALID", G.landmark_pair_mahalanobis, lp.CLS["cube"], [(3, 9)], np.full(3, 0.05))      # cubes: covariances only
    L, _ = device(gpu, "lc_cube", 0)
    cov, st, _ = L.get_landmark_pair_covariances(lp.CLS["cube"], [(0, 0)])
    assert st.tolist() == [INVALID] and not cov.any()


def _same(x, y, i, j, what):
    for f in ("d2", "C", "r", "route", "status"):
        assert np.array_equal(x[f][i], y[f][j]), (what, f)


@pytest.mark.parametrize("kind,counts", [("point", (43, 129)), ("cylinder", (19, 55))])
def test_a_pair_does_not_depend_on_the_list(gpu, kind, counts):
    """Bit for bit: each pair of a list one longer than a sweep equals the call that gives it alone, in a permuted list and in a list
    mixing the routes — with the host's own route choice and with every pair forced down route 1, where the list spans two sweeps.
    (b, a) gives (a, b)'s d2 within the bound and its r negated."""
    c = lp.case("dup40", 1)
    G, _ = device(gpu, "dup40", 1)
    vals = og.device_values(G)
    cls, sg = lp.CLS[kind], lp.SIGMA[kind]
    base, _, _, _ = lp.planted(c, kind, vals)
    far = np.array([(0, 130), (6, 130), (100, 230)], np.uint64)       # observers 30 poses apart: the substitution
    uniq = np.concatenate([base, far])
    for forced in (False, True):
        if forced:
            os.environ["SLIDE_LM_PAIR_SUBSTITUTE"] = "1"              # the library's test aid: read at every call
        try:
            alone = [G.landmark_pair_mahalanobis(cls, uniq[k:k + 1], sg) for k in range(len(uniq))]
            routes = np.array([a["route"][0] for a in alone])
            assert (routes == 1).all() if forced else set(routes.tolist()) == {0, 1}
            assert all(a["status"][0] == 0 for a in alone)
            for n in counts:
                pick = np.arange(n) % len(uniq)
                whole = G.landmark_pair_mahalanobis(cls, uniq[pick], sg)
                perm = np.random.default_rng(n).permutation(n)
                shuffled = G.landmark_pair_mahalanobis(cls, uniq[pick[perm]], sg)
                for i in range(n):
                    _same(whole, alone[pick[i]], i, 0, (kind, forced, n, i, "alone"))
                    _same(shuffled, whole, i, perm[i], (kind, forced, n, i, "permuted"))
        finally:
            os.environ.pop("SLIDE_LM_PAIR_SUBSTITUTE", None)
    fwd = G.landmark_pair_mahalanobis(cls, base, sg)
    bwd = G.landmark_pair_mahalanobis(cls, base[:, ::-1], sg)
    _, Cs, d2 = lp.ref_pairs(c, kind, base, vals)
    assert np.array_equal(bwd["r"], -fwd["r"]) and np.array_equal(bwd["route"], fwd["route"])
    for k in range(len(base)):
        assert abs(bwd["d2"][k] - fwd["d2"][k]) / d2[k] <= og.gate_bound(c, Cs[k])


def test_status_words_and_state_refusals(gpu):
    """An unknown key, a landmark without a factor and a == b, each next to served neighbours; the whole-call refusals before the
    first solve, after chi2 and after an add."""
    G, _ = lp.device_graph(gpu, "dup40", 0, solve=False)
    G.add_point_landmark(999, [1.0, 2.0, 3.0])                          # never observed
    sg = lp.SIGMA["point"]
    some = [(0, 100), (3, 103)]
    _raises("SLIDE_ERR_INVALID", G.landmark_pair_mahalanobis, 2, some, sg)               # before the first solve
    _raises("SLIDE_ERR_INVALID", G.get_landmark_pair_covariances, 2, some)
    assert G.gauss_newton(1) == 0
    good = G.landmark_pair_mahalanobis(2, some, sg)
    assert (good["status"] == 0).all() and (good["d2"] > 0).all()
    mixed = [some[0], (0, 777), (999, 0), (0, 999), (3, 3), some[1]]
    out = G.landmark_pair_mahalanobis(2, mixed, sg)
    assert out["status"].tolist() == [0, MISSING, MISSING, MISSING, INVALID, 0]
    assert out["dof"].tolist() == [3] * 6
    for k in (1, 2, 3, 4):
        assert out["d2"][k] == 0 and not out["C"][k].any() and not out["r"][k].any() and out["route"][k] == 0
    for f in ("d2", "C", "r", "route"):
        assert np.array_equal(out[f][[0, 5]], good[f]), f
    cov, st, _ = G.get_landmark_pair_covariances(2, mixed)
    assert st.tolist() == [0, MISSING, MISSING, MISSING, INVALID, 0] and not cov[1:5].any() and cov[0].any() and cov[5].any()
    empty = G.landmark_pair_mahalanobis(2, np.zeros((0, 2)), sg)
    assert len(empty["d2"]) == 0 and empty["C"].shape == (0, 9, 9)
    assert G.get_landmark_pair_covariances(1, np.zeros((0, 2)))[0].shape == (0, 18, 18)
    _raises("SLIDE_ERR_INVALID", G.landmark_pair_mahalanobis, 2, some, [0.05, 0.0, 0.05])       # an argument refusal on a live graph
    _raises("SLIDE_ERR_INVALID", G.landmark_pair_mahalanobis, 1, some, np.full(3, 0.05))
    again = G.landmark_pair_mahalanobis(2, some, sg)                    # the graph is only read
    for f in ("d2", "C", "r"):
        assert np.array_equal(again[f], good[f])
    G.chi2()
    _raises("SLIDE_ERR_INVALID", G.landmark_pair_mahalanobis, 2, some, sg)               # chi2() clears the factorisation
    _raises("SLIDE_ERR_INVALID", G.get_landmark_pair_covariances, 2, some)
    assert G.gauss_newton(1) == 0
    assert (G.landmark_pair_mahalanobis(2, some, sg)["status"] == 0).all()
    G.add_range_bearing(0, 5, 999, [1.0, 0.0, 0.0], 4.0)
    G.tile_profile()                                                    # (merges and uploads what is pending)
    _raises("SLIDE_ERR_INVALID", G.landmark_pair_mahalanobis, 2, some, sg)               # the graph changed since the last solve
    _raises("SLIDE_ERR_INVALID", G.get_landmark_pair_covariances, 2, some)
    assert G.gauss_newton(1) == 0
    assert (G.landmark_pair_mahalanobis(2, some, sg)["status"] == 0).all()
    batch = gpu.CholBatch(1)                                            # a graph joined to a CholBatch
    G.join_chol_batch(batch, 0)
    _raises("SLIDE_ERR_INVALID", G.landmark_pair_mahalanobis, 2, some, sg)
    _raises("SLIDE_ERR_INVALID", G.get_landmark_pair_covariances, 2, some)
    G.join_chol_batch(None)


# ---- the search -------------------------------------------------------------------------------------------------------------------
def _check_search(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])          # the set AND the order
    assert got[2].shape == want[2].shape
    assert (np.abs(got[2] - want[2]) <= 1e-12 * want[2]).all()


@pytest.mark.parametrize("n", lp.SEARCH_SIZES)
def test_pairs_within_vs_brute_force(gpu, n):
    xyz, labels = lp.search_points(n)
    r = lp.clear_radius(xyz, 1.0)
    want = lp.brute_pairs(xyz, r)
    _check_search(gpu.pairs_within(xyz, r), want)
    _check_search(gpu.pairs_within(xyz, r, labels), lp.brute_pairs(xyz, r, labels))
    if n >= 2:
        k = int(np.flatnonzero((want[0] == 0) & (want[1] == n - 1))[0])                 # the two coincident points
        assert want[2][k] == 0.0 and gpu.pairs_within(xyz, r)[2][k] == 0.0
    # an all-inside cluster: the dense output, n (n - 1) / 2 pairs
    big = lp.clear_radius(xyz, 7.5)
    every = gpu.pairs_within(xyz, big)
    assert len(every[0]) == n * (n - 1) // 2
    _check_search(every, lp.brute_pairs(xyz, big))


def test_pairs_within_capacity(gpu):
    import ctypes as C
    xyz, _ = lp.search_points(65)
    want = lp.brute_pairs(xyz, 1.0)
    total = len(want[0])
    assert total > 2
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    for cap, rc_want in ((total - 1, -3), (total, 0)):                                     # SLIDE_ERR_CAPACITY one short
        oi, oj, dist, tot = np.full(total, 77, np.int32), np.full(total, 77, np.int32), np.full(total, 77.0), np.zeros(1, np.int64)
        rc = gpu.lib().slide_pairs_within(P(xyz), None, C.c_int(65), C.c_double(1.0), C.c_int64(cap), P(oi), P(oj), P(dist), P(tot))
        assert rc == rc_want and tot[0] == total
        if rc:
            assert (oi == 77).all() and (oj == 77).all() and (dist == 77).all()            # nothing but n_pairs is written
        else:
            _check_search((oi, oj, dist), want)


def test_graph_search_equals_the_standalone_call(gpu):
    """pose_list_graph(G, 65): 65 points around one pose.  The graph form equals slide_pairs_within on the values read back — every
    landmark of the class, a selection in an order of its own, and with labels — and returns landmark keys."""
    G = gpu.SlideGraph(gpu.default_params())
    gg.pose_list_graph(G, 65)
    assert G.gauss_newton(1) == 0
    xyz = np.array([G.get_landmark(2, l)[1] for l in range(65)])
    r = lp.clear_radius(xyz, 1.2)
    want = gpu.pairs_within(xyz, r)
    assert len(want[0]) > 20
    _check_search(lp.brute_pairs(xyz, r), want)
    ia, ib, dist = G.landmark_pairs_within(2, r)
    assert np.array_equal(ia, want[0].astype(np.uint64)) and np.array_equal(ib, want[1].astype(np.uint64)) and np.array_equal(dist, want[2])
    sel = np.random.default_rng(5).permutation(65)[:40].astype(np.uint64)
    labels = (np.arange(40) % 3).astype(np.int32)
    for lab in (None, labels):
        w = gpu.pairs_within(xyz[sel.astype(int)], r, lab)
        ia, ib, dist = G.landmark_pairs_within(2, r, sel, lab)
        assert np.array_equal(ia, sel[w[0]]) and np.array_equal(ib, sel[w[1]]) and np.array_equal(dist, w[2])
    with pytest.raises(KeyError):
        G.landmark_pairs_within(2, r, [0, 1, 700])
    assert len(G.landmark_pairs_within(0, r)[0]) == 0                                      # no cylinder in this graph
    _raises("SLIDE_ERR_INVALID", G.landmark_pairs_within, 2, 0.0)


@pytest.mark.parametrize("chart", [0, 1])
def test_duplicate_landmarks_finds_exactly_the_planted_ones(gpu, chart):
    """The search at 0.75 m proposes the duplicates AND the distinct neighbours 0.6 m away; the test keeps exactly the planted
    duplicates, the revisit 900 / 901 (half a metre apart after 35 poses of drift) among them."""
    c = lp.case("dup40", chart)
    G, W = device(gpu, "dup40", chart)
    for kind in ("point", "cylinder"):
        planted = sorted((a, b) for a, b, f in W.pairs[kind] if f)
        near = G.landmark_pairs_within(lp.CLS[kind], 0.75)
        assert len(near[0]) >= len(W.pairs[kind])                                          # the distinct neighbours are proposed too
        ia, ib, d2, dist = G.duplicate_landmarks(lp.CLS[kind], 0.75, lp.SIGMA[kind])
        assert sorted(zip(ia.tolist(), ib.tolist())) == planted, (kind, ia, ib)
        assert (d2 <= og.QUANTILE[lp.DIM[kind]]).all() and (dist <= 0.75).all()
    ia, ib, _, dist = G.duplicate_landmarks(2, 0.75, lp.SIGMA["point"])
    k = list(zip(ia.tolist(), ib.tolist())).index(lp.REVISIT)
    assert dist[k] > 0.4
