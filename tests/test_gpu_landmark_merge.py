"""Landmark fusion on the device (slide_graph_merge_landmarks, lm_merge_kernels.hip's k_lm_merge_fuse) against a reference that holds
no merge code: the graph built through landmark_merge_cases.Rekey, keys mapped drop -> keep, solved by gn_reference's QR.

Tolerances.  Every Gauss-Newton step: gn_reference.tolerance, computed from the case, as test_gpu_gn_step.check_steps does.  The
streaming updates after a merge: the same bound at the tracked linearisation points (stream_graphs.check_step's, what
test_gpu_stream_step's toggle case holds every update to); the incremental and the non-incremental twin each meet it against the one
reference, so they agree within the sum of their two bounds.  The fused estimate: 32 D eps (sum of kappa(H_i) + kappa(sum H_i))
max(1, |x_ref|_inf) per cluster.  chi2: r.r of the rekeyed reference at the device's values; a residual is a difference of values of
size M divided by a sigma, so each carries an error of at most d = 64 eps M / min sigma, and r.r one of 2 |r|_1 d + m d^2.  Bits where
the text says bits."""
import numpy as np
import pytest

import landmark_merge_cases as lm
import landmark_pair_cases as lp
import stream_graphs as sg
from gn_reference import EPS, Reference, scaled_error, tolerance
from test_gn_reference import numdiff_floor
from test_gpu_gn_step import check_steps, gpu_values
from test_gpu_marginals import _raises

pytestmark = pytest.mark.gpu

KINDS = ("point", "cylinder")
CLS = lm.CLS


def merged_dup40(gpu, chart, solve_first=3, fuse=False):
    """dup40 on the device with every true pair of both classes merged -> (G, W, rows, the rekeyed reference, the merges' dicts)."""
    G, W = lm.device_graph(gpu, "dup40", chart)
    rows = {kind: lm.true_pairs(W, kind) for kind in KINDS}
    if solve_first:
        assert G.gauss_newton(solve_first) == 0
    res = {}
    for n, kind in enumerate(KINDS):
        if fuse and n:
            assert G.gauss_newton(1) == 0          # (fusion reads the resident linearisation: the first merge retired it)
        res[kind] = G.merge_landmarks(CLS[kind], rows[kind], fuse)
    ref, _ = lm.reference("dup40", chart, lm.drop_map(rows))
    return G, W, rows, ref, res


def check_merge_words(rows, res, moved=2):
    for kind in KINDS:
        assert res[kind]["status"].tolist() == [0] * len(rows[kind])
        assert res[kind]["moved"].tolist() == [moved] * len(rows[kind])
        assert np.array_equal(res[kind]["into"], rows[kind][:, 0])


# ---- 1. one step against the rekeyed graph ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("mode", ["after_solve", "before_solve", "fused"])
def test_step_after_merge_vs_rekeyed_reference(gpu, chart, mode):
    """Each Gauss-Newton step of the merged device graph against the QR step of the rekeyed factor list: merged after three steps,
    merged before any solve (pending entries merged first, the tombstones' factor-less H_ll^-1 path from the first pass on), and
    merged with fusion."""
    G, _, rows, ref, res = merged_dup40(gpu, chart, solve_first=0 if mode == "before_solve" else 3, fuse=mode == "fused")
    check_merge_words(rows, res)
    check_steps(ref, G, steps=2, values=None if mode == "before_solve" else gpu_values(G, ref))


# ---- 2. solve() after a merge is the full step; later updates are incremental again ---------------------------------------------------
def _step_check(ref, G, vals, call):
    dx, H = ref.step(vals)
    assert call() == 0
    new = gpu_values(G, ref)
    tol, kappa = tolerance(H, dx, ref.magnitude(vals), numdiff_floor(ref, dx, H, vals))
    err = scaled_error(ref.tangent(vals, new), dx, H)
    return new, err, tol, dx, H


@pytest.mark.parametrize("chart", [0, 1])
def test_solve_after_merge_is_full_then_incremental(gpu, chart):
    og, Wo = None, None
    twins = []
    for inc in (True, False):
        G, W = lm.device_graph(gpu, "dup40", chart)
        rows = {kind: lm.true_pairs(W, kind) for kind in KINDS}
        if og is None:
            og, Wo = lm.oracle_graph("dup40", chart, lm.drop_map(rows))
        assert G.gauss_newton(3) == 0
        for kind in KINDS:
            G.merge_landmarks(CLS[kind], rows[kind], False)
        ref = Reference(og, chart)
        before = G.incremental_stats()
        vals = gpu_values(G, ref)
        new, err, tol, _, _ = _step_check(ref, G, vals, G.solve)          # solve(), not gauss_newton(1)
        print(f"[lm-merge] chart {chart} solve() after the merge: scaled error {err:.3e} tolerance {tol:.3e}")
        assert err <= tol, (err, tol)
        after = G.incremental_stats()
        assert after["full"] == before["full"] + 1 and after["incremental"] == before["incremental"] and after["last_first_column"] == 0
        G.set_incremental(inc)
        tr = sg.Tracker(chart)
        for k, key in enumerate(ref.vkey):
            tr.theta[int(key)], tr.vtype[int(key)], tr.est[int(key)] = vals[k].copy(), int(ref.vtype[k]), new[k].copy()
        twins.append((G, W, tr, after))
    for k in (40, 41, 42):
        lm.extra_frame(Wo, k)                                              # (through Rekey: the dropped keys' observations on the survivors)
        ref = Reference(og, chart)
        got, tols, scale = [], [], None
        for G, W, tr, _ in twins:
            lm.extra_frame(W, k)                                           # (the device is handed the DROPPED keys: the alias serves them)
            moved, margin = tr.relinearise()
            assert margin > sg.MARGIN
            for q, key in enumerate(ref.vkey):
                if int(key) not in tr.theta:
                    tr.theta[int(key)], tr.vtype[int(key)] = ref.values[q].copy(), int(ref.vtype[q])
            vals = np.array([tr.theta[int(key)] for key in ref.vkey])
            new, err, tol, dx, H = _step_check(ref, G, vals, G.solve)
            print(f"[lm-merge] chart {chart} frame {k}: {len(moved)} relinearised, scaled error {err:.3e} tolerance {tol:.3e}, {G.incremental_stats()}")
            assert err <= tol, (k, err, tol)
            for q, key in enumerate(ref.vkey):
                tr.est[int(key)] = new[q].copy()
            got.append(new); tols.append(tol)
            scale = scale or (np.sqrt(np.diag(H)), dx)
        w, dx = scale
        apart = float(np.linalg.norm(w * ref.tangent(got[1], got[0])) / np.linalg.norm(w * dx))
        print(f"[lm-merge] chart {chart} frame {k}: twins apart {apart:.3e} (bound {tols[0] + tols[1]:.3e})")
        assert apart <= tols[0] + tols[1], (k, apart, tols)
    (A, _, _, a0), (B, _, _, b0) = twins
    assert A.incremental_stats()["incremental"] > a0["incremental"]       # incremental again
    assert B.incremental_stats()["incremental"] == b0["incremental"]
    for G in (A, B):                                                       # the observations handed to dropped keys sit on the survivors
        ow = G.observation_weights()
        pts = ow["lm_idx"][ow["cls"] == 2]
        assert (pts == 33).sum() == 4 + 3 and not (pts == 133).any()


# ---- 3. structure ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart", [0, 1])
def test_structure_after_merge(gpu, chart):
    G0, _ = lm.device_graph(gpu, "dup40", chart)
    prof_before = G0.tile_profile().copy()
    n_before = G0.stats()["n_lm"]
    G, W, rows, ref, res = merged_dup40(gpu, chart)
    check_merge_words(rows, res)
    drop = lm.drop_map(rows)
    S, _ = lm.device_graph(gpu, "dup40", chart, drop)                      # built rekeyed from scratch
    prof = G.tile_profile()
    assert np.array_equal(prof, S.tile_profile())
    assert prof[0] > prof_before[0] and (prof >= prof_before).all()        # the revisit pair grows the first column's reach
    assert n_before == 38 + 18 and G.stats()["n_lm"] == n_before - len(drop) == S.stats()["n_lm"]
    assert G.stats()["n_factors"] == G0.stats()["n_factors"] == S.stats()["n_factors"]
    for kind in KINDS:
        cls = CLS[kind]
        kept, dropped = set(rows[kind][:, 0].tolist()), set(rows[kind][:, 1].tolist())
        for keep, d in rows[kind].tolist():
            st_k, v_k = G.get_landmark(cls, keep)
            st_d, v_d = G.get_landmark(cls, d)
            assert st_k == 0 and st_d == 0 and np.array_equal(v_k, v_d)
            assert G.landmark_alias(cls, d) == keep and G.landmark_alias(cls, keep) == keep
        others = [200 + k for k in range(0, 34, 3) if kind == "point" or k % 6 == 0]
        for idx in others:
            assert G.landmark_alias(cls, idx) == idx
        with pytest.raises(KeyError):
            G.landmark_alias(cls, 777)
        ia, ib, _ = G.landmark_pairs_within(cls, 1.0e3)
        live = kept | set(others)
        assert set(ia.tolist()) | set(ib.tolist()) == live and len(ia) == len(live) * (len(live) - 1) // 2      # no tombstone, no alias
        ow = G.observation_weights()
        named = ow["lm_idx"][ow["cls"] == cls]
        assert set(named.tolist()) == live and all((named == k).sum() == 4 for k in kept)
    # chi2 at the device's values against r.r of the rekeyed reference
    total = G.chi2()["total"]
    vals = gpu_values(G, ref)
    _, _, _, r = ref.linearize(vals)
    want = float(r @ r)
    d = 64 * EPS * float(np.abs(vals).max()) / float(ref.fsig[ref.fsig > 0].min())
    bound = 2 * float(np.abs(r).sum()) * d + len(r) * d * d
    print(f"[lm-merge] chart {chart} chi2 {total:.12g} reference {want:.12g} apart {abs(total - want):.3e} (bound {bound:.3e})")
    assert abs(total - want) <= bound


# ---- 4. shared observers and list lengths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart", [0, 1])
def test_two_factors_from_one_pose(gpu, chart):
    """The distinct neighbours k / 200 + k share the observers k and k + 1: merged, those poses hold two factors on one landmark."""
    G, W = lm.device_graph(gpu, "dup40", chart)
    rows = {kind: np.array([(a, b) for a, b, f in W.pairs[kind] if not f and a < 100], np.uint64) for kind in KINDS}
    assert len(rows["point"]) == 12 and len(rows["cylinder"]) == 6
    assert G.gauss_newton(3) == 0
    res = {kind: G.merge_landmarks(CLS[kind], rows[kind], False) for kind in KINDS}
    check_merge_words(rows, res, moved=3)
    ref, _ = lm.reference("dup40", chart, lm.drop_map(rows))
    per_pose, per_lm = ref.list_lengths()
    assert per_lm[ref.lm_var(2, 0)] == 5 and per_pose[ref.pose_var(0, 0)] == 4      # pose 0: point 0 twice, cylinder 0 twice
    check_steps(ref, G, steps=2, values=gpu_values(G, ref))


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("na,nb", [(24, 1), (32, 32), (64, 1)])
def test_merged_list_lengths(gpu, chart, kind, na, nb):
    """The merged landmark's factor list at 25, 64 and 65 entries: one more than LM_RED_MAX, a full wave, a second factor on a lane.
    The graph is uploaded (tile_profile) but not solved when it is merged, so resident rows are re-pointed and the two steps checked
    are the large first ones.  (Measurements here are exact: merged after convergence the graph would stand at its optimum but for
    the centimetres between the two fits, a step of 1e-8 of the values in the Jacobi-scaled norm, where the residuals' own rounding
    - which gn_reference.tolerance does not model, its kappa term being relative to the step - is all that is left to compare.)"""
    name = ("count", CLS[kind], na, nb)
    G, _ = lm.device_graph(gpu, name, chart)
    G.tile_profile()
    assert G.stats()["n_lm"] == 3
    res = G.merge_landmarks(CLS[kind], [(0, 1)], False)
    assert res["moved"].tolist() == [nb] and res["status"].tolist() == [0] and G.stats()["n_lm"] == 2
    ref, _ = lm.reference(name, chart, {(CLS[kind], 1): 0})
    _, per_lm = ref.list_lengths()
    assert per_lm[ref.lm_var(CLS[kind], 0)] == na + nb
    check_steps(ref, G, steps=2)


# ---- 5. fusion -----------------------------------------------------------------------------------------------------------------------------
def _trip40(gpu, chart):
    """trip40 after gauss_newton(2) (values V read), gauss_newton(1): linearised at V, estimate read back -> (G, W, ref, V, estimates)."""
    G, W = lm.device_graph(gpu, "trip40", chart)
    ref, _ = lm.reference("trip40", chart)
    assert G.gauss_newton(2) == 0
    V = gpu_values(G, ref)
    assert G.gauss_newton(1) == 0
    return G, W, ref, V, gpu_values(G, ref)


def _cluster_rows(clusters):
    return np.array([(mem[0], m) for mem in clusters for m in mem[1:]], np.uint64).reshape(-1, 2)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_estimate(gpu, chart, kind):
    """x of every cluster of one class — pairs, triples (300 + k) and clusters with a factor-less member (400 + k) — against
    (sum H_i)^-1 sum H_i est_i in numpy, H_i from the reference's Jacobian at V, est_i the estimates read back before the merge."""
    G, W, ref, V, E = _trip40(gpu, chart)
    cls, clusters = CLS[kind], W.clusters[kind]
    est = {int(m): E[ref.lm_var(cls, m)] for mem in clusters for m in mem}
    want = [lm.fusion_reference(ref, V, kind, mem)(est) for mem in clusters]
    rows = _cluster_rows(clusters)
    res = G.merge_landmarks(cls, rows, True)
    assert res["status"].tolist() == [0] * len(rows), res["status"]
    sizes, factorless = set(), 0
    for mem, (x_ref, kap) in zip(clusters, want):
        st, v = G.get_landmark(cls, mem[0])
        assert st == 0
        x = lp.tangent(kind, v)
        bound = lm.fusion_bound(kind, kap, x_ref)
        err = float(np.abs(x - x_ref).max())
        sizes.add(len(mem))
        factorless += any(m >= 400 for m in mem)
        print(f"[lm-merge] chart {chart} {kind} cluster {mem}: |x - x_ref|_inf {err:.3e} bound {bound:.3e} (kappa sum {kap:.3e})")
        assert err <= bound, (kind, mem, err, bound)
        assert not np.array_equal(v, est[mem[0]])                          # (it moved: the survivor did not simply keep its estimate)
        for m in mem[1:]:
            assert np.array_equal(G.get_landmark(cls, m)[1], v)
    assert {2, 3} <= sizes and (factorless >= 2 or kind == "cylinder")
    assert G.gauss_newton(1) == 0 and np.isfinite(G.chi2()["total"])


@pytest.mark.parametrize("chart", [0, 1])
def test_cubes_keep_the_survivors_estimate(gpu, chart):
    G, W, _, _, _ = _trip40(gpu, chart)
    clusters = W.clusters["cube"]
    assert len(clusters) >= 2
    before = {mem[0]: G.get_landmark(1, mem[0])[1] for mem in clusters}
    res = G.merge_landmarks(1, _cluster_rows(clusters), True)
    assert res["status"].tolist() == [0] * len(clusters) and res["moved"].tolist() == [2] * len(clusters)
    for mem in clusters:
        assert np.array_equal(G.get_landmark(1, mem[0])[1], before[mem[0]]) and np.array_equal(G.get_landmark(1, mem[1])[1], before[mem[0]])
    ref, _ = lm.reference("trip40", chart, {(1, int(d)): int(k) for k, d in _cluster_rows(clusters)} | {(2, 400 + k): k for k in (0, 12, 24)})
    check_steps(ref, G, steps=1, values=gpu_values(G, ref))


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_bits_depend_on_the_cluster_alone(gpu, chart, kind):
    """Three identical graphs: the class's whole list in order; the list shuffled and reversed; one triple alone (no other cluster
    in the call), its pairs in the other order.  The triple's fused bits are the same in all three."""
    runs = [_trip40(gpu, chart) for _ in range(3)]
    for _, _, _, _, E in runs[1:]:
        assert np.array_equal(E, runs[0][4])                               # the premise: the three graphs stand at the same bits
    W = runs[0][1]
    cls, clusters = CLS[kind], W.clusters[kind]
    rows = _cluster_rows(clusters)
    triple = next(mem for mem in clusters if len(mem) == 3 and mem[2] < 400)
    lists = [rows, rows[np.random.default_rng(8).permutation(len(rows))][::-1], _cluster_rows([triple])[::-1]]
    out = []
    for (G, _, _, _, _), lst in zip(runs, lists):
        res = G.merge_landmarks(cls, lst, True)
        assert (res["status"] == 0).all()
        out.append(G.get_landmark(cls, triple[0])[1])
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2]), out


# ---- 6. chains, statuses, refusals ---------------------------------------------------------------------------------------------------------
def test_chains_and_status_words(gpu):
    G, _ = lm.device_graph(gpu, "dup40", 0)
    assert G.gauss_newton(1) == 0
    n0 = G.stats()["n_lm"]
    a, b, c, d = 3, 103, 203, 0
    res = G.merge_landmarks(2, [(a, b), (a, c), (b, c)], False)
    assert res["moved"].tolist() == [2, 3, 0] and res["status"].tolist() == [0, 0, 0] and res["into"].tolist() == [a, a, a]
    assert [G.landmark_alias(2, k) for k in (a, b, c)] == [a, a, a] and G.stats()["n_lm"] == n0 - 2
    res = G.merge_landmarks(2, [(d, a)], False)                            # a second call: b and c are carried along
    assert res["moved"].tolist() == [7] and res["into"].tolist() == [d]
    assert [G.landmark_alias(2, k) for k in (a, b, c, d)] == [d] * 4 and G.stats()["n_lm"] == n0 - 3
    res = G.merge_landmarks(2, [(6, 777), (777, 6), (6, 6), (6, 106), (b, c)], False)
    assert res["status"].tolist() == [lm.MISSING, lm.MISSING, lm.INVALID, 0, 0]
    assert res["moved"].tolist() == [0, 0, 0, 2, 0] and res["into"].tolist() == [0, 0, 6, 6, d]
    assert G.stats()["n_lm"] == n0 - 4
    with pytest.raises(KeyError):
        G.landmark_alias(2, 777)
    empty = G.merge_landmarks(2, np.zeros((0, 2)), False)
    assert len(empty["into"]) == 0
    # the dropped key: a new value on it is refused as inserted twice, an observation lands on the survivor
    G.add_point_landmark(b, [1.0, 2.0, 3.0])
    with pytest.raises(gpu.SlideError, match="inserted twice"):
        G.gauss_newton(1)
    assert G.gauss_newton(1) == 0
    ow = G.observation_weights()
    assert (ow["lm_idx"][ow["cls"] == 2] == d).sum() == 2 + 7 and not np.isin(ow["lm_idx"][ow["cls"] == 2], [a, b, c, 106]).any()
    ref, _ = lm.reference("dup40", 0, {(2, a): d, (2, b): d, (2, c): d, (2, 106): 6})
    check_steps(ref, G, steps=1, values=gpu_values(G, ref))


def test_state_refusals_and_queries_after_a_merge(gpu):
    G, W = lm.device_graph(gpu, "dup40", 0)
    pts, cyl = lm.true_pairs(W, "point"), lm.true_pairs(W, "cylinder")
    some = pts[:2]
    _raises("SLIDE_ERR_INVALID", G.merge_landmarks, 2, some, True)                          # fuse before any solve
    assert G.gauss_newton(1) == 0
    G.add_point_landmark(999, [1.0, 2.0, 3.0])
    G.add_range_bearing(0, 5, 999, [1.0, 0.0, 0.0], 4.0)
    _raises("SLIDE_ERR_INVALID", G.merge_landmarks, 2, some, True)                          # fuse with a pending landmark and factor
    assert G.gauss_newton(1) == 0
    G.chi2()
    _raises("SLIDE_ERR_INVALID", G.merge_landmarks, 2, some, True)                          # fuse after chi2()
    assert G.stats()["n_lm"] == 57 and G.landmark_alias(2, 100) == 100                         # nothing changed
    assert G.gauss_newton(1) == 0
    res = G.merge_landmarks(2, pts, True)
    assert (res["status"] == 0).all()
    sg3 = lp.SIGMA["point"]
    for call in ((G.get_pose_covariances, 0, [1]), (G.get_landmark_covariances, 2, [0]), (G.marginal_traces,),
                 (G.landmark_pair_mahalanobis, 2, [(0, 200)], sg3), (G.get_landmark_pair_covariances, 2, [(0, 200)]),
                 (G.observation_mahalanobis, [("point", 0, 5, 0, [1.0, 0.0, 0.0], 4.0)]), (G.merge_landmarks, 0, cyl, True)):
        _raises("SLIDE_ERR_INVALID", *call)                                                  # until the next solve
    assert G.gauss_newton(1) == 0
    G.get_pose_covariances(0, [1])
    assert G.get_landmark_covariances(2, [100]).shape == (1, 3, 3)
    assert G.marginal_traces()[3] == 39 - len(pts)                                          # the point landmarks: no tombstone counted
    assert (G.landmark_pair_mahalanobis(2, [(0, 200)], sg3)["status"] == 0).all()
    assert (G.observation_mahalanobis([("point", 0, 5, 100, [1.0, 0.0, 0.0], 4.0)])["status"] == 0).all()      # (through the alias)
    assert (G.landmark_pair_mahalanobis(2, [(0, 100)], sg3)["status"] == lm.INVALID).all()  # one landmark now
    assert (G.merge_landmarks(0, cyl, True)["status"] == 0).all()
    assert G.gauss_newton(1) == 0
    for kind in KINDS:                                                                       # merged, no pair is left to find
        assert len(G.duplicate_landmarks(CLS[kind], 0.75, lp.SIGMA[kind])[0]) == 0
    # graphs that are not served
    H, _ = lm.device_graph(gpu, "dup40", 0)
    assert H.gauss_newton(1) == 0
    batch = gpu.CholBatch(1)
    H.join_chol_batch(batch, 0)
    _raises("SLIDE_ERR_INVALID", H.merge_landmarks, 2, some, False)
    H.join_chol_batch(None)
    H.set_shared([2], [0], [0])
    _raises("SLIDE_ERR_INVALID", H.merge_landmarks, 2, some, False)
    _raises("SLIDE_ERR_INVALID", H.merge_landmarks, 2, some, True)
    assert H.stats()["n_lm"] == 56


# ---- 7. merge_duplicates end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chart", [0, 1])
def test_merge_duplicates_end_to_end(gpu, chart):
    G, W = lm.device_graph(gpu, "dup40", chart)
    rows = {}
    for kind in KINDS:
        assert G.gauss_newton(1) == 0
        ia, ib, d2, res = G.merge_duplicates(CLS[kind], 0.75, lp.SIGMA[kind], prob=0.99)
        rows[kind] = lm.true_pairs(W, kind)
        assert sorted(zip(ia.tolist(), ib.tolist())) == sorted(map(tuple, rows[kind].tolist())), (kind, ia, ib)
        assert np.array_equal(res["pairs"], rows[kind][np.lexsort((rows[kind][:, 1], rows[kind][:, 0]))])
        assert (res["status"] == 0).all() and (res["moved"] == 2).all() and (d2 <= gpu.chi2_quantile(0.99, lm.DIM[kind])).all()
    ref, _ = lm.reference("dup40", chart, lm.drop_map(rows))
    check_steps(ref, G, steps=2, values=gpu_values(G, ref))
    assert np.isfinite(G.chi2()["total"])
