"""The numpy reference of the observation loss (tests/observation_loss_cases.py) alone: the weight function at its kinks, that the
graphs of test_gpu_observation_loss.py are what their docstrings say, that every case keeps an inlier on every landmark, and the
planted scenario's figures.  No product code is involved."""
import numpy as np
import pytest

import observation_loss_cases as oc
import robust_cases as rc
from gn_reference import Reference
from oracle import pyoracle as po


def test_weights_at_the_kinks():
    k = rc.DEFAULT[rc.HUBER]
    assert list(rc.weight(rc.HUBER, 0.0, [0.0, k, np.nextafter(k, 2.0), 2 * k])) == [1.0, 1.0, k / np.nextafter(k, 2.0), 0.5]
    assert list(rc.weight(rc.DCS, 0.0, [0.0, 1.0])) == [1.0, 1.0] and rc.weight(rc.DCS, 0.0, np.sqrt(3.0)) == pytest.approx(0.25, rel=1e-15)
    assert rc.weight(rc.DCS, 9.0, 3.0) == 1.0 and rc.weight(rc.DCS, 9.0, 9.0) == pytest.approx((18.0 / 90.0) ** 2)
    assert rc.weight(rc.CAUCHY, 0.0, 0.1) == pytest.approx(0.5) and rc.weight(rc.GEMAN_MCCLURE, 3.0, 3.0) == pytest.approx(0.25)
    for kind in rc.KINDS.values():
        assert rc.weight(kind, 0.0, 1e30) == rc.W_MIN
    # the s2 comparison's atol of 1e-12 is a whitened norm of 1e-6: below every kink, and there no weight moves by more than 1e-10
    # (Cauchy at its default k = 0.1: 1e-12 / k^2, up to rounding), a tenth of the weights' rtol
    for kind in rc.KINDS.values():
        assert abs(rc.weight(kind, 0.0, 1e-6) - rc.weight(kind, 0.0, 0.0)) < 1.01e-10


def mixed(chart=0):
    og = po.OracleGraph(oc.params(chart)[0])
    _, planted = oc.mixed_graph(og, oc.mixed_cube_sigmas(chart))
    return Reference(og, chart), planted


@pytest.mark.parametrize("chart", [0, 1])
def test_mixed_graph_plants_what_it_says(chart):
    ref, planted = mixed(chart)
    lf = oc.lf_index(ref)
    assert [int(t) for t in ref.ftype[lf][:6]] == [po.F_BR, po.F_CUBE, po.F_CYL] * 2      # (interleaved)
    s = np.sqrt(rc.whitened_norms2(ref)[lf])
    q = sorted(planted)
    assert len(q) == 10 and {int(ref.ftype[lf[f]]) for f in q} == {po.F_BR, po.F_CUBE, po.F_CYL}
    assert np.allclose(s[q], [planted[f] for f in q], rtol=1e-6), (s[q], planted)
    sel = oc.selected(ref)
    for kind in rc.KINDS.values():
        w = np.ones(len(ref.ftype))
        w[sel] = rc.weight(kind, 0.0, np.sqrt(rc.whitened_norms2(ref)[sel]))
        assert oc.landmarks_keep_an_inlier(ref, w), kind
        wl = dict(zip(q, w[lf][q]))
        for f, t in planted.items():
            if kind == rc.HUBER:
                assert (wl[f] == 1.0) == (t < 1.345), (f, t)
            if kind == rc.DCS:
                assert (wl[f] == 1.0) == (t < 1.0), (f, t)
            if t == 60.0:
                assert wl[f] < 0.03
    dx, _, w, _, _ = oc.obs_step(ref, ref.values, rc.HUBER, 0.0, sel)
    assert np.linalg.norm(dx) > 1e-2 and (w[sel] < 1.0).sum() >= 5


@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_bearing_range_edges(N):
    og = po.OracleGraph(oc.params()[0])
    moved = oc.br_edge_graph(og, N)
    ref = Reference(og, 0)
    lf = oc.lf_index(ref)
    assert len(lf) == N and (ref.ftype[lf] == po.F_BR).all() and ref.n <= 300
    assert moved[0] == 0 and moved[-1] == N - 1 and all(q in moved for b in (256, 512) for q in (b - 1, b) if q < N)
    _, _, w, s2, _ = oc.obs_step(ref, ref.values, rc.CAUCHY, 0.0, oc.selected(ref))
    assert (w[lf] < 1.0).all() and (w[lf][moved] < 0.01).all()      # (Cauchy: every factor shows, the moved ones by far)
    assert oc.landmarks_keep_an_inlier(ref, w)                      # (N = 1: the one factor is moved and still keeps 1e-3 of H_ll)


@pytest.mark.parametrize("n_nbr", [1, 7, 8, 9, 17])
def test_cube_cylinder_edges(n_nbr):
    og = po.OracleGraph(oc.params()[0])
    moved = oc.nbr_edge_graph(og, n_nbr)
    ref = Reference(og, 0)
    lf = oc.lf_index(ref)
    t = ref.ftype[lf]
    assert len(lf) == 2 * n_nbr and (t[0::2] == po.F_BR).all() and np.isin(t[1::2], (po.F_CUBE, po.F_CYL)).all()
    assert (t != po.F_BR).sum() == n_nbr and all(t[f] != po.F_BR for f in moved)
    _, _, w, _, _ = oc.obs_step(ref, ref.values, rc.CAUCHY, 0.0, oc.selected(ref))
    assert oc.landmarks_keep_an_inlier(ref, w)
    first = [1, 3][:n_nbr] + [2 * q + 1 for q in (12, 13) if q < n_nbr]      # (the factors that create their landmark: no residual)
    later = np.setdiff1d(np.arange(len(lf)), first)
    assert (w[lf][first] == 1.0).all() and (w[lf][later] < 1.0).all()       # (Cauchy: every factor with a residual shows)


def test_both_graph():
    og = po.OracleGraph(oc.params()[0])
    fan = rc.Fan(og)
    gross = oc.both_graph(fan)
    ref = Reference(og, 0)
    assert ref.n <= 300 and -(-6 * 44 // 64) > 4
    s = np.sqrt(rc.whitened_norms2(ref))
    assert s[oc.lf_index(ref)[gross]] > 30 and s[rc.selected(ref, fan.origin)].max() > 1000
    _, _, w, _, _ = oc.obs_step(ref, ref.values, rc.HUBER, 0.0, oc.selected(ref), closure=(rc.HUBER, 0.0, rc.selected(ref, fan.origin)))
    assert oc.landmarks_keep_an_inlier(ref, w) and w[oc.lf_index(ref)[gross]] < 0.05


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("kind", sorted(rc.KINDS.values()))
def test_mixed_graph_steps_are_well_posed(kind, chart):
    """The three steps the GPU test compares: under a one-ulp change of the linearisation point the numpy step itself moves by less
    than a quarter of gn_reference.tolerance (the GPU linearises at a point that differs from its read-back by as much)."""
    from gn_reference import scaled_error, tolerance
    ref, _ = mixed(chart)
    rng = np.random.default_rng(5)
    vals, sel = ref.values, oc.selected(ref)
    for s in range(3):
        dx, H, _, _, floor = oc.obs_step(ref, vals, kind, 0.0, sel)
        tol, _ = tolerance(H, dx, ref.magnitude(vals), floor)
        for _ in range(3):
            dx2 = oc.obs_step(ref, vals * (1 + rng.uniform(-1, 1, vals.shape) * 1.1e-16), kind, 0.0, sel)[0]
            assert scaled_error(dx2, dx, H) <= 0.25 * tol, (s, tol)
        vals = ref.retract(vals, dx)


_PLAIN = {}


@pytest.mark.parametrize("kind", [rc.GEMAN_MCCLURE, rc.DCS])
def test_planted_false_matches(kind):
    """Six observations that measure the neighbouring landmark: the plain solve is off by more than a metre, the redescending losses
    recover the trajectory, give the six a weight below 0.1 and leave every other observation above 0.9."""
    cpu = oc.planted_reference(kind)
    ref, bad = cpu["ref"], cpu["bad"]
    assert len(bad) == 6 and len(cpu["w"]) == 138
    good = np.setdiff1d(np.arange(len(cpu["w"])), bad)
    err = rc.pose_error(ref, cpu["values"], cpu["T"])
    if not _PLAIN:
        vals, _, _ = oc.obs_irls(ref, 0, 0.0, cpu["sel"], oc.PLANTED_STEPS)
        _PLAIN["err"] = rc.pose_error(ref, vals, cpu["T"])
    print(f"[obs-loss] planted kind {kind}: pose error {err:.4f} m (plain {_PLAIN['err']:.4f} m), false matches' weights <= {cpu['w'][bad].max():.3e}, "
          f"the others' >= {cpu['w'][good].min():.4f}")
    assert _PLAIN["err"] > 1.0
    assert err <= 0.1
    assert (cpu["w"][bad] < 0.1).all() and (cpu["w"][good] > 0.9).all()
    full = np.ones(len(ref.ftype))
    full[oc.lf_index(ref)] = cpu["w"]
    assert oc.landmarks_keep_an_inlier(ref, full)
