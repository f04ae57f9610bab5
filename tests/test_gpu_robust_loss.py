"""The robust loss on loop-closure and relative-measurement factors (slide_graph_set_robust_loss: iteratively reweighted least
squares, k_robust_reweight ahead of the linearisation) against the numpy robust step of tests/robust_cases.py: every
gauss_newton(1) / solve() of the product is compared with the least-squares step of the full whitened Jacobian in which the selected
factors carry sigma0 / sqrt(w), w taken at the linearisation point — gn_reference.tolerance and scaled_error as test_gpu_gn_step.py
uses them."""
import ctypes as C

import numpy as np
import pytest

import robust_cases as rc
import stream_graphs as sg
from gn_reference import Reference, scaled_error, tolerance
from oracle import pyoracle as po
from test_gpu_gn_step import gpu_values

pytestmark = pytest.mark.gpu

NAME = "k_robust_reweight"


def build_pair(gpu, build, chart):
    """(reference, SlideGraph, Fan over both, what the builder returned)."""
    og = po.OracleGraph(po.OrcParams.default(pose_chart=chart))
    G = gpu.SlideGraph(gpu.default_params(pose_chart=chart))
    fan = rc.Fan(G, og)
    out = build(fan)
    return Reference(og, chart), G, fan, out


def check_robust_steps(ref, G, kind, param, sel, steps, values=None, tag=""):
    """check_steps of test_gpu_gn_step.py with the reweighted reference.  -> (values, last w, last s2, per-step (tol, |W dx|, min W))."""
    vals = ref.values if values is None else values
    w = s2 = None
    rec = []
    for s in range(steps):
        dx, H, w, s2, floor = rc.robust_step(ref, vals, kind, param, sel)
        assert G.gauss_newton(1) == 0
        new = gpu_values(G, ref)
        got = ref.tangent(vals, new)
        tol, kappa = tolerance(H, dx, ref.magnitude(vals), floor)
        err = scaled_error(got, dx, H)
        print(f"[robust] {tag} step {s}: scaled_error {err:.3e} tolerance {tol:.3e} kappa {kappa:.3e}")
        assert err <= tol, (s, err, tol, kappa)
        wd = np.sqrt(np.diag(H))
        rec.append((tol, float(np.linalg.norm(wd * dx)), float(wd.min())))
        vals = new
    return vals, w, s2, rec


def closure_rows(fan):
    return [(k, o) for k, o in zip(fan.keys, fan.origin) if o]


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("kind", sorted(rc.KINDS))
def test_one_step_against_the_reference(gpu, kind, chart):
    """A chain whose closures have whitened norms 0.3 (an inlier: w = 1 under Huber and DCS), 1.03 and 1.4 (just past DCS's and
    Huber's kinks), 3000 (gross), plus a closure onto a perturbed pose and a relative measurement: three single steps."""
    ref, G, fan, _ = build_pair(gpu, rc.chain_graph, chart)
    sel = rc.selected(ref, fan.origin)
    k = rc.KINDS[kind]
    s0 = np.sqrt(rc.whitened_norms2(ref)[sel])
    assert np.allclose(s0[:4], [0.3, 1.03, 1.4, 3000.0], rtol=1e-6)
    w0 = rc.weight(k, 0.0, s0)
    if kind == "huber":
        assert w0[0] == 1.0 and w0[1] == 1.0 and 0.95 < w0[2] < 1.0 and w0[3] < 1e-3
    if kind == "dcs":
        assert w0[0] == 1.0 and 0.9 < w0[1] < 1.0 and w0[3] == rc.W_MIN
    G.set_robust_loss(kind)
    check_robust_steps(ref, G, k, 0.0, sel, 3, tag=f"{kind} chart {chart}")


@pytest.mark.parametrize("N", [1, 127, 128, 129, 257])
def test_thread_count_edges(gpu, N):
    """N between factors, the kernel's block 128 wide: the selected factors first, last and on both sides of every block boundary,
    odometry everywhere else.  Under Cauchy (k = 0.1) every factor with any residual is down-weighted, so an odometry factor that the
    kernel touched, or a selected one it missed, moves the step away from the reference's."""
    ref, G, fan, selq = build_pair(gpu, lambda g: rc.edge_graph(g, N), 0)
    assert len(fan.origin) == N and [q for q, o in enumerate(fan.origin) if o] == selq
    sel = rc.selected(ref, fan.origin)
    G.set_robust_loss("cauchy")
    _, w, s2, _ = check_robust_steps(ref, G, rc.CAUCHY, 0.0, sel, 1, tag=f"edges N {N}")
    cw = G.closure_weights()
    assert cw["n"] == len(selq) and (w[sel] < 0.5).all()
    assert np.allclose(cw["weight"], w[sel], rtol=1e-9, atol=0) and np.allclose(cw["s2"], s2[sel], rtol=1e-9, atol=0)


def test_exact_when_nothing_is_down_weighted(gpu):
    """Huber with every closure an inlier: w = 1, sigma0 / sqrt(1) = sigma0 bit for bit, and so are the poses after two steps."""
    runs = []
    for loss in (None, "huber"):
        G = gpu.SlideGraph(gpu.default_params())
        rc.inlier_graph(G)
        if loss:
            G.set_robust_loss(loss)
        assert G.gauss_newton(2) == 0
        runs.append(np.array([G.get_pose12(0, k)[1] for k in range(12)]))
        if loss:
            cw = G.closure_weights()
            assert cw["n"] == 3 and (cw["weight"] == 1.0).all() and (cw["s2"] < rc.DEFAULT[rc.HUBER] ** 2).all()
    assert np.array_equal(runs[0], runs[1])
    assert np.abs(runs[0][:, 9:] - np.array([e[:3] for e in rc.inlier_graph(rc._Recorder()).est])).max() > 1e-3      # (the steps moved the chain)


@pytest.mark.parametrize("mask", [1, 2])
def test_class_mask(gpu, mask):
    """Bit 0 alone: the relative measurements keep weight 1; bit 1 alone: the loop closures do; odometry never moves (the step is
    the reference's, in which only the selected class is reweighted — Cauchy, so every reweighted factor shows)."""
    ref, G, fan, _ = build_pair(gpu, rc.mask_graph, 0)
    sel = rc.selected(ref, fan.origin, mask)
    assert sel.sum() == 2
    G.set_robust_loss("cauchy", closures=bool(mask & 1), relative_meas=bool(mask & 2))
    check_robust_steps(ref, G, rc.CAUCHY, 0.0, sel, 2, tag=f"mask {mask}")
    cw = G.closure_weights()
    assert list(cw["kind"]) == [1, 2, 2, 1]
    on = cw["kind"] == (1 if mask == 1 else 2)
    assert (cw["weight"][~on] == 1.0).all() and (cw["weight"][on] < 0.5).all() and (cw["s2"] > 0).all()


def readback_graph(G):
    """Five poses near the origin, two loop closures and a relative measurement with residuals of decimetres to metres: the
    residuals are well conditioned (|t| / |e| of order ten), so weights and norms can be compared to 1e-12."""
    W = rc.gg.World(G, 5, seed=15, origin=(0.1, 0.2, 0.0), noise=0.02)
    G.add_loop_closure(rc._rel(W, 0, 3, dt=(0.5, 0.2, -0.1), drot=(0.02, 0.0, 0.2)), 0, 0, 3, 0)
    R1, t1 = W.T[1][0] @ rc.gg.rot([0, 0, 0.2]), W.T[1][1] + np.array([1.0, 1.0, 0.0])
    G.set_prior(1, rc.gg.p7(R1, t1))
    Ra, ta = W.T[4]
    G.add_relative_meas(rc.gg.p7(Ra.T @ R1 @ rc.gg.rot([0.1, 0, 0]), Ra.T @ (t1 - ta) + np.array([0.4, -0.3, 0.0])), 4, 0, 0, 1)
    G.add_loop_closure(rc._rel(W, 1, 4, dt=(2.0, 0.0, 0.0)), 4, 0, 1, 0)      # (from the later pose to the earlier one: the keys' order is the call's)
    return W


@pytest.mark.parametrize("kind", ["huber", "cauchy"])
def test_read_back(gpu, kind):
    """closure_weights() after a step: the numpy weights and s^2 at the linearisation point to 1e-12 relative, keys and order as
    inserted, a smaller cap still reports the full count; before the first solve it is refused."""
    ref, G, fan, _ = build_pair(gpu, readback_graph, 0)
    G.set_robust_loss(kind)
    with pytest.raises(gpu.SlideError, match="INVALID.*solve first"):
        G.closure_weights()
    sel = rc.selected(ref, fan.origin)
    s2 = rc.whitened_norms2(ref)[sel]
    w = rc.weight(rc.KINDS[kind], 0.0, np.sqrt(s2))
    assert (w > rc.W_MIN).all() and (w < 1.0).all()
    assert G.gauss_newton(1) == 0
    cw = G.closure_weights()
    rows = closure_rows(fan)
    assert cw["n"] == 3 and list(cw["kind"]) == [o for _, o in rows] == [1, 2, 1]
    got_keys = list(zip(cw["from_robot"], cw["from_idx"], cw["to_robot"], cw["to_idx"]))
    assert [tuple(int(x) for x in k) for k in got_keys] == [k for k, _ in rows] == [(0, 0, 0, 3), (0, 4, 1, 0), (0, 4, 0, 1)]
    print(f"[robust] read-back {kind}: weight rel. error {np.abs(cw['weight'] / w - 1).max():.3e}, s2 rel. error {np.abs(cw['s2'] / s2 - 1).max():.3e}")
    assert np.abs(cw["weight"] / w - 1).max() <= 1e-12
    assert np.abs(cw["s2"] / s2 - 1).max() <= 1e-12
    part = G.closure_weights(cap=2)
    assert part["n"] == 3 and len(part["weight"]) == 2 and np.array_equal(part["weight"], cw["weight"][:2])
    assert G.closure_weights(cap=0)["n"] == 3


def test_off_means_off(gpu):
    """The stage is listed by get_profile exactly while a loss is set, and after set_robust_loss(0) the next step is the plain
    reference step (every sigma back at its base value) with every weight 1."""
    ref, G, fan, _ = build_pair(gpu, rc.chain_graph, 0)
    sel = rc.selected(ref, fan.origin)
    G.set_profiling(True)
    plain = gpu.SlideGraph(gpu.default_params())
    rc.chain_graph(plain)
    plain.set_profiling(True)
    assert plain.gauss_newton(1) == 0 and NAME not in plain.get_profile() and "linearize" in plain.get_profile()
    G.set_robust_loss("dcs")
    vals, w, _, _ = check_robust_steps(ref, G, rc.DCS, 0.0, sel, 1, tag="off: dcs on")
    prof = G.get_profile()
    assert prof[NAME]["launches"] == 1 and prof["linearize"]["launches"] == 1
    assert (w[sel] < 1.0).any()
    G.set_robust_loss(0)
    assert NAME not in G.get_profile()
    vals, _, s2, _ = check_robust_steps(ref, G, 0, 0.0, sel, 1, values=vals, tag="off: plain")
    assert NAME not in G.get_profile()
    cw = G.closure_weights()
    assert (cw["weight"] == 1.0).all() and np.allclose(cw["s2"], s2[sel], rtol=1e-9)
    G.set_robust_loss(None)
    assert NAME not in G.get_profile()


@pytest.mark.parametrize("chart", [0, 1])
def test_incremental_path(gpu, chart):
    """A 36-frame stream with loop closures added at frames 24 (to pose 4) and 30 (to pose 9) under Huber: later updates start
    above those poses (pose0), so the closures keep their linearisation AND the weight it was made with.  Per update the incremental
    graph and one that re-factors everything are both compared with the reweighted least-squares step at the tracked linearisation
    points (stream_graphs.check_step, the bound of test_gpu_stream_step.py), and a third graph with the wildfire bound at 1e-3
    stays within that threshold of the exact one."""
    thr = 1e-3
    P, loops = 36, {24: 4, 30: 9}
    og = po.OracleGraph(po.OrcParams.default(pose_chart=chart))
    Gs = [gpu.SlideGraph(gpu.default_params(pose_chart=chart)) for _ in range(3)]
    inc, full, wf = Gs
    full.set_incremental(False)
    wf.set_wildfire(thr)
    for G in Gs:
        G.set_robust_loss("huber")
    fan = rc.Fan(inc, full, wf, og)
    S = sg.Stream([fan], P, seed=3, every=2)
    tr = sg.Tracker(chart)
    kept, worst = 0, 0.0
    for k in range(P):
        S.frame(k)
        if k in loops:
            S.loop(loops[k], k)
        ref = Reference(og, chart)
        _, margin = tr.relinearise()
        assert margin > sg.MARGIN
        for v, key in enumerate(ref.vkey):
            if int(key) not in tr.theta:
                tr.theta[int(key)] = ref.values[v].copy()
                tr.vtype[int(key)] = int(ref.vtype[v])
        theta = np.array([tr.theta[int(key)] for key in ref.vkey])
        sel = rc.selected(ref, fan.origin)
        dx, H, w, _, floor = rc.robust_step(ref, theta, rc.HUBER, 0.0, sel)
        for G in Gs:
            assert G.solve() == 0
        got = [gpu_values(G, ref) for G in Gs]
        for key, row in zip(ref.vkey, got[0]):
            tr.est[int(key)] = row.copy()
        for g in got[:2]:
            mag = ref.magnitude(theta)
            tol, kappa = tolerance(H, dx, mag, floor)
            err = scaled_error(ref.tangent(theta, g), dx, H)
            worst = max(worst, err / tol)
            assert err <= tol, (k, err, tol, kappa)
        assert np.abs(got[2][:, :12] - got[0][:, :12]).max() <= thr, k
        st = inc.incremental_stats()
        lo = min([loops[f] for f in loops if f <= k], default=None)
        if lo is not None and k not in loops and 64 * st["last_first_column"] > 6 * (lo + 1):
            cw = inc.closure_weights()
            assert (cw["weight"] < 1.0).all() and np.allclose(cw["weight"], w[sel], rtol=1e-9)
            kept += 1
    print(f"[robust] stream chart {chart}: worst scaled_error / tolerance {worst:.3e}, {kept} updates kept a down-weighted closure")
    assert kept >= 3
    assert inc.incremental_stats()["incremental"] > 10 and full.incremental_stats()["incremental"] == 0
    print(f"[robust] stream chart {chart}: the wildfire bound kept {wf.wildfire_stats()['kept_total']} blocks")


_PLANTED = {}


def planted(kind):
    if kind not in _PLANTED:
        _PLANTED[kind] = rc.planted_reference(kind)
    return _PLANTED[kind]


@pytest.mark.parametrize("kind", ["geman_mcclure", "dcs"])
def test_planted_closures(gpu, kind):
    """The CPU test's scenario with the same step count: every step within the reference step's bound, the final weights on the same
    side of 0.1 and 0.9, and the final poses within the CPU reference's by the steps' bounds accumulated: step s contributes
    tolerance_s |W_s dx_s| / min(W_s), the unscaled size of an error that the scaled bound admits."""
    k = rc.KINDS[kind]
    cpu = planted(k)
    ref, G, fan, T = build_pair(gpu, rc.planted_graph, 0)
    sel = rc.selected(ref, fan.origin)
    G.set_robust_loss(kind, cpu["param"])
    vals, _, _, rec = check_robust_steps(ref, G, k, cpu["param"], sel, rc.PLANTED_STEPS, tag=f"planted {kind}")
    cw = G.closure_weights()
    nt = len(rc.TRUE_CLOSURES)
    # (the weights of the LAST linearisation: the point before the last step, as the reference's)
    assert (cw["weight"][:nt] > 0.9).all() and (cw["weight"][nt:] < 0.1).all(), cw["weight"]
    assert (cpu["w"][:nt] > 0.9).all() and (cpu["w"][nt:] < 0.1).all()
    bound = sum(tol * nrm / wmin for tol, nrm, wmin in rec)
    diff = float(np.linalg.norm(ref.tangent(cpu["values"], vals)))
    err = rc.pose_error(ref, vals, T)
    print(f"[robust] planted {kind}: |gpu - cpu| {diff:.3e} bound {bound:.3e}, pose error {err:.4e} m")
    assert diff <= bound
    assert err <= 0.02


def test_refusals(gpu):
    """Bad kind, bad mask, and the sharded / joint calls while a loss is set: SLIDE_ERR_INVALID with a message."""
    G = gpu.SlideGraph(gpu.default_params())
    rc.mask_graph(G)
    L = gpu.lib()
    for kind in (-1, 5):
        with pytest.raises(gpu.SlideError, match="INVALID.*kind"):
            G.set_robust_loss(kind)
    with pytest.raises(ValueError):
        G.set_robust_loss("tukey")
    for m in (4, 7, -1):
        assert L.slide_graph_set_robust_loss(G.h, C.c_int(1), C.c_double(0.0), C.c_int(m)) == -1
        assert "class_mask" in gpu.api.last_error()
    G.set_robust_loss("huber")
    assert G.gauss_newton(1) == 0
    batch = gpu.CholBatch(1)
    for call in (lambda: G.join_chol_batch(batch, 0), lambda: G.dist_phase(0, 0), lambda: G.dist_pass_local(0)):
        with pytest.raises(gpu.SlideError, match="INVALID.*robust loss"):
            call()
    G.set_robust_loss(None)
    G.join_chol_batch(batch, 0)
    with pytest.raises(gpu.SlideError, match="INVALID.*joined a batch"):
        G.set_robust_loss("huber")
    G.join_chol_batch(None)
    G.set_robust_loss("huber")
    assert G.gauss_newton(1) == 0 and G.closure_weights()["n"] == 4
