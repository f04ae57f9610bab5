"""The robust loss on the landmark observation factors (slide_graph_set_observation_loss: iteratively reweighted least squares fused
into the linearisation kernel, k_lin_lf_robust) against the numpy step of tests/observation_loss_cases.py: every gauss_newton(1) /
solve() of the product is compared with the least-squares step of the full whitened Jacobian in which the selected factors carry
sigma / sqrt(w), w taken at the linearisation point — gn_reference.tolerance and scaled_error as test_gpu_robust_loss.py uses them;
weights at rtol 1e-9, s^2 at rtol 1e-9 + atol 1e-12."""
import ctypes as C
import os

import numpy as np
import pytest

import observation_loss_cases as oc
import robust_cases as rc
import stream_graphs as sg
from gn_reference import Reference, scaled_error, tolerance
from oracle import pyoracle as po
from test_gpu_gn_step import gpu_values

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def build_pair(gpu, build, chart=0, fan=False):
    """(reference, SlideGraph, what the builder returned[, the Fan over both])."""
    op, gp = oc.params(chart)
    og = po.OracleGraph(op)
    G = gpu.SlideGraph(gpu.default_params(**gp))
    if fan:
        f = rc.Fan(G, og)
        out = build(f)
        return Reference(og, chart), G, out, f
    build(og)
    out = build(G)
    return Reference(og, chart), G, out


def check_weights(G, ref, w, s2, tag=""):
    """observation_weights() against the reference's per-factor w and s^2 (arrays over all factors of the export)."""
    lf = oc.lf_index(ref)
    ow = G.observation_weights()
    assert ow["n"] == len(lf) == len(ow["weight"])
    keys = list(zip(ow["robot"].tolist(), ow["pose_idx"].tolist(), ow["cls"].tolist(), ow["lm_idx"].tolist()))
    assert keys == oc.factor_keys(ref)
    dw = np.abs(ow["weight"] / w[lf] - 1).max()
    ds = (np.abs(ow["s2"] - s2[lf]) / (1e-9 * np.abs(s2[lf]) + 1e-12)).max()
    print(f"[obs-loss] {tag}: weights' rel. error {dw:.3e}, s2 error / (1e-9 s2 + 1e-12) {ds:.3e}")
    assert np.allclose(ow["weight"], w[lf], rtol=1e-9, atol=0)
    assert np.allclose(ow["s2"], s2[lf], rtol=1e-9, atol=1e-12)
    return ow


def check_obs_steps(ref, G, kind, param, sel, steps, values=None, tag="", closure=None):
    """check_robust_steps of test_gpu_robust_loss.py with the observation loss's reference step; the read-back is checked after
    every step.  -> (values, last w, last s2, per-step (tol, |W dx|, min W))."""
    vals = ref.values if values is None else values
    w = s2 = None
    rec = []
    for s in range(steps):
        dx, H, w, s2, floor = oc.obs_step(ref, vals, kind, param, sel, closure)
        assert G.gauss_newton(1) == 0
        new = gpu_values(G, ref)
        got = ref.tangent(vals, new)
        tol, kappa = tolerance(H, dx, ref.magnitude(vals), floor)
        err = scaled_error(got, dx, H)
        print(f"[obs-loss] {tag} step {s}: scaled_error {err:.3e} tolerance {tol:.3e} kappa {kappa:.3e}")
        assert err <= tol, (s, err, tol, kappa)
        check_weights(G, ref, w, s2, f"{tag} step {s}")
        wd = np.sqrt(np.diag(H))
        rec.append((tol, float(np.linalg.norm(wd * dx)), float(wd.min())))
        vals = new
    return vals, w, s2, rec


_SIG = {}


def mixed(gpu, chart=0):
    if chart not in _SIG:
        _SIG[chart] = oc.mixed_cube_sigmas(chart)
    ref, G, (_, planted) = build_pair(gpu, lambda g: oc.mixed_graph(g, _SIG[chart]), chart)
    return ref, G, planted


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("kind", sorted(rc.KINDS))
def test_one_step_against_the_reference(gpu, kind, chart):
    """(1) Points, cubes and cylinders interleaved, observations planted at whitened norms 0.97 / 1.03 (DCS's kink), 1.3 / 1.4
    (Huber's) and 60 in every class: three single steps."""
    ref, G, planted = mixed(gpu, chart)
    q = sorted(planted)
    s0 = np.sqrt(rc.whitened_norms2(ref)[oc.lf_index(ref)][q])
    assert np.allclose(s0, [planted[f] for f in q], rtol=1e-6)
    G.set_observation_loss(kind)
    check_obs_steps(ref, G, rc.KINDS[kind], 0.0, oc.selected(ref), 3, tag=f"{kind} chart {chart}")


@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_bearing_range_thread_edges(gpu, N):
    """(2) N bearing-range factors, one thread each in workgroups of 256: the moved observations first, last and on both sides of
    every boundary.  Under Cauchy (k = 0.1) every factor is down-weighted, so one the kernel missed, or took for another, moves the
    step and its own weight away from the reference's."""
    ref, G, moved = build_pair(gpu, lambda g: oc.br_edge_graph(g, N))
    assert len(oc.lf_index(ref)) == N
    G.set_observation_loss("cauchy")
    _, w, _, _ = check_obs_steps(ref, G, rc.CAUCHY, 0.0, oc.selected(ref), 1, tag=f"br edges N {N}")
    assert (w[oc.lf_index(ref)][moved] < 0.01).all()


@pytest.mark.parametrize("n_nbr", [1, 7, 8, 9, 17])
def test_cube_cylinder_lane_edges(gpu, n_nbr):
    """(3) n_nbr cube / cylinder factors, 32 lanes each and eight per workgroup, every one behind a bearing-range factor: the
    one-thread region's threads must skip them and the 32-lane region's must skip the rest."""
    ref, G, _ = build_pair(gpu, lambda g: oc.nbr_edge_graph(g, n_nbr))
    assert (ref.ftype[oc.lf_index(ref)] != po.F_BR).sum() == n_nbr
    G.set_observation_loss("cauchy")
    check_obs_steps(ref, G, rc.CAUCHY, 0.0, oc.selected(ref), 2, tag=f"nbr edges {n_nbr}")


@pytest.mark.parametrize("bit", [0, 1, 2])
def test_class_mask(gpu, bit):
    """(4) Each bit alone: only that class is reweighted (Cauchy: every factor of it with a residual shows), the others read 1."""
    ref, G, _ = mixed(gpu)
    sel = oc.selected(ref, 1 << bit)
    G.set_observation_loss("cauchy", points=bit == 0, cubes=bit == 1, cylinders=bit == 2)
    check_obs_steps(ref, G, rc.CAUCHY, 0.0, sel, 2, tag=f"mask bit {bit}")
    ow = G.observation_weights()
    on = ow["cls"] == (2, 1, 0)[bit]
    assert on.sum() == 12 and (ow["weight"][~on] == 1.0).all() and (ow["weight"][on] < 0.5).sum() >= 3
    assert (ow["s2"][~on] > 0.5).sum() >= 6          # (the unweighted s^2 of the classes left out is reported all the same)


def test_off_means_off_bit_for_bit(gpu):
    """(5) The poses after two steps are the same bits on a graph that never saw the call, after kind 0, under Huber at k = 1e12
    (the robust kernel runs, every w is 1) and after set-then-clear; the linearisation is one launch per step either way and no
    profile stage appears."""
    def run(prep, profile=False):
        _, G, _ = mixed(gpu)
        G.set_profiling(profile)
        prep(G)
        if profile:
            assert G.gauss_newton(1) == 0
            return G
        assert G.gauss_newton(2) == 0
        return np.array([G.get_pose12(0, k)[1] for k in range(12)]), np.array([G.get_landmark(1, k)[1] for k in range(0, 8, 2)])

    def set_then_clear(G):
        G.set_observation_loss("cauchy")
        G.set_observation_loss(None)

    preps = {"never": lambda G: None, "kind 0": lambda G: G.set_observation_loss(0), "huber 1e12": lambda G: G.set_observation_loss("huber", 1e12),
             "set, clear": set_then_clear}
    runs = {tag: run(p) for tag, p in preps.items()}
    for tag in preps:
        assert np.array_equal(runs[tag][0], runs["never"][0]) and np.array_equal(runs[tag][1], runs["never"][1]), tag
    down = run(lambda G: G.set_observation_loss("huber"))
    assert np.abs(down[0] - runs["never"][0]).max() > 1e-4      # (and the default Huber does move the same graph)
    plain, huge = run(preps["never"], True), run(preps["huber 1e12"], True)
    pp, ph = plain.get_profile(), huge.get_profile()
    assert sorted(pp) == sorted(ph) and pp["linearize"]["launches"] == ph["linearize"]["launches"] == 1
    ow = huge.observation_weights()
    assert (ow["weight"] == 1.0).all() and ow["s2"].max() > 3000
    assert np.allclose(plain.observation_weights()["s2"], ow["s2"], rtol=1e-12, atol=0)      # (summed from the records / recorded by the kernel)


def test_both_losses_at_once(gpu):
    """(6) A gross closure and a gross observation, Huber on the closures and Cauchy on the observations: every step is the
    reference's with both reweightings, both read-backs are right; five block columns, so the second and third step replay a
    captured pass, and the loss changed after it (to Huber, then to the points' class alone left out) takes effect on the next
    step: the pass is captured again."""
    ref, G, gross, fan = build_pair(gpu, oc.both_graph, fan=True)
    csel, sel = rc.selected(ref, fan.origin), oc.selected(ref)
    clo = (rc.HUBER, 0.0, csel)
    G.set_robust_loss("huber")
    G.set_observation_loss("cauchy")
    vals, w, s2, _ = check_obs_steps(ref, G, rc.CAUCHY, 0.0, sel, 3, tag="both: cauchy", closure=clo)
    assert w[oc.lf_index(ref)[gross]] < 1e-3 and G.stats()["n_pose"] == 45 and len(G.tile_profile()) == 5
    cw = G.closure_weights()
    assert np.allclose(cw["weight"], w[csel], rtol=1e-9) and np.allclose(cw["s2"], s2[csel], rtol=1e-9) and cw["weight"].min() < 0.1
    G.set_observation_loss("huber")
    vals, w2, _, _ = check_obs_steps(ref, G, rc.HUBER, 0.0, sel, 2, values=vals, tag="both: huber", closure=clo)
    assert w2[oc.lf_index(ref)[gross]] > 10 * w[oc.lf_index(ref)[gross]]
    G.set_observation_loss("huber", points=False)
    vals, w3, _, _ = check_obs_steps(ref, G, rc.HUBER, 0.0, oc.selected(ref, 6), 2, values=vals, tag="both: points left out", closure=clo)
    assert (w3[oc.lf_index(ref)] == 1.0).all()
    assert np.allclose(G.closure_weights()["weight"], w3[csel], rtol=1e-9)


@pytest.mark.parametrize("chart", [0, 1])
def test_incremental_path(gpu, chart):
    """(7) A 36-frame stream with landmarks under Huber; frames 15, 21 and 27 observe the point first seen three frames earlier
    once more, with a range 4 to 6 sigma off.  Three graphs as in test_gpu_robust_loss.py::test_incremental_path: incremental, full
    re-factorisation, wildfire bound at 1e-3; per update the first two are compared with the reweighted step at the tracked
    linearisation points and the read-back of the incremental one with the reference's weights there.  Later updates start above a
    down-weighted observation's pose (pose0): the record keeps, bit for bit, the weight the update before reported."""
    thr = 1e-3
    P = 36
    op, gp = oc.params(chart)
    og = po.OracleGraph(op)
    Gs = [gpu.SlideGraph(gpu.default_params(**gp)) for _ in range(3)]
    inc, full, wf = Gs
    full.set_incremental(False)
    wf.set_wildfire(thr)
    for G in Gs:
        G.set_observation_loss("huber")
    # (initial values 0.01 m / 0.002 rad off: under the 0.05 sigmas of these graphs the default 0.1 m would have every update
    # relinearise old poses, and no update would start above anything)
    S = sg.Stream([inc, full, wf, og], P, seed=3, every=2, noise=0.002)
    tr = sg.Tracker(chart)
    off = {}                       # frame -> (landmark, range offset): the point created at frame k - 3 is seen again from pose k
    for k, d in ((15, 0.2), (21, -0.25), (27, 0.3)):
        off[k] = (("point", 1000 + k - 3), d)
    assert all(lm in S.spec for lm, _ in off.values())
    marks = {}                     # factor number among the landmark factors -> (pose, weight after the update before this one)
    kept, worst = 0, 0.0
    for k in range(P):
        S.frame(k)
        if k in off:
            S.observe(*off[k][0], k, rng_offset=off[k][1])
        ref = Reference(og, chart)
        lf = oc.lf_index(ref)
        _, margin = tr.relinearise()
        assert margin > sg.MARGIN
        for v, key in enumerate(ref.vkey):
            if int(key) not in tr.theta:
                tr.theta[int(key)] = ref.values[v].copy()
                tr.vtype[int(key)] = int(ref.vtype[v])
        theta = np.array([tr.theta[int(key)] for key in ref.vkey])
        dx, H, w, s2, floor = oc.obs_step(ref, theta, rc.HUBER, 0.0, oc.selected(ref))
        for G in Gs:
            assert G.solve() == 0
        got = [gpu_values(G, ref) for G in Gs]
        for key, row in zip(ref.vkey, got[0]):
            tr.est[int(key)] = row.copy()
        for g in got[:2]:
            tol, kappa = tolerance(H, dx, ref.magnitude(theta), floor)
            err = scaled_error(ref.tangent(theta, g), dx, H)
            worst = max(worst, err / tol)
            assert err <= tol, (k, err, tol, kappa)
        assert np.abs(got[2][:, :12] - got[0][:, :12]).max() <= thr, k
        ow = inc.observation_weights()
        assert ow["n"] == len(lf)
        assert np.allclose(ow["weight"], w[lf], rtol=1e-9, atol=0) and np.allclose(ow["s2"], s2[lf], rtol=1e-9, atol=1e-12), k
        if k in off:
            f = len(lf) - 1
            assert ow["weight"][f] < 0.5 and int(ow["pose_idx"][f]) == k
            marks[f] = (k, ow["weight"][f])
        st = inc.incremental_stats()
        print(f"[obs-loss] stream chart {chart} frame {k}: first re-factored column {st['last_first_column']} of {st['block_columns']}, marks {marks}")
        for f, (p, w0) in marks.items():
            if p < k and 64 * st["last_first_column"] > 6 * (p + 1):      # (the update started above the observation's pose)
                assert ow["weight"][f] == w0 and w0 < 1.0, (k, f)
                kept += 1
            marks[f] = (p, ow["weight"][f])      # (an update from a lower pose on relinearises the factor: a new weight, the reference's)
    print(f"[obs-loss] stream chart {chart}: worst scaled_error / tolerance {worst:.3e}, {kept} (update, kept down-weighted observation) pairs")
    assert kept >= 3
    assert inc.incremental_stats()["incremental"] > 10 and full.incremental_stats()["incremental"] == 0


def test_back_end(gpu):
    """(8) The tiny golden replay through SlideBackend: Huber at k = 1e12 gives the plain replay's poses bit for bit; under the
    default Huber every landmark factor is listed with a weight in (0, 1]."""
    from slide_slam_amd.replay import replay_single
    z = np.load(os.path.join(HERE, "golden", "replay_tiny.npz"))
    log = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    runs = {}
    for tag, prm in (("plain", None), ("huge", 1e12), ("huber", 0.0)):
        gb = gpu.SlideBackend(gpu.default_params(), 1)
        if prm is not None:
            gb.graph.set_observation_loss("huber", prm)
        out = replay_single(gb, log)
        n = len(out["pose7"])
        runs[tag] = (np.array(out["pose7"]), np.array([gb.graph.get_pose12(0, k)[1] for k in range(n)]), gb)
    assert np.array_equal(runs["plain"][0], runs["huge"][0]) and np.array_equal(runs["plain"][1], runs["huge"][1])
    gb = runs["huber"][2]
    st = gb.graph.stats()
    ow = gb.graph.observation_weights()
    assert ow["n"] == st["n_factors"] - st["n_pose"] > 100          # (one prior and n_pose - 1 odometry factors are the rest)
    assert len(ow["weight"]) == ow["n"] and (ow["weight"] > 0.0).all() and (ow["weight"] <= 1.0).all()
    assert set(ow["cls"].tolist()) <= {0, 1, 2} and (ow["robot"] == 0).all()
    print(f"[obs-loss] back-end: {ow['n']} landmark factors, {(ow['weight'] < 1).sum()} down-weighted, smallest weight {ow['weight'].min():.3e}")


_PLANTED = {}


def planted(kind):
    if kind not in _PLANTED:
        _PLANTED[kind] = oc.planted_reference(kind)
    return _PLANTED[kind]


@pytest.mark.parametrize("kind", ["geman_mcclure", "dcs"])
def test_planted_false_matches(gpu, kind):
    """(9) The CPU test's scenario and step count: every step within the reference step's bound, the six false matches' final
    weights below 0.1 and all others above 0.9, the final poses within the numpy IRLS's by the steps' bounds accumulated (as
    test_gpu_robust_loss.py::test_planted_closures), and an RMS pose error of at most 0.1 m (numpy: 0.050 m; the plain solve of the
    same graph: 1.90 m)."""
    k = rc.KINDS[kind]
    cpu = planted(k)
    ref, G, (T, bad) = build_pair(gpu, oc.planted_graph)
    G.set_observation_loss(kind, cpu["param"])
    vals, _, _, rec = check_obs_steps(ref, G, k, cpu["param"], oc.selected(ref), oc.PLANTED_STEPS, tag=f"planted {kind}")
    ow = G.observation_weights()
    good = np.setdiff1d(np.arange(ow["n"]), bad)
    # (the weights of the LAST linearisation: the point before the last step, as the reference's)
    print(f"[obs-loss] planted {kind}: false matches' weights <= {ow['weight'][bad].max():.3e}, the others' >= {ow['weight'][good].min():.4f}")
    assert (ow["weight"][bad] < 0.1).all() and (ow["weight"][good] > 0.9).all()
    assert (cpu["w"][bad] < 0.1).all() and (cpu["w"][good] > 0.9).all()
    bound = sum(tol * nrm / wmin for tol, nrm, wmin in rec)
    diff = float(np.linalg.norm(ref.tangent(cpu["values"], vals)))
    err = rc.pose_error(ref, vals, T)
    print(f"[obs-loss] planted {kind}: |gpu - cpu| {diff:.3e} bound {bound:.3e}, pose error {err:.4e} m")
    assert diff <= bound
    assert err <= 0.1


def test_refusals(gpu):
    """(10) Bad kind, bad mask, NaN; the sharded / joint calls while a loss is set and the set call after joining; the read-back
    before the first solve and with a cap below n."""
    ref, G, _ = mixed(gpu)
    L = gpu.lib()
    for kind in (-1, 5):
        with pytest.raises(gpu.SlideError, match="INVALID.*set_observation_loss: kind"):
            G.set_observation_loss(kind)
    with pytest.raises(ValueError):
        G.set_observation_loss("tukey")
    for m in (8, 15, -1):
        assert L.slide_graph_set_observation_loss(G.h, C.c_int(1), C.c_double(0.0), C.c_int(m)) == -1
        assert "set_observation_loss: class_mask" in gpu.api.last_error()
    with pytest.raises(gpu.SlideError, match="INVALID.*set_observation_loss: param is not a number"):
        G.set_observation_loss("huber", float("nan"))
    with pytest.raises(gpu.SlideError, match="INVALID.*get_observation_weights.*solve first"):
        G.observation_weights()
    G.set_observation_loss("huber")
    assert G.gauss_newton(1) == 0
    batch = gpu.CholBatch(1)
    for call in (lambda: G.join_chol_batch(batch, 0), lambda: G.dist_phase(0, 0), lambda: G.dist_pass_local(0)):
        with pytest.raises(gpu.SlideError, match="INVALID.*observation loss"):
            call()
    ow = G.observation_weights()
    n = len(oc.lf_index(ref))
    part = G.observation_weights(cap=7)
    assert ow["n"] == part["n"] == n and len(part["weight"]) == 7 and np.array_equal(part["weight"], ow["weight"][:7])
    assert np.array_equal(part["lm_idx"], ow["lm_idx"][:7]) and G.observation_weights(cap=0)["n"] == n
    out = C.c_int(0)
    assert L.slide_graph_get_observation_weights(G.h, C.c_int(3), None, None, None, None, None, None, C.byref(out)) == 0 and out.value == n
    G.set_observation_loss(None)
    G.join_chol_batch(batch, 0)
    with pytest.raises(gpu.SlideError, match="INVALID.*set_observation_loss.*joined a batch"):
        G.set_observation_loss("huber")
    G.join_chol_batch(None)
    G.set_observation_loss("huber")
    assert G.gauss_newton(1) == 0 and G.observation_weights()["n"] == n
