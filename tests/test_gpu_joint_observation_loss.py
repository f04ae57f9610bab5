"""The observation loss on the exact joint multi-robot pass (slide_chol_batch_set_observation_loss: k_lin_lf_robust_b in k_lin_lf_b's
place in every batched pass) against the numpy reweighted joint step of tests/joint_observation_loss_cases.py.  The shards run in a
sibling of test_gpu_joint_step.py's Run built with observation_loss_cases.params (both sigmas 0.05); every one_pass() is compared
with the least-squares step of the joint graph's full whitened Jacobian in which the selected landmark factors carry
sigma / sqrt(w), w taken at the point the pass starts from.  The bar is gn_reference.tolerance alone; weights are read back and
compared at rtol 1e-9, s^2 at rtol 1e-9 + 1e-12 (the single-graph test's bars), s^2 of the observations moved by TIGHT sigmas or more
at rtol 1e-9 alone; read_values keeps asserting that every replica of a shared landmark agrees bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_graphs as jg                                                       # noqa: E402
import joint_observation_loss_cases as jo                                       # noqa: E402
import joint_robust_cases as jr                                                 # noqa: E402
import observation_loss_cases as oc                                             # noqa: E402
import robust_cases as rc                                                       # noqa: E402
from gn_reference import scaled_error, tolerance                                # noqa: E402
from test_gpu_joint_marginals import dense_inverse                              # noqa: E402
from test_gpu_joint_step import Run                                             # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = {v: k for k, v in rc.KINDS.items()}
_CASES = {}


def case(name):
    """The builders are deterministic and a Run does not change its J: built once (two_pass builds twice)."""
    if name not in _CASES:
        _CASES[name] = {"kinds": jo.kinds_case, "both": jo.both_case, "r1": lambda: jo.members_case(1), "r3": lambda: jo.members_case(3),
                        "planted": jo.planted_case}[name]() if isinstance(name, str) else jo.edge_case(*name)
    return _CASES[name]


class ObsRun(Run):
    """test_gpu_joint_step.Run with the reference and the shards under observation_loss_cases.params(chart)."""

    def __init__(self, s, J, chart=0, pcg_iters=0):
        import torch
        from slide_slam_amd.distributed import PassDriver, setup_local_shards
        self.dev = torch.device("cuda", 0)
        self.J, self.chart = J, chart
        self.ref = jo.reference(J, chart)
        self.shards, assoc = jg.build(J, lambda: s.SlideGraph(s.default_params(**oc.params(chart)[1])))
        self.gid = assoc[0]
        self.batch = s.CholBatch(J.R)
        for t, sh in enumerate(self.shards):
            sh.graph.join_chol_batch(self.batch, t)
        bufs, self.info = setup_local_shards(self.shards, None, device=self.dev, assoc=assoc)
        self.drv = PassDriver(self.shards, bufs, self.info["n_slots"], batch=self.batch, device=self.dev, pcg_iters=pcg_iters,
                              arrow=not pcg_iters, sep_dim=self.info["sep_dim"], sep_prof=self.info.get("sep_prof"))
        if J.relmeas:
            assert self.drv.setup_ghosts(J.relmeas) > 0
        self.rows = jo.batch_rows(J)
        self.f = jo.batch_to_export(J, self.ref)
        self.tight = np.isin(self.f, jo.moved_factors(J, self.ref, jo.TIGHT))


def sync():
    import torch
    torch.cuda.synchronize()


def set_loss(run, kind, param=0.0, mask=7):
    """Through the driver where it runs exact joint passes, else (one robot: no separator, a plain batched pass) on the batch."""
    target = run.drv if run.drv.arrow else run.batch
    target.set_observation_loss(NAMES.get(kind, kind) if kind else None, param, points=bool(mask & 1), cubes=bool(mask & 2),
                                cylinders=bool(mask & 4))


def check_weights(run, w, s2, tag=""):
    """CholBatch.observation_weights() against the reference's w and s^2 of the pass's linearisation: rows, keys and order
    (slot, the member's insertion order), the weights at rtol 1e-9, s^2 at rtol 1e-9 + 1e-12 and, for the observations moved by
    TIGHT sigmas or more (s >= 1 there: test_joint_observation_loss_reference.py), at rtol 1e-9 alone.  -> the read-back."""
    ow = run.batch.observation_weights()
    f = run.f
    assert ow["n"] == len(f) == len(ow["weight"])
    got = list(zip(ow["slot"].tolist(), ow["pose_idx"].tolist(), ow["cls"].tolist(), ow["lm_idx"].tolist()))
    assert got == [(r, p, c, l) for (r, p, c, l, _) in run.rows]
    if len(f):
        dw = np.abs(ow["weight"] / w[f] - 1).max()
        ds = (np.abs(ow["s2"] - s2[f]) / (1e-9 * np.abs(s2[f]) + 1e-12)).max()
        print(f"[joint-obs-loss] {tag}: read-back of {len(f)} rows, weights' rel. error {dw:.3e}, s2 error / (1e-9 s2 + 1e-12) {ds:.3e}")
        assert np.allclose(ow["weight"], w[f], rtol=1e-9, atol=0)
        assert np.allclose(ow["s2"], s2[f], rtol=1e-9, atol=1e-12)
        t = run.tight
        assert np.allclose(ow["s2"][t], s2[f][t], rtol=1e-9, atol=0) and (s2[f][t] >= 1.0).all()
    return ow


def check_passes(run, kind, param=0.0, mask=7, steps=2, vals=None, tag="", need_effect=True, closure=None, after=None, moving=None):
    """`steps` passes, each against the reweighted joint step at the point it starts from (gn_reference.tolerance alone) and with
    the read-back of its weights.  closure: (kind, param, selection) of the batch's closure loss, set as well.  moving: the first
    so many passes must move the graph by more than 1e-6 (default: all; the planted scenario's measurements are exact, its later
    passes have converged).
    -> (values, last w, last s2, per-pass (tolerance, |W dx|, min W))."""
    ref = run.ref
    sel = oc.selected(ref, mask)
    if vals is None:
        vals = run.values()
        assert np.array_equal(vals, ref.values)
    w = s2 = None
    rec = []
    for s in range(steps):
        dx, H, w, s2, floor = oc.obs_step(ref, vals, kind, param, sel, closure)
        run.drv.one_pass()
        sync()
        new = run.values()
        tol, kappa = tolerance(H, dx, ref.magnitude(vals), floor)
        err = scaled_error(ref.tangent(vals, new), dx, H)
        print(f"[joint-obs-loss] {tag} pass {s}: scaled_error {err:.3e} tolerance {tol:.3e} kappa {kappa:.3e}")
        assert np.linalg.norm(dx) > 1e-6 or s >= (steps if moving is None else moving)
        assert err <= tol, (s, err, tol, kappa)
        if kind and need_effect:
            # (the loss shows: the plain step at this point lies outside the bound, so a pass that ignored the loss would fail)
            assert scaled_error(ref.step(vals)[0], dx, H) > 10 * tol
        check_weights(run, w, s2, f"{tag} pass {s}")
        if after is not None:
            after(run, vals, w, s2)
        wd = np.sqrt(np.diag(H))
        rec.append((tol, float(np.linalg.norm(wd * dx)), float(wd.min())))
        vals = new
    return vals, w, s2, rec


def poses(run):
    return np.array([sh.graph.get_pose12(0, k)[1] for r, sh in enumerate(run.shards) for k in range(run.J.sizes[r])])


# ---- 1: the four kinds, both charts -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("kind", sorted(rc.KINDS))
def test_kinds_and_charts(gpu, kind, chart):
    """2 robots of 12 poses; points, cubes and cylinders, private and shared, observations moved to both sides of the kinks and
    gross ones in every class, a down-weighted observation of a shared landmark in each robot: two passes; at both points the
    plain joint step lies more than 10 tolerances away."""
    r = ObsRun(gpu, case("kinds"), chart)
    try:
        set_loss(r, rc.KINDS[kind])
        _, w, _, _ = check_passes(r, rc.KINDS[kind], tag=f"{kind} chart {chart}")
        assert (w[r.f] < 1.0).sum() >= 8
    finally:
        r.close()


# ---- 2: the edges of both regions of the launch, each class bit alone ---------------------------------------------------------------

@pytest.mark.parametrize("bit", [0, 1, 2])
@pytest.mark.parametrize("n_br,n_nbr", jo.EDGES)
def test_region_edges(gpu, n_br, n_nbr, bit):
    """Robot 0: n_br bearing-range factors (one thread each, workgroups of 256) and n_nbr cube / cylinder factors (32 lanes each,
    eight per workgroup) with moved observations on both sides of every boundary; robot 1 has three bearing-range factors and no
    cube or cylinder, robot 2 no landmark factor at all, and the grid sized for robot 0 overruns both.  Cauchy on one class: every
    factor of it with a residual shows, the others read 1."""
    r = ObsRun(gpu, case((n_br, n_nbr)), 0)
    try:
        set_loss(r, rc.CAUCHY, mask=1 << bit)
        check_passes(r, rc.CAUCHY, mask=1 << bit, steps=1, tag=f"edges {n_br}/{n_nbr} bit {bit}", need_effect=bit == 0)
        ow = r.batch.observation_weights()
        on = ow["cls"] == (2, 1, 0)[bit]
        assert (ow["weight"][~on] == 1.0).all() and int((ow["slot"] == 0).sum()) == n_br + n_nbr and not (ow["slot"] == 2).any()
        if bit == 0:
            assert (ow["weight"][on] < 1.0).all()
    finally:
        r.close()


# ---- 3: batch sizes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 3])
def test_members(gpu, R):
    """R = 1: one robot, a plain batched pass with no separator, the loss set on the batch; R = 3: shared with the next robot."""
    r = ObsRun(gpu, case(f"r{R}"), 0)
    try:
        assert r.drv.arrow == (R > 1)
        set_loss(r, rc.HUBER)
        _, w, _, _ = check_passes(r, rc.HUBER, tag=f"R {R}")
        assert (w[r.f] < 1.0).any()          # (the gross observation stays past Huber's k)
    finally:
        r.close()


# ---- 4: off means off -------------------------------------------------------------------------------------------------------------

def test_off_means_off(gpu):
    """Two passes give the same poses bit for bit on a batch that never saw the call, with kind 0, with Huber at k = 1e12 (the
    robust kernel runs, every w is exactly 1: x * 1.0 == x) and after set then clear; the read-back without a loss reports w = 1 and
    the same s^2."""
    def run(prepare):
        r = ObsRun(gpu, case("kinds"), 0)
        try:
            prepare(r)
            r.drv.one_pass()
            r.drv.one_pass()
            sync()
            return poses(r), r.batch.observation_weights()
        finally:
            r.close()

    base, ow0 = run(lambda r: None)
    assert (ow0["weight"] == 1.0).all() and ow0["n"] == len(jo.batch_rows(case("kinds")))
    off, owo = run(lambda r: set_loss(r, 0))
    assert np.array_equal(base, off) and np.array_equal(owo["s2"], ow0["s2"])
    huge, owh = run(lambda r: set_loss(r, rc.HUBER, 1e12))
    assert (owh["weight"] == 1.0).all() and np.allclose(owh["s2"], ow0["s2"], rtol=1e-9, atol=1e-12)
    assert np.array_equal(base, huge)
    cleared, owc = run(lambda r: (set_loss(r, rc.GEMAN_MCCLURE), set_loss(r, 0)))
    assert np.array_equal(base, cleared) and (owc["weight"] == 1.0).all() and np.array_equal(owc["s2"], ow0["s2"])
    # set, one reweighted pass, clear: nothing of the members was rewritten - two further passes are the plain joint steps
    r = ObsRun(gpu, case("kinds"), 0)
    try:
        set_loss(r, rc.GEMAN_MCCLURE)
        vals, w, _, _ = check_passes(r, rc.GEMAN_MCCLURE, steps=1, tag="off: on")
        set_loss(r, 0)
        check_passes(r, 0, steps=2, vals=vals, tag="off: cleared")
    finally:
        r.close()


# ---- 5: the cut pass --------------------------------------------------------------------------------------------------------------

def test_cut_pass_matches_the_whole_pass(gpu):
    """PassDriver.force_parts on one process: the poses and the weights of the whole pass, bit for bit."""
    out = []
    for parts in (False, True):
        r = ObsRun(gpu, case("kinds"), 0)
        try:
            r.drv.force_parts = parts
            set_loss(r, rc.CAUCHY)
            if parts:
                check_passes(r, rc.CAUCHY, tag="cut pass")
            else:
                r.drv.one_pass()
                r.drv.one_pass()
                sync()
            ow = r.batch.observation_weights()
            out.append((poses(r), ow["weight"], ow["s2"]))
        finally:
            r.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert (out[0][1] < 1.0).all()


# ---- 6: changing the loss between passes ------------------------------------------------------------------------------------------

def test_changing_the_loss_recaptures(gpu):
    """Huber, two passes (the second replays the captured pass); then Cauchy on points and cylinders only: the next pass is the
    reference's under the new loss; then the same loss set again (a re-capture of the same pass)."""
    r = ObsRun(gpu, case("kinds"), 0)
    try:
        set_loss(r, rc.HUBER)
        vals, _, _, _ = check_passes(r, rc.HUBER, steps=2, tag="change: huber")
        with_huber = r.batch.observation_weights()
        set_loss(r, rc.CAUCHY, mask=5)
        vals, _, _, _ = check_passes(r, rc.CAUCHY, mask=5, steps=1, vals=vals, tag="change: cauchy, points and cylinders", need_effect=False)
        ow = r.batch.observation_weights()
        assert (ow["weight"][ow["cls"] == 1] == 1.0).all() and (ow["weight"][ow["cls"] != 1] < with_huber["weight"][ow["cls"] != 1]).any()
        set_loss(r, rc.CAUCHY, mask=5)
        check_passes(r, rc.CAUCHY, mask=5, steps=1, vals=vals, tag="change: set again", need_effect=False)
    finally:
        r.close()


# ---- 7: both losses at once -------------------------------------------------------------------------------------------------------

def test_both_losses(gpu):
    """Huber on the observations and Cauchy on the closures and inter-robot measurements of one batch: the step is the reference's
    with both; the observation read-back as above, the closure read-back still at 1e-12 with both ends of every inter-robot
    factor bit for bit."""
    J = case("both")
    r = ObsRun(gpu, J, 0)
    try:
        assert len(J.relmeas) == 2 and len(J.closures) == 2
        csel = jr.selection(J, r.ref)
        set_loss(r, rc.HUBER)
        r.drv.set_robust_loss("cauchy")

        def closure_read_back(run, vals, w, s2):
            cw = run.batch.closure_weights()
            exp = J.expected_rows(run.ref)
            assert cw["n"] == len(exp)
            f = np.array([e[7] for e in exp], int)
            assert np.abs(cw["weight"] / w[f] - 1).max() <= 1e-12 and np.abs(cw["s2"] / s2[f] - 1).max() <= 1e-12
            ends = {}
            for g, a, b in zip(cw["ghost_id"], cw["weight"], cw["s2"]):
                if g >= 0:
                    ends.setdefault(int(g), []).append((a, b))
            assert sorted(ends) == list(range(len(J.relmeas)))
            for g, lst in ends.items():
                assert len(lst) == 2 and lst[0] == lst[1], (g, lst)
        _, w, _, _ = check_passes(r, rc.HUBER, tag="both", closure=(rc.CAUCHY, 0.0, csel), after=closure_read_back)
        assert (w[csel] < 0.5).all() and (w[r.f] < 1.0).sum() >= 8
    finally:
        r.close()


# ---- 8: the joint queries describe the reweighted system --------------------------------------------------------------------------

def test_marginals_of_the_reweighted_system(gpu):
    """After a pass under Geman-McClure, get_pose_covariances on the batch against the inverse of the reweighted H at the point the
    pass linearised, Jacobi-scaled, with test_gpu_joint_marginals.dense_inverse's tolerance (what test_gpu_joint_info_gain.py
    uses); the inverse of the unweighted H lies outside it.  A setter call makes the query wait for the next pass."""
    r = ObsRun(gpu, case("kinds"), 0)
    try:
        ref = r.ref
        set_loss(r, rc.GEMAN_MCCLURE)
        vals = r.values()
        _, _, w, _, _ = oc.obs_step(ref, vals, rc.GEMAN_MCCLURE, 0.0, oc.selected(ref))
        plain = dense_inverse(ref, vals)[0]
        base = ref.fsig
        ref.fsig = base / np.sqrt(w)[:, None]
        try:
            Sig, wj, tol, kappa = dense_inverse(ref, vals)
        finally:
            ref.fsig = base
        r.drv.one_pass()
        sync()
        scale = np.abs(Sig * np.outer(wj, wj)).max()
        worst = other = 0.0
        for rr in range(r.J.R):
            blocks = r.batch.get_pose_covariances(rr, np.arange(r.J.sizes[rr]))
            for k, b in enumerate(blocks):
                v = ref.pose_var(rr, k)
                o0, o1 = ref.off[v], ref.off[v + 1]
                ww = np.outer(wj[o0:o1], wj[o0:o1])
                worst = max(worst, float(np.abs((b - Sig[o0:o1, o0:o1]) * ww).max() / scale))
                other = max(other, float(np.abs((b - plain[o0:o1, o0:o1]) * ww).max() / scale))
        print(f"[joint-obs-loss] marginals: worst / tolerance {worst / tol:.3e} (tol {tol:.2e}, kappa {kappa:.2e}); against the unweighted inverse {other / tol:.3e}")
        assert worst <= tol and other > 10 * tol
        set_loss(r, rc.HUBER)
        with pytest.raises(gpu.SlideError):
            r.batch.get_pose_covariances(0, [0])
    finally:
        r.close()


# ---- 9: the planted scenario ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["geman_mcclure", "dcs"])
def test_planted_scenario(gpu, kind):
    """test_joint_observation_loss_reference.py's scenario and step count: every pass within the reference step's bound at its own
    point, and at the end the CPU run of the numpy reference as the yardstick for poses and weights alike (the method of
    test_gpu_joint_robust_loss.py).
    Poses: step s admits an unscaled error of tolerance_s |W_s dx_s| / min(W_s); the final values lie within the sum B_8 of the eight.
    Weights: they are those of the LAST linearisation, whose point lies within B_7 of the CPU run's.  Every false observation is a
    bearing-range factor; its whitened residual (two bearing rows, one range row, sigma 0.05) moves by at most
    K = (2 + 2 / rho_min) B_7 / sigma when pose and point move by B_7 in all (the pose's rotation and translation and the point's
    position each by at most B_7; a bearing moves by a displacement over the range rho, rho_min = 2 m here, and by the rotation
    itself).  So |d s^2| <= 2 s K + K^2 and, since |d ln w / d s^2| <= 2 / (c^2 + s^2) for both losses (Phi for c^2; zero inside
    DCS's kink), |w_gpu / w_cpu - 1| <= expm1(2 |d s^2| / (c^2 + max(s^2 - |d s^2|, 0))), plus the 1e-9 of the read-back.
    Asserted per factor."""
    k = rc.KINDS[kind]
    cpu = jo.planted_reference(k)
    J = cpu["J"]
    r = ObsRun(gpu, J, 0)
    try:
        set_loss(r, k, jo.PLANTED_PARAM[k])
        vals, w, s2, rec = check_passes(r, k, jo.PLANTED_PARAM[k], steps=jo.PLANTED_STEPS, tag=f"planted {kind}", need_effect=False, moving=2)
        ref = r.ref
        ow = r.drv.observation_weights()
        assert np.array_equal(ow["robot"], ow["slot"])
        got = ow["weight"]
        unscaled = [tol * nrm / wmin for tol, nrm, wmin in rec]
        b7, b8 = sum(unscaled[:-1]), sum(unscaled)
        pts, s2c, wc = cpu["trace"][-1][0], cpu["trace"][-1][4][r.f], cpu["w"][r.f]
        rho = np.array([np.linalg.norm(pts[int(ref.fv[f, 0]), 9:12] - pts[int(ref.fv[f, 1]), :3]) for f in r.f])
        assert rho.min() >= 2.0
        c2 = jo.PLANTED_PARAM[k] ** 2 if k == rc.GEMAN_MCCLURE else jo.PLANTED_PARAM[k]
        K = (2.0 + 2.0 / 2.0) * b7 / jo.SIGMA
        ds2 = 2.0 * np.sqrt(s2c) * K + K * K
        allow = 1e-9 + np.expm1(2.0 * ds2 / (c2 + np.maximum(s2c - ds2, 0.0)))
        wdiff = np.abs(got / wc - 1)
        diff = float(np.linalg.norm(ref.tangent(cpu["values"], vals)))
        err = jr.planted_truth_error(J, ref, vals)
        bad = np.isin(r.f, cpu["bad"])
        print(f"[joint-obs-loss] planted {kind}: |gpu - cpu| {diff:.3e} bound {b8:.3e}, RMS pose error {err:.4e} m, weights vs cpu run "
              f"{wdiff.max():.3e}, largest weight difference / its bound {(wdiff / allow).max():.3e}; false <= {got[bad].max():.3e}, true >= {got[~bad].min():.4f}")
        assert (wdiff <= allow).all(), (wdiff, allow)
        assert diff <= b8
        assert err <= jr.planted_truth_error(J, ref, cpu["values"]) + b8          # (an RMS of position differences is at most |gpu - cpu|)
    finally:
        r.close()


# ---- 10: refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals(gpu):
    """Each by code and message: a bad kind, a bad mask, a NaN param; the read-back before a pass, after a change of loss, after a
    member left, with cap below n; PCG in both orders; the per-graph setter on a member and a join with a per-graph loss, both
    still refused; the driver without a batch or without exact joint passes."""
    from slide_slam_amd.distributed import PassDriver
    L = gpu.lib()
    batch = gpu.CholBatch(2)
    for kind in (-1, 5):
        with pytest.raises(gpu.SlideError, match="INVALID.*chol_batch_set_observation_loss.*kind"):
            batch.set_observation_loss(kind)
    with pytest.raises(ValueError):
        batch.set_observation_loss("tukey")
    for m in (8, 15, -1):
        assert L.slide_chol_batch_set_observation_loss(C.c_void_p(batch.h), C.c_int(1), C.c_double(0.0), C.c_int(m)) == -1
        assert "class_mask" in gpu.api.last_error()
    with pytest.raises(gpu.SlideError, match="INVALID.*not a number"):
        batch.set_observation_loss("huber", float("nan"))
    batch.set_observation_loss("huber")
    with pytest.raises(gpu.SlideError, match="INVALID.*observation loss"):
        batch.set_pcg(5)
    batch.set_pcg(0)
    batch.set_observation_loss(None)
    batch.set_pcg(5)
    with pytest.raises(gpu.SlideError, match="INVALID.*PCG"):
        batch.set_observation_loss("huber")
    batch.set_pcg(0)
    batch.set_observation_loss("cauchy")
    with pytest.raises(gpu.SlideError, match="INVALID.*pass first"):
        batch.observation_weights()
    batch.set_observation_loss(None)

    r = ObsRun(gpu, case("kinds"), 0)
    try:
        set_loss(r, rc.HUBER)
        with pytest.raises(gpu.SlideError, match="INVALID.*pass first"):
            r.batch.observation_weights()
        r.drv.one_pass()
        sync()
        ow = r.batch.observation_weights()
        part = r.batch.observation_weights(cap=5)                 # (cap below n: the full count, the first rows)
        assert part["n"] == ow["n"] > 5 and len(part["weight"]) == 5
        for key in ("slot", "pose_idx", "cls", "lm_idx", "weight", "s2"):
            assert np.array_equal(part[key], ow[key][:5])
        big = r.batch.observation_weights(cap=ow["n"] - 1)        # (the cut falls inside the last member)
        assert np.array_equal(big["weight"], ow["weight"][:-1])
        assert r.batch.observation_weights(cap=0)["n"] == ow["n"]
        # a member's own read-back does not know the batch's loss: w = 1, s^2 of the scaled record
        own = r.shards[0].graph.observation_weights()
        n0 = int((ow["slot"] == 0).sum())
        assert own["n"] == n0 and (own["weight"] == 1.0).all()
        assert np.allclose(own["s2"], (ow["weight"] * ow["s2"])[:n0], rtol=1e-9, atol=1e-12)
        # the per-graph calls keep refusing
        with pytest.raises(gpu.SlideError, match="INVALID.*set_observation_loss.*joined a batch.*slide_chol_batch_set_observation_loss"):
            r.shards[0].graph.set_observation_loss("huber")
        set_loss(r, rc.CAUCHY)                  # (a changed loss: nothing was linearised under it yet)
        with pytest.raises(gpu.SlideError, match="INVALID.*pass first"):
            r.batch.observation_weights()
        r.drv.one_pass()
        sync()
        assert r.batch.observation_weights()["n"] == ow["n"]
        r.shards[1].graph.join_chol_batch(None)                   # (a member left)
        with pytest.raises(gpu.SlideError, match="INVALID.*pass first"):
            r.batch.observation_weights()
        r.shards[1].graph.set_observation_loss("huber")           # (no member any more: its own loss may be set ...)
        with pytest.raises(gpu.SlideError, match="INVALID.*join_chol_batch.*observation loss"):
            r.shards[1].graph.join_chol_batch(r.batch, 1)         # (... and then it cannot join)
        r.shards[1].graph.set_observation_loss(None)
    finally:
        r.close()

    rp = ObsRun(gpu, case("kinds"), 0, pcg_iters=3)
    try:
        with pytest.raises(ValueError, match="exact joint"):
            rp.drv.set_observation_loss("huber")
        with pytest.raises(gpu.SlideError, match="INVALID.*PCG"):
            rp.batch.set_observation_loss("huber")
        loose = PassDriver([], [], 0)
        with pytest.raises(ValueError, match="exact joint"):
            loose.set_observation_loss("huber")
    finally:
        rp.close()
