"""The robust loss on the exact joint multi-robot pass (slide_chol_batch_set_robust_loss: k_robust_reweight_b between k_relin_b and
the linearisation of every batched pass) against the numpy reweighted joint step of tests/joint_robust_cases.py.  The shards run in
test_gpu_joint_step.py's Run harness; every one_pass() is compared with the least-squares step of the joint graph's full whitened
Jacobian in which the selected factors — the robots' loop closures and the inter-robot relative-pose factors — carry
sigma0 / sqrt(w), w taken at the point the pass starts from.  The bar is gn_reference.tolerance alone; weights and whitened norms
are read back and compared at 1e-12 relative, and the two ends of every inter-robot factor bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_robust_cases as jr                                                 # noqa: E402
import robust_cases as rc                                                       # noqa: E402
from gn_reference import scaled_error, tolerance                                # noqa: E402
from test_gpu_joint_step import Run                                             # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = {v: k for k, v in rc.KINDS.items()}


def sync():
    import torch
    torch.cuda.synchronize()


def set_loss(run, kind, param=0.0, mask=3):
    """Through the driver where it runs exact joint passes, else (one robot: no separator, a plain batched pass) on the batch."""
    target = run.drv if run.drv.arrow else run.batch
    target.set_robust_loss(NAMES.get(kind, kind) if kind else None, param, closures=bool(mask & 1), relative_meas=bool(mask & 2))


def check_weights(run, w, s2, mask=3, kind=1, tag="", norms=True):
    """CholBatch.closure_weights() against the reference's w and s^2 of the pass's linearisation: rows, keys and order, 1e-12, and
    the two ends of every inter-robot factor bit for bit.  norms=False (the planted scenario, whose true factors end at s << 1,
    where s^2 is a difference of nearly equal numbers): the weights only.  -> the read-back."""
    J, ref = run.J, run.ref
    cw = run.batch.closure_weights()
    exp = J.expected_rows(ref)
    assert cw["n"] == len(exp) == len(cw["weight"])
    got = list(zip(cw["slot"], cw["from_robot"], cw["from_idx"], cw["to_robot"], cw["to_idx"], cw["kind"], cw["ghost_id"]))
    assert [tuple(int(x) for x in g) for g in got] == [e[:7] for e in exp]
    f = np.array([e[7] for e in exp], int)
    on = np.array([bool(kind) and bool((mask >> (e[5] - 1)) & 1) for e in exp], bool)
    if len(exp):
        we = np.where(on, w[f], 1.0)
        ew, es = np.abs(cw["weight"] / we - 1).max(), np.abs(cw["s2"] / s2[f] - 1).max()
        print(f"[joint-robust] {tag}: read-back of {len(exp)} rows, weight rel. error {ew:.3e}, s2 rel. error {es:.3e}")
        assert (cw["weight"][~on] == 1.0).all()
        assert ew <= 1e-12 and (es <= 1e-12 or not norms)
    ends = {}
    for g, a, b in zip(cw["ghost_id"], cw["weight"], cw["s2"]):
        if g >= 0:
            ends.setdefault(int(g), []).append((a, b))
    assert sorted(ends) == list(range(len(J.relmeas)))
    for g, lst in ends.items():
        assert len(lst) == 2 and lst[0] == lst[1], (g, lst)           # (both ends: the same bits)
    return cw


def check_passes(run, kind, param=0.0, mask=3, steps=2, vals=None, tag="", need_effect=True, norms=True):
    """`steps` passes, each against the reweighted joint step at the point it starts from (gn_reference.tolerance alone) and with
    the read-back of its weights.  -> (values, last w, last s2, per-pass (tolerance, |W dx|, min W))."""
    ref = run.ref
    sel = jr.selection(run.J, ref, mask)
    if vals is None:
        vals = run.values()
        assert np.array_equal(vals, ref.values)
    w = s2 = None
    rec = []
    for s in range(steps):
        dx, H, w, s2, floor = rc.robust_step(ref, vals, kind, param, sel)
        run.drv.one_pass()
        sync()
        new = run.values()
        tol, kappa = tolerance(H, dx, ref.magnitude(vals), floor)
        err = scaled_error(ref.tangent(vals, new), dx, H)
        print(f"[joint-robust] {tag} pass {s}: scaled_error {err:.3e} tolerance {tol:.3e} kappa {kappa:.3e}")
        assert np.linalg.norm(dx) > 1e-6
        assert err <= tol, (s, err, tol, kappa)
        if kind and need_effect and sel.any():
            # (the loss shows: the plain step at this point lies outside the bound, so a pass that ignored the loss would fail)
            assert scaled_error(ref.step(vals)[0], dx, H) > 10 * tol
        check_weights(run, w, s2, mask, kind, tag, norms)
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
    """2 robots of 14 poses, 3 inter-robot measurements, 2 in-robot closures per robot, all displaced: two passes."""
    r = Run(gpu, jr.kinds_case(), chart)
    try:
        set_loss(r, rc.KINDS[kind])
        check_passes(r, rc.KINDS[kind], tag=f"{kind} chart {chart}")
    finally:
        r.close()


# ---- 2: mixed gh_first, batch sizes -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["mixed_3", "mixed_1", "nothing_selected"])
def test_mixed_members(gpu, case):
    """mixed_3: robot 0 holds ghost factors (its pose first key and second key, pose 5 carrying two) and no closure, robot 2
    closures and no ghost factor, robot 1 both; mixed_1: one robot, closures only, a plain batched pass (no separator);
    nothing_selected: a member with neither."""
    J = {"mixed_3": lambda: jr.mixed_case(3), "mixed_1": lambda: jr.mixed_case(1), "nothing_selected": jr.nothing_selected_case}[case]()
    if case == "mixed_3":
        on0 = [(a == 0, b == 0) for (_, a, b, _, _) in J.relmeas]
        assert (True, False) in on0 and (False, True) in on0
        assert sum(1 for (ka, a, b, _, kb) in J.relmeas if (a, ka) == (0, 5) or (b, kb) == (0, 5)) == 2
        assert not any(q == 0 for q, *_ in J.closures) and any(q == 2 for q, *_ in J.closures)
        assert not any(2 in (a, b) for (_, a, b, _, _) in J.relmeas)
    if case == "nothing_selected":
        assert not any(q == 2 for q, *_ in J.closures) and not any(2 in (a, b) for (_, a, b, _, _) in J.relmeas)
    r = Run(gpu, J, 0)
    try:
        assert r.drv.arrow == (J.R > 1)
        set_loss(r, rc.HUBER)
        check_passes(r, rc.HUBER, tag=case)
    finally:
        r.close()


# ---- 3: block edges of the 128-thread launch --------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 127, 128, 129, 257])
def test_thread_count_edges(gpu, N):
    """Robot 0's n_between + n_ghost = N (joint_robust_cases.edge_case): closures up to the between / ghost boundary, ghost factors
    behind it, on the last thread of a block and the first of the next; robot 1 has 7 poses, so the shared grid overruns it.  Under
    Cauchy every reweighted factor shows in the step."""
    J = jr.edge_case(N)
    r = Run(gpu, J, 0)
    try:
        set_loss(r, rc.CAUCHY)
        _, w, _, _ = check_passes(r, rc.CAUCHY, tag=f"edges N {N}")
        cw = r.batch.closure_weights()
        n0 = int((cw["slot"] == 0).sum())
        n_clo0 = sum(q == 0 for q, *_ in J.closures)
        assert n0 == n_clo0 + (1 if N == 1 else 2) and J.sizes[0] - 1 + n0 == N
        assert (cw["weight"] < 0.5).all()
    finally:
        r.close()


# ---- 4: class mask ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", [1, 2])
def test_class_mask(gpu, mask):
    """Closures only leaves the ghost factors at their base sigmas (weight read back as 1), relative measurements only the
    closures: the step is the reference's in which only the selected class is reweighted."""
    r = Run(gpu, jr.kinds_case(), 0)
    try:
        set_loss(r, rc.CAUCHY, mask=mask)
        check_passes(r, rc.CAUCHY, mask=mask, tag=f"mask {mask}")
        cw = r.batch.closure_weights()
        on = cw["kind"] == (1 if mask == 1 else 2)
        assert on.any() and (~on).any()
        assert (cw["weight"][~on] == 1.0).all() and (cw["weight"][on] < 0.5).all() and (cw["s2"] > 0).all()
    finally:
        r.close()


# ---- 5: read-back -----------------------------------------------------------------------------------------------------------------

def test_read_back(gpu):
    """Refused before a pass; after one: rows, keys, order, w and s^2 at 1e-12 (check_weights), a smaller cap still reports the
    full count, and the driver's merged view has one row per inter-robot measurement with virtual robot indices."""
    J = jr.kinds_case()
    r = Run(gpu, J, 0)
    try:
        set_loss(r, rc.HUBER)
        with pytest.raises(gpu.SlideError, match="INVALID.*pass first"):
            r.batch.closure_weights()
        _, w, s2, _ = check_passes(r, rc.HUBER, steps=1, tag="read-back")
        cw = r.batch.closure_weights()
        assert cw["n"] == 2 * len(J.relmeas) + len(J.closures)
        part = r.batch.closure_weights(cap=3)
        assert part["n"] == cw["n"] and len(part["weight"]) == 3 and np.array_equal(part["weight"], cw["weight"][:3])
        assert np.array_equal(part["ghost_id"], cw["ghost_id"][:3])
        assert r.batch.closure_weights(cap=0)["n"] == cw["n"]
        m = r.drv.closure_weights()
        rel_f, clo_f = J.factor_rows(r.ref)
        assert [(int(a), int(ka), int(b), int(kb)) for a, ka, b, kb in zip(m["relmeas"]["from_robot"], m["relmeas"]["from_idx"],
                                                                          m["relmeas"]["to_robot"], m["relmeas"]["to_idx"])] \
            == [(a, ka, b, kb) for (ka, a, b, _, kb) in J.relmeas]
        assert np.abs(m["relmeas"]["weight"] / w[rel_f] - 1).max() <= 1e-12 and np.abs(m["relmeas"]["s2"] / s2[rel_f] - 1).max() <= 1e-12
        order = [c for q in range(J.R) for c, (rr, *_) in enumerate(J.closures) if rr == q]
        assert list(m["between"]["robot"]) == [J.closures[c][0] for c in order]
        assert np.abs(m["between"]["weight"] / w[clo_f[order]] - 1).max() <= 1e-12
        set_loss(r, rc.CAUCHY)                  # (a changed loss: nothing was linearised under it yet)
        with pytest.raises(gpu.SlideError, match="INVALID.*pass first"):
            r.batch.closure_weights()
    finally:
        r.close()


# ---- 6: off means off -------------------------------------------------------------------------------------------------------------

def test_off_means_off(gpu):
    """Two passes give the same poses bit for bit on a batch that never saw the call, with kind 0, with Huber at k = 1e12 (every
    weight exactly 1: sigma0 / sqrt(1) is sigma0), and after set then clear."""
    def run(prepare):
        r = Run(gpu, jr.kinds_case(), 0)
        try:
            prepare(r)
            r.drv.one_pass()
            r.drv.one_pass()
            sync()
            out = poses(r)
            cw = r.batch.closure_weights()
            return out, cw
        finally:
            r.close()

    base, cw0 = run(lambda r: None)
    assert (cw0["weight"] == 1.0).all() and (cw0["s2"] > 1.0).all()
    off, _ = run(lambda r: set_loss(r, 0))
    assert np.array_equal(base, off)
    huge, cwh = run(lambda r: set_loss(r, rc.HUBER, 1e12))
    assert (cwh["weight"] == 1.0).all() and np.abs(cwh["s2"] / cw0["s2"] - 1).max() <= 1e-12
    assert np.array_equal(base, huge)
    cleared, cwc = run(lambda r: (set_loss(r, rc.GEMAN_MCCLURE), set_loss(r, 0)))
    assert np.array_equal(base, cleared) and (cwc["weight"] == 1.0).all()
    # set, one reweighted pass, clear: the sigmas are back — two further passes are the plain joint steps at their points
    r = Run(gpu, jr.kinds_case(), 0)
    try:
        set_loss(r, rc.GEMAN_MCCLURE)
        vals, w, _, _ = check_passes(r, rc.GEMAN_MCCLURE, steps=1, tag="off: on")
        assert (w[jr.selection(r.J, r.ref)] < 1.0).all()
        set_loss(r, 0)
        check_passes(r, 0, steps=2, vals=vals, tag="off: cleared")
    finally:
        r.close()


# ---- 7: the cut pass --------------------------------------------------------------------------------------------------------------

def test_cut_pass_matches_the_whole_pass(gpu):
    """PassDriver.force_parts on one process ([20] 0 2): the poses and the weights of the whole pass, bit for bit."""
    out = []
    for parts in (False, True):
        r = Run(gpu, jr.kinds_case(), 0)
        try:
            r.drv.force_parts = parts
            set_loss(r, rc.CAUCHY)
            if parts:
                check_passes(r, rc.CAUCHY, tag="cut pass")
            else:
                r.drv.one_pass()
                r.drv.one_pass()
                sync()
            cw = r.batch.closure_weights()
            out.append((poses(r), cw["weight"], cw["s2"]))
        finally:
            r.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    assert (out[0][1] < 1.0).all()


# ---- 8: changing the loss between passes ------------------------------------------------------------------------------------------

def test_changing_the_loss_recaptures(gpu):
    """Huber, one pass; then Cauchy on the relative measurements only: the second pass is the reference's under the new loss."""
    r = Run(gpu, jr.kinds_case(), 0)
    try:
        set_loss(r, rc.HUBER)
        vals, _, _, _ = check_passes(r, rc.HUBER, steps=1, tag="change: huber")
        set_loss(r, rc.CAUCHY, mask=2)
        check_passes(r, rc.CAUCHY, mask=2, steps=1, vals=vals, tag="change: cauchy, relative only")
    finally:
        r.close()


# ---- 9: the planted scenario ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["geman_mcclure", "dcs"])
def test_planted_scenario(gpu, kind):
    """test_joint_robust_reference.py's scenario and step count: every pass within the reference step's bound at its own point, and
    at the end the CPU run of the numpy reference as the yardstick for poses and weights alike.
    Poses: step s admits an unscaled error of tolerance_s |W_s dx_s| / min(W_s); the final poses lie within the sum B_8 of the eight.
    Weights: they are those of the LAST linearisation, whose point lies within B_7 (the first seven passes) of the CPU run's.  A
    factor's residual e moves by at most L B_7 with L = 3 (1 + d): two poses, a rotation moving the relative translation by the
    poses' distance d, and 1.5 for the slope of the chart's log at residuals up to 1 rad (1 + tan^2(1/2) = 1.3 for Cayley).  So
    |d s| <= K = L B_7 / min(sigma), |d s^2| <= 2 s K + K^2, and since |d ln w / d s^2| <= 2 / (c^2 + s^2) for both losses (Phi for
    c^2; zero inside DCS's kink, continuous across it), |w_gpu / w_cpu - 1| <= expm1(2 |d s^2| / (c^2 + max(s^2 - |d s^2|, 0))),
    plus the 1e-12 of the read-back.  Asserted per factor."""
    k = rc.KINDS[kind]
    cpu = jr.planted_reference(k)
    J = cpu["J"]
    r = Run(gpu, J, 0)
    try:
        set_loss(r, k, jr.PLANTED_PARAM[k])
        vals, w, s2, rec = check_passes(r, k, jr.PLANTED_PARAM[k], steps=jr.PLANTED_STEPS, tag=f"planted {kind}", need_effect=False,
                                            norms=False)
        ref, sel = r.ref, cpu["sel"]
        cw = r.drv.closure_weights()
        got = np.concatenate([cw["relmeas"]["weight"], cw["between"]["weight"]])      # (the export's order: inter-robot, then closures, robot by robot)
        assert np.abs(got / w[sel] - 1).max() <= 1e-12          # (numpy at the GPU's own point; check_passes did it row by row)
        unscaled = [tol * nrm / wmin for tol, nrm, wmin in rec]
        b7, b8 = sum(unscaled[:-1]), sum(unscaled)
        pts, s2c = cpu["trace"][-1][0], cpu["trace"][-1][4][sel]
        c2 = jr.PLANTED_PARAM[k] ** 2 if k == rc.GEMAN_MCCLURE else jr.PLANTED_PARAM[k]
        allow = np.zeros(len(got))
        for j, f in enumerate(np.flatnonzero(sel)):
            d = np.linalg.norm(pts[int(ref.fv[f, 0]), 9:12] - pts[int(ref.fv[f, 1]), 9:12])
            K = 3.0 * (1.0 + d) * b7 / ref.fsig[f, :6].min()
            ds2 = 2.0 * np.sqrt(s2c[j]) * K + K * K
            allow[j] = 1e-12 + np.expm1(2.0 * ds2 / (c2 + max(s2c[j] - ds2, 0.0)))
        wdiff = np.abs(got / cpu["w"] - 1)
        diff = float(np.linalg.norm(ref.tangent(cpu["values"], vals)))
        err = jr.planted_truth_error(J, ref, vals)
        print(f"[joint-robust] planted {kind}: |gpu - cpu| {diff:.3e} bound {b8:.3e}, RMS pose error {err:.4e} m, "
              f"weights vs cpu run {wdiff.max():.3e}, largest weight difference / its bound {(wdiff / allow).max():.3e}")
        assert (wdiff <= allow).all(), (wdiff, allow)
        assert diff <= b8
        assert err <= jr.planted_truth_error(J, ref, cpu["values"]) + b8          # (an RMS of position differences is at most |gpu - cpu|)
    finally:
        r.close()


# ---- 10: refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals(gpu):
    """Loss with PCG in both orders, bad kind and mask, the driver without a batch or without exact joint passes."""
    from slide_slam_amd.distributed import PassDriver
    L = gpu.lib()
    batch = gpu.CholBatch(2)
    for kind in (-1, 5):
        with pytest.raises(gpu.SlideError, match="INVALID.*kind"):
            batch.set_robust_loss(kind)
    with pytest.raises(ValueError):
        batch.set_robust_loss("tukey")
    for m in (4, 7, -1):
        assert L.slide_chol_batch_set_robust_loss(C.c_void_p(batch.h), C.c_int(1), C.c_double(0.0), C.c_int(m)) == -1
        assert "class_mask" in gpu.api.last_error()
    batch.set_robust_loss("huber")
    with pytest.raises(gpu.SlideError, match="INVALID.*robust loss"):
        batch.set_pcg(5)
    batch.set_pcg(0)
    batch.set_robust_loss(None)
    batch.set_pcg(5)
    with pytest.raises(gpu.SlideError, match="INVALID.*PCG"):
        batch.set_robust_loss("huber")
    batch.set_pcg(0)
    batch.set_robust_loss("cauchy")
    with pytest.raises(gpu.SlideError, match="INVALID.*pass first"):
        batch.closure_weights()
    batch.set_robust_loss(None)
    # the driver: un-batched shards, and a batched PCG driver
    r = Run(gpu, jr.kinds_case(), 0, pcg_iters=3)
    try:
        with pytest.raises(ValueError, match="exact joint"):
            r.drv.set_robust_loss("huber")
        with pytest.raises(gpu.SlideError, match="INVALID.*PCG"):
            r.batch.set_robust_loss("huber")
        loose = PassDriver([], [], 0)
        with pytest.raises(ValueError, match="exact joint"):
            loose.set_robust_loss("huber")
    finally:
        r.close()
