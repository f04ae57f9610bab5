"""The builders and the numpy reference of the observation loss on the joint multi-robot graph (tests/joint_observation_loss_cases.py)
on the CPU, before any GPU run: the shards hold the joint graph's factors and the batch's factor order maps onto the export's one
to one; no loss gives the plain joint step; under every loss and mask the GPU tests set, at every point they linearise at, every
landmark keeps an observation of weight W_KEPT and every observation moved by TIGHT sigmas or more stands at s >= 1; the longest
sequence of passes is well posed; the
planted scenario's figures; and the new entry points exist (the one test here that needs the feature)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_graphs as jg                                                      # noqa: E402
import joint_observation_loss_cases as jo                                      # noqa: E402
import joint_robust_cases as jr                                                # noqa: E402
import observation_loss_cases as oc                                            # noqa: E402
import robust_cases as rc                                                      # noqa: E402
from gn_reference import Reference, scaled_error, tolerance                    # noqa: E402
from oracle import pyoracle as po                                              # noqa: E402

KINDS = sorted(rc.KINDS.values())
_REF = {}


def case(name, chart=0):
    """(J, ref) of a named case, built once."""
    if (name, chart) not in _REF:
        J = {"kinds": jo.kinds_case, "both": jo.both_case, "r1": lambda: jo.members_case(1), "r3": lambda: jo.members_case(3)}.get(name)
        J = J() if J is not None else jo.edge_case(*name)
        _REF[(name, chart)] = (J, jo.reference(J, chart))
    return _REF[(name, chart)]


def lf_types(ref):
    return ref.ftype[oc.lf_index(ref)]


# ---- the builders -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["kinds", "both", "r1", "r3", (1, 1), (257, 9)], ids=str)
def test_shards_hold_the_joint_graphs_factors(name):
    """Per robot the shard's landmark factors are the joint graph's of that robot: the same count, classes and measurements in
    the order batch_rows lists, and batch_to_export is a bijection onto the export's landmark factors."""
    J, ref = case(name)
    shards, _ = jg.build(J, lambda: po.OracleGraph(oc.params(0)[0]))
    rows = jo.batch_rows(J)
    f = jo.batch_to_export(J, ref)
    assert sorted(f.tolist()) == oc.lf_index(ref).tolist()                     # (a bijection)
    at = 0
    for r, sh in enumerate(shards):
        sref = Reference(sh.graph, 0)
        lf = oc.lf_index(sref)
        mine = [q for q in rows if q[0] == r]
        assert len(mine) == len(lf)
        assert [(p, c, l) for (_, p, c, l) in oc.factor_keys(sref)] == [(p, c, l) for (_, p, c, l, _) in mine]
        fj = f[at:at + len(lf)]
        assert np.array_equal(sref.ftype[lf], ref.ftype[fj]) and np.array_equal(sref.fz[lf], ref.fz[fj])
        assert np.array_equal(sref.fsig[lf], ref.fsig[fj])
        at += len(lf)
    assert at == len(f)


def test_kinds_case_is_what_it_says():
    J, ref = case("kinds")
    assert J.R == 2 and J.sizes == [12, 12]
    lf = oc.lf_index(ref)
    assert {int(t) for t in lf_types(ref)} == {po.F_BR, po.F_CUBE, po.F_CYL}
    shared = jo.shared_landmarks(J)
    assert {c for c, _ in shared} == {0, 1, 2} and len(shared) < len(J.lms)
    mv = jo.moved_factors(J, ref)
    assert {int(t) for t in ref.ftype[mv]} == {po.F_BR, po.F_CUBE, po.F_CYL}
    s = np.sqrt(rc.whitened_norms2(ref))
    print("[joint-obs-loss] kinds case: whitened norms of the moved observations", np.round(s[mv], 2))
    assert (s[mv] < 1.345).any() and ((s[mv] > 1.345) & (s[mv] < 5)).any() and (s[mv] > 30).any()      # (on both sides of the kinks, and gross)
    # a down-weighted observation of a shared landmark in each robot (Huber: w < 1)
    w = rc.weight(rc.HUBER, 0.0, s)
    keys = oc.factor_keys(ref)
    pos = {int(f): i for i, f in enumerate(lf)}
    for r in range(2):
        assert any(w[f] < 0.5 and keys[pos[int(f)]][0] == r and (keys[pos[int(f)]][2], keys[pos[int(f)]][3]) in shared for f in mv)


@pytest.mark.parametrize("n_br,n_nbr", jo.EDGES)
def test_edge_case_counts(n_br, n_nbr):
    J, ref = case((n_br, n_nbr))
    rows = jo.batch_rows(J)
    t0 = [c for (r, _, c, _, _) in rows if r == 0]
    assert t0.count(2) == n_br and len(t0) - t0.count(2) == n_nbr
    t1 = [c for (r, _, c, _, _) in rows if r == 1]
    assert len(t1) == 3 and set(t1) == {2}                                     # (no cube or cylinder: n_nbr = 0)
    assert not any(r == 2 for (r, *_) in rows)                                 # (no landmark factor at all)
    assert ref.n <= 1000
    br = [i for i, c in enumerate(t0) if c == 2]
    mv = set(jo.moved_factors(J, ref).tolist())
    f = jo.batch_to_export(J, ref)
    for q in {0, n_br - 1} | {q for b in (256, 512) for q in (b - 1, b) if q < n_br}:
        assert int(f[br[q]]) in mv, q


# ---- no loss: the plain joint step -------------------------------------------------------------------------------------------------

def test_no_loss_is_the_plain_joint_step():
    J, ref = case("kinds")
    dx, H, w, s2, _ = oc.obs_step(ref, ref.values, 0, 0.0, oc.selected(ref))
    dx0, H0 = ref.step(ref.values)
    assert np.array_equal(dx, dx0) and np.array_equal(H, H0) and (w == 1.0).all()
    dxh = oc.obs_step(ref, ref.values, rc.HUBER, 1e12, oc.selected(ref))[0]
    assert np.array_equal(dxh, dx0)


# ---- the condition of every GPU test: an inlier on every landmark, moved observations at s >= 1 ---------------------------------------

CHANGE = [(rc.HUBER, 0.0, 7, None, 2), (rc.CAUCHY, 0.0, 5, None, 2)]      # the longest sequence on one Run: four passes


def sequences():
    """(tag, case name, chart, [(kind, param, mask, closure loss or None, steps)]) of every sequence of passes the GPU tests run."""
    out = []
    for chart in (0, 1):
        for kind in KINDS:
            out.append((f"kinds {kind} chart {chart}", "kinds", chart, [(kind, 0.0, 7, None, 2)]))
    for e in jo.EDGES:
        for bit in range(3):
            out.append((f"edges {e} bit {bit}", e, 0, [(rc.CAUCHY, 0.0, 1 << bit, None, 1)]))
    out.append(("r1", "r1", 0, [(rc.HUBER, 0.0, 7, None, 2)]))
    out.append(("r3", "r3", 0, [(rc.HUBER, 0.0, 7, None, 2)]))
    out.append(("cut", "kinds", 0, [(rc.CAUCHY, 0.0, 7, None, 2)]))
    out.append(("change", "kinds", 0, CHANGE))
    out.append(("off", "kinds", 0, [(rc.GEMAN_MCCLURE, 0.0, 7, None, 1), (0, 0.0, 7, None, 2)]))
    out.append(("both", "both", 0, [(rc.HUBER, 0.0, 7, rc.CAUCHY, 2)]))
    out.append(("marginal", "kinds", 0, [(rc.GEMAN_MCCLURE, 0.0, 7, None, 1)]))
    return out


@pytest.mark.parametrize("seq", sequences(), ids=lambda q: q[0])
def test_every_landmark_keeps_an_inlier(seq):
    """Condition, not measurement: along every sequence, at every linearisation point, every landmark - a shared one over all its
    observers - keeps an observation of weight >= W_KEPT, and every observation moved by jo.TIGHT sigmas or more has s >= 1 (its s^2 is then no difference of
    nearly equal numbers).  Runs on the CPU, before anything runs on a GPU."""
    _, name, chart, parts = seq
    J, ref = case(name, chart)
    mv = jo.moved_factors(J, ref, jo.TIGHT)
    vals = ref.values
    for kind, param, mask, clo, n in parts:
        closure = (clo, 0.0, jr.selection(J, ref)) if clo else None
        trace, vals = jo.steps(ref, kind, param, oc.selected(ref, mask), n, vals, closure)
        for (_, dx, _, w, s2, _) in trace:
            assert np.linalg.norm(dx) > 1e-6
            wl = np.where(oc.selected(ref), w, 1.0)
            assert oc.landmarks_keep_an_inlier(ref, wl), seq[0]
            if len(mv):
                assert (s2[mv] >= 1.0).all(), (seq[0], np.sqrt(s2[mv]).min())


@pytest.mark.parametrize("chart", [0, 1])
def test_longest_sequence_is_well_posed(chart):
    """The passes of the longest sequence (three and more on one Run: CHANGE): under a one-ulp change of the linearisation point the
    numpy step itself moves by less than a quarter of gn_reference.tolerance (the GPU linearises at a point that differs from its
    read-back by as much) - the guard of test_observation_loss_reference.py, for the same reason."""
    J, ref = case("kinds", chart)
    rng = np.random.default_rng(5)
    vals = ref.values
    for kind, param, mask, _, n in CHANGE:
        sel = oc.selected(ref, mask)
        for s in range(n):
            dx, H, _, _, floor = oc.obs_step(ref, vals, kind, param, sel)
            tol, _ = tolerance(H, dx, ref.magnitude(vals), floor)
            for _ in range(3):
                dx2 = oc.obs_step(ref, vals * (1 + rng.uniform(-1, 1, vals.shape) * 1.1e-16), kind, param, sel)[0]
                assert scaled_error(dx2, dx, H) <= 0.25 * tol, (kind, s, tol)
            vals = ref.retract(vals, dx)


def test_the_loss_shows_in_the_step():
    """The GPU tests' teeth: the plain joint step lies more than 10 tolerances from the reweighted one at both points of the kinds case."""
    J, ref = case("kinds")
    for kind in KINDS:
        vals = ref.values
        for _ in range(2):
            dx, H, _, _, floor = oc.obs_step(ref, vals, kind, 0.0, oc.selected(ref))
            tol, _ = tolerance(H, dx, ref.magnitude(vals), floor)
            assert scaled_error(ref.step(vals)[0], dx, H) > 10 * tol
            vals = ref.retract(vals, dx)
    for e in jo.EDGES:          # (the edges' bearing-range bit under Cauchy as well)
        J, ref = case(e)
        dx, H, _, _, floor = oc.obs_step(ref, ref.values, rc.CAUCHY, 0.0, oc.selected(ref, 1))
        tol, _ = tolerance(H, dx, ref.magnitude(ref.values), floor)
        assert scaled_error(ref.step(ref.values)[0], dx, H) > 10 * tol


# ---- the planted scenario -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [rc.GEMAN_MCCLURE, rc.DCS])
def test_planted_false_matches(kind):
    """Nine observations that measure the neighbouring shared landmark (three per robot): figures of the numpy run, printed and
    asserted with the margins that run shows (DESIGN section 7 records them)."""
    cpu = jo.planted_reference(kind)
    J, ref, bad = cpu["J"], cpu["ref"], cpu["bad"]
    lf = oc.lf_index(ref)
    good = np.setdiff1d(lf, bad)
    assert len(bad) == 3 * jo.PLANTED_FALSE and J.R == 3
    shared = set(jo.shared_landmarks(J))
    assert all((c, g) in shared for c, g, _ in J.false)
    err = jr.planted_truth_error(J, ref, cpu["values"])
    plain = jr.planted_truth_error(J, ref, cpu["plain"])
    w = cpu["w"]
    print(f"[joint-obs-loss] planted kind {kind}: RMS pose error {err:.4f} m (plain {plain:.4f} m, start "
          f"{jr.planted_truth_error(J, ref, ref.values):.4f} m), false observations' weights <= {w[bad].max():.3e}, the true ones' >= {w[good].min():.4f}")
    assert plain > PLANTED_PLAIN_MIN
    assert err <= PLANTED_ERR_MAX
    assert (w[bad] < PLANTED_W_FALSE_MAX).all() and (w[good] > PLANTED_W_TRUE_MIN).all()
    assert oc.landmarks_keep_an_inlier(ref, w)
    for (_, _, _, wq, _, _) in cpu["trace"]:
        assert oc.landmarks_keep_an_inlier(ref, wq)


# the numpy run shows (Geman-McClure c = 3 / DCS Phi = 9): plain 1.855 m; reweighted 0.0010 / 0.0041 m; the false observations' weights
# <= 1.6e-3 / 6.7e-3, the true ones' >= 0.9999 / 1.0.  Asserted with a factor of about three to spare.
PLANTED_PLAIN_MIN, PLANTED_ERR_MAX, PLANTED_W_FALSE_MAX, PLANTED_W_TRUE_MIN = 1.0, 0.015, 0.02, 0.99


# ---- the entry points ---------------------------------------------------------------------------------------------------------------

def test_exports_and_methods():
    """Fails without the feature; needs no GPU."""
    from slide_slam_amd import api
    from slide_slam_amd.distributed import PassDriver
    for name in ("slide_chol_batch_set_observation_loss", "slide_chol_batch_get_observation_weights"):
        assert name in api.EXPORTS
    for cls in (api.CholBatch, PassDriver):
        assert callable(getattr(cls, "set_observation_loss")) and callable(getattr(cls, "observation_weights"))
    loose = PassDriver([], [], 0)          # (the CPU rehearsal: no batch)
    with pytest.raises(ValueError, match="exact joint"):
        loose.set_observation_loss("huber")
    with pytest.raises(ValueError, match="exact joint"):
        loose.observation_weights()
