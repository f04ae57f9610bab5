"""The builders and the numpy reference of the robust loss on the joint multi-robot graph (tests/joint_robust_cases.py), on the CPU,
before any GPU run: the shards hold exactly the joint graph's factors (in-robot loop closures included), the reweighted step with no
loss is Reference.step, every selected factor's whitened norm stays >= 1 where the GPU tests compare s^2 at 1e-12, and the planted
scenario separates false from true factors in the reference alone."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_robust_cases as jr                                                 # noqa: E402
import robust_cases as rc                                                       # noqa: E402
from gn_reference import Reference                                              # noqa: E402
from oracle import pyoracle as po                                               # noqa: E402
from test_joint_reference import joint_reference, oracle_setup, read_values, whitened_sq      # noqa: E402

EDGES = [1, 127, 128, 129, 257]
CASES = [("kinds", jr.kinds_case), ("mixed_3", lambda: jr.mixed_case(3)), ("mixed_1", lambda: jr.mixed_case(1)),
         ("nothing_selected", jr.nothing_selected_case)] + [(f"edge_{n}", (lambda n=n: jr.edge_case(n))) for n in EDGES]
SMALL = [c for c in CASES if c[0] not in ("edge_257",)]
PASSES = 2                      # passes per case of test_gpu_joint_robust_loss.py


@pytest.mark.parametrize("name,make", SMALL, ids=[c[0] for c in SMALL])
def test_shards_hold_the_joint_graph(name, make):
    """Counts per factor type and the whitened residuals: the shards' sum plus the inter-robot factors (held by both robots as
    ghosts, counted once from the joint graph) is the joint graph's — the closures went into both targets with the same numbers."""
    J = make()
    ref, _ = joint_reference(J, 0)
    srefs = []
    shards, gid, info, _ = oracle_setup(J, 0, lambda shs: srefs.extend(Reference(sh.graph, 0) for sh in shs))
    assert np.array_equal(read_values(shards, gid, ref, J.sizes), ref.values)
    total, counts = 0.0, np.zeros(5, int)
    for r, (sh, sref) in enumerate(zip(shards, srefs)):
        svals = sref.values.copy()
        for cls in range(3):
            for loc in range(len(gid[r][cls])):
                v = sh.graph.get_landmark(cls, loc)[1]
                svals[sref.lm_var(cls, loc), : len(v)] = v
        total += whitened_sq(sref, svals)
        counts += np.bincount(sref.ftype, minlength=5)
    rel_f, clo_f = J.factor_rows(ref)
    assert len(rel_f) == len(J.relmeas) and len(clo_f) == len(J.closures)
    for f, (ka, a, b, _, kb) in zip(rel_f, J.relmeas):
        assert (int(ref.fv[f, 0]), int(ref.fv[f, 1])) == (ref.pose_var(a, ka), ref.pose_var(b, kb))
    for f, (r, i, k, _) in zip(clo_f, J.closures):
        assert (int(ref.fv[f, 0]), int(ref.fv[f, 1])) == (ref.pose_var(r, i), ref.pose_var(r, k))
    counts[po.F_BETWEEN] += len(rel_f)
    assert np.array_equal(counts, np.bincount(ref.ftype, minlength=5))
    rel_sq = whitened_sq(ref, factors=np.asarray(rel_f, int)) if len(rel_f) else 0.0
    full = whitened_sq(ref)
    assert np.isclose(total + rel_sq, full, rtol=1e-12, atol=0), (total + rel_sq, full)
    sel = jr.selection(J, ref)
    assert sel.sum() == len(rel_f) + len(clo_f) and sel[rel_f].all() and sel[clo_f].all()
    assert jr.selection(J, ref, 1).sum() == len(clo_f) and jr.selection(J, ref, 2).sum() == len(rel_f)


def test_edge_cases_reach_their_thread_counts():
    """Robot 0's between + ghost factors number N, with selected factors where edge_case's docstring puts them."""
    for N in EDGES:
        J = jr.edge_case(N)
        n_gh = sum((a == 0) + (b == 0) for (_, a, b, _, _) in J.relmeas)
        n_clo = sum(r == 0 for r, *_ in J.closures)
        n_bt = J.sizes[0] - 1 + n_clo
        assert n_bt + n_gh == N, (N, n_bt, n_gh)
        if N > 1:
            assert n_gh == 2 and n_clo >= 1             # (the last between factor is a closure: selected on both sides of the boundary)
            firsts = [a == 0 for (_, a, b, _, _) in J.relmeas]
            assert True in firsts and False in firsts
        if N == 257:
            assert J.sizes[0] - 1 <= 127                # (threads 127 and 128 are closures)
        assert J.sizes[1] == 7


def test_no_loss_is_the_plain_step():
    J = jr.kinds_case()
    ref, _ = joint_reference(J, 0)
    dx0, H0 = ref.step(ref.values)
    dx, H, w, _, _ = rc.robust_step(ref, ref.values, 0, 0.0, jr.selection(J, ref))
    assert np.array_equal(dx, dx0) and np.array_equal(H, H0) and (w == 1.0).all()


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_selected_norms_stay_above_one(name, make):
    """At every point the GPU tests linearise at under mask 3 (PASSES reweighted steps of the reference under each loss the GPU
    tests set on the case, with its default parameter; `kinds`: all four on both charts, `mixed_3`: all four, the others Huber and
    Cauchy), every selected factor has s >= 1: s^2 carries no cancellation, and 1e-12 on the read-back holds."""
    J = make()
    charts = (0, 1) if name == "kinds" else (0,)
    kinds = sorted(rc.KINDS.values()) if name in ("kinds", "mixed_3") else [rc.HUBER, rc.CAUCHY]
    for chart in charts:
        ref, _ = joint_reference(J, chart)
        sel = jr.selection(J, ref)
        for kind in kinds:
            trace, _ = jr.steps(J, ref, kind, 0.0, 3, PASSES)
            for _, dx, _, w, s2, _ in trace:
                assert np.sqrt(s2[sel]).min() >= 1.0, (name, chart, kind, np.sqrt(s2[sel]).min())
                assert (w[sel] < 1.0).any() and np.linalg.norm(dx) > 1e-6


# (loss, parameter, mask) per pass of the GPU tests on kinds_case that do not keep one loss under mask 3
SEQUENCES = {
    "class_mask_1": [(rc.CAUCHY, 0.0, 1)] * 2,
    "class_mask_2": [(rc.CAUCHY, 0.0, 2)] * 2,
    "changing_the_loss": [(rc.HUBER, 0.0, 3), (rc.CAUCHY, 0.0, 2)],
    "off_after_a_reweighted_pass": [(rc.GEMAN_MCCLURE, 0.0, 3), (0, 0.0, 3), (0, 0.0, 3)],
    "off": [(0, 0.0, 3)] * 2,
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_listed_norms_stay_above_one_along_the_other_sequences(name):
    """The read-back lists EVERY closure and inter-robot factor, selected or not (the unselected with s^2 = |r|^2), and the GPU
    tests compare each s^2 at 1e-12: along the passes of test_class_mask, test_changing_the_loss_recaptures and
    test_off_means_off every listed factor keeps s >= 1 at every point linearised at."""
    J = jr.kinds_case()
    ref, _ = joint_reference(J, 0)
    listed = jr.selection(J, ref)
    vals = ref.values
    for kind, param, mask in SEQUENCES[name]:
        trace, vals = jr.steps(J, ref, kind, param, mask, 1, vals)
        s = np.sqrt(trace[0][4][listed])
        assert s.min() >= 1.0, (name, kind, mask, s.min())


@pytest.mark.parametrize("kind", ["geman_mcclure", "dcs"])
def test_planted_scenario(kind):
    """3 robots of 20 poses, four true inter-robot measurements, two false ones, a true and a false in-robot closure
    (joint_robust_cases.planted_case, which says how c = 1.5 and Phi = c^2 = 2.25 were chosen); 8 steps of the numpy reference
    reach, on the selected factors and on every robot's poses against the ground truth:

        loss            true weights (min)   false weights (max)   RMS pose error   loss-free RMS pose error
        geman_mcclure   0.6850               1.407e-02             5.975e-02 m      1.248 m
        dcs             1.0000               5.887e-02             6.567e-02 m      1.248 m

    The GPU test compares the final weights at 1e-12.  A weight's relative error is 2 |delta s^2| / (c^2 + s^2) (both losses, Phi
    for c^2; DCS inside its kink: none) with |delta s^2| = 2 s |delta s| and |delta s| about 1e-15 |t| / sigma for poses of
    magnitude |t| ~ 10 m: 1e-14 for the inter-robot factors (sigma ~ 0.5) whatever s is, and 1e-11 for the closures (sigma 1e-3),
    for which 4 s / (c^2 + s^2) <= 0.01 is asserted below — the true closure ends far inside the kernel, the false one far outside.
    So the true factors need no s >= 1 here.  Under DCS no factor may sit at the kink s^2 = Phi."""
    k = rc.KINDS[kind]
    P = jr.planted_reference(k)
    J, ref, sel = P["J"], P["ref"], P["sel"]
    false = jr.planted_false_mask(J)
    assert len(false) == sel.sum() == 8
    w = P["w"]
    err = jr.planted_truth_error(J, ref, P["values"])
    plain = jr.planted_truth_error(J, ref, P["plain"])
    print(f"[joint-robust] planted {kind}: true weights min {w[~false].min():.4f}, false weights max {w[false].max():.3e}, "
          f"RMS pose error {err:.4e} m, loss-free {plain:.4e} m")
    assert w[~false].min() > 0.5 and w[false].max() < 0.1, w
    assert err < 0.1 * plain, (err, plain)
    c2 = jr.PLANTED_PARAM[k] ** 2 if k == rc.GEMAN_MCCLURE else jr.PLANTED_PARAM[k]
    s2 = P["trace"][-1][4][sel]
    clo = s2[len(J.relmeas):]
    assert (4.0 * np.sqrt(clo) / (c2 + clo)).max() <= 0.01
    if k == rc.DCS:
        assert (np.abs(s2 / c2 - 1.0) > 1e-3).all()
