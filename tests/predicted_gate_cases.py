"""The observation gate at a PREDICTED pose (slide_graph_predicted_observation_mahalanobis): the dense reference, the device's route in
numpy and the planted generator (test infrastructure for test_predicted_gate_host.py, test_gpu_predicted_gate.py and
test_gpu_backend_gate.py; not a test).

The quantity.  Pose k = (robot, from_idx) is in the graph with estimate X_k; X_n is the predicted pose and rel the odometry step whose
Between factor add_keypose_between(robot, from_idx, ., rel7, est7) would add, with sigmas odom x max(|t_rel|, 0.01).  The reference
takes that sentence literally: the AUGMENTED H
    [[H + P_k H_F^T H_F P_k^T,  P_k H_F^T H_T],  [H_T^T H_F P_k^T,  H_T^T H_T]]
is built from ObsCase.H (the full unreduced H of tests/gn_reference.py at the linearisation point) and the oracle's Between Jacobians
orc_linearize(F_BETWEEN, X_k, X_n, rel, sigmas) at the values in use, inverted densely, and a candidate — r, Ap, Al by the oracle's
orc_linearize at (X_n, the landmark's value), z and the sigmas by observation_gate_cases.add_rules — gives
    C_ref = I + A Sig_aug[sel, sel] A^T  over the NEW pose's and the landmark's coordinates,   d2_ref = r^T C_ref^-1 r.
pred_block_form restates the device's route in numpy: the closed form of the augmented marginal on top of schur_form's reduced
system, never forming the augmented H.

A candidate is the tuple SlideGraph.predicted_observation_mahalanobis takes: observation_mahalanobis's own, its robot and pose_idx
fields ignored (written here as the from pose's)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import closure_cases as cc
import closure_gate_cases as cg
import gn_graphs as gg
import observation_gate_cases as og
from oracle import pyoracle as po

NOISE_FLOOR = 0.01      # slide_params_t::noise_floor's default (graph.cpp:54-60)
QUANTILE = og.QUANTILE


def odom_sigma(c):
    """noise_model_odom_vec of the case's graphs (observation_gate_cases.GRAPHS; 0.1 by default)."""
    name = getattr(c, "name", None)
    okw = og.GRAPHS[name][1] if name in og.GRAPHS else {}
    return np.asarray(okw.get("odom_sigma", [0.1] * 6), float)


def between_sigmas(odom, rel7):
    """add_keypose_between's own rule: odom x max(|t_rel|, noise_floor)."""
    return np.asarray(odom, float) * max(float(np.linalg.norm(np.asarray(rel7, float)[:3])), NOISE_FLOOR)


def pose12_of(p7):
    R, t = cc._pose(p7, np.float64)
    return np.ascontiguousarray(np.concatenate([R.ravel(), t]))


def between_jacobians(chart, xk12, xn12, rel7, sg6):
    """H_F, H_T (6 x 6 each, whitened) of the Between factor from X_k to X_n measuring rel, by the oracle."""
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    xf, xt = np.ascontiguousarray(xk12, float), np.ascontiguousarray(xn12, float)
    z = pose12_of(rel7)
    s6 = np.ascontiguousarray(sg6, float)
    rr, J0, J1 = np.zeros(9), np.zeros(81), np.zeros(81)
    m = po.lib().orc_linearize(C.c_int(po.F_BETWEEN), P(xf), C.c_int(po.V_POSE), P(xt), P(z), P(s6), C.c_int(chart), C.c_double(1e-6), P(rr),
                               P(J0), P(J1), C.c_int(1))
    assert m == 6
    return J0[:36].reshape(6, 6).copy(), J1[:36].reshape(6, 6).copy()


def at_prediction(vals, est7):
    """vals with every pose replaced by the predicted one: where a candidate of the prediction is linearised."""
    x12 = pose12_of(est7)
    return og.Values(lambda r, i: x12, vals.lm)


def ref_gate(c, robot, from_idx, rel7, est7, cands, vals, odom=None):
    """Lists r, C_ref and the array d2_ref of the candidates at the predicted pose est7 behind pose (robot, from_idx), on the dense
    inverse of the augmented H.  c: an ObsCase (or what it holds: H, ref, chart and the sigmas add_rules reads)."""
    ref, N = c.ref, c.H.shape[0]
    sg6 = between_sigmas(odom_sigma(c) if odom is None else odom, rel7)
    HF, HT = between_jacobians(c.chart, vals.pose12(robot, from_idx), pose12_of(est7), rel7, sg6)
    vk = ref.pose_var(robot, from_idx)
    ks = np.arange(ref.off[vk], ref.off[vk + 1])
    Ha = np.zeros((N + 6, N + 6))
    Ha[:N, :N] = c.H
    Ha[np.ix_(ks, ks)] += HF.T @ HF
    Ha[np.ix_(ks, np.arange(N, N + 6))] = HF.T @ HT
    Ha[np.ix_(np.arange(N, N + 6), ks)] = HT.T @ HF
    Ha[N:, N:] = HT.T @ HT
    Sig = np.linalg.inv(Ha)
    pv = at_prediction(vals, est7)
    rs, Cs, d2 = [], [], np.zeros(len(cands))
    for i, cand in enumerate(cands):
        r, Ap, Al = og.linearize(c, cand, pv)
        A = np.hstack([Ap, Al])
        vl = ref.lm_var(og.KIND[cand[0]][2], cand[3])
        sel = np.concatenate([np.arange(N, N + 6), np.arange(ref.off[vl], ref.off[vl + 1])])
        Cm = np.eye(len(r)) + A @ Sig[np.ix_(sel, sel)] @ A.T
        rs.append(r); Cs.append(Cm)
        d2[i] = r @ np.linalg.solve(Cm, r)
    return rs, Cs, d2


def adjoint(T):
    """Ad(T) in [rot, trans] order: [[R, 0], [hat(t) R, R]]."""
    R, t = T
    hat = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ad = np.zeros((6, 6))
    Ad[:3, :3], Ad[3:, :3], Ad[3:, 3:] = R, hat @ R, R
    return Ad


def pred_block_form(c, robot, from_idx, rel7, est7, cand, vals, odom=None):
    """C by the route the device takes: schur_form's reduced pose system S and Schur records of the UNCHANGED graph, and
        C = I + Al H_ll^-1 Al^T + Ap diag(s^2) Ap^T + B^T S^-1 B,   B = P_k^T (Ap Ad)^T - sum_f P_{p_f}^T F_f Al^T,
    Ad = Ad(X_n^-1 X_k), s the Between's sigmas."""
    ref = c.ref
    og.schur_form(c, (cand[0], robot, from_idx) + tuple(cand[3:]), vals)      # (fills c._schur; its value is not used)
    J, row0, pcols, prow, H, S = c._schur
    s6 = between_sigmas(odom_sigma(c) if odom is None else odom, rel7)
    Xk, Xn = cg.pose_of(vals.pose12(robot, from_idx)), cc._pose(est7, np.float64)
    Ad = adjoint(cc._mul(cc._inv(Xn), Xk))
    r, Ap, Al = og.linearize(c, cand, at_prediction(vals, est7))
    m = len(r)
    vk, vl = ref.pose_var(robot, from_idx), ref.lm_var(og.KIND[cand[0]][2], cand[3])
    lc = np.arange(ref.off[vl], ref.off[vl + 1])
    Hinv = np.linalg.inv(H[np.ix_(lc, lc)])
    B = np.zeros((len(pcols), m))
    B[prow[vk]:prow[vk] + 6] += (Ap @ Ad).T
    for f in np.flatnonzero(ref.fv[:, 1] == vl):
        if int(ref.ftype[f]) not in (po.F_BR, po.F_CUBE, po.F_CYL):
            continue
        rows = np.arange(row0[f], row0[f + 1])
        q = int(ref.fv[f, 0])
        E = J[np.ix_(rows, np.arange(ref.off[q], ref.off[q + 1]))].T @ J[np.ix_(rows, lc)]
        B[prow[q]:prow[q] + 6] -= (E @ Hinv) @ Al.T
    return np.eye(m) + Al @ Hinv @ Al.T + Ap @ np.diag(s6 ** 2) @ Ap.T + B.T @ np.linalg.solve(S, B)


# ---- predictions and candidates ----------------------------------------------------------------------------------------------------
def predict(vals, robot, from_idx, step, xi=None):
    """(rel7, est7) of the prediction behind pose (robot, from_idx): rel = step x exp(xi), est = the values' pose o rel."""
    rel = step if xi is None else cc._mul(step, (cc._rotvec(np.asarray(xi, float)[:3]), np.asarray(xi, float)[3:]))
    est = cc._mul(cg.pose_of(vals.pose12(robot, from_idx)), rel)
    return cc.p7(rel), cc.p7(est)


STEP = (gg.rot([0.02, -0.03, 0.15]), np.array([0.9, 0.2, 0.05]))      # an odometry step for the graphs that have no next pose


def perturbed_list(c, vals, from_idx, est7, pairs, seed=3):
    """Candidates (kind, landmark) of `pairs` measured from the PREDICTED pose at the landmark's own value in vals, moved by a
    fixed-seed vector of 0.5, 2 or 6 x the factor's sigmas in turn (0.3 of them for points, whose sigma is 1 m by default)."""
    rng = np.random.default_rng(seed)
    X = cc._pose(est7, np.float64)
    out = []
    for n, (kind, l) in enumerate(pairs):
        m = og.KIND[kind][3]
        u = rng.normal(0, 1, m)
        u = (0.3 if kind == "point" else 1.0) * og.SCALES[n % 3] * u / np.linalg.norm(u) * np.sqrt(m)
        out.append(og.observe(c, kind, 0, from_idx, l, X, og.lm_value(kind, vals.lm(kind, l)), u))
    return out


# (graph -> (from poses: the first, a middle one, the newest; (kind, landmark) of the candidates).  chain40 / planted40: points every
# third pose, cylinders at even and cubes at odd multiples of three, landmark k seen from poses k .. k + 3; point 39 and cube 39 have
# ONE observer.  lc_*: landmark 0 of the class seen from all 12 poses, point 1 from poses 0 and 1.)
FROMS = {"chain40": (0, 20, 39), "planted40": (0, 20, 39), "lc_point": (0, 5, 11), "lc_cube": (0, 5, 11), "lc_cylinder": (0, 5, 11)}
LANDMARKS = {
    "chain40": [("point", 0), ("point", 18), ("point", 39), ("cylinder", 0), ("cylinder", 18), ("cylinder", 36), ("cube", 3), ("cube", 21),
                ("cube", 39)],
    "planted40": [("point", 0), ("point", 36), ("cylinder", 18), ("cylinder", 36), ("cube", 21), ("cube", 39)],
    "lc_point": [("point", 0), ("point", 1)], "lc_cube": [("cube", 0), ("point", 1)], "lc_cylinder": [("cylinder", 0), ("point", 1)],
}


PLANTED_SEED = 1


def planted(c, vals=None, seed=PLANTED_SEED):
    """planted40.  The predicted pose 40 = the estimate of pose 39 o (the TRUE last step x noise drawn at the odometry sigmas); the
    true pose 40 = the true pose 39 o that step.  For every landmark k in 27 .. 39 of each class a TRUE candidate — the ground
    truth's geometry of landmark k from the true pose 40, noise drawn at the factor's sigmas — and a FALSE one: the PREVIOUS landmark
    of the class measured the same way, tried against landmark k.  Asserted here, under d2_ref alone: every true one lies below 0.75
    of its class's 0.99 quantile, every false one above 1.5 of it.  -> (rel7, est7, candidates, truth flags, d2_ref, dof)."""
    assert c.name == "planted40"
    vals = vals or c.cpu_values
    rng = np.random.default_rng(seed)
    T = c.world.T
    step = cc._mul(cc._inv(T[38]), T[39])
    T40 = cc._mul(T[39], step)
    odom = odom_sigma(c)
    rel7, est7 = predict(vals, 0, 39, step, rng.normal(0, 1, 6) * between_sigmas(odom, cc.p7(step)))
    out, flags = [], []
    for kind in ("point", "cylinder", "cube"):
        m = og.KIND[kind][3]
        truth = c.world.truth[kind]
        ids = sorted(truth)
        for n, k in enumerate(ids):
            if not (27 <= k <= 39) or n == 0:
                continue
            out.append(og.observe(c, kind, 0, 39, k, T40, truth[k], rng.normal(0, 1, m)))
            flags.append(True)
            out.append(og.observe(c, kind, 0, 39, k, T40, truth[ids[n - 1]], rng.normal(0, 1, m)))
            flags.append(False)
    flags = np.array(flags)
    dof = np.array([og.KIND[x[0]][3] for x in out])
    q = np.array([QUANTILE[int(d)] for d in dof])
    _, _, d2 = ref_gate(c, 0, 39, rel7, est7, out, vals)
    assert (d2[flags] < 0.75 * q[flags]).all() and (d2[~flags] > 1.5 * q[~flags]).all(), (d2 / q, flags)
    return rel7, est7, out, flags, d2, dof
