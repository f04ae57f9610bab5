"""The joint-compatibility test of landmark observations (slide_graph_observation_joint_compatibility): the dense reference, the
selection rule in numpy and the case generators (test infrastructure for test_joint_compat_host.py and test_gpu_joint_compat.py; not
a test).

The reference extends observation_gate_cases' own.  With Sigma the dense inverse of the full, unreduced H and r_i, A_i = [Ap_i | Al_i]
of the group's candidates from the oracle's orc_linearize, stacked in the caller's order,
    C_ref = I + A Sig[u, u] A^T  over the union u of the candidates' coordinates, cross blocks included,   d2_ref = r^T C_ref^-1 r.
The rule (ref_rule) is the call's: the candidates in the caller's order, S the accepted set; candidate i with m_i rows is accepted iff
d2_single = r_i^T C_ii^-1 r_i <= q(m_i) and d2_joint = the stacked d2 of S + {i} <= q(|S| + m_i), q = scipy.stats.chi2.ppf(prob, .);
prob = 0 accepts everything.  schur_route restates the device's route (B_i^T S^-1 B_j off the diagonal, I + G0_i + B_i^T S^-1 B_i on
it) and is checked against C_ref in test_joint_compat_host.py.  Everything here runs without a device."""
from __future__ import annotations

import numpy as np
from scipy.stats import chi2

import gn_graphs as gg
import observation_gate_cases as og
from oracle import pyoracle as po

MARGIN = 1e-3          # every comparison a decision test relies on stands at least this far (relative) from its quantile


def rows_of(cands):
    return [og.KIND[x[0]][3] for x in cands]


def stacked_ref(c, cands, vals):
    """r (n), C_ref (n x n) and the candidates' row offsets (len + 1) of the group stacked in the given order."""
    ms = rows_of(cands)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(int)
    n = int(off[-1])
    r, A = np.zeros(n), np.zeros((n, c.Sig.shape[0]))
    for i, cand in enumerate(cands):
        ri, Ap, Al = og.linearize(c, cand, vals)
        r[off[i]:off[i + 1]] = ri
        A[off[i]:off[i + 1], c.sel(cand[0], cand[1], cand[2], cand[3])] = np.hstack([Ap, Al])
    used = np.flatnonzero(np.abs(A).sum(axis=0) > 0)
    Au = A[:, used]
    return r, np.eye(n) + Au @ c.Sig[np.ix_(used, used)] @ Au.T, off


def _cond(C):
    w = np.linalg.eigvalsh(C)
    return float(w[-1] / w[0])


def ref_rule(r, C, off, prob):
    """The call's rule on the stacked reference.  -> dict: accepted, d2_single, d2_joint, dof_joint (per candidate), group_d2,
    group_dof, group_count, cond_single / cond_joint (the condition number of the matrix each figure was solved with) and margin, the
    smallest relative distance of any comparison from its quantile (inf when prob == 0)."""
    k = len(off) - 1
    out = dict(accepted=np.zeros(k, bool), d2_single=np.zeros(k), d2_joint=np.zeros(k), dof_joint=np.zeros(k, int),
               cond_single=np.zeros(k), cond_joint=np.zeros(k))
    S = np.zeros(0, int)
    margin = np.inf
    d2S = 0.0
    for i in range(k):
        rows = np.arange(off[i], off[i + 1])
        Cii = C[np.ix_(rows, rows)]
        d1 = float(r[rows] @ np.linalg.solve(Cii, r[rows]))
        idx = np.concatenate([S, rows])
        Cs = C[np.ix_(idx, idx)]
        dj = float(r[idx] @ np.linalg.solve(Cs, r[idx]))
        out["d2_single"][i], out["d2_joint"][i], out["dof_joint"][i] = d1, dj, len(idx)
        out["cond_single"][i], out["cond_joint"][i] = _cond(Cii), _cond(Cs)
        ok = True
        if prob > 0:
            q1, qj = float(chi2.ppf(prob, len(rows))), float(chi2.ppf(prob, len(idx)))
            margin = min(margin, abs(d1 / q1 - 1), abs(dj / qj - 1))
            ok = d1 <= q1 and dj <= qj
        out["accepted"][i] = ok
        if ok:
            S, d2S = idx, dj
    out.update(group_d2=d2S, group_dof=len(S), group_count=int(out["accepted"].sum()), margin=margin)
    return out


def ref_group(c, cands, vals, prob):
    """stacked_ref + ref_rule; a decision (prob > 0) must stand MARGIN from every quantile it is compared with."""
    r, C, off = stacked_ref(c, cands, vals)
    out = ref_rule(r, C, off, prob)
    out.update(r=r, C=C, off=off)
    if prob > 0:
        assert out["margin"] >= MARGIN, out["margin"]
    return out


def schur_route(c, cands, vals):
    """The stacked C by the route the device takes, in numpy (observation_gate_cases.schur_form's pieces): B_i = P_p^T Ap_i^T -
    sum_f P_{p_f}^T F_f Al_i^T, block (i, j) = B_i^T S^-1 B_j for i != j and I + Al_i H_ll^-1 Al_i^T + B_i^T S^-1 B_i on the diagonal.
    The landmarks of the group are distinct."""
    og.schur_form(c, cands[0], vals)          # (the graph's own part, cached on the case)
    J, row0, pcols, prow, H, S = c._schur
    ref = c.ref
    Bs, G0 = [], []
    for cand in cands:
        _, Ap, Al = og.linearize(c, cand, vals)
        m = Ap.shape[0]
        vp, vl = ref.pose_var(cand[1], cand[2]), ref.lm_var(og.KIND[cand[0]][2], cand[3])
        lc = np.arange(ref.off[vl], ref.off[vl + 1])
        Hinv = np.linalg.inv(H[np.ix_(lc, lc)])
        B = np.zeros((len(pcols), m))
        B[prow[vp]:prow[vp] + 6] += Ap.T
        for f in np.flatnonzero(ref.fv[:, 1] == vl):
            if int(ref.ftype[f]) not in (po.F_BR, po.F_CUBE, po.F_CYL):
                continue
            rows = np.arange(row0[f], row0[f + 1])
            q = int(ref.fv[f, 0])
            E = J[np.ix_(rows, np.arange(ref.off[q], ref.off[q + 1]))].T @ J[np.ix_(rows, lc)]
            B[prow[q]:prow[q] + 6] -= (E @ Hinv) @ Al.T
        Bs.append(B)
        G0.append(Al @ Hinv @ Al.T)
    Ball = np.hstack(Bs)
    C = Ball.T @ np.linalg.solve(S, Ball)
    o = 0
    for g in G0:
        m = g.shape[0]
        C[o:o + m, o:o + m] += np.eye(m) + g
        o += m
    return C


# ---- generators -------------------------------------------------------------------------------------------------------------------
def noisy_group(c, vals, triples, seed, scale=1.0):
    """(kind, pose, landmark) triples measured at the values' own geometry moved by fixed-seed noise of `scale` sigmas (0.3 of it for
    points, whose sigma is 1 m / 1 rad under the defaults: the range stays positive)."""
    rng = np.random.default_rng(seed)
    return [og.at_estimate(c, vals, kind, 0, p, l, (0.3 if kind == "point" else 1.0) * scale * rng.normal(0, 1, og.KIND[kind][3]))
            for kind, p, l in triples]


PLANTED_POSE, PLANTED_POINTS, PLANTED_SEED = 39, (18, 21, 24, 27, 30, 33), 5


def planted_true(c):
    """planted40: six point candidates from pose 39 to the points 18 .. 33 (pose 39 observes none of them yet), the ground truth's
    geometry with unit noise drawn from default_rng(5): a hypothesis that is true as a whole."""
    assert c.name == "planted40"
    rng = np.random.default_rng(PLANTED_SEED)
    T = c.world.T
    return [og.observe(c, "point", 0, PLANTED_POSE, k, T[PLANTED_POSE], c.world.truth["point"][k], rng.normal(0, 1, 3)) for k in PLANTED_POINTS]


def planted_moved(c, vals, s, only=None):
    """The same six at the ground truth's geometry with the range moved by +/- s sqrt(C_ii[2][2]) sigmas, signs alternating (C_ii the
    individual innovation covariance of planted_true's candidate at vals): each passes alone for s = 2.5, the set cannot be explained
    by one pose error.  only: the candidates that are moved (the others keep planted_true's noise)."""
    true = planted_true(c)
    _, _, Cs, _ = og.ref_gate(c, true, vals)
    T = c.world.T
    out = []
    for i, k in enumerate(PLANTED_POINTS):
        if only is not None and i not in only:
            out.append(true[i])
            continue
        u = np.array([0.0, 0.0, (1 if i % 2 == 0 else -1) * s * np.sqrt(Cs[i][2, 2])])
        out.append(og.observe(c, "point", 0, PLANTED_POSE, k, T[PLANTED_POSE], c.world.truth["point"][k], u))
    return out


# ---- a graph with many point landmarks (the LDS boundary and the capacity need 129 distinct ones) ------------------------------------
MANY_POINTS = 133          # point landmarks 1 .. 133 (landmark_count_graph's own point 1 and 132 more); cylinder 0 is seen from every pose


def many_points_graph(g):
    """gn_graphs.landmark_count_graph(cylinder, 12 poses) with 132 more point landmarks, each seen from two neighbouring poses."""
    W = gg.landmark_count_graph(g, 0, 12)
    rng = np.random.default_rng(77)
    for l in range(2, MANY_POINTS + 1):
        p = l % 11
        W.point(l, gg.around(W, p, rng), [p, p + 1])
    return W


og.GRAPHS.setdefault("lc_many_points", (many_points_graph, {}, {}))
