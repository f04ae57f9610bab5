"""The joint-compatibility test of landmark observations on the JOINT multi-robot graph
(slide_chol_batch_observation_joint_compatibility): the stacked dense reference, the numpy restatement of the device's route and the
group generators (test infrastructure for test_batch_joint_compat_host.py and test_gpu_batch_joint_compat.py; not a test).

The reference side is joint_observation_gate_cases' (JointObsCase, sel, linearize, at_estimate, with_slot) stacked as
joint_compat_cases stacks the single graph's: with Sigma the dense inverse of the joint H and r_i, A_i = [Ap_i | Al_i] of the group's
candidates in the caller's order,
    C_ref = I + A Sig[u, u] A^T  over the union u of the candidates' coordinates,
and the rule is joint_compat_cases.ref_rule itself.  A candidate is CholBatch.observation_mahalanobis's tuple (an optional trailing
lm_slot).  A SHARED landmark may be named twice in a group — it is one variable of the reference whichever replica names it, and the
two candidates' columns of A overlap there; a PRIVATE one may not (the device's route has no cross term through H_ll^-1).
Everything here runs without a device."""
from __future__ import annotations

import numpy as np

import joint_compat_cases as jc
import joint_graphs as jg
import joint_observation_gate_cases as jo
from oracle import pyoracle as po

MARGIN = jc.MARGIN
KIND = jo.KIND


def rows_of(cands):
    return [KIND[x[0]][3] for x in cands]


def stacked_ref(c, cands, vals):
    """r (n), C_ref (n x n) and the candidates' row offsets (len + 1) of the group stacked in the given order."""
    off = np.concatenate([[0], np.cumsum(rows_of(cands))]).astype(int)
    n = int(off[-1])
    r, A = np.zeros(n), np.zeros((n, c.Sig.shape[0]))
    for i, cand in enumerate(cands):
        ri, Ap, Al = jo.linearize(c, cand, vals)
        r[off[i]:off[i + 1]] = ri
        A[off[i]:off[i + 1], c.sel(cand)] = np.hstack([Ap, Al])
    used = np.flatnonzero(np.abs(A).sum(axis=0) > 0)
    Au = A[:, used]
    return r, np.eye(n) + Au @ c.Sig[np.ix_(used, used)] @ Au.T, off


def ref_group(c, cands, vals, prob):
    """stacked_ref + joint_compat_cases.ref_rule; a decision (prob > 0) must stand MARGIN from every quantile it is compared with."""
    r, C, off = stacked_ref(c, cands, vals)
    out = jc.ref_rule(r, C, off, prob)
    out.update(r=r, C=C, off=off)
    if prob > 0:
        assert out["margin"] >= MARGIN, out["margin"]
    return out


# ---- the device's route, in numpy ---------------------------------------------------------------------------------------------------
def pieces(c, cand, vals):
    """(B, G0) of one candidate on joint_observation_gate_cases.joint_system's K, as block_form builds them.  Private landmark:
    G0 = Al H_ll^-1 Al^T, B = P_p^T Ap^T - sum_{f in factors(l)} P_{p_f}^T F_f Al^T.  Shared landmark (a row block of K): G0 = 0,
    B = P_p^T Ap^T + P_l^T Al^T."""
    Y = jo.joint_system(c)
    ref = c.ref
    base, ls = jo.split(cand)
    r, Ap, Al = jo.linearize(c, cand, vals)
    m = len(r)
    vp, vl = ref.pose_var(base[1], base[2]), c.lm_var(ls, base[0], base[3])
    B = np.zeros((Y["nk"], m))
    B[Y["krow"][vp]:Y["krow"][vp] + 6] += Ap.T
    G0 = np.zeros((m, m))
    if vl in Y["krow"]:
        B[Y["krow"][vl]:Y["krow"][vl] + m] += Al.T
    else:
        lc = np.arange(ref.off[vl], ref.off[vl + 1])
        Hinv = np.linalg.inv(Y["H0"][np.ix_(lc, lc)])
        G0 = Al @ Hinv @ Al.T
        for f in np.flatnonzero(ref.fv[:, 1] == vl):
            if int(ref.ftype[f]) not in (po.F_BR, po.F_CUBE, po.F_CYL):
                continue
            rows = np.arange(Y["row0"][f], Y["row0"][f + 1])
            q = int(ref.fv[f, 0])
            E = Y["J"][np.ix_(rows, np.arange(ref.off[q], ref.off[q + 1]))].T @ Y["J"][np.ix_(rows, lc)]
            B[Y["krow"][q]:Y["krow"][q] + 6] -= (E @ Hinv) @ Al.T
    return B, G0


def block_route(c, cands, vals, lambda_sign=-1.0):
    """The stacked C by the route the device takes: block (i, j) = [i == j] (I + G0_i) + W_i^T D W_j with L W = B on K = L D L^T, the
    candidates' columns of B side by side.  B is zero on the lambda rows; W there is L22^-1 (0 - L21 W1) and the gram counts those
    rows with lambda_sign (D = -I).  No private landmark is named twice; a shared one may be."""
    Y = jo.joint_system(c)
    Bs, G0s = zip(*[pieces(c, cand, vals) for cand in cands])
    B = np.hstack(Bs)
    W1 = np.linalg.solve(Y["L11"], B)
    W2 = np.linalg.solve(Y["L22"], -Y["L21"] @ W1) if Y["n_lam"] else np.zeros((0, B.shape[1]))
    C = W1.T @ W1 + lambda_sign * (W2.T @ W2)
    o = 0
    for g in G0s:
        m = g.shape[0]
        C[o:o + m, o:o + m] += np.eye(m) + g
        o += m
    return C


# ---- landmarks and groups ---------------------------------------------------------------------------------------------------------
def landmarks(c, kinds=("point", "cylinder", "cube")):
    """(kind, global id, robots) of the case's landmarks, points first, in the Joint's order within a kind."""
    out = []
    for kind in kinds:
        cls = KIND[kind][2]
        out += [(kind, g, sorted({r for r, _ in obs})) for k, g, _, obs in c.J.lms if k == cls]
    return out


def name(c, lm, slot, via=None):
    """(kind, lm_slot, local id): the landmark as a pose of `slot` names it — through its own replica where it has one, else through
    the lowest robot that holds it; via: the replica to name it through."""
    kind, g, robots = lm
    ls = via if via is not None else (slot if slot in robots else robots[0])
    return kind, ls, jo.local_id(c, ls, KIND[kind][2], g)


def measured(c, vals, rows, seed, scale=1.0):
    """(slot, pose, landmark, via or None) rows measured at the values' own geometry moved by fixed-seed noise of `scale` sigmas (0.3
    of it for points, whose sigma is 1 m / 1 rad under the defaults)."""
    rng = np.random.default_rng(seed)
    out = []
    for slot, p, lm, via in rows:
        kind, ls, l = name(c, lm, slot, via)
        u = (0.3 if kind == "point" else 1.0) * scale * rng.normal(0, 1, KIND[kind][3])
        out.append(jo.at_estimate(c, vals, kind, slot, p, l, u, ls))
    return out


def renamed(c, cand, lm, via):
    """The candidate with its landmark named through the replica of `via`: the same measurement, another (lm_slot, local id)."""
    base, _ = jo.split(cand)
    _, ls, l = name(c, lm, base[1], via)
    return jo.with_slot(base[:3] + (l,) + base[4:], ls)


def is_cross(cand, c=None):
    return jo.split(cand)[1] != cand[1]


def eval_groups(c, vals, seed=100):
    """The evaluate-only groups, name -> candidates: two points and six landmarks from robot 0's last pose (own private, private of
    the other robot, shared), a mixed-class group and its permutation, a group whose candidates sit at poses of two robots, a
    cross-robot group (robot 0's pose against landmarks only robot 1 holds), and a group that names one shared point twice — from a
    pose of each robot through that robot's own replica — with the same group named through the swapped replicas."""
    J = c.J
    lms = landmarks(c)
    P0, P1 = J.sizes[0] - 1, J.sizes[1] - 1
    pts = [x for x in lms if x[0] == "point"]
    priv = lambda r, kind=None: [x for x in lms if x[2] == [r] and (kind is None or x[0] == kind)]      # noqa: E731
    shar = lambda kind=None: [x for x in lms if len(x[2]) > 1 and (kind is None or x[0] == kind)]        # noqa: E731
    six = (priv(0, "point")[:2] + priv(1, "point")[:2] + shar("point")[:2] + priv(0, "cylinder")[:1] + priv(1, "cube")[:1] + shar("cylinder")[:1])[:6]
    assert len(six) == 6 and any(x[2] == [0] for x in six) and any(x[2] == [1] for x in six) and any(len(x[2]) > 1 for x in six)
    mixed = [(0, P0, priv(0, "point")[0], None), (0, P0 - 1, (priv(0, "cylinder") + shar("cylinder"))[0], None), (0, P0, shar("point")[0], None),
             (0, P0, (priv(1, "cube") + priv(0, "cube") + shar("cube"))[0], None), (0, P0 - 1, priv(1, "point")[0], None)]
    perm = [4, 2, 0, 3, 1]
    sp = shar("point")[0]
    a, b = sp[2][:2]
    twice = [(a, J.sizes[a] - 1, sp, a), (a, J.sizes[a] - 1, priv(a, "point")[0], None), (b, J.sizes[b] - 2, sp, b),
             (b, J.sizes[b] - 2, (priv(b, "cylinder") + priv(b, "cube"))[0], None)]
    g = {
        "2 points at one pose": measured(c, vals, [(0, P0, x, None) for x in pts[:2]], seed),
        "6 at one pose": measured(c, vals, [(0, P0, x, None) for x in six], seed + 1),
        "mixed": measured(c, vals, mixed, seed + 2),
        "two robots": measured(c, vals, [(0, P0, priv(0, "point")[0], None), (1, P1 - 1, priv(1, "point")[0], None), (0, P0, shar("point")[0], None),
                                         (1, P1 - 1, shar()[-1], None)], seed + 3),
        "cross-robot": measured(c, vals, [(0, P0 - (i % 2), x, None) for i, x in enumerate(priv(1)[:4])], seed + 4),
        "shared twice": measured(c, vals, twice, seed + 5),
    }
    g["mixed, permuted"] = [g["mixed"][k] for k in perm]
    t = g["shared twice"]
    g["shared twice, swapped"] = [renamed(c, t[0], sp, b), t[1], renamed(c, t[2], sp, a), t[3]]
    assert all(is_cross(x) for x in g["cross-robot"]) and len(g["cross-robot"]) >= 2
    assert jo.split(t[0])[1] != jo.split(t[2])[1] and c.sel(t[0])[6] == c.sel(t[2])[6]
    assert [jo.split(x)[1] for x in g["shared twice, swapped"]][::2] == [b, a]
    return g


def all_from(c, vals, slot, pose, seed, scale=1.0, limit=None):
    """Every landmark of the job (the first `limit` of them: points, cylinders, cubes) from one pose: one frame's worth of matches
    onto the whole joint map."""
    return measured(c, vals, [(slot, pose, x, None) for x in landmarks(c)[:limit]], seed, scale)


def some_group(c, vals, seed=200):
    """For a Joint of any make: from robot 0's last pose up to two private landmarks of each robot and up to two shared ones."""
    lms = landmarks(c)
    rows = [x for x in lms if x[2] == [0]][:2] + [x for x in lms if x[2] == [1]][:2] + [x for x in lms if len(x[2]) > 1][:2]
    assert len(rows) >= 3 and len({len(x[2]) > 1 for x in rows}) == 2
    return measured(c, vals, [(0, c.J.sizes[0] - 1, x, None) for x in rows], seed)


# ---- the planted hypotheses (PlantedJoint: two robots of 14 poses) ------------------------------------------------------------------
PLANTED_SLOT, PLANTED_POSE, PLANTED_SEED, PLANTED_S = 0, 13, 5, 2.5


def planted_targets(c):
    """Six points robot 0's last pose does not observe yet: its own two newest private points, the two newest private points of
    robot 1 (cross-robot) and a shared point of each robot's making (through robot 0's replica) — four of six cross-robot or shared."""
    lms = landmarks(c, ("point",))
    own = [x for x in lms if x[2] == [0]][-2:]
    other = [x for x in lms if x[2] == [1]][-2:]
    sh = [x for x in lms if len(x[2]) > 1]
    out = [own[0], other[0], sh[1], own[1], other[1], sh[-1]]
    assert len({x[1] for x in out}) == 6
    assert not any((PLANTED_SLOT, PLANTED_POSE) in c.J.observers(2, x[1]) for x in out)
    return out


def _planted(c, lm, u):
    kind, ls, l = name(c, lm, PLANTED_SLOT)
    T = c.J.T(PLANTED_SLOT, PLANTED_POSE)
    return jo.with_slot(jo.og.observe(c, kind, PLANTED_SLOT, PLANTED_POSE, l, T, c.J.truth[2, lm[1]], u), ls)


def planted_true(c):
    """The targets measured at the ground truth's geometry with unit noise drawn from default_rng(PLANTED_SEED): true as a whole."""
    rng = np.random.default_rng(PLANTED_SEED)
    return [_planted(c, lm, rng.normal(0, 1, 3)) for lm in planted_targets(c)]


def planted_moved(c, vals, s=PLANTED_S):
    """joint_compat_cases.planted_moved's construction: the same six at the ground truth's geometry with the range moved by
    +/- s sqrt(C_ii[2][2]) sigmas, signs alternating, C_ii the individual innovation covariance of planted_true's candidate at vals."""
    _, _, Cs, _ = jo.ref_gate(c, planted_true(c), vals)
    return [_planted(c, lm, np.array([0.0, 0.0, (1 if i % 2 == 0 else -1) * s * np.sqrt(Cs[i][2, 2])])) for i, lm in enumerate(planted_targets(c))]


# ---- two robots with many point landmarks (the LDS boundary and the capacity need 129 distinct ones) ---------------------------------
MANY_POINTS = 134


def many_points_joint(seed=23):
    """joint_compat_cases.many_points_graph's two-robot sibling: two robots of 12 poses, a cylinder seen from every pose of robot 0
    and 134 points, point l near pose (l // 2) % 11 of robot l % 2 and seen from that pose and the next; every 16th also from a
    pose of the other robot (shared)."""
    J = jg.Joint([12, 12], seed=seed)
    rng = np.random.default_rng(seed)
    J.cylinder(jg._near(J, 0, 5, rng), [0.05, -0.02, 1.0], 0.3, [(0, k) for k in range(12)])
    for l in range(MANY_POINTS):
        r, p = l % 2, (l // 2) % 11
        obs = [(r, p), (r, p + 1)] + ([(1 - r, p)] if l % 16 == 0 else [])
        J.point(jg._near(J, r, p, rng), obs)
    return J


def many_group(c, vals, n, seed, cyl=False, scale=1.0):
    """n distinct points (the first n, private and shared), point i from pose i % 12 of robot (i // 3) % 2 — about half of them
    cross-robot — and, with cyl, the cylinder from pose 5 of robot 1 behind them."""
    pts = landmarks(c, ("point",))
    rows = [((i // 3) % 2, i % 12, pts[i], None) for i in range(n)]
    if cyl:
        rows.append((1, 5, landmarks(c, ("cylinder",))[0], None))
    return measured(c, vals, rows, seed, scale)
