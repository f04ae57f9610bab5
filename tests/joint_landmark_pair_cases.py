"""The duplicate-landmark queries on the JOINT multi-robot graph (slide_chol_batch_landmark_pair_mahalanobis /
_get_landmark_pair_covariances / _landmark_pairs_within): the dense reference, the numpy restatement of the device's route and the
planted generator (test infrastructure for test_joint_landmark_pair_host.py and test_gpu_joint_landmark_pairs.py; not a test).

The reference is landmark_pair_cases' on the joint graph of joint_observation_gate_cases.JointObsCase: Sigma the dense inverse of the
joint Gauss-Newton H at the values before the pass (test_gpu_joint_marginals.dense_inverse, with its `tol`); for a pair of one class
    Sig_d = Sig_aa + Sig_bb - Sig_ab - Sig_ba,   r = (value_b - value_a) / sigma in the class's tangent order,
    C_ref = I + diag(1 / sigma) Sig_d diag(1 / sigma),   d2_ref = r^T C_ref^-1 r.
A pair is a row (slot_a, idx_a, slot_b, idx_b): idx the landmark's LOCAL index in the graph of its slot (Joint.local_ids maps it to
the reference's global id), so a shared landmark named through either replica resolves to the same variable.  Everything here runs
without a device."""
from __future__ import annotations

import numpy as np

import joint_graphs as jg
import joint_observation_gate_cases as jo
import landmark_pair_cases as lp
import observation_gate_cases as og
from oracle import pyoracle as po

SIGMA, CLS, DIM = lp.SIGMA, lp.CLS, lp.DIM
QUANTILE = og.QUANTILE
BR_SIGMA = 0.02
DUP_OKW = dict(jo.PLANTED_OKW, bearing_sigma=BR_SIGMA)                # the oracle's parameters
DUP_KW = dict(jo.PLANTED_KW, bearing_range_sigma=BR_SIGMA)            # the product's
DUP_SEED = 23


def sel(c, kind, row):
    sa, ia, sb, ib = (int(x) for x in row)
    off = c.ref.off
    va, vb = c.lm_var(sa, kind, ia), c.lm_var(sb, kind, ib)
    return np.concatenate([np.arange(off[va], off[va + 1]), np.arange(off[vb], off[vb + 1])])


def ref_joint_cov(c, kind, row):
    """[[Saa, Sab], [Sba, Sbb]] off the dense inverse of the joint H."""
    s = sel(c, kind, row)
    return c.Sig[np.ix_(s, s)]


def ref_pairs(c, kind, rows, vals, sigma=None):
    """Lists r, C_ref and the array d2_ref of the pairs of one class at vals (a JointValues)."""
    sg = SIGMA[kind] if sigma is None else np.asarray(sigma, float)
    D = DIM[kind]
    rs, Cs, d2 = [], [], np.zeros(len(rows))
    for k, row in enumerate(rows):
        sa, ia, sb, ib = (int(x) for x in row)
        S = ref_joint_cov(c, kind, row)
        Sd = S[:D, :D] + S[D:, D:] - S[:D, D:] - S[D:, :D]
        r = (lp.tangent(kind, vals.lm(sb, kind, ib)) - lp.tangent(kind, vals.lm(sa, kind, ia))) / sg
        Cm = np.eye(D) + Sd / np.outer(sg, sg)
        rs.append(r); Cs.append(Cm)
        d2[k] = r @ np.linalg.solve(Cm, r)
    return rs, Cs, d2


def is_shared(c, slot, kind, idx):
    return len(c.robots_of(slot, kind, idx)) > 1


# ---- the device's route, in numpy ---------------------------------------------------------------------------------------------------
def pair_block_form(c, kind, row, sigma=None, lambda_sign=-1.0, cov=False):
    """What the device forms, on joint_observation_gate_cases.joint_system's K = L D L^T: the hypothesis has Al = -I / sigma on a and
    +I / sigma on b and no pose block.  A PRIVATE side: G0 += Al H_ll^-1 Al^T and B -= P_{p_f}^T F_f Al^T over its factors, F_f =
    E_f H_ll^-1; a SHARED side (a row block of K): B += P_l^T Al^T, nothing in G0.  W = L^-1 B, the lambda rows counted with
    lambda_sign (D = -I).  cov = False: C = I + G0 + W^T D W (D x D).  cov = True: Al the unit columns of a's and then b's
    coordinates, and G0 + W^T D W is the pair's joint marginal (2 D x 2 D)."""
    Y = jo.joint_system(c)
    ref = c.ref
    D = DIM[kind]
    sg = SIGMA[kind] if sigma is None else np.asarray(sigma, float)
    sa, ia, sb, ib = (int(x) for x in row)
    m = 2 * D if cov else D
    B, G0 = np.zeros((Y["nk"], m)), np.zeros((m, m))
    for side, (s, i) in enumerate(((sa, ia), (sb, ib))):
        if cov:
            Al = np.zeros((m, D))
            Al[D * side:D * side + D] = np.eye(D)
        else:
            Al = (1.0 if side else -1.0) * np.diag(1.0 / sg)
        vl = c.lm_var(s, kind, i)
        if vl in Y["krow"]:
            B[Y["krow"][vl]:Y["krow"][vl] + D] += Al.T
            continue
        lc = np.arange(ref.off[vl], ref.off[vl + 1])
        Hinv = np.linalg.inv(Y["H0"][np.ix_(lc, lc)])
        G0 += Al @ Hinv @ Al.T
        for f in np.flatnonzero(ref.fv[:, 1] == vl):
            if int(ref.ftype[f]) not in (po.F_BR, po.F_CUBE, po.F_CYL):
                continue
            rows = np.arange(Y["row0"][f], Y["row0"][f + 1])
            q = int(ref.fv[f, 0])
            E = Y["J"][np.ix_(rows, np.arange(ref.off[q], ref.off[q + 1]))].T @ Y["J"][np.ix_(rows, lc)]
            B[Y["krow"][q]:Y["krow"][q] + 6] -= (E @ Hinv) @ Al.T
    W1 = np.linalg.solve(Y["L11"], B)
    W2 = np.linalg.solve(Y["L22"], -Y["L21"] @ W1) if Y["n_lam"] else np.zeros((0, m))
    return (0.0 if cov else np.eye(m)) + G0 + W1.T @ W1 + lambda_sign * (W2.T @ W2)


def side_pairs(c, kind):
    """{note: row} of the four side combinations a case holds of one class: private-private in one graph, private-private across
    graphs, private-shared, shared-shared (two DIFFERENT shared landmarks, the second named through its higher replica)."""
    J = c.J
    cls = CLS[kind]
    priv, shar = {}, []
    for k, g, _, obs in J.lms:
        if k != cls:
            continue
        robots = sorted({r for r, _ in obs})
        if len(robots) == 1:
            priv.setdefault(robots[0], []).append(jo.local_id(c, robots[0], cls, g))
        else:
            shar.append((g, robots))
    out = {}
    one = next((r for r in sorted(priv) if len(priv[r]) > 1), None)
    if one is not None:
        out["private-private, one graph"] = (one, priv[one][0], one, priv[one][-1])
    if len(priv) > 1:
        a, b = sorted(priv)[:2]
        out["private-private, across"] = (a, priv[a][0], b, priv[b][0])
    if priv and shar:
        a = sorted(priv)[-1]
        g, robots = shar[0]
        out["private-shared"] = (a, priv[a][-1], robots[0], jo.local_id(c, robots[0], cls, g))
    if len(shar) > 1:
        (g0, r0), (g1, r1) = shar[0], shar[-1]
        out["shared-shared"] = (r0[0], jo.local_id(c, r0[0], cls, g0), r1[-1], jo.local_id(c, r1[-1], cls, g1))
    return out


def other_replica(c, kind, slot, idx):
    """The same shared landmark named through another robot's replica."""
    cls = CLS[kind]
    g = int(c.gid[slot][cls][idx])
    o = next(r for r in c.robots_of(slot, kind, idx) if r != slot)
    return o, jo.local_id(c, o, cls, g)


# ---- the planted job ----------------------------------------------------------------------------------------------------------------
class DupJoint(jo.PlantedJoint):
    """PlantedJoint's two robots of 14 poses with, for k = 0, 3, 6, 9 and a centre near pose k of robot 0: point a seen by robot 0
    from poses k, k + 1; point b AT THE SAME PLACE seen by robot 1 from k, k + 1, k + 2 (a cross-robot duplicate); point e at the same
    place seen by robot 0 from k + 2, k + 3 (a same-robot duplicate); point d 1.0 m aside (+y) seen by robot 1 from k, k + 1, k + 2 (a
    distinct object); where k % 6 == 0 the same four as cylinders around a centre of their own, d offset +x by 1.0 m; two inter-robot
    relative-pose factors (0, 2) -> (1, 3) and (1, 9) -> (0, 8), so the job has lambda rows; and one private re-mapping of
    PlantedJoint's first shared point: the same truth seen again by its first robot from REMAP_POSES (a private-shared true pair).
    dups[kind]: (robot a, global id a, robot b, global id b, True: one object, cross: the two ends are not private landmarks of one
    robot)."""
    REMAP_POSES = (3, 4)

    def __init__(self, seed=DUP_SEED):
        super().__init__(seed=seed)
        rng = np.random.default_rng(seed + 7)
        self.dups = {"point": [], "cylinder": []}
        for k in (0, 3, 6, 9):
            for kind in ("point", "cylinder") if k % 6 == 0 else ("point",):
                centre = jg._near(self, 0, k, rng)
                aside = centre + (np.array([0.0, 1.0, 0.0]) if kind == "point" else np.array([1.0, 0.0, 0.0]))
                views = dict(a=[(0, k), (0, k + 1)], b=[(1, k), (1, k + 1), (1, k + 2)], e=[(0, k + 2), (0, k + 3)],
                             d=[(1, k), (1, k + 1), (1, k + 2)])
                g = {}
                for name, obs in views.items():
                    at = aside if name == "d" else centre
                    if kind == "point":
                        g[name] = self.point(at, obs)
                        self.truth[2, g[name]] = at
                    else:
                        g[name] = self.cylinder(at, og.RAY, 0.25, obs)
                        self.truth[0, g[name]] = (at, og.RAY, 0.25)
                rob = dict(a=0, b=1, e=0, d=1)
                for x, y, flag in (("a", "b", True), ("a", "e", True), ("e", "b", True), ("a", "d", False), ("b", "d", False), ("e", "d", False)):
                    self.dups[kind].append((rob[x], g[x], rob[y], g[y], flag, rob[x] != rob[y]))
        self.relative(0, 2, 1, 3)
        self.relative(1, 9, 0, 8)
        gs, obs = next((g, obs) for cls, g, _, obs in self.lms if cls == 2 and len({r for r, _ in obs}) > 1)
        r = obs[0][0]
        assert not {(r, p) for p in self.REMAP_POSES} & set(obs)
        gm = self.point(self.truth[2, gs], [(r, p) for p in self.REMAP_POSES])
        self.truth[2, gm] = self.truth[2, gs]
        self.remap = (r, gm, r, gs)
        self.dups["point"].append((r, gm, r, gs, True, True))


def dup_case(chart, seed=DUP_SEED):
    return jo.JointObsCase(DupJoint(seed), chart, **DUP_OKW)


def planted(c, kind, vals=None):
    """DupJoint's pairs of one class -> (rows (n, 4), flags (True: one object), cross (n,), d2_ref).  Asserted here, under d2_ref
    alone — landmark_pair_cases.planted's condition: every true pair lies below 0.25 of the 0.99 quantile of its D, every distinct
    pair above 1.5 of it."""
    assert isinstance(c.J, DupJoint)
    vals = vals or c.cpu_values
    cls = CLS[kind]
    rows = np.array([(ra, jo.local_id(c, ra, cls, ga), rb, jo.local_id(c, rb, cls, gb)) for ra, ga, rb, gb, _, _ in c.J.dups[kind]], np.int64)
    flags = np.array([f for *_, f, _ in c.J.dups[kind]])
    cross = np.array([x for *_, x in c.J.dups[kind]])
    _, _, d2 = ref_pairs(c, kind, rows, vals)
    q = QUANTILE[DIM[kind]]
    assert (d2[flags] < 0.25 * q).all() and (d2[~flags] > 1.5 * q).all(), (kind, d2 / q, flags)
    return rows, flags, cross, d2


# ---- the search ---------------------------------------------------------------------------------------------------------------------
def job_landmarks(c, kind):
    """The job's landmarks of one class as the search lists them: (slot, local idx, group) in (slot, local idx) order, a shared
    landmark once, through its lowest replica; group = the slot of a private landmark, -1 - its variable for a shared one."""
    cls = CLS[kind]
    out = []
    for s in range(c.J.R):
        for i in range(len(c.gid[s][cls])):
            robots = c.robots_of(s, kind, i)
            if len(robots) > 1 and robots[0] != s:
                continue
            out.append((s, i, s if len(robots) == 1 else -1 - c.lm_var(s, kind, i)))
    return out


def anchor(kind, v):
    v = np.asarray(v, float)
    return v[9:12].copy() if kind == "cube" else v[:3].copy()


def brute_job_pairs(entries, xyz, radius, cross_only=False):
    """landmark_pair_cases.brute_pairs over the union's anchors; cross_only drops the pairs whose two groups are equal.  ->
    (slot_a, idx_a, slot_b, idx_b, dist), sorted by position."""
    i, j, dist = lp.brute_pairs(xyz, radius)
    e = np.array(entries, np.int64).reshape(-1, 3)
    if cross_only:
        keep = e[i, 2] != e[j, 2]
        i, j, dist = i[keep], j[keep], dist[keep]
    return e[i, 0], e[i, 1], e[j, 0], e[j, 1], dist
