"""The individual-compatibility gate of landmark observations on the JOINT multi-robot graph
(slide_chol_batch_observation_mahalanobis): the dense reference, the numpy restatement of the device's route and the list generators
(test infrastructure for test_joint_observation_gate_host.py and test_gpu_joint_observation_gate.py; not a test).

The reference side is the single-graph gate's (tests/observation_gate_cases.py: add_rules, linearize, gate_bound, observe) on the joint
graph of tests/joint_graphs.py: Sigma the dense inverse of the joint Gauss-Newton H at the values before the pass
(test_gpu_joint_marginals.dense_inverse, with its Jacobi weights, `tol` and `kappa`), r / Ap / Al from the oracle's orc_linearize at
the pose and landmark values a caller passes in, C_ref = I + A Sigma[sel, sel] A^T and d2_ref in numpy.

A candidate is the tuple CholBatch.observation_mahalanobis takes: SlideGraph.observation_mahalanobis's with a SLOT where that names a
robot (robot r's graph sits in slot r and calls its own poses robot 0) and an optional trailing lm_slot, the slot whose graph holds the
landmark; lm_idx is the landmark's LOCAL index in that graph (Joint.local_ids maps it to the joint reference's global id).  Everything
here runs without a device: the estimate a generator needs on the CPU is the reference's own joint Gauss-Newton step."""
from __future__ import annotations

import numpy as np

import gn_graphs as gg
import joint_graphs as jg
import observation_gate_cases as og
from gn_reference import Reference
from oracle import pyoracle as po
from test_gpu_joint_marginals import dense_inverse

QUANTILE = og.QUANTILE
KIND = og.KIND
NARGS = {"point": 6, "cube": 7, "cylinder": 8}      # a candidate tuple's length without lm_slot
CLS_KIND = {0: "cylinder", 1: "cube", 2: "point"}


def split(cand):
    """(the candidate without its lm_slot, the landmark's slot)"""
    n = NARGS[cand[0]]
    return tuple(cand[:n]), int(cand[n]) if len(cand) > n else int(cand[1])


def reference(J, chart, **okw):
    og_ = po.OracleGraph(po.OrcParams.default(pose_chart=chart, **okw))
    J.emit_joint(og_)
    return Reference(og_, chart)


class JointValues:
    """Where a candidate is linearised: pose12(slot, idx) -> 12 doubles, lm(slot, kind, local idx) -> the landmark's value."""

    def __init__(self, pose12, lm):
        self.pose12, self.lm = pose12, lm

    def of(self, lm_slot):
        """The single-graph Values observation_gate_cases.linearize reads, for a candidate whose landmark sits in lm_slot."""
        return og.Values(self.pose12, lambda kind, idx: self.lm(lm_slot, kind, idx))


def shard_values(shards):
    """The device's estimates, shard by shard (every graph calls its own poses robot 0)."""
    def pose12(slot, idx):
        st, p = shards[slot].graph.get_pose12(0, idx)
        assert st == 0
        return p

    def lm(slot, kind, idx):
        st, v = shards[slot].graph.get_landmark(KIND[kind][2], idx)
        assert st == 0
        return v
    return JointValues(pose12, lm)


class JointObsCase:
    """One Joint under one chart: the joint reference; at() fixes the linearisation point (default: the reference's initial values,
    where the first pass linearises) and with it H, its inverse, the Jacobi weights, tol, kappa and the reference's own one-step
    estimate.  Has what observation_gate_cases.add_rules / linearize / gate_bound read of an ObsCase.  okw: the oracle parameters'
    keywords (the sigmas the add calls choose)."""

    def __init__(self, J, chart, ref=None, vals=None, params=None, **okw):
        P = params if params is not None else po.OrcParams.default(pose_chart=chart, **okw)
        self.J, self.chart = J, chart
        self.bearing_sigma, self.cyl_sigma, self.cube_vec = float(P.bearing_sigma), float(P.cyl_sigma), np.array(list(P.cube_sigma))
        self.ref = ref if ref is not None else reference(J, chart, **okw)
        self.gid = J.local_ids()
        self.at(self.ref.values if vals is None else vals)

    def at(self, vals, H=None, Sig=None, tol=None):
        """H / Sig / tol given: a system of the caller's own at vals (a reweighted one)."""
        self.vals = vals
        if Sig is None:
            self.Sig, self.w, self.tol, self.kappa = dense_inverse(self.ref, vals)
            self.scale = float(np.abs(self.Sig * np.outer(self.w, self.w)).max())
            dx, self.H = self.ref.step(vals)
            self.est = self.ref.retract(vals, dx)
        else:
            self.H, self.Sig, self.tol = H, Sig, tol
        self.__dict__.pop("_system", None)
        est, ref = getattr(self, "est", None), self.ref
        if est is not None:
            self.cpu_values = JointValues(lambda s, i: np.ascontiguousarray(est[ref.pose_var(s, i)][:12]),
                                          lambda s, kind, i: np.ascontiguousarray(est[self.lm_var(s, kind, i)]))
        return self

    def lm_var(self, slot, kind, idx):
        cls = KIND[kind][2]
        return self.ref.lm_var(cls, int(self.gid[slot][cls][idx]))

    def robots_of(self, slot, kind, idx):
        cls = KIND[kind][2]
        return sorted({r for r, _ in self.J.observers(cls, int(self.gid[slot][cls][idx]))})

    def sel(self, cand):
        base, ls = split(cand)
        vp, vl = self.ref.pose_var(base[1], base[2]), self.lm_var(ls, base[0], base[3])
        off = self.ref.off
        return np.concatenate([np.arange(off[vp], off[vp + 1]), np.arange(off[vl], off[vl + 1])])


def linearize(c, cand, vals):
    base, ls = split(cand)
    return og.linearize(c, base, vals.of(ls))


def ref_gate(c, cands, vals):
    """Lists r, A = [Ap | Al], C_ref and the array d2_ref of the candidates at vals."""
    rs, As, Cs, d2 = [], [], [], np.zeros(len(cands))
    for k, cand in enumerate(cands):
        r, Ap, Al = linearize(c, cand, vals)
        A = np.hstack([Ap, Al])
        sel = c.sel(cand)
        Cm = np.eye(len(r)) + A @ c.Sig[np.ix_(sel, sel)] @ A.T
        rs.append(r); As.append(A); Cs.append(Cm)
        d2[k] = r @ np.linalg.solve(Cm, r)
    return rs, As, Cs, d2


gate_bound = og.gate_bound


# ---- the device's route, in numpy ---------------------------------------------------------------------------------------------------
def joint_system(c):
    """What an exact joint pass factors, built from the reference's whitened Jacobian at c.vals: K = L D L^T over [the poses of every
    robot and the SHARED landmarks (observed by more than one robot: the separator, not eliminated) | six lambda rows per inter-robot
    relative-pose factor], with every PRIVATE landmark eliminated into its robot's poses and the inter-robot factors entering through
    their lambda rows only, K = [[S, Jlam^T], [Jlam, -I]]: D = +I on the first block and -I on the second."""
    if "_system" in c.__dict__:
        return c._system
    ref = c.ref
    i, j, v, res = ref.linearize(c.vals)
    Jm = np.zeros((len(res), ref.n))
    np.add.at(Jm, (i, j), v)
    row0 = np.concatenate([[0], np.cumsum([og.ROWS[int(t)] for t in ref.ftype])])
    nv = len(ref.vtype)
    robot_of = {ref.pose_var(r, k): r for r in range(c.J.R) for k in range(c.J.sizes[r])}
    lmf = np.isin(ref.ftype, (po.F_BR, po.F_CUBE, po.F_CYL))
    seen_by = {}
    for f in np.flatnonzero(lmf):
        seen_by.setdefault(int(ref.fv[f, 1]), set()).add(robot_of[int(ref.fv[f, 0])])
    lam_f = [f for f in range(len(ref.ftype)) if int(ref.ftype[f]) == po.F_BETWEEN and int(ref.fv[f, 1]) >= 0
             and robot_of[int(ref.fv[f, 0])] != robot_of[int(ref.fv[f, 1])]]
    lam_rows = np.concatenate([np.arange(row0[f], row0[f + 1]) for f in lam_f]) if lam_f else np.zeros(0, int)
    own = np.setdiff1d(np.arange(len(res)), lam_rows)
    H0 = Jm[own].T @ Jm[own]
    kvars = [k for k in range(nv) if int(ref.vtype[k]) == po.V_POSE or len(seen_by.get(k, ())) > 1]
    kcols = np.concatenate([np.arange(ref.off[k], ref.off[k + 1]) for k in kvars])
    krow, o = {}, 0
    for k in kvars:
        krow[k] = o
        o += int(ref.off[k + 1] - ref.off[k])
    S = H0[np.ix_(kcols, kcols)].copy()
    for k in range(nv):
        if k in krow:
            continue
        lc = np.arange(ref.off[k], ref.off[k + 1])
        Hkl = H0[np.ix_(kcols, lc)]
        S -= Hkl @ np.linalg.solve(H0[np.ix_(lc, lc)], Hkl.T)
    L11 = np.linalg.cholesky(S)
    Jlam = Jm[np.ix_(lam_rows, kcols)]
    assert not np.delete(Jm[lam_rows], kcols, axis=1).any()
    L21 = np.linalg.solve(L11, Jlam.T).T
    L22 = np.linalg.cholesky(np.eye(len(lam_rows)) + L21 @ L21.T)
    c._system = dict(J=Jm, row0=row0, H0=H0, krow=krow, nk=len(kcols), L11=L11, L21=L21, L22=L22, n_lam=len(lam_rows))
    return c._system


def block_form(c, cand, vals, lambda_sign=-1.0):
    """C by the route the device takes: C = I + G0 + W^T D W with L W = B on joint_system's K = L D L^T.
    Private landmark: G0 = Al H_ll^-1 Al^T, B = P_p^T Ap^T - sum_{f in factors(l)} P_{p_f}^T F_f Al^T, F_f = E_f H_ll^-1.
    Shared landmark (a row block of K): G0 = 0, B = P_p^T Ap^T + P_l^T Al^T.  B is zero on the lambda rows; W there is
    L22^-1 (0 - L21 W1), and the gram counts those rows with lambda_sign (D = -I)."""
    Y = joint_system(c)
    ref = c.ref
    base, ls = split(cand)
    r, Ap, Al = linearize(c, cand, vals)
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
    W1 = np.linalg.solve(Y["L11"], B)
    W2 = np.linalg.solve(Y["L22"], -Y["L21"] @ W1) if Y["n_lam"] else np.zeros((0, m))
    return np.eye(m) + G0 + W1.T @ W1 + lambda_sign * (W2.T @ W2)


# ---- candidates ---------------------------------------------------------------------------------------------------------------------
CUBE_MAX_ANGLE = 2.0      # rad: the largest rotational residual of a generated cube candidate (at_estimate)


def with_slot(cand, lm_slot):
    return cand if lm_slot is None or lm_slot == cand[1] else tuple(cand) + (int(lm_slot),)


def at_estimate(c, vals, kind, slot, pose_idx, lm_idx, u, lm_slot=None):
    """observation_gate_cases.observe at the values' own pose (slot, pose_idx) and landmark (lm_slot or slot, lm_idx): u = zeros gives
    a candidate whose residual is zero there."""
    ls = slot if lm_slot is None else lm_slot
    X = og.cg.pose_of(vals.pose12(slot, pose_idx))
    lm = og.lm_value(kind, vals.lm(ls, kind, lm_idx))
    if kind == "cube":
        # A cube's rotational sigma is 0.1 rad per metre of distance, so six sigmas reach past pi, where the factor's error (a
        # logarithm) has no derivative and the central differences of the device and of the oracle alike amplify their rounding by
        # 1 / (pi - angle): the rotation part is cut to CUBE_MAX_ANGLE, the rest of the displacement stays.
        u = np.array(u, float)
        ang = float(np.linalg.norm(u[:3] * og.cube_sigmas(c, X, (lm[0], lm[1]))[:3]))
        if ang > CUBE_MAX_ANGLE:
            u[:3] *= CUBE_MAX_ANGLE / ang
    return with_slot(og.observe(c, kind, slot, pose_idx, lm_idx, X, lm, u), lm_slot)


def local_id(c, r, cls, g):
    return int(np.flatnonzero(c.gid[r][cls] == g)[0])


def named_pairs(c):
    """(kind, slot, pose, lm_slot, local lm idx, note) of the list compared with the reference, per class the Joint holds: a private
    landmark with a pose that observes it, one that does not, its robot's first and last pose, a pose of ANOTHER robot (cross-robot
    onto a private landmark), the first of them again (a repeat); a shared landmark from a pose of its first robot, named through that
    robot's replica and through the second robot's (the two must agree bit for bit), and from a pose of the second robot named through
    the first's replica (cross-robot onto a shared landmark)."""
    J = c.J
    out = []
    for cls in (2, 0, 1):
        kind = CLS_KIND[cls]
        priv = [(g, obs) for k, g, _, obs in J.lms if k == cls and len({r for r, _ in obs}) == 1]
        shar = [(g, obs) for k, g, _, obs in J.lms if k == cls and len({r for r, _ in obs}) > 1]
        if priv:
            g, obs = priv[len(priv) // 2]
            r = obs[0][0]
            l = local_id(c, r, cls, g)
            seen = {k for _, k in obs}
            free = next(k for k in range(J.sizes[r] - 2, 0, -1) if k not in seen)
            o = (r + 1) % J.R
            out += [(kind, r, obs[0][1], r, l, "observer"), (kind, r, free, r, l, "not an observer"), (kind, r, 0, r, l, "first pose"),
                    (kind, r, J.sizes[r] - 1, r, l, "last pose"), (kind, o, min(obs[0][1] + 1, J.sizes[o] - 1), r, l, "cross-robot, private"),
                    (kind, r, obs[0][1], r, l, "repeat")]
        if shar:
            g, obs = shar[0]
            a, b = sorted({r for r, _ in obs})[:2]
            la, lb = local_id(c, a, cls, g), local_id(c, b, cls, g)
            pa = next(k for r, k in obs if r == a)
            pb = min(pa + 2, J.sizes[b] - 1)
            out += [(kind, a, pa, a, la, "shared, own replica"), (kind, a, pa, b, lb, "shared, other replica"),
                    (kind, b, pb, a, la, "cross-robot, shared"), (kind, b, pb, b, lb, "cross-robot, shared, own replica")]
    return out


SCALES = og.SCALES


def perturbed_list(c, vals, extra=(), seed=3):
    """named_pairs(c) + extra, each measured at the values' own geometry moved by a fixed-seed vector of 0.5, 2 or 6 x the factor's
    sigmas (0.3 of them for points: a point's sigma is 1 m / 1 rad under the defaults); a (pose, landmark variable) met again gets the
    same measurement, so a shared landmark's two names carry the same numbers."""
    rng = np.random.default_rng(seed)
    out, seen = [], {}
    for n, (kind, s, p, ls, l, _) in enumerate(list(named_pairs(c)) + list(extra)):
        key = (s, p, c.lm_var(ls, kind, l))
        m = KIND[kind][3]
        if key not in seen:
            u = rng.normal(0, 1, m)
            seen[key] = (0.3 if kind == "point" else 1.0) * SCALES[n % 3] * u / np.linalg.norm(u) * np.sqrt(m)
        out.append(at_estimate(c, vals, kind, s, p, l, seen[key], ls))
    return out


# ---- the planted list ---------------------------------------------------------------------------------------------------------------
PLANTED_BR_SIGMA, PLANTED_CYL_SIGMA = 0.05, 0.1
PLANTED_CUBE_VEC = [0.02] * 9          # (x the cube's distance, about 6 m: the default 0.1 is 0.6 rad / 0.6 m there, wider than the map's spacing)
PLANTED_OKW = dict(bearing_sigma=PLANTED_BR_SIGMA, cyl_sigma=PLANTED_CYL_SIGMA, cube_sigma=PLANTED_CUBE_VEC)                      # the oracle's parameters
PLANTED_KW = dict(bearing_range_sigma=PLANTED_BR_SIGMA, cylinder_sigma=PLANTED_CYL_SIGMA, noise_model_cube_vec=PLANTED_CUBE_VEC)    # the product's
PLANTED_SEED = 1


class PlantedJoint(jg.Joint):
    """Two robots of 14 poses side by side, initial values 0.002 rad / 0.01 m from the ground truth (planted40's noise), and the ground
    truth of every landmark kept in truth[(cls, global id)]: near every second pose of each robot a point and a cylinder or cube seen
    from three consecutive poses of that robot, every third of these landmarks also from two poses of the other robot (shared)."""

    def __init__(self, seed=21, P=14):
        super().__init__([P, P], seed=seed, spacing=3.0)
        rng = np.random.default_rng(seed)
        self.truth = {}
        n = 0
        for r in range(2):
            for k in range(0, P - 2, 2):
                for cls in (2, (n // 2) % 2):
                    obs = [(r, j) for j in range(k, k + 3)]
                    if n % 3 == 0:
                        obs += [(1 - r, k), (1 - r, k + 1)]
                    centre = jg._near(self, r, k, rng)
                    if cls == 2:
                        g = self.point(centre, obs)
                        self.truth[2, g] = centre
                    elif cls == 0:
                        g = self.cylinder(centre, og.RAY, 0.25, obs)
                        self.truth[0, g] = (centre, og.RAY, 0.25)
                    else:
                        Rc, sc = gg.rot([0.1, 0.2, rng.uniform(-3, 3)]), np.array([0.8, 1.5, 0.6])
                        g = self.cube(Rc, centre, sc, obs)
                        self.truth[1, g] = (Rc, centre, sc)
                    n += 1

    def _world(self, G, r, robot):
        return gg.World(G, self.sizes[r], seed=self.seed + 31 * r, step=self.step, origin=(1.0, 2.0 + self.spacing * r, 0.5), noise=0.002,
                        robot=robot)


def planted_list(c, vals=None, seed=PLANTED_SEED):
    """On a PlantedJoint: for every landmark, TRUE candidates measuring the GROUND TRUTH's geometry of the landmark with noise drawn at
    the factor's sigmas, from a pose of its own robot that does not observe it yet and from a pose of the OTHER robot (cross-robot: onto
    a private landmark through lm_slot, onto a shared one through the pose's own replica), and a FALSE one: the detection of another
    landmark of the class (at least 3 m away) tried against it, from the own robot or, every second time, from the other.  Asserted
    here, under d2_ref alone: every true one lies below 0.75 of its class's quantile, every false one above twice that quantile.
    -> (candidates, truth flags, d2_ref, dof)."""
    J = c.J
    assert isinstance(J, PlantedJoint)
    vals = vals or c.cpu_values
    rng = np.random.default_rng(seed)
    out, flags = [], []
    n = 0
    for cls, g, _, obs in J.lms:
        kind = CLS_KIND[cls]
        m = KIND[kind][3]
        robots = sorted({r for r, _ in obs})
        r = obs[0][0]
        o = 1 - r
        k0 = min(k for rr, k in obs if rr == r)
        centre = lambda key: np.asarray(J.truth[key] if key[0] == 2 else J.truth[key][0 if key[0] == 0 else 1], float)      # noqa: E731
        p = k0 + 3 if k0 + 3 < J.sizes[r] else k0 - 1
        l = local_id(c, r, cls, g)
        out.append(og.observe(c, kind, r, p, l, J.T(r, p), J.truth[cls, g], rng.normal(0, 1, m)))
        flags.append(True)
        po_ = min(k0 + 2, J.sizes[o] - 1)
        if o in robots:
            cross = og.observe(c, kind, o, po_, local_id(c, o, cls, g), J.T(o, po_), J.truth[cls, g], rng.normal(0, 1, m))
        else:
            cross = with_slot(og.observe(c, kind, o, po_, l, J.T(o, po_), J.truth[cls, g], rng.normal(0, 1, m)), r)
        out.append(cross)
        flags.append(True)
        others = [key for key in J.truth if key[0] == cls and key[1] != g and np.linalg.norm(centre(key) - centre((cls, g))) > 3.0]
        wrong = others[n % len(others)]
        s = r if n % 2 == 0 else o
        ps = p if s == r else po_
        out.append(with_slot(og.observe(c, kind, s, ps, l, J.T(s, ps), J.truth[wrong], rng.normal(0, 1, m)), r))
        flags.append(False)
        n += 1
    flags = np.array(flags)
    dof = np.array([KIND[x[0]][3] for x in out])
    q = np.array([QUANTILE[int(d)] for d in dof])
    _, _, _, d2 = ref_gate(c, out, vals)
    assert (d2[flags] < 0.75 * q[flags]).all() and (d2[~flags] > 2 * q[~flags]).all(), (d2 / q, flags)
    return out, flags, d2, dof


def planted_case(chart):
    return JointObsCase(PlantedJoint(), chart, **PLANTED_OKW)


def long_lists(c, vals, seed=9):
    """129 points, 43 cubes and 55 cylinders (one more than a sweep holds of each), 24 distinct candidates of each class repeated:
    random poses of any robot against random landmarks of any robot's graph (private and shared, about half of them cross-robot)."""
    J = c.J
    rng = np.random.default_rng(seed)
    lists = {}
    for kind, count in (("point", 129), ("cube", 43), ("cylinder", 55)):
        cls, m = KIND[kind][2], KIND[kind][3]
        scale = 0.5 if kind == "point" else 1.5
        base = []
        while len(base) < 24:
            s, ls = int(rng.integers(J.R)), int(rng.integers(J.R))
            if len(c.gid[ls][cls]) == 0:
                continue
            base.append(at_estimate(c, vals, kind, s, int(rng.integers(J.sizes[s])), int(rng.integers(len(c.gid[ls][cls]))),
                                    rng.normal(0, scale, m), ls))
        lists[kind] = [base[i % 24] for i in range(count)]
    return lists
