"""The individual-compatibility gate of landmark observations (slide_graph_observation_mahalanobis): the dense reference and the case
generators (test infrastructure for test_observation_gate_host.py and test_gpu_observation_gate.py; not a test).

The reference is built as closure_gate_cases builds its own.  Sigma is the dense inverse of the full, unreduced H of
tests/gn_reference.py at the linearisation point (test_gpu_marginals.dense_inverse, with its tolerance `tol` and `kappa`); r, Ap and
Al of a candidate come from the oracle's orc_linearize(F_BR / F_CUBE / F_CYL, ...) at the given pose and landmark values, under the
graph's chart, with z and the sigmas built HERE in numpy by the add calls' rules (add_rules); then
    C_ref = I + A Sig[sel, sel] A^T  over the pose's and the landmark's coordinates,   d2_ref = r^T C_ref^-1 r.
schur_form restates the device's route in numpy (H_ll^-1, F = E H_ll^-1, B, the reduced pose system) and is checked against C_ref
in test_observation_gate_host.py.  Everything here runs without a device; the GPU tests evaluate the same candidates at the values read
back with get_pose12 / get_landmark.

A candidate is the tuple SlideGraph.observation_mahalanobis takes:
    ("point", robot, pose_idx, lm_idx, bearing, range) | ("cube", robot, pose_idx, idx, pose7, cube7, scale) |
    ("cylinder", robot, pose_idx, idx, pose7, root, ray, radius)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import closure_cases as cc
import closure_gate_cases as cg
import gn_graphs as gg
from gn_reference import Reference
from oracle import pyoracle as po
from test_gpu_marginals import chain40, dense_inverse

# the 0.99 quantiles of chi-square with 3 / 7 / 9 degrees of freedom
QUANTILE = {3: 11.345, 7: 18.475, 9: 21.666}
# kind -> (factor type, variable type, SLIDE_CLS_*, rows = landmark dimension)
KIND = {"point": (po.F_BR, po.V_POINT, 2, 3), "cube": (po.F_CUBE, po.V_CUBE, 1, 9), "cylinder": (po.F_CYL, po.V_CYL, 0, 7)}
ROWS = {po.F_PRIOR: 6, po.F_BETWEEN: 6, po.F_BR: 3, po.F_CUBE: 9, po.F_CYL: 7}
PLANTED_BR_SIGMA, PLANTED_CYL_SIGMA = 0.05, 0.1
RAY = np.array([0.0, 0.05, 1.0]) / np.linalg.norm([0.0, 0.05, 1.0])


def planted40(g):
    """noisy40's trajectory (closure_gate_cases: chain40's world behind odometry noise, initial values half a sigma from the truth)
    with pose_count_graph's landmarks: a point, and a cylinder or a cube, every third pose, each seen from up to four consecutive
    poses.  The ground truth of every landmark is kept in W.truth[kind][idx]."""
    W = gg.World(cg.NoisyOdom(g, cc.ODOM_SIGMA6, cg.NOISY_SEED), 40, seed=3, noise=0.002)
    rng = np.random.default_rng(103)
    W.truth = {"point": {}, "cylinder": {}, "cube": {}}
    for k in range(0, 40, 3):
        obs = list(range(k, min(40, k + 4)))
        xyz = gg.around(W, k, rng)
        W.point(k, xyz, obs)
        W.truth["point"][k] = xyz
        if k % 2 == 0:
            root = gg.around(W, k, rng)
            W.cylinder(k, root, RAY, 0.25, obs)
            W.truth["cylinder"][k] = (root, RAY, 0.25)
        else:
            R, t, sc = gg.rot([0.1, 0.2, rng.uniform(-3, 3)]), gg.around(W, k, rng), np.array([0.8, 1.5, 0.6])
            W.cube(k, R, t, sc, obs)
            W.truth["cube"][k] = (R, t, sc)
    return W


def _lc(cls):
    return lambda g: gg.landmark_count_graph(g, cls, 12)


# name -> (builder, oracle parameters' keywords, the product's default_params keywords)
GRAPHS = {
    "chain40": (chain40, {}, {}),
    "lc_cylinder": (_lc(0), {}, {}), "lc_cube": (_lc(1), {}, {}), "lc_point": (_lc(2), {}, {}),
    "planted40": (planted40, dict(odom_sigma=list(cc.ODOM_SIGMA6), bearing_sigma=PLANTED_BR_SIGMA, cyl_sigma=PLANTED_CYL_SIGMA),
                  dict(noise_model_odom_vec=list(cc.ODOM_SIGMA6), bearing_range_sigma=PLANTED_BR_SIGMA, cylinder_sigma=PLANTED_CYL_SIGMA)),
}


def device_graph(gpu, name, chart, solve=True):
    build, _, kw = GRAPHS[name]
    G = gpu.SlideGraph(gpu.default_params(pose_chart=chart, **kw))
    W = build(G)
    if solve:
        assert G.gauss_newton(1) == 0
    return G, W


class Values:
    """Where a candidate is linearised: pose12(robot, idx) -> 12 doubles, lm(kind, idx) -> the landmark's value (3 / 15 / 7)."""

    def __init__(self, pose12, lm):
        self.pose12, self.lm = pose12, lm


def device_values(G):
    def pose12(robot, idx):
        st, p = G.get_pose12(robot, idx)
        assert st == 0
        return p

    def lm(kind, idx):
        st, v = G.get_landmark(KIND[kind][2], idx)
        assert st == 0
        return v
    return Values(pose12, lm)


class ObsCase:
    """One graph under one chart: the reference, its H, Sigma, Jacobi weights, tolerance and kappa, the sigmas the add calls choose,
    the world (ground truth) and the reference's own one-step estimate.  Built once per (name, chart) and never changed: case()."""

    def __init__(self, name, chart):
        build, okw, _ = GRAPHS[name]
        P = po.OrcParams.default(pose_chart=chart, **okw)
        og = po.OracleGraph(P)
        self.name, self.chart = name, chart
        self.bearing_sigma, self.cyl_sigma, self.cube_vec = float(P.bearing_sigma), float(P.cyl_sigma), np.array(list(P.cube_sigma))
        self.world = build(og)
        self.ref = Reference(og, chart)
        self.set_H(*dense_inverse(self.ref))
        dx, _ = self.ref.step()
        self.est = self.ref.retract(self.ref.values, dx)
        self.cpu_values = Values(lambda r, i: np.ascontiguousarray(self.est[self.ref.pose_var(r, i)][:12]),
                                 lambda kind, i: np.ascontiguousarray(self.est[self.ref.lm_var(KIND[kind][2], i)]))

    def set_H(self, H, Sig, w, tol, kappa):
        self.H, self.Sig, self.w, self.tol, self.kappa = H, Sig, w, tol, kappa

    def sel(self, kind, robot, pose_idx, lm_idx):
        vp, vl = self.ref.pose_var(robot, pose_idx), self.ref.lm_var(KIND[kind][2], lm_idx)
        return np.concatenate([np.arange(self.ref.off[vp], self.ref.off[vp + 1]), np.arange(self.ref.off[vl], self.ref.off[vl + 1])])


@functools.lru_cache(maxsize=None)
def case(name, chart):
    return ObsCase(name, chart)


# ---- the add calls' rules, in numpy -----------------------------------------------------------------------------------------------
def add_rules(c, cand):
    """(z (15, zero padded), sigma (9, zero padded)) of the factor the class's add call stores for the candidate's arguments:
    add_range_bearing z = [bearing / |bearing|, range], bearing_range_sigma; add_cube z = [loc R, loc t, scale] with
    loc = pose_world^-1 cube_world, noise_model_cube_vec x max(|loc.t|, 0.1); add_cylinder z = [pose^-1 root, R^T ray, radius],
    cylinder_sigma."""
    kind = cand[0]
    z, sg = np.zeros(15), np.zeros(9)
    if kind == "point":
        b = np.asarray(cand[4], float)
        z[:3], z[3] = b / np.linalg.norm(b), float(cand[5])
        sg[:3] = c.bearing_sigma
    elif kind == "cube":
        X, Cw = cc._pose(cand[4], np.float64), cc._pose(cand[5], np.float64)
        loc = cc._mul(cc._inv(X), Cw)
        z[:9], z[9:12], z[12:15] = loc[0].ravel(), loc[1], np.asarray(cand[6], float)
        sg[:] = c.cube_vec * max(float(np.linalg.norm(loc[1])), 0.1)
    else:
        X = cc._pose(cand[4], np.float64)
        z[:3] = X[0].T @ (np.asarray(cand[5], float) - X[1])
        z[3:6] = X[0].T @ np.asarray(cand[6], float)
        z[6] = float(cand[7])
        sg[:7] = c.cyl_sigma
    return z, sg


def linearize(c, cand, vals):
    """r (m), Ap (m x 6), Al (m x D) of the candidate at vals, whitened, by the oracle's orc_linearize."""
    ft, vt, _, m = KIND[cand[0]]
    z, sg = add_rules(c, cand)
    x0 = np.ascontiguousarray(vals.pose12(cand[1], cand[2]), float)
    x1 = np.zeros(15)
    v = np.asarray(vals.lm(cand[0], cand[3]), float)
    x1[:len(v)] = v
    r, J0, J1 = np.zeros(9), np.zeros(81), np.zeros(81)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    got = po.lib().orc_linearize(C.c_int(ft), P(x0), C.c_int(vt), P(x1), P(z), P(sg), C.c_int(c.chart), C.c_double(1e-6), P(r), P(J0), P(J1),
                                 C.c_int(1))
    assert got == m
    return r[:m].copy(), J0[:6 * m].reshape(m, 6).copy(), J1[:m * m].reshape(m, m).copy()


def ref_gate(c, cands, vals):
    """Lists r, A = [Ap | Al], C_ref and the array d2_ref of the candidates at vals."""
    rs, As, Cs, d2 = [], [], [], np.zeros(len(cands))
    for k, cand in enumerate(cands):
        r, Ap, Al = linearize(c, cand, vals)
        A = np.hstack([Ap, Al])
        sel = c.sel(cand[0], cand[1], cand[2], cand[3])
        Cm = np.eye(len(r)) + A @ c.Sig[np.ix_(sel, sel)] @ A.T
        rs.append(r); As.append(A); Cs.append(Cm)
        d2[k] = r @ np.linalg.solve(Cm, r)
    return rs, As, Cs, d2


def gate_bound(c, C_ref):
    """The permitted relative error of d2 (and, entry-wise against the largest entry of C_ref, of C and r): tol x cond(C_ref), floor
    1e-12 — test_gpu_closure_gate.py's bound."""
    return max(c.tol * float(np.linalg.cond(C_ref)), 1e-12)


def schur_form(c, cand, vals):
    """C by the route the device takes, in numpy: with J the reference's whitened Jacobian at the linearisation point, H_ll = sum Jl^T Jl
    over the landmark's factors, F_f = (Jp_f^T Jl_f) H_ll^-1, S the pose system with EVERY landmark eliminated,
        C = I + Al H_ll^-1 Al^T + B^T S^-1 B,   B = P_p^T Ap^T - sum_f P_{p_f}^T F_f Al^T."""
    ref = c.ref
    if not hasattr(c, "_schur"):          # (the graph's own part, once per case)
        i, j, v, res = ref.linearize()
        J = np.zeros((len(res), ref.n))
        np.add.at(J, (i, j), v)
        row0 = np.concatenate([[0], np.cumsum([ROWS[int(t)] for t in ref.ftype])])
        pose_vars = [k for k in range(len(ref.vtype)) if int(ref.vtype[k]) == po.V_POSE]
        pcols = np.concatenate([np.arange(ref.off[k], ref.off[k + 1]) for k in pose_vars])
        prow = {k: 6 * n for n, k in enumerate(pose_vars)}
        H = J.T @ J
        S = H[np.ix_(pcols, pcols)].copy()
        for k in range(len(ref.vtype)):
            if int(ref.vtype[k]) == po.V_POSE:
                continue
            lc = np.arange(ref.off[k], ref.off[k + 1])
            Hpl = H[np.ix_(pcols, lc)]
            S -= Hpl @ np.linalg.solve(H[np.ix_(lc, lc)], Hpl.T)
        c._schur = (J, row0, pcols, prow, H, S)
    J, row0, pcols, prow, H, S = c._schur
    r, Ap, Al = linearize(c, cand, vals)
    m = len(r)
    vp, vl = ref.pose_var(cand[1], cand[2]), ref.lm_var(KIND[cand[0]][2], cand[3])
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
    return np.eye(m) + Al @ Hinv @ Al.T + B.T @ np.linalg.solve(S, B)


# ---- candidates -------------------------------------------------------------------------------------------------------------------
def _sphere_noise(b, n2):
    """The unit vector a tangent step n2 (2) away from b on the sphere."""
    a = np.eye(3)[int(np.argmin(np.abs(b)))]
    b1 = np.cross(b, a)
    b1 /= np.linalg.norm(b1)
    b2 = np.cross(b, b1)
    th = float(np.linalg.norm(n2))
    if th < 1e-300:
        return b.copy()
    return np.cos(th) * b + np.sin(th) * (n2[0] * b1 + n2[1] * b2) / th


def cube_sigmas(c, X, Cw):
    return c.cube_vec * max(float(np.linalg.norm(cc._mul(cc._inv(X), Cw)[1])), 0.1)


def observe(c, kind, robot, pose_idx, lm_idx, X, lm, u):
    """The candidate (kind, robot, pose_idx, lm_idx, ...) that measures the landmark value lm (point xyz | cube (R, t, scale) |
    cylinder (root, ray, radius)) from the pose X = (R, t), moved by u (m) x the factor's sigmas (zeros: the geometry itself)."""
    u = np.asarray(u, float)
    R, t = X
    if kind == "point":
        n = u * c.bearing_sigma
        q = R.T @ (np.asarray(lm, float) - t)
        rho = float(np.linalg.norm(q))
        return ("point", robot, pose_idx, lm_idx, _sphere_noise(q / rho, n[:2]), rho + n[2])
    if kind == "cube":
        Rc, tc, sc = lm
        n = u * cube_sigmas(c, X, (Rc, tc))
        Cw = cc._mul((Rc, np.asarray(tc, float)), (cc._rotvec(n[:3]), n[3:6]))
        return ("cube", robot, pose_idx, lm_idx, gg.p7(R, t), gg.p7(*Cw), np.asarray(sc, float) + n[6:9])
    root, ray, rad = lm
    n = u * c.cyl_sigma
    return ("cylinder", robot, pose_idx, lm_idx, gg.p7(R, t), np.asarray(root, float) + n[3:6], np.asarray(ray, float) + n[:3], float(rad) + n[6])


def lm_value(kind, v):
    """The landmark value get_landmark / the reference hold (xyz | R t scale | root ray radius) as observe takes it."""
    v = np.asarray(v, float)
    if kind == "point":
        return v[:3].copy()
    if kind == "cube":
        return v[:9].reshape(3, 3).copy(), v[9:12].copy(), v[12:15].copy()
    return v[:3].copy(), v[3:6].copy(), float(v[6])


def at_estimate(c, vals, kind, robot, pose_idx, lm_idx, u):
    """observe() at the values' own pose and landmark: u = zeros gives a candidate whose residual is zero there."""
    return observe(c, kind, robot, pose_idx, lm_idx, cg.pose_of(vals.pose12(robot, pose_idx)), lm_value(kind, vals.lm(kind, lm_idx)), u)


# (kind, pose, landmark) of the lists compared with the reference.  chain40: landmark k is seen from poses k .. k + 3 (points every
# third pose, cylinders at even and cubes at odd multiples of three; point 39 and cube 39 have ONE observer, pose 39).  Per class: a
# pose that observes the landmark and one that does not, the first and the last pose, a landmark with one observer, the same (pose,
# landmark) twice.  lc_*: landmark 0 of the class is seen from all 12 poses, point 1 from poses 0 and 1.
PAIRS = {
    "chain40": [("point", 1, 0), ("point", 7, 0), ("point", 0, 21), ("point", 39, 39), ("point", 20, 39), ("point", 39, 3), ("point", 1, 0),
                ("cylinder", 7, 6), ("cylinder", 13, 6), ("cylinder", 0, 24), ("cylinder", 39, 36), ("cylinder", 0, 0), ("cylinder", 13, 6),
                ("cube", 4, 3), ("cube", 12, 3), ("cube", 0, 27), ("cube", 39, 39), ("cube", 25, 39), ("cube", 39, 9), ("cube", 4, 3)],
    "lc_cylinder": [("cylinder", 0, 0), ("cylinder", 11, 0), ("cylinder", 5, 0), ("cylinder", 5, 0), ("point", 7, 1), ("point", 0, 1)],
    "lc_cube": [("cube", 0, 0), ("cube", 11, 0), ("cube", 5, 0), ("cube", 5, 0), ("point", 7, 1), ("point", 0, 1)],
    "lc_point": [("point", 0, 0), ("point", 11, 0), ("point", 5, 0), ("point", 5, 0), ("point", 7, 1), ("point", 0, 1)],
}
SCALES = (0.5, 2.0, 6.0)


def perturbed_list(c, vals, seed=3):
    """PAIRS[c.name], each measured at the values' own geometry moved by a fixed-seed vector of 0.5, 2 or 6 x the factor's sigmas (the
    scales in turn, 0.3 of them for points; exact repeats of a (pose, landmark) get the same measurement)."""
    rng = np.random.default_rng(seed)
    out, seen = [], {}
    for n, (kind, p, l) in enumerate(PAIRS[c.name]):
        if (kind, p, l) in seen:
            out.append(out[seen[kind, p, l]])
            continue
        m = KIND[kind][3]
        u = rng.normal(0, 1, m)
        seen[kind, p, l] = len(out)
        # (a point's sigma is 1 m / 1 rad under the default bearing_range_sigma: 0.3 of the scale keeps its range positive)
        out.append(at_estimate(c, vals, kind, 0, p, l, (0.3 if kind == "point" else 1.0) * SCALES[n % 3] * u / np.linalg.norm(u) * np.sqrt(m)))
    return out


PLANTED_SEED = 1


def planted_list(c, vals=None, seed=PLANTED_SEED):
    """planted40: for every landmark k in 3 .. 27 of each class, two TRUE candidates — the GROUND TRUTH's geometry of landmark k from
    poses k + 4 and k - 1 (neither observes it yet), with noise drawn at the factor's sigmas — and one FALSE one: a detection of the
    landmark 12 ids on (same class) from pose k + 4, tried against landmark k.  Asserted here, under d2_ref alone: every true one
    lies below 0.75 of its class's quantile, every false one above twice that quantile.  -> (candidates, truth flags, d2_ref, dof)."""
    assert c.name == "planted40"
    vals = vals or c.cpu_values
    rng = np.random.default_rng(seed)
    T = c.world.T
    out, flags = [], []
    for kind in ("point", "cylinder", "cube"):
        m = KIND[kind][3]
        truth = c.world.truth[kind]
        for k in sorted(truth):
            if not (3 <= k <= 27 and k + 12 in truth):
                continue
            for p in (k + 4, k - 1):
                out.append(observe(c, kind, 0, p, k, T[p], truth[k], rng.normal(0, 1, m)))
                flags.append(True)
            out.append(observe(c, kind, 0, k + 4, k, T[k + 4], truth[k + 12], rng.normal(0, 1, m)))
            flags.append(False)
    flags = np.array(flags)
    dof = np.array([KIND[x[0]][3] for x in out])
    q = np.array([QUANTILE[int(d)] for d in dof])
    _, _, _, d2 = ref_gate(c, out, vals)
    assert (d2[flags] < 0.75 * q[flags]).all() and (d2[~flags] > 2 * q[~flags]).all(), (d2 / q, flags)
    return out, flags, d2, dof
