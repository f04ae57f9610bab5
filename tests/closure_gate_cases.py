"""The individual-compatibility gate of loop closures and the joint marginal of pose pairs (slide_graph_closure_mahalanobis /
slide_graph_get_pose_pair_covariances): the dense reference and the case generators (test infrastructure for
test_closure_gate_host.py and test_gpu_closure_gate.py; not a test).

The reference is built from material the suite already trusts: Sigma is the dense inverse of the full, unreduced H of
tests/gn_reference.py at the linearisation point (test_gpu_marginals.dense_inverse, with its tolerance `tol` and `kappa`); r and A of a
closure come from the oracle's orc_linearize(F_BETWEEN, ...) at the two estimate poses, under the graph's chart; then
    C_ref = I + A Sig_pp A^T,   d2_ref = r^T C_ref^-1 r          in numpy.
Everything here runs without a device.  The estimate a generator needs on the CPU is the reference's own Gauss-Newton step
(Reference.step + retract: what gauss_newton(1) is checked against in test_gpu_gn_step.py); the GPU tests evaluate the same closures
at the poses read back with get_pose12.

The graphs: chain40, loop36 and two_robots of test_gpu_marginals under both charts, and `noisy40`, chain40's trajectory with
odometry noise: the Between measurements are the true steps times noise drawn at the odometry sigmas the graph is told (closure_cases.ODOM_SIGMA6), so the
estimate drifts from the ground truth the way Sigma says it may."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import closure_cases as cc
import gn_graphs as gg
from gn_reference import Reference
from oracle import pyoracle as po
from test_gpu_marginals import chain40, dense_inverse, loop36, two_robots

GATE2 = 16.81                        # the 0.99 quantile of chi-square with 6 degrees of freedom (slide_closure_params_t::gate squared)
SIGMA6 = cc.CLOSURE_SIGMA6


class NoisyOdom:
    """A graph seen through odometry noise: every add_keypose_between measurement is multiplied by a tangent vector drawn at `odom`
    (seeded by the step, so the oracle graph and the device graph receive the same values); everything else passes through."""

    def __init__(self, g, odom, seed):
        self._g, self._odom, self._seed = g, np.asarray(odom, float), seed

    def __getattr__(self, name):
        return getattr(self._g, name)

    def add_keypose_between(self, robot, frm, to, rel7, est7):
        rng = np.random.default_rng([self._seed, robot, int(to)])
        n = rng.normal(0, 1, 6) * self._odom
        rel = cc._mul(cc._pose(rel7, np.float64), (cc._rotvec(n[:3]), n[3:]))
        self._g.add_keypose_between(robot, frm, to, cc.p7(rel), est7)


# One drift realisation serves every closure of a list, so their d2 are correlated: under seed 40 sixty true closures averaged 6.8 (a
# drift well out in its own distribution), under 41 they average 2.7 with none above 6.8.  The planted cases need the latter.
NOISY_SEED = 41


def noisy40(g):
    """chain40's trajectory (the same World, 240 rows) behind odometry noise, a point landmark every third pose.  The initial values
    start 0.002 rad / 0.01 m from the truth instead of chain40's 0.02 / 0.1: half an odometry sigma, not five, so that the one
    Gauss-Newton step the tests take ends where the linear model says it does (from five sigmas the step's second-order remainder is
    as large as the marginal sigmas themselves, and true closures came out at d2 of 11 to 18 under d2_ref)."""
    W = gg.World(NoisyOdom(g, cc.ODOM_SIGMA6, NOISY_SEED), 40, seed=3, noise=0.002)
    rng = np.random.default_rng(103)
    for k in range(0, 40, 3):
        W.point(k, gg.around(W, k, rng), list(range(k, min(40, k + 4))))
    return W


# name -> (builder, the odometry sigmas both graphs are created with, or None for the defaults)
GRAPHS = {"chain40": (chain40, None), "loop36": (loop36, None), "two_robots": (two_robots, None), "noisy40": (noisy40, cc.ODOM_SIGMA6)}


def device_graph(gpu, name, chart, solve=True):
    build, odom = GRAPHS[name]
    kw = {} if odom is None else {"noise_model_odom_vec": list(odom)}
    G = gpu.SlideGraph(gpu.default_params(pose_chart=chart, **kw))
    W = build(G)
    if solve:
        assert G.gauss_newton(1) == 0
    return G, W


class GateCase:
    """One graph under one chart: the reference's H, Sigma, Jacobi weights, tolerance and kappa; the ground truth (World) of robot 0;
    the reference's own one-step estimate.  Built once per (name, chart) and never changed: case()."""

    def __init__(self, name, chart):
        build, odom = GRAPHS[name]
        kw = {} if odom is None else {"odom_sigma": list(odom)}
        og = po.OracleGraph(po.OrcParams.default(pose_chart=chart, **kw))
        self.name, self.chart = name, chart
        self.world = build(og)
        self.ref = Reference(og, chart)
        self.H, self.Sig, self.w, self.tol, self.kappa = dense_inverse(self.ref)
        self.scale = float(np.abs(self.Sig * np.outer(self.w, self.w)).max())
        dx, _ = self.ref.step()
        self.est = self.ref.retract(self.ref.values, dx)

    def off(self, robot, idx):
        return int(self.ref.off[self.ref.pose_var(robot, idx)])

    def cpu_pose12(self, robot, idx):
        return np.ascontiguousarray(self.est[self.ref.pose_var(robot, idx)][:12])

    def pair_sigma(self, ra, ia, rb, ib):
        """(12 x 12 joint marginal of the reference, the Jacobi weights of its twelve coordinates)"""
        sel = np.concatenate([np.arange(6) + self.off(ra, ia), np.arange(6) + self.off(rb, ib)])
        return self.Sig[np.ix_(sel, sel)], self.w[sel]


@functools.lru_cache(maxsize=None)
def case(name, chart):
    return GateCase(name, chart)


def pose_of(x12):
    x12 = np.asarray(x12, float)
    return x12[:9].reshape(3, 3).copy(), x12[9:12].copy()


def measured(pose12, fr, fi, tr, ti, xi, sigma6=SIGMA6):
    """The closure tuple (from_robot, from_idx, to_robot, to_idx, rel7, sigma6) measuring X_from^-1 X_to of the poses pose12(robot, idx)
    gives, times the tangent vector xi ([rot, trans]; zeros: the relative pose itself)."""
    F, T = pose_of(pose12(fr, fi)), pose_of(pose12(tr, ti))
    xi = np.asarray(xi, float)
    rel = cc._mul(cc._mul(cc._inv(F), T), (cc._rotvec(xi[:3]), xi[3:]))
    return (fr, fi, tr, ti, cc.p7(rel), np.asarray(sigma6, float).copy())


def ref_gate(c, closures, pose12):
    """r (L, 6), A (L, 6, 12), C_ref (L, 6, 6), d2_ref (L) of the closures at the poses pose12(robot, idx) returns."""
    L = po.lib()
    n = len(closures)
    r, A, Cm, d2 = np.zeros((n, 6)), np.zeros((n, 6, 12)), np.zeros((n, 6, 6)), np.zeros(n)
    rr, J0, J1 = np.zeros(9), np.zeros(81), np.zeros(81)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    for k, (fr, fi, tr, ti, rel7, sg) in enumerate(closures):
        xf, xt = np.ascontiguousarray(pose12(fr, fi), float), np.ascontiguousarray(pose12(tr, ti), float)
        R, t = cc._pose(rel7, np.float64)
        z = np.ascontiguousarray(np.concatenate([R.ravel(), t]))
        s6 = np.ascontiguousarray(np.broadcast_to(np.asarray(sg, float), (6,)))
        m = L.orc_linearize(C.c_int(po.F_BETWEEN), P(xf), C.c_int(po.V_POSE), P(xt), P(z), P(s6), C.c_int(c.chart), C.c_double(1e-6),
                            P(rr), P(J0), P(J1), C.c_int(1))
        assert m == 6
        r[k] = rr[:6]
        A[k, :, :6], A[k, :, 6:] = J0[:36].reshape(6, 6), J1[:36].reshape(6, 6)
        Sp, _ = c.pair_sigma(fr, fi, tr, ti)
        Cm[k] = np.eye(6) + A[k] @ Sp @ A[k].T
        d2[k] = r[k] @ np.linalg.solve(Cm[k], r[k])
    return r, A, Cm, d2


def gate_bound(c, C_ref):
    """The permitted relative error of d2 (and, entry-wise against the largest entry, of C and r): tol x cond(C_ref), floor 1e-12."""
    return max(c.tol * float(np.linalg.cond(C_ref)), 1e-12)


# ---- the lists ------------------------------------------------------------------------------------------------------------------------
PAIRS = {
    # first with last pose, neighbours, both orders, a pose of the first tile with one of the last (rows 18.. and 222.. of 256), a pose
    # whose six rows straddle a tile boundary (pose 10: rows 60 .. 65)
    "chain40": [(0, 0, 0, 39), (0, 39, 0, 0), (0, 5, 0, 6), (0, 6, 0, 5), (0, 3, 0, 37), (0, 37, 0, 3), (0, 10, 0, 11), (0, 10, 0, 30)],
    "loop36": [(0, 0, 0, 35), (0, 35, 0, 0), (0, 17, 0, 18), (0, 18, 0, 17), (0, 2, 0, 33), (0, 10, 0, 20)],
    # poses of two different robots, both orders
    "two_robots": [(0, 0, 0, 23), (0, 23, 0, 0), (0, 0, 1, 15), (1, 15, 0, 0), (0, 10, 1, 4), (1, 4, 0, 10), (1, 3, 1, 12), (0, 5, 0, 6),
                   (0, 23, 1, 0)],
}
ENDS = {
    "chain40": [(0, 39, 0, 0), (0, 0, 0, 39), (0, 30, 0, 2), (0, 37, 0, 3), (0, 6, 0, 5), (0, 25, 0, 10)],
    "loop36": [(0, 35, 0, 1), (0, 20, 0, 3), (0, 3, 0, 20), (0, 18, 0, 17), (0, 30, 0, 12), (0, 9, 0, 27)],
    "two_robots": [(0, 23, 0, 1), (0, 20, 1, 2), (1, 15, 0, 0), (1, 14, 1, 1), (0, 3, 1, 12), (0, 6, 0, 5)],
}
SCALES = (0.5, 2.0, 10.0)


def perturbed_list(name, pose12, seed=3):
    """For every pair of ends of the graph, three closures measured at the estimate's own relative pose times a fixed-seed tangent
    vector of 0.5 x, 2 x and 10 x the closure's stated sigmas; the sigmas themselves vary per closure (0.5 x to 4 x CLOSURE_SIGMA6,
    each component by itself)."""
    rng = np.random.default_rng(seed)
    out = []
    for e in ENDS[name]:
        for sc in SCALES:
            sg = SIGMA6 * rng.uniform(0.5, 4.0, 6)
            u = rng.normal(0, 1, 6)
            out.append(measured(pose12, *e, sc * sg * u / np.linalg.norm(u) * np.sqrt(6.0), sg))
    return out


def planted_list(c, pose12=None, seed=1, n_true=8, n_false=4):
    """noisy40: closures from late poses back to early ones — true ones measure the GROUND TRUTH's relative pose times noise drawn at
    their stated sigmas, false ones the same displaced by about 0.3 rad and 3 m (closure_cases.measure).  Asserted here, under d2_ref
    alone: every true one lies below 16.81 / 2, every false one above 4 x 16.81.  Returns (closures, truth flags, d2_ref)."""
    assert c.name == "noisy40"
    rng = np.random.default_rng(seed)
    T = [tuple(x) for x in c.world.T]
    flags = np.array([True] * n_true + [False] * n_false)
    rng.shuffle(flags)
    out = []
    for ok in flags:
        i = int(rng.integers(25, 40))
        j = int(rng.integers(0, 12))
        out.append((0, i, 0, j, cc.p7(cc.measure(T[i], T[j], rng, false=not ok)), SIGMA6.copy()))
    _, _, _, d2 = ref_gate(c, out, pose12 or c.cpu_pose12)
    assert d2[flags].max() < GATE2 / 2 and d2[~flags].min() > 4 * GATE2, (d2[flags].max(), d2[~flags].min())
    return out, flags, d2


def aliased_list(c, pose12=None, seed=5):
    """noisy40, one list for the gate AND slide_graph_select_closures: eight true closures (noise at PLANTED_SCALE x their sigmas, as
    closure_cases' planted cases: the clique solver then returns all of them), one isolated false closure, and three false closures
    that agree with each other — each measures F^-1 D T with the SAME world-frame displacement D, as a second place that looks like the
    first produces, so every cycle through two of them closes.  Asserted here, on the CPU: d2_ref puts the four false ones above 16.81
    and the eight true ones below; the restatement of the consistency score (closure_cases.restate, at the same poses, with the
    graph's odometry sigmas) scores the three aliased closures consistent with each other and with no true one; the oracle's CLIPPER
    on that matrix keeps true closures only, and on the false closures alone keeps the three aliased ones.  Returns (closures, kinds, d2_ref): kinds 0 true, 1 isolated false,
    2 aliased false."""
    assert c.name == "noisy40"
    pose12 = pose12 or c.cpu_pose12
    rng = np.random.default_rng(seed)
    T = [tuple(x) for x in c.world.T]
    kinds = np.array([0] * 8 + [1] + [2] * 3)
    rng.shuffle(kinds)
    D = (cc._rotvec([0.0, 0.05, 0.35]), np.array([2.5, -1.5, 0.3]))
    out = []
    for kd in kinds:
        i, j = int(rng.integers(25, 40)), int(rng.integers(0, 12))
        if kd == 2:
            z = cc._mul(cc._mul(cc._inv(pose_of(pose12(0, i))), D), pose_of(pose12(0, j)))
        else:
            z = cc.measure(T[i], T[j], rng, false=kd == 1, scale=cc.PLANTED_SCALE)
        out.append((0, i, 0, j, cc.p7(z), SIGMA6.copy()))
    _, _, _, d2 = ref_gate(c, out, pose12)
    assert d2[kinds == 0].max() < GATE2 < d2[kinds != 0].min(), d2
    p7 = lambda r, i: cc.p7(pose_of(pose12(r, i)))
    d, M = cc.restate([p7(0, x[1]) for x in out], [p7(0, x[3]) for x in out], [x[4] for x in out], [x[5] for x in out],
                      [x[1] for x in out], [x[3] for x in out], odom_sigma6=cc.ODOM_SIGMA6)
    al, tr = np.nonzero(kinds == 2)[0], np.nonzero(kinds == 0)[0]
    assert all(M[a, b] > 0.5 for a in al for b in al if a != b), M[np.ix_(al, al)]      # the aliased ones agree with each other
    assert not M[np.ix_(al, tr)].any()                                                  # ... and with no true closure
    # the oracle's CLIPPER keeps true closures only — and, left alone with the false ones, keeps the three aliased ones as a set:
    # mutual consistency cannot tell them from a true group
    fa = np.nonzero(kinds != 0)[0]
    assert set(cc.oracle_select(M)) <= set(tr.tolist()) and len(cc.oracle_select(M)) >= 3
    assert [int(fa[i]) for i in cc.oracle_select(M[np.ix_(fa, fa)])] == al.tolist()
    return out, kinds, d2
