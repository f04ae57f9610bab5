"""A robust (iteratively reweighted) Gauss-Newton step in numpy on top of tests/gn_reference.py, and the graphs the robust-loss tests
share (test infrastructure for test_robust_reference.py and test_gpu_robust_loss.py).  No product code is involved.

The rule (GTSAM's noiseModel::Robust::WhitenSystem): for a selected between factor with base sigmas sigma0, s = |r|_2 of its whitened
residual r at the linearisation point (Reference.linearize), w = mEstimator::weight(s), and the factor enters the step with
sigma0 / sqrt(w).  Selected: loop closures (origin 1, mask bit 0) and relative measurements (origin 2, mask bit 1); odometry never.

Fan forwards the seam's calls to several graphs at once (a SlideGraph and the recording OracleGraph) and notes the origin of every
between factor in insertion order; the oracle's export keeps that order."""
from __future__ import annotations

import numpy as np

import gn_graphs as gg
from gn_reference import Reference
from oracle import pyoracle as po

HUBER, CAUCHY, GEMAN_MCCLURE, DCS = 1, 2, 3, 4
KINDS = {"huber": HUBER, "cauchy": CAUCHY, "geman_mcclure": GEMAN_MCCLURE, "dcs": DCS}
DEFAULT = {HUBER: 1.345, CAUCHY: 0.1, GEMAN_MCCLURE: 1.0, DCS: 1.0}
W_MIN = 1e-12
ROWS = {po.F_PRIOR: 6, po.F_BETWEEN: 6, po.F_BR: 3, po.F_CUBE: 9, po.F_CYL: 7}
CLOSURE_SIGMA = 1e-3       # noise_model_odom_vec (0.1) * 0.01: what add_loop_closure gives every coordinate under the default parameters


def weight(kind, param, s):
    """mEstimator::weight of the four losses at whitened norm s (array), clamped from below at W_MIN."""
    s = np.asarray(s, float)
    c = DEFAULT[kind] if param <= 0 else float(param)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == HUBER:
            w = np.where(s <= c, 1.0, c / s)
        elif kind == CAUCHY:
            w = c * c / (c * c + s * s)
        elif kind == GEMAN_MCCLURE:
            w = (c * c / (c * c + s * s)) ** 2
        elif kind == DCS:
            w = np.where(s * s <= c, 1.0, (2.0 * c / (c + s * s)) ** 2)
        else:
            raise ValueError(kind)
    return np.maximum(w, W_MIN)


class Fan:
    """Forwards every call to all of `graphs`; origin[i] = 0 odometry / 1 loop closure / 2 relative measurement of the i-th between
    factor, keys[i] = (from_robot, from_idx, to_robot, to_idx) of it."""

    def __init__(self, *graphs):
        self.graphs, self.origin, self.keys = graphs, [], []

    def __getattr__(self, name):
        def call(*a):
            if name == "add_keypose_between":
                self.origin.append(0)
                self.keys.append((a[0], a[1], a[0], a[2]))
            elif name in ("add_loop_closure", "add_relative_meas"):
                self.origin.append(1 if name == "add_loop_closure" else 2)
                self.keys.append((a[2], a[1], a[4], a[3]))
            for g in self.graphs:
                getattr(g, name)(*a)
        return call


def row_offsets(ref):
    return np.concatenate([[0], np.cumsum([ROWS[int(t)] for t in ref.ftype])])


def selected(ref, origin, mask=3):
    """Per factor of the export: True where the robust loss applies (origin: Fan.origin, aligned with the export's between factors)."""
    bt = np.flatnonzero(ref.ftype == po.F_BETWEEN)
    assert len(bt) == len(origin), (len(bt), len(origin))
    sel = np.zeros(len(ref.ftype), bool)
    for f, o in zip(bt, origin):
        sel[f] = o > 0 and bool((mask >> (o - 1)) & 1)
    return sel


def whitened_norms2(ref, values=None):
    """s^2 per factor at `values` under the graph's base sigmas."""
    _, _, _, r = ref.linearize(values)
    off = row_offsets(ref)
    return np.array([float(r[off[f]:off[f + 1]] @ r[off[f]:off[f + 1]]) for f in range(len(ref.ftype))])


def robust_step(ref, values, kind, param, sel):
    """One reweighted step at `values`: (dx, H, w per factor (1 where the loss does not apply), s^2 per factor, numdiff floor).
    kind 0: the plain step."""
    from test_gn_reference import numdiff_floor
    s2 = whitened_norms2(ref, values)
    w = np.ones(len(ref.ftype))
    if kind:
        w[sel] = weight(kind, param, np.sqrt(s2[sel]))
    base = ref.fsig
    ref.fsig = base.copy()
    ref.fsig[:, :6] = np.where(sel[:, None], base[:, :6] / np.sqrt(w)[:, None], base[:, :6])
    try:
        dx, H = ref.step(values)
        floor = numdiff_floor(ref, dx, H, values)
    finally:
        ref.fsig = base
    return dx, H, w, s2, floor


def irls(ref, kind, param, sel, steps, values=None):
    """`steps` reweighted steps from `values` -> (values, weights of the last step's linearisation, per-step (dx, H))."""
    vals = ref.values if values is None else values
    w, trace = np.ones(len(ref.ftype)), []
    for _ in range(steps):
        dx, H, w, _, _ = robust_step(ref, vals, kind, param, sel)
        trace.append((dx, H))
        vals = ref.retract(vals, dx)
    return vals, w, trace


# ---- graphs ------------------------------------------------------------------------------------------------------------------------

def _rel(W, i, k, dt=(0.0, 0.0, 0.0), drot=(0.0, 0.0, 0.0)):
    """The ground truth's relative pose i -> k, then moved by a rotation and a translation in k's frame: where both poses stand at
    the truth, Local(measured, x_i^-1 x_k) is (about) -(drot, dt)."""
    (Ra, ta), (Rb, tb) = W.T[i], W.T[k]
    R, t = Ra.T @ Rb, Ra.T @ (tb - ta)
    D = gg.rot(drot)
    return gg.p7(R @ D, t + R @ np.asarray(dt, float))


def chain_graph(G, P=12, seed=11):
    """A P-pose chain (robot 0) whose initial values are exact for poses 0 .. 7, with closures measured on those poses plus a
    translation of s * sigma: whitened norms 0.3 (an inlier of every loss with a kink), 1.03 (just past DCS's kink s^2 = 1), 1.4
    (just past Huber's k = 1.345), 3000 (gross), and one relative measurement to a second robot's pose that is 0.5 m off.  The last
    poses' initial values are perturbed, so the step moves the chain."""
    W = gg.World(G, P, seed=seed, noise=0.0, perturb={k: [0.03, -0.02, 0.01] for k in range(8, P)})
    sg = CLOSURE_SIGMA
    for (i, k), s in (((0, 3), 0.3), ((1, 5), 1.03), ((2, 6), 1.4), ((3, 7), 3000.0)):
        G.add_loop_closure(_rel(W, i, k, dt=(s * sg, 0.0, 0.0)), i, 0, k, 0)
    G.add_loop_closure(_rel(W, 4, P - 1), 4, 0, P - 1, 0)                      # (to a perturbed pose: a residual from the perturbation)
    R1, t1 = W.T[2][0] @ gg.rot([0, 0, 0.4]), W.T[2][1] + np.array([0.5, 1.0, 0.0])
    G.set_prior(1, gg.p7(R1, t1))
    Ra, ta = W.T[2]
    G.add_relative_meas(gg.p7((Ra.T @ R1) @ gg.rot([0.0, 0.0, 0.05]), Ra.T @ (t1 - ta) + np.array([0.5, 0.0, 0.0])), 2, 0, 0, 1)
    return W


def inlier_graph(G, P=12, seed=12):
    """A chain with perturbed initial values and closures whose residuals at every point the first steps visit stay far below Huber's
    k = 1.345: the closures' ends are exact and pinned (the first poses, next to the prior), measured exactly."""
    W = gg.World(G, P, seed=seed, noise=0.0, perturb={k: [0.02, 0.01, -0.01] for k in range(6, P)})
    for i, k in ((0, 2), (1, 3), (0, 4)):
        G.add_loop_closure(_rel(W, i, k), i, 0, k, 0)
    return W


def edge_graph(G, N, seed=13):
    """Exactly N between factors.  The selected ones (a relative measurement to a second robot's only pose at index 0, loop closures
    elsewhere) sit first, last and on both sides of every 128-boundary below N; all the others are odometry.  -> the selected
    indices."""
    sel = sorted({0, N - 1} | {q for b in (128, 256) for q in (b - 1, b) if q < N})
    n_odo = N - len(sel)
    rec = _Recorder()
    W = gg.World(rec, n_odo + 1, seed=seed, noise=0.002, full3d=False)
    calls = iter(rec.calls)
    G.set_prior(*next(calls)[1])
    R1, t1 = W.T[0][0] @ gg.rot([0, 0, -0.3]), W.T[0][1] + np.array([0.0, -2.0, 0.0])
    G.set_prior(1, gg.p7(R1, t1))
    last = 0
    for q in range(N):
        if q == 0:
            Ra, ta = W.T[0]
            G.add_relative_meas(gg.p7(Ra.T @ R1, Ra.T @ (t1 - ta) + np.array([0.3, 0.0, 0.0])), 0, 0, 0, 1)
        elif q in sel:
            i = max(0, last - 3 - (q % 3))
            assert i != last
            G.add_loop_closure(_rel(W, i, last, dt=(0.002 * (1 + q % 5), 0.001, 0.0)), i, 0, last, 0)
        else:
            G.add_keypose_between(*next(calls)[1])
            last += 1
    return sel


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append((name, a))


def mask_graph(G, P=10, seed=14):
    """A chain with two loop closures and two relative measurements (to a second robot's pose), all with residuals."""
    W = gg.World(G, P, seed=seed, noise=0.004)
    G.add_loop_closure(_rel(W, 0, 4, dt=(0.004, 0.0, 0.0)), 0, 0, 4, 0)
    R1, t1 = W.T[3][0] @ gg.rot([0, 0, 0.2]), W.T[3][1] + np.array([1.0, 1.0, 0.0])
    G.set_prior(1, gg.p7(R1, t1))
    for k, off in ((3, 0.3), (6, -0.2)):
        Ra, ta = W.T[k]
        G.add_relative_meas(gg.p7(Ra.T @ R1, Ra.T @ (t1 - ta) + np.array([off, 0.0, 0.0])), k, 0, 0, 1)
    G.add_loop_closure(_rel(W, 2, 8, dt=(0.0, 0.05, 0.0)), 2, 0, 8, 0)
    return W


# ---- the planted scenario ----------------------------------------------------------------------------------------------------------
PLANTED_STEPS = 8
PLANTED_PARAM = {GEMAN_MCCLURE: 30.0, DCS: 900.0}       # c and Phi = c^2: the kernel's width in whitened units, see planted_graph
TRUE_CLOSURES = [(k, k + 20) for k in (0, 3, 6, 9, 12, 15)]
FALSE_CLOSURES = [(5, 33), (11, 27)]


def planted_graph(G, seed=21):
    """Two laps of a 20-pose planar circle (40 poses, 1 m steps): pose k + 20 revisits pose k.  Odometry carries noise of 1e-4 rad and
    3e-4 m per step and the initial values are its dead-reckoned chain, so the second lap has drifted by a few millimetres — a few
    closure sigmas (1e-3) — when the closures arrive.  Six true closures (k, k + 20) with noise of one closure sigma; two false ones
    between places half a lap apart that claim they coincide up to (3 m, -2 m) and 1 rad: whitened norms of several thousand.
    A redescending loss only keeps what starts inside its kernel, so the kernel is as wide as the drift the closures have to
    correct: c = 30 sigmas (Geman-McClure), Phi = c^2 (DCS) — PLANTED_PARAM.  -> ground-truth poses (R, t)."""
    rng = np.random.default_rng(seed)
    n, lap = 40, 20
    th = 2 * np.pi / lap
    T = [(gg.rot([0, 0, 0.0]), np.zeros(3))]
    for k in range(1, n):
        R, t = T[-1]
        R2 = R @ gg.rot([0, 0, th])
        T.append((R2, t + R2 @ np.array([1.0, 0.0, 0.0])))
    G.set_prior(0, gg.p7(*T[0]))
    est = [T[0]]
    for k in range(1, n):
        (Ra, ta), (Rb, tb) = T[k - 1], T[k]
        Rr = Ra.T @ Rb @ gg.rot(rng.normal(0, 1e-4, 3) * [0, 0, 1])
        tr = Ra.T @ (tb - ta) + rng.normal(0, 3e-4, 3) * [1, 1, 0]
        Re, te = est[-1]
        est.append((Re @ Rr, te + Re @ tr))
        G.add_keypose_between(0, k - 1, k, gg.p7(Rr, tr), gg.p7(*est[-1]))
    for i, k in TRUE_CLOSURES:
        (Ra, ta), (Rb, tb) = T[i], T[k]
        G.add_loop_closure(gg.p7(Ra.T @ Rb @ gg.rot(rng.normal(0, CLOSURE_SIGMA, 3) * [0, 0, 1]),
                                 Ra.T @ (tb - ta) + rng.normal(0, CLOSURE_SIGMA, 3) * [1, 1, 0]), i, 0, k, 0)
    for i, k in FALSE_CLOSURES:
        G.add_loop_closure(gg.p7(gg.rot([0, 0, 1.0]), np.array([3.0, -2.0, 0.0])), i, 0, k, 0)
    return T


def pose_error(ref, values, T):
    """RMS position error of robot 0's poses against the ground truth (metres)."""
    err = [np.linalg.norm(values[ref.pose_var(0, k), 9:12] - T[k][1]) for k in range(len(T))]
    return float(np.sqrt(np.mean(np.square(err))))


def planted_reference(kind, chart=0, seed=21):
    """The numpy IRLS on the planted scenario -> dict(ref, sel, origin, T, values, w, trace)."""
    og = po.OracleGraph(po.OrcParams.default(pose_chart=chart))
    fan = Fan(og)
    T = planted_graph(fan, seed)
    ref = Reference(og, chart)
    sel = selected(ref, fan.origin)
    param = PLANTED_PARAM.get(kind, 0.0)
    vals, w, trace = irls(ref, kind, param, sel, PLANTED_STEPS)
    return dict(ref=ref, sel=sel, origin=fan.origin, T=T, values=vals, w=w[sel] if kind else np.ones(int(sel.sum())), trace=trace, param=param)

