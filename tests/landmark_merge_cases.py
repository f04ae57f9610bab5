"""Landmark fusion (slide_graph_merge_landmarks): the independent reference and the case generators (test infrastructure for
test_landmark_merge_host.py and test_gpu_landmark_merge.py; not a test).

The reference holds no merge code.  Rekey forwards a builder's calls to a graph with the landmark keys mapped drop -> keep: it skips
add_point_landmark of a dropped key and passes exists=True for a dropped cylinder's or cube's first observation.  The builder draws
the same random numbers, because only names change, so gn_reference.Reference(Rekey(OracleGraph)) is the merged graph as data: the
survivor holds its own initial value and every factor of both.

Graphs: landmark_pair_cases.dup40 (true duplicates k / 100 + k, the revisit 900 / 901 across the profile, distinct neighbours 200 + k
that share observers); trip40, its pattern with triples (300 + k), factor-less members (400 + k) and cube pairs; merge_count_graph,
two landmarks at one place with na and nb factors (the merged list crosses k_landmark's lane and wave counts)."""
from __future__ import annotations

import functools

import numpy as np

import closure_cases as cc
import closure_gate_cases as cg
import gn_graphs as gg
import landmark_pair_cases as lp
import observation_gate_cases as og
from gn_reference import EPS, Reference
from oracle import pyoracle as po

CLS = lp.CLS
DIM = lp.DIM
KEY_TAG = {0: "l", 1: "c", 2: "u"}
MISSING, INVALID, NOT_SPD = 1, -1, -2


class Rekey:
    """A graph seen through a merge: drop maps (cls, dropped idx) -> kept idx."""

    def __init__(self, g, drop):
        self._g, self._drop = g, dict(drop)

    def __getattr__(self, name):
        return getattr(self._g, name)

    def add_point_landmark(self, idx, xyz):
        if (2, int(idx)) not in self._drop:
            self._g.add_point_landmark(idx, xyz)

    def add_range_bearing(self, robot, pose_idx, lm_idx, bearing, rng):
        self._g.add_range_bearing(robot, pose_idx, self._drop.get((2, int(lm_idx)), lm_idx), bearing, rng)

    def add_cube(self, robot, pose_idx, idx, pose7, cube7, scale, exists):
        d = (1, int(idx)) in self._drop
        self._g.add_cube(robot, pose_idx, self._drop.get((1, int(idx)), idx), pose7, cube7, scale, exists or d)

    def add_cylinder(self, robot, pose_idx, idx, pose7, root, ray, radius, exists):
        d = (0, int(idx)) in self._drop
        self._g.add_cylinder(robot, pose_idx, self._drop.get((0, int(idx)), idx), pose7, root, ray, radius, exists or d)


# ---- graphs -----------------------------------------------------------------------------------------------------------------------
CUBE_SCALE = np.array([0.8, 1.5, 0.6])


def trip40(g):
    """dup40's trajectory and pattern.  Every third pose k: point k (poses k, k + 1) and point 100 + k at the same place (k + 2,
    k + 3); where k % 6 == 3 a third copy 300 + k (k + 4, k + 5); where k % 12 == 0 a copy 400 + k that no pose observes.  Every sixth
    pose the same pair as cylinders, a third copy where k % 12 == 6; every ninth pose a pair of cubes.  W.clusters[kind]: the members
    of every object, smallest key first."""
    W = gg.World(cg.NoisyOdom(g, cc.ODOM_SIGMA6, cg.NOISY_SEED), 40, seed=3, noise=0.002)
    rng = np.random.default_rng(207)
    W.clusters = {"point": [], "cylinder": [], "cube": []}
    for k in range(0, 34, 3):
        xyz = gg.around(W, k, rng)
        W.point(k, xyz, [k, k + 1])
        W.point(100 + k, xyz, [k + 2, k + 3])
        mem = [k, 100 + k]
        if k % 6 == 3:
            W.point(300 + k, xyz, [k + 4, k + 5])
            mem.append(300 + k)
        if k % 12 == 0:
            W.G.add_point_landmark(400 + k, xyz + rng.normal(0, 0.05, 3))
            mem.append(400 + k)
        W.clusters["point"].append(mem)
        if k % 6 == 0:
            root = gg.around(W, k, rng)
            W.cylinder(k, root, og.RAY, 0.25, [k, k + 1])
            W.cylinder(100 + k, root, og.RAY, 0.25, [k + 2, k + 3])
            mem = [k, 100 + k]
            if k % 12 == 6:
                W.cylinder(300 + k, root, og.RAY, 0.25, [k + 4, k + 5])
                mem.append(300 + k)
            W.clusters["cylinder"].append(mem)
        if k % 9 == 0:
            R, t = gg.rot([0.1, 0.2, rng.uniform(-3, 3)]), gg.around(W, k, rng)
            W.cube(k, R, t, CUBE_SCALE, [k, k + 1])
            W.cube(100 + k, R, t, CUBE_SCALE, [k + 2, k + 3])
            W.clusters["cube"].append([k, 100 + k])
    return W


FIT_OFFSET = np.array([0.03, -0.02, 0.01])      # two fits of one object differ by centimetres


def merge_count_graph(cls, na, nb):
    """A chain of na + nb poses; landmark 0 of class cls (0 cylinder, 2 point) seen from the first na, landmark 1 — the same object
    fitted FIT_OFFSET away, so that the merged graph's optimum is neither's — from the last nb; point 7 from the first two poses.  Merged, landmark 0 holds na + nb factors."""
    def build(g):
        P = na + nb
        W = gg.World(g, P, seed=2, step=0.3)
        c = W.T[P // 2][1] + W.T[P // 2][0] @ np.array([5.0, 1.0, 0.5])
        ray = np.array([0.05, -0.02, 1.0]) / np.linalg.norm([0.05, -0.02, 1.0])
        for idx, obs, at in ((0, range(na), c), (1, range(na, P), c + FIT_OFFSET)):
            if cls == 0:
                W.cylinder(idx, at, ray, 0.3, obs)
            else:
                W.point(idx, at, obs)
        W.point(7, c + np.array([1.0, -2.0, 0.3]), range(2))
        return W
    return build


_DUP_KW = og.GRAPHS["dup40"][1:]
BUILDERS = {"dup40": (lp.dup40,) + _DUP_KW, "trip40": (trip40,) + _DUP_KW}


def builder(name):
    """(build, the oracle parameters' keywords, the product's default_params keywords); name: a registered graph, or
    ("count", cls, na, nb)."""
    if isinstance(name, tuple):
        return merge_count_graph(*name[1:]), {}, {}
    return BUILDERS[name]


def oracle_graph(name, chart, drop=None):
    """(OracleGraph built through Rekey(drop), its world)."""
    build, okw, _ = builder(name)
    g = po.OracleGraph(po.OrcParams.default(pose_chart=chart, **okw))
    W = build(Rekey(g, drop or {}))
    return g, W


@functools.lru_cache(maxsize=None)
def _reference(name, chart, drop_items):
    g, W = oracle_graph(name, chart, dict(drop_items))
    return Reference(g, chart), W


def reference(name, chart, drop=None):
    """The Reference of the graph rekeyed by drop (none: the graph as built) and its world; built once, never changed."""
    return _reference(name, chart, tuple(sorted((drop or {}).items())))


def device_graph(gpu, name, chart, drop=None):
    """(SlideGraph, world): the graph built through Rekey(drop) — from scratch, no merge call."""
    build, _, kw = builder(name)
    G = gpu.SlideGraph(gpu.default_params(pose_chart=chart, **kw))
    W = build(Rekey(G, drop or {}))
    return G, W


def true_pairs(W, kind):
    """dup40's planted true pairs of one class as (keep, drop) rows: the smaller key survives."""
    return np.array([(a, b) for a, b, f in W.pairs[kind] if f], np.uint64).reshape(-1, 2)


def drop_map(rows_by_kind):
    """{kind: (keep, drop) rows} -> Rekey's map."""
    return {(CLS[kind], int(d)): int(k) for kind, rows in rows_by_kind.items() for k, d in rows}


def dup40_truth(W):
    """Where dup40 put its objects: {(kind, k): xyz / root}, its own draws repeated."""
    rng = np.random.default_rng(103)
    out = {}
    for k in range(0, 34, 3):
        out["point", k] = gg.around(W, k, rng)
        if k % 6 == 0:
            out["cylinder", k] = gg.around(W, k, rng)
    out["point", lp.REVISIT[0]] = gg.around(W, 1, rng)
    return out


def extra_frame(W, k):
    """Key frame k behind dup40's last: odometry on an extended ground truth, then observations of the DROPPED keys 133 (point) and,
    at odd k, 130 (cylinder, exists=True) and of the distinct point 233.  Deterministic in k, so every graph of a test gets the same
    calls."""
    assert k == len(W.T)
    truth = dup40_truth(W)
    rng = np.random.default_rng([77, k])
    R, t = W.T[k - 1]
    Rn = R @ gg.rot(rng.normal(0, 0.15, 3))
    tn = t + Rn @ np.array([1.0, 0.1 * rng.normal(), 0.05 * rng.normal()])
    W.T.append((Rn, tn))
    est = gg.p7(Rn @ gg.rot(rng.normal(0, W.noise, 3)), tn + rng.normal(0, W.noise * 5, 3))
    W.G.add_keypose_between(0, k - 1, k, gg.p7(R.T @ Rn, R.T @ (tn - t)), est)
    W.est.append(est)
    for idx, xyz in ((133, truth["point", 33]), (233, truth["point", 33] + lp.OFFSET["point"])):
        q = Rn.T @ (xyz - tn)
        W.G.add_range_bearing(0, k, idx, q / np.linalg.norm(q), float(np.linalg.norm(q)))
    if k % 2:
        W.G.add_cylinder(0, k, 130, est, truth["cylinder", 30], og.RAY, 0.25, True)


# ---- the fusion's reference -------------------------------------------------------------------------------------------------------
def fusion_reference(ref, V, kind, members):
    """x_ref = (sum H_i)^-1 sum H_i est_i over `members` (keys of one class) and the bound's condition numbers.  H_i: the landmark's
    own block of J^T J at the linearisation point V (Reference.linearize); est_i: rows of `est` in tangent order.  -> a function of
    the estimates: est -> (x_ref, bound factor kappa(H_a) + kappa(H_b) + ... + kappa(sum)), members without factors left out."""
    i, j, v, r = ref.linearize(V)
    J = np.zeros((len(r), ref.n))
    np.add.at(J, (i, j), v)
    Hs = {}
    for m in members:
        k = ref.lm_var(CLS[kind], int(m))
        cols = np.arange(ref.off[k], ref.off[k + 1])
        Hs[int(m)] = J[:, cols].T @ J[:, cols]

    def at(est):
        D = DIM[kind]
        A, b, kap = np.zeros((D, D)), np.zeros(D), 0.0
        for m in members:
            H = Hs[int(m)]
            if not H.any():
                continue
            A += H
            b += H @ lp.tangent(kind, est[int(m)])
            kap += np.linalg.cond(H)
        x = np.linalg.solve(A, b)
        return x, kap + np.linalg.cond(A)
    return at


def fusion_bound(kind, kappas, x_ref):
    """32 D eps (kappa(H_a) + kappa(H_b) + kappa(H_a + H_b)) max(1, |x_ref|_inf): the forward error of two D x D inversions and one
    solve."""
    return 32 * DIM[kind] * EPS * kappas * max(1.0, float(np.abs(x_ref).max()))
