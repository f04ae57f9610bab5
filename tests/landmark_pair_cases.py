"""The duplicate-landmark queries (slide_graph_landmark_pair_mahalanobis / _get_landmark_pair_covariances / slide_pairs_within): the
dense reference and the case generators (test infrastructure for test_landmark_pair_host.py and test_gpu_landmark_pairs.py; not a
test).

The reference is built as observation_gate_cases builds its own: Sigma is the dense inverse of the full, unreduced H of
tests/gn_reference.py at the linearisation point (test_gpu_marginals.dense_inverse, with its tolerance `tol` and `kappa`); for a pair
(a, b) of one class
    Sig_d = Sig_aa + Sig_bb - Sig_ab - Sig_ba  from the four blocks,
    d     = value_b - value_a in the class's tangent order (point xyz; cylinder [ray, root, radius]) at the values given,
    C_ref = I + diag(1 / sigma) Sig_d diag(1 / sigma),   r = d / sigma,   d2_ref = r^T C_ref^-1 r.
schur_form restates the device's route in numpy (H_ll^-1, F = E H_ll^-1, B over the reduced pose system) and is checked against C_ref
in test_landmark_pair_host.py.  Everything here runs without a device; the GPU tests evaluate the same pairs at the values read back
with get_landmark.

The graph dup40 is planted40's trajectory with, every third pose k up to 33: point k seen from poses k, k + 1; point 100 + k AT THE
SAME PLACE seen from k + 2, k + 3 (a true duplicate: the object lost its match and was initialised again); point 200 + k 0.6 m to the
side seen from k, k + 1, k + 2 (a distinct object); every sixth pose the same three as cylinders; and a revisit, point 900 seen from
poses 1, 2 and point 901 at the same place seen from 37, 38."""
from __future__ import annotations

import numpy as np

import closure_cases as cc
import closure_gate_cases as cg
import gn_graphs as gg
import observation_gate_cases as og
from oracle import pyoracle as po

BR_SIGMA, CYL_SIGMA = 0.02, 0.1
# the hypothesis' model noise: two fits of one object differ by centimetres
SIGMA = {"point": np.full(3, 0.05), "cylinder": np.array([0.02, 0.02, 0.02, 0.05, 0.05, 0.05, 0.02])}
CLS = {"point": 2, "cylinder": 0, "cube": 1}
DIM = {"point": 3, "cylinder": 7, "cube": 9}
OFFSET = {"point": np.array([0.0, 0.6, 0.0]), "cylinder": np.array([0.6, 0.0, 0.0])}
REVISIT = (900, 901)


def dup40(g):
    W = gg.World(cg.NoisyOdom(g, cc.ODOM_SIGMA6, cg.NOISY_SEED), 40, seed=3, noise=0.002)
    rng = np.random.default_rng(103)
    W.pairs = {"point": [], "cylinder": []}       # (a, b, True: one object)
    for k in range(0, 34, 3):
        xyz = gg.around(W, k, rng)
        W.point(k, xyz, [k, k + 1])
        W.point(100 + k, xyz, [k + 2, k + 3])
        W.point(200 + k, xyz + OFFSET["point"], [k, k + 1, k + 2])
        W.pairs["point"] += [(k, 100 + k, True), (k, 200 + k, False), (100 + k, 200 + k, False)]
        if k % 6 == 0:
            root = gg.around(W, k, rng)
            W.cylinder(k, root, og.RAY, 0.25, [k, k + 1])
            W.cylinder(100 + k, root, og.RAY, 0.25, [k + 2, k + 3])
            W.cylinder(200 + k, root + OFFSET["cylinder"], og.RAY, 0.25, [k, k + 1, k + 2])
            W.pairs["cylinder"] += [(k, 100 + k, True), (k, 200 + k, False), (100 + k, 200 + k, False)]
    xyz = gg.around(W, 1, rng)
    W.point(REVISIT[0], xyz, [1, 2])
    W.point(REVISIT[1], xyz, [37, 38])
    W.pairs["point"].append((REVISIT[0], REVISIT[1], True))
    return W


og.GRAPHS["dup40"] = (dup40, dict(odom_sigma=list(cc.ODOM_SIGMA6), bearing_sigma=BR_SIGMA, cyl_sigma=CYL_SIGMA),
                      dict(noise_model_odom_vec=list(cc.ODOM_SIGMA6), bearing_range_sigma=BR_SIGMA, cylinder_sigma=CYL_SIGMA))


def case(name, chart):
    return og.case(name, chart)


def device_graph(gpu, name, chart, solve=True):
    return og.device_graph(gpu, name, chart, solve)


def tangent(kind, v):
    """A landmark's value (get_landmark / the reference) in its tangent order: point xyz; cylinder [root, ray, radius] -> [ray, root,
    radius]."""
    v = np.asarray(v, float)
    return v[:3].copy() if kind == "point" else np.concatenate([v[3:6], v[:3], v[6:7]])


def cols(c, kind, idx):
    k = c.ref.lm_var(CLS[kind], idx)
    return np.arange(c.ref.off[k], c.ref.off[k + 1])


def ref_joint_cov(c, kind, a, b):
    """[[Saa, Sab], [Sba, Sbb]] off the dense inverse."""
    sel = np.concatenate([cols(c, kind, a), cols(c, kind, b)])
    return c.Sig[np.ix_(sel, sel)]


def ref_pairs(c, kind, pairs, vals, sigma=None):
    """Lists r, C_ref and the array d2_ref of the pairs (a, b) of one class at vals."""
    sg = SIGMA[kind] if sigma is None else np.asarray(sigma, float)
    D = DIM[kind]
    rs, Cs, d2 = [], [], np.zeros(len(pairs))
    for k, (a, b) in enumerate(pairs):
        S = ref_joint_cov(c, kind, int(a), int(b))
        Sd = S[:D, :D] + S[D:, D:] - S[:D, D:] - S[D:, :D]
        r = (tangent(kind, vals.lm(kind, int(b))) - tangent(kind, vals.lm(kind, int(a)))) / sg
        Cm = np.eye(D) + Sd / np.outer(sg, sg)
        rs.append(r); Cs.append(Cm)
        d2[k] = r @ np.linalg.solve(Cm, r)
    return rs, Cs, d2


def planted(c, kind, vals=None):
    """dup40's pairs of one class -> (pairs (n, 2), flags (True: one object), d2_ref, distances).  Asserted here, under d2_ref alone:
    every true pair lies below 0.25 of the 0.99 quantile of its D (2.84 / 4.62), every distinct pair above 1.5 of it (17.0 / 27.7)."""
    assert c.name == "dup40"
    vals = vals or c.cpu_values
    rows = c.world.pairs[kind]
    pairs = np.array([(a, b) for a, b, _ in rows], np.uint64)
    flags = np.array([f for _, _, f in rows])
    _, _, d2 = ref_pairs(c, kind, pairs, vals)
    q = og.QUANTILE[DIM[kind]]
    assert (d2[flags] < 0.25 * q).all() and (d2[~flags] > 1.5 * q).all(), (kind, d2 / q, flags)
    dist = np.array([np.linalg.norm(np.asarray(vals.lm(kind, int(b)), float)[:3] - np.asarray(vals.lm(kind, int(a)), float)[:3]) for a, b in pairs])
    return pairs, flags, d2, dist


def schur_form(c, kind, a, b, sigma=None):
    """C by the route the device takes, in numpy: with J the reference's whitened Jacobian at the linearisation point, Hinv_l the
    inverse of the landmark's own block of H, F_f = (Jp_f^T Jl_f) Hinv_l, S the pose system with EVERY landmark eliminated and
    Al = -I / sigma on a, +I / sigma on b,
        C = I + Al_a Hinv_a Al_a^T + Al_b Hinv_b Al_b^T + B^T S^-1 B,   B = - sum_{l in a, b} sum_{f in factors(l)} P_{p_f}^T F_f Al_l^T."""
    ref = c.ref
    sg = SIGMA[kind] if sigma is None else np.asarray(sigma, float)
    D = DIM[kind]
    if not hasattr(c, "_pair_schur"):          # (the graph's own part, once per case)
        i, j, v, res = ref.linearize()
        J = np.zeros((len(res), ref.n))
        np.add.at(J, (i, j), v)
        row0 = np.concatenate([[0], np.cumsum([og.ROWS[int(t)] for t in ref.ftype])])
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
        c._pair_schur = (J, row0, pcols, prow, H, S)
    J, row0, pcols, prow, H, S = c._pair_schur
    Cm = np.eye(D)
    B = np.zeros((len(pcols), D))
    for idx, Al in ((a, -np.diag(1.0 / sg)), (b, np.diag(1.0 / sg))):
        vl = ref.lm_var(CLS[kind], int(idx))
        lc = np.arange(ref.off[vl], ref.off[vl + 1])
        Hinv = np.linalg.inv(H[np.ix_(lc, lc)])
        Cm += Al @ Hinv @ Al.T
        for f in np.flatnonzero(ref.fv[:, 1] == vl):
            if int(ref.ftype[f]) not in (po.F_BR, po.F_CUBE, po.F_CYL):
                continue
            rows = np.arange(row0[f], row0[f + 1])
            q = int(ref.fv[f, 0])
            E = J[np.ix_(rows, np.arange(ref.off[q], ref.off[q + 1]))].T @ J[np.ix_(rows, lc)]
            B[prow[q]:prow[q] + 6] -= (E @ Hinv) @ Al.T
    return Cm + B.T @ np.linalg.solve(S, B)


# ---- the fixed-radius search ------------------------------------------------------------------------------------------------------
def brute_pairs(xyz, radius, labels=None):
    """Every i < j with |x_i - x_j| <= radius (and equal labels), sorted by (i, j), with the distances: numpy, in double, the sum
    taken as (dx dx + dy dy) + dz dz."""
    xyz = np.asarray(xyz, float).reshape(-1, 3)
    n = len(xyz)
    d = xyz[:, None, :] - xyz[None, :, :]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    keep = np.triu(np.ones((n, n), bool), 1) & (dist <= radius)
    if labels is not None:
        lab = np.asarray(labels)
        keep &= lab[:, None] == lab[None, :]
    i, j = np.nonzero(keep)
    return i.astype(np.int32), j.astype(np.int32), dist[i, j]


def clear_radius(xyz, radius):
    """The radius itself, after asserting that no distance of the set lies within 1e-9 relative of it (a device that contracted the
    products could decide such a pair the other way)."""
    xyz = np.asarray(xyz, float).reshape(-1, 3)
    if len(xyz) > 1:
        d = np.linalg.norm(xyz[:, None, :] - xyz[None, :, :], axis=2)[np.triu_indices(len(xyz), 1)]
        assert (np.abs(d - radius) > 1e-9 * radius).all(), radius
    return radius


SEARCH_SIZES = (0, 1, 2, 63, 64, 65, 257)


def search_points(n, seed=11):
    """n points in a 4 m cube (radius 1: about 5% of the pairs), two of them coincident from n = 2 on; labels of three kinds."""
    rng = np.random.default_rng([seed, n])
    xyz = rng.uniform(0.0, 4.0, (n, 3))
    if n >= 2:
        xyz[n - 1] = xyz[0]
    return xyz, rng.integers(0, 3, n).astype(np.int32)
