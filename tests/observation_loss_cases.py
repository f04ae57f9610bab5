"""A robust (iteratively reweighted) Gauss-Newton step on the LANDMARK OBSERVATION factors in numpy, on top of tests/gn_reference.py,
and the graphs the observation-loss tests share (test infrastructure for test_observation_loss_reference.py and
test_gpu_observation_loss.py).  No product code is involved.

The rule (GTSAM's noiseModel::Robust::WhitenSystem): for a selected landmark factor with m rows (bearing-range 3, cube 9, cylinder 7),
s = |r|_2 of its whitened residual r at the linearisation point (Reference.linearize), w = mEstimator::weight(s) (robust_cases.weight),
and the factor enters the step as sqrt(w) [r | J]: its sigmas fsig[f, :m] divided by sqrt(w).  Selected: mask bit 0 the bearing-range
factors, bit 1 the cubes, bit 2 the cylinders.  A closure loss (robust_cases) may be applied in the same step."""
from __future__ import annotations

import numpy as np

import gn_graphs as gg
import robust_cases as rc
from gn_reference import Reference
from oracle import pyoracle as po

BIT = {po.F_BR: 0, po.F_CUBE: 1, po.F_CYL: 2}
CLS_OF = {po.F_BR: 2, po.F_CUBE: 1, po.F_CYL: 0}        # SLIDE_CLS_* of the factor's landmark: cylinder 0, cube 1, ellipsoid / point 2
SIGMA = 0.05                                            # bearing_range_sigma and cylinder_sigma of the cases that need residuals past a kink
W_KEPT = 1e-3                                           # "an inlier on every landmark": some observation of it keeps at least this weight


def params(chart=0):
    """(oracle parameters, keyword arguments of the product's default_params) with both sigmas at SIGMA."""
    return (po.OrcParams.default(pose_chart=chart, bearing_sigma=SIGMA, cyl_sigma=SIGMA),
            dict(pose_chart=chart, bearing_range_sigma=SIGMA, cylinder_sigma=SIGMA))


def lf_index(ref):
    """The landmark factors of the export, in insertion order (the order of slide_graph_get_observation_weights)."""
    return np.flatnonzero(np.isin(ref.ftype, list(BIT)))


def selected(ref, mask=7):
    return np.array([int(t) in BIT and bool((mask >> BIT[int(t)]) & 1) for t in ref.ftype])


def factor_keys(ref):
    """(robot, pose_idx, cls, lm_idx) of every landmark factor, insertion order."""
    out = []
    for f in lf_index(ref):
        kp, kl = int(ref.vkey[ref.fv[f, 0]]), int(ref.vkey[ref.fv[f, 1]])
        out.append(("xyzmnopqrstvw".index(chr(kp >> 56)), kp & ((1 << 56) - 1), CLS_OF[int(ref.ftype[f])], kl & ((1 << 56) - 1)))
    return out


def obs_step(ref, values, kind, param, sel, closure=None):
    """One reweighted step at `values` -> (dx, H, w per factor (1 where no loss applies), s^2 per factor, numdiff floor).
    closure: (kind, param, selection) of robust_cases' loss on the between factors, applied as well."""
    from test_gn_reference import numdiff_floor
    s2 = rc.whitened_norms2(ref, values)
    w = np.ones(len(ref.ftype))
    if kind:
        w[sel] = rc.weight(kind, param, np.sqrt(s2[sel]))
    if closure is not None and closure[0]:
        w[closure[2]] = rc.weight(closure[0], closure[1], np.sqrt(s2[closure[2]]))
    base = ref.fsig
    ref.fsig = base / np.sqrt(w)[:, None]      # (every row of the factor; unused columns do not matter)
    try:
        dx, H = ref.step(values)
        floor = numdiff_floor(ref, dx, H, values)
    finally:
        ref.fsig = base
    return dx, H, w, s2, floor


def obs_irls(ref, kind, param, sel, steps, values=None):
    """`steps` reweighted steps from `values` -> (values, weights of the last step's linearisation, per-step (dx, H))."""
    vals = ref.values if values is None else values
    w, trace = np.ones(len(ref.ftype)), []
    for _ in range(steps):
        dx, H, w, _, _ = obs_step(ref, vals, kind, param, sel)
        trace.append((dx, H))
        vals = ref.retract(vals, dx)
    return vals, w, trace


def landmarks_keep_an_inlier(ref, w):
    """Every landmark has an observation of weight >= W_KEPT: none is left to the floor, where H_ll would be of order 1e-12."""
    best = {}
    for f in lf_index(ref):
        l = int(ref.fv[f, 1])
        best[l] = max(best.get(l, 0.0), float(w[f]))
    return all(v >= W_KEPT for v in best.values())


# ---- graphs ------------------------------------------------------------------------------------------------------------------------

def _point_obs(G, W, k, idx, xyz, d_rng=0.0):
    R, t = W.T[k]
    q = R.T @ (np.asarray(xyz, float) - t)
    G.add_range_bearing(0, k, idx, q / np.linalg.norm(q), float(np.linalg.norm(q)) + d_rng)


RAY = np.array([0.0, 0.05, 1.0]) / np.linalg.norm([0.0, 0.05, 1.0])
CUBE_SCALE = np.array([0.8, 1.5, 0.6])
# whitened norms planted in mixed_graph: just below / past DCS's kink s^2 = 1 and Huber's k = 1.345, and a gross one
TARGETS = (0.97, 1.03, 1.3, 1.4, 60.0)


def mixed_graph(G, cube_sigma6=None, P=12, seed=41):
    """A P-pose chain, poses 0 .. 7 exact and the rest perturbed (so the step moves the chain), with a point, a cube and a cylinder
    landmark at poses 0, 2, 4, 6, interleaved, each seen from three consecutive poses and created exact.  (None hangs on the
    perturbed tail alone: with landmarks at pose 8 the numpy step itself moved by 1.6 times its tolerance under a one-ulp change of the
    linearisation point at the third Cauchy step; test_observation_loss_reference.py keeps that figure below a quarter.)  Observations of the landmarks
    at poses 0 .. 5 from exact poses are moved so that their whitened norms are TARGETS: a point's range, a cylinder's radius (both
    under SIGMA), a cube's first scale (under the sigma the graph chose for that factor: cube_sigma6[idx], read from a first
    build's export — fsig[f, 6]; None: no cube is moved).  -> (world, {factor number among the landmark factors: target})."""
    W = gg.World(G, P, seed=seed, noise=0.0, perturb={k: [0.03, -0.02, 0.01] for k in range(8, P)})
    rng = np.random.default_rng(seed + 100)
    plan = {("point", 0, 1): TARGETS[0], ("point", 0, 2): TARGETS[3], ("point", 2, 3): TARGETS[4], ("point", 4, 5): TARGETS[1],
            ("cyl", 0, 1): TARGETS[1], ("cyl", 2, 4): TARGETS[2], ("cyl", 4, 6): TARGETS[4],
            ("cube", 0, 2): TARGETS[3], ("cube", 2, 3): TARGETS[0], ("cube", 4, 5): TARGETS[4]}
    planted, nf = {}, 0
    lms = []
    for k in range(0, 8, 2):
        lms.append((k, gg.around(W, k, rng), gg.around(W, k, rng), gg.around(W, k, rng), gg.rot([0.1, 0.2, rng.uniform(-3, 3)])))
    for k, pxyz, cxyz, yxyz, cR in lms:
        G.add_point_landmark(k, pxyz)
    for n in range(3):                                    # observation n of every landmark: the classes alternate factor by factor
        for k, pxyz, cxyz, yxyz, cR in lms:
            j = k + n
            t = plan.get(("point", k, j), 0.0)
            _point_obs(G, W, j, k, pxyz, t * SIGMA)
            if t:
                planted[nf] = t
            nf += 1
            t = plan.get(("cube", k, j), 0.0) if cube_sigma6 is not None else 0.0
            ds = np.array([t * cube_sigma6[k, j], 0.0, 0.0]) if t else 0.0
            G.add_cube(0, j, k, W.est[j], gg.p7(cR, cxyz), CUBE_SCALE + ds, n > 0)
            if t:
                planted[nf] = t
            nf += 1
            t = plan.get(("cyl", k, j), 0.0)
            G.add_cylinder(0, j, k, W.est[j], yxyz, RAY, 0.25 + t * SIGMA, n > 0)
            if t:
                planted[nf] = t
            nf += 1
    return W, planted


def mixed_cube_sigmas(chart=0):
    """fsig[f, 6] of every cube factor of mixed_graph, by (cube idx, pose idx): the sigma of the scale row a planted cube moves."""
    og = po.OracleGraph(params(chart)[0])
    mixed_graph(og)
    ref = Reference(og, chart)
    out = {}
    for (_, pidx, cls, lidx), f in zip(factor_keys(ref), lf_index(ref)):
        if cls == 1:
            out[lidx, pidx] = float(ref.fsig[f, 6])
    return out


def br_edge_graph(G, N, seed=42):
    """Exactly N bearing-range factors: six poses (slightly perturbed: every factor has a small residual) see up to 86 points in
    turn.  The factors first, last and on both sides of every 256-boundary below N measure a range 0.1 .. 0.2 m off.
    -> the moved factors' numbers."""
    moved = sorted({0, N - 1} | {q for b in (256, 512) for q in (b - 1, b) if q < N})
    W = gg.World(G, 6, seed=seed, noise=0.002, step=0.5)
    rng = np.random.default_rng(seed + 100)
    q = 0
    for l in range(-(-N // 6)):
        xyz = gg.around(W, l % 6, rng)
        G.add_point_landmark(l, xyz + rng.normal(0, 0.002, 3))
        for k in range(6):
            if q == N:
                break
            _point_obs(G, W, k, l, xyz, (0.1 + 0.02 * (q % 5)) if q in moved else 0.0)
            q += 1
    return moved


def nbr_edge_graph(G, n_nbr, seed=43):
    """Exactly n_nbr cube / cylinder factors (alternating), each behind a bearing-range factor: the 32-lane region runs over the list
    of the former (eight per workgroup), the one-thread region over all factors.  Cube / cylinder q // 12 is seen from pose
    (q // 2) % 6; created 0.01 m off, so every later observation of it has a residual (the first one creates the landmark from
    its own measurement and has none).  The factors first, last and on both sides of the workgroup boundaries measure a scale / a
    radius 0.05 off.  -> the moved factors' numbers among the landmark factors."""
    moved_q = sorted({0, n_nbr - 1} | {q for q in (7, 8, 15, 16) if q < n_nbr})
    W = gg.World(G, 6, seed=seed, noise=0.002, step=0.5)
    rng = np.random.default_rng(seed + 100)
    spec = {}
    moved = []
    for q in range(n_nbr):
        k, i, cyl = (q // 2) % 6, q // 12, q % 2 == 1
        pxyz = gg.around(W, k, rng)
        G.add_point_landmark(q, pxyz + rng.normal(0, 0.002, 3))
        _point_obs(G, W, k, q, pxyz, 0.01)
        new = (cyl, i) not in spec
        if new:
            spec[cyl, i] = (gg.around(W, 0, rng), gg.rot([0.1, 0.2, rng.uniform(-3, 3)]))
        xyz, cR = spec[cyl, i]
        off = np.array([0.01, -0.01, 0.01]) if new else 0.0
        d = 0.05 if q in moved_q else 0.0
        if cyl:
            G.add_cylinder(0, k, i, W.est[k], xyz + off, RAY, 0.25 + d, not new)
        else:
            G.add_cube(0, k, i, W.est[k], gg.p7(cR, xyz + off), CUBE_SCALE + np.array([d, 0.0, 0.0]), not new)
        if q in moved_q:
            moved.append(2 * q + 1)
    return moved


def both_graph(G, P=44, seed=44):
    """robust_cases.chain_graph at P poses (closures with whitened norms 0.3 .. 3000; five block columns, so repeated steps replay a
    captured pass) plus point landmarks on the exact poses 0 .. 7, one of them with a gross observation.  -> the gross factor's
    number among the landmark factors."""
    W = rc.chain_graph(G, P, seed)
    rng = np.random.default_rng(seed + 100)
    nf, gross = 0, None
    for l in range(4):
        xyz = gg.around(W, 2 * l, rng)
        G.add_point_landmark(l, xyz)
        for k in (2 * l, 2 * l + 1, (2 * l + 2) % 8):
            bad = l == 1 and k == 3
            _point_obs(G, W, k, l, xyz, 2.0 if bad else 0.01 * (k + 1))
            if bad:
                gross = nf
            nf += 1
    return gross


# ---- the planted scenario ----------------------------------------------------------------------------------------------------------
PLANTED_STEPS = 8
PLANTED_PARAM = {rc.GEMAN_MCCLURE: 3.0, rc.DCS: 9.0}
PLANTED_LMS = (2, 8, 14, 20, 26, 32)


def planted_graph(G, seed=31):
    """A 24-pose chain (gn_graphs.World, noise 0.01) and 36 point landmarks, landmark l near pose k0 = (l 24) // 36 and seen from the
    four poses k0 - 1 .. k0 + 2 (those that exist) with noise of 0.01 m on the measured point.  The third observation of
    landmarks PLANTED_LMS measures landmark l + 1 instead: a false match of the data association between neighbours.
    -> (ground-truth poses, the false observations' numbers among the landmark factors)."""
    W = gg.World(G, 24, seed=seed, noise=0.01)
    rng = np.random.default_rng(seed + 103)      # (the map's generator: one for which the numpy reference alone holds every condition
    #                                               of the tests with a margin — test_observation_loss_reference.py prints the figures)
    xyz = [gg.around(W, (l * 24) // 36, rng) for l in range(36)]
    bad, nf = [], 0
    for l in range(36):
        G.add_point_landmark(l, xyz[l] + rng.normal(0, 0.01, 3))
        k0 = (l * 24) // 36
        obs = [k for k in range(k0 - 1, k0 + 3) if 0 <= k < 24]
        for n, k in enumerate(obs):
            false = l in PLANTED_LMS and n == 2
            R, t = W.T[k]
            q = R.T @ (xyz[l + 1 if false else l] - t) + rng.normal(0, 0.01, 3)
            G.add_range_bearing(0, k, l, q / np.linalg.norm(q), float(np.linalg.norm(q)))
            if false:
                bad.append(nf)
            nf += 1
    return W.T, bad


def planted_reference(kind, chart=0, seed=31):
    """The numpy IRLS on the planted scenario -> dict(ref, sel, T, bad, values, w (per landmark factor), trace, param)."""
    og = po.OracleGraph(params(chart)[0])
    T, bad = planted_graph(og, seed)
    ref = Reference(og, chart)
    sel = selected(ref)
    param = PLANTED_PARAM.get(kind, 0.0)
    vals, w, trace = obs_irls(ref, kind, param, sel, PLANTED_STEPS)
    return dict(ref=ref, sel=sel, T=T, bad=bad, values=vals, w=w[lf_index(ref)], trace=trace, param=param)
