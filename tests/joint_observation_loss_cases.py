"""Multi-robot graphs with displaced (false) landmark observations and the reweighted joint Gauss-Newton step in numpy (test
infrastructure for test_joint_observation_loss_reference.py and test_gpu_joint_observation_loss.py).  No product code is involved.

The reweighted joint step is observation_loss_cases.obs_step applied to the joint graph's Reference (the selection from
observation_loss_cases.selected, optionally with joint_robust_cases' closure loss in the same step).  test_joint_reference's
joint_reference fixes the default sigmas; residuals have to reach past the losses' kinks, so reference() and the shards of the GPU
harness are built with observation_loss_cases.params(chart): bearing_range_sigma = cylinder_sigma = 0.05.

ObsJoint is joint_robust_cases.RobustJoint (closures may take part) whose landmarks start close to the truth (LM_NOISE), so that a
whitened norm is what the builder plants, plus move(): observation n of a landmark measures a range (point), a radius (cylinder) or
a first scale (cube) that is off by d.  The joint graph and the shards receive the same moved measurement, so both hold the same
factor."""
from __future__ import annotations

import numpy as np

import gn_graphs as gg
import joint_graphs as jg
import joint_robust_cases as jr
import observation_loss_cases as oc
import robust_cases as rc
from gn_reference import Reference
from oracle import pyoracle as po

SIGMA = oc.SIGMA
CUBE_SIGMA = 0.6         # a cube factor's sigma at the distances of these cases, about (0.4 .. 1.0)
TIGHT = 2.0              # observations moved by this many sigmas or more keep s >= 1 along every sequence of the tests: their s^2 is compared at rtol alone
LM_NOISE = 0.01          # a point's initial value: 0.2 sigma per coordinate off the truth
POSE_NOISE = 0.002       # gn_graphs.World's: the initial poses are off by 0.002 rad and 0.01 m (0.2 sigma)


class ObsJoint(jr.RobustJoint):
    def __init__(self, sizes, seed=0, spacing=4.0, step=1.0, noise=POSE_NOISE, cube_sigma=None):
        super().__init__(sizes, seed, spacing, step, noise)
        self.moved = []          # (cls, gid, call number, whitened displacement)
        self.cube_sigma = cube_sigma or {}      # (gid, call number) -> the sigma the graph chose for that cube factor (two_pass)

    def _offsets(self, robots):
        """Joint._offsets at a fifth of its size: a cube or cylinder starts 0.01 m and 0.004 rad off in every replica."""
        return {r: (gg.rot(self.rng.normal(0, 0.004, 3)), self.rng.normal(0, LM_NOISE, 3)) for r in robots}

    def point(self, xyz, obs):
        g = super().point(xyz, obs)
        spec = self.lms[-1][2]
        for r in spec["init"]:          # (Joint.point starts a point 0.05 m = one sigma per coordinate off)
            spec["init"][r] = np.asarray(xyz, float) + (LM_NOISE / 0.05) * (spec["init"][r] - np.asarray(xyz, float))
        return g

    def move(self, cls, g, n, t):
        """Observation n (in the order given to point / cylinder / cube) of landmark (cls, g) measures t sigmas more: a point's
        range, a cylinder's radius (SIGMA), a cube's first scale (the sigma the graph chose for that factor, which grows with the
        cube's distance: cube_sigma, read from a first build's export by two_pass; CUBE_SIGMA without it).  Not a cube's or
        cylinder's first observation by a robot (it creates the replica)."""
        d = t * (self.cube_sigma.get((g, n), CUBE_SIGMA) if cls == 1 else SIGMA)
        for c, gq, spec, obs in self.lms:
            if c == cls and gq == g:
                call = list(spec["calls"][n])
                if cls == 2:
                    call[3] = call[3] + d
                elif cls == 0:
                    assert not call[6]
                    call[5] = call[5] + d
                else:
                    assert not call[5]
                    call[4] = call[4] + np.array([d, 0.0, 0.0])
                spec["calls"][n] = tuple(call)
                self.moved.append((cls, g, n, t))
                return
        raise KeyError((cls, g))


def two_pass(build):
    """build(cube_sigma) twice: the second time with the cube factors' sigmas (fsig[f, 6], the first scale's) of the first build."""
    J = build(None)
    ref = reference(J)
    key = {k: int(f) for k, f in zip(oc.factor_keys(ref), oc.lf_index(ref))}
    sig = {}
    for cls, g, spec, _ in J.lms:
        if cls == 1:
            for n, call in enumerate(spec["calls"]):
                sig[g, n] = float(ref.fsig[key[call[0], int(call[1]), 1, g], 6])
    return build(sig)


def reference(J, chart=0):
    """test_joint_reference.joint_reference under observation_loss_cases.params."""
    og = po.OracleGraph(oc.params(chart)[0])
    J.emit_joint(og)
    return Reference(og, chart)


# ---- factor order: the batch lists (slot, member insertion order); the joint export has its own ---------------------------------------

def batch_rows(J):
    """What CholBatch.observation_weights lists: per slot the robot's landmark factors in the order its shard receives them
    -> [(slot, pose_idx, cls, local lm_idx, global id)]."""
    gid = J.local_ids()
    rows = []
    for r in range(J.R):
        loc = [{int(g): i for i, g in enumerate(gid[r][cls])} for cls in range(3)]
        for cls, g, spec, obs in J.lms:
            if g not in loc[cls]:
                continue
            for c in spec["calls"]:
                if c[0] == r:
                    rows.append((r, int(c[1]), cls, loc[cls][g], int(g)))
    return rows


def batch_to_export(J, ref):
    """Export factor index of every row of batch_rows, through (robot, pose, class, landmark gid).  A pose observes a landmark at
    most once in every case here, so the key names one factor."""
    key = {}
    for (robot, pidx, cls, lidx), f in zip(oc.factor_keys(ref), oc.lf_index(ref)):
        assert (robot, pidx, cls, lidx) not in key
        key[robot, pidx, cls, lidx] = int(f)
    return np.array([key[r, p, c, g] for (r, p, c, _, g) in batch_rows(J)], int)


def moved_factors(J, ref, at_least=0.0):
    """Export factor index of every observation moved by at_least sigmas or more."""
    out = []
    key = {k: int(f) for k, f in zip(oc.factor_keys(ref), oc.lf_index(ref))}
    for cls, g, n, t in J.moved:
        if t < at_least:
            continue
        for c, gq, spec, _ in J.lms:
            if c == cls and gq == g:
                call = spec["calls"][n]
                out.append(key[call[0], int(call[1]), cls, g])
    return np.array(out, int)


def shared_landmarks(J):
    return [(cls, g) for cls, g, _, obs in J.lms if len({r for r, _ in obs}) > 1]


def steps(ref, kind, param, sel, n, values=None, closure=None):
    """n reweighted joint steps from `values` -> [(values the step starts from, dx, H, w, s2, floor)], final values."""
    vals = ref.values if values is None else values
    out = []
    for _ in range(n):
        dx, H, w, s2, floor = oc.obs_step(ref, vals, kind, param, sel, closure)
        out.append((vals, dx, H, w, s2, floor))
        vals = ref.retract(vals, dx)
    return out, vals


# ---- (a) the kinds ------------------------------------------------------------------------------------------------------------------
# whitened displacements planted on top of the 0.2 .. 0.5 sigma the initial values are off by: around DCS's kink s^2 = 1 and Huber's
# k = 1.345, past both, and gross
TARGETS = (0.9, 1.1, 1.3, 1.5, 3.0, 40.0)


def kinds_case(seed=51, P=12, extra=None):
    """2 robots of P poses.  Per robot a private point, cube and cylinder and a point, cube and cylinder shared with the other robot
    (seen three times by the robot, twice by the other), every one with a moved observation - TARGETS in turn, in sigmas of 0.05 -
    and one shared POINT per robot whose observation by the OTHER robot is gross: a down-weighted observation of a shared landmark
    in each robot.  Every landmark keeps unmoved observations."""
    return two_pass(lambda sig: _kinds(seed, P, sig, extra))


def _kinds(seed, P, sig, extra):
    J = ObsJoint([P, P], seed=seed, cube_sigma=sig)
    rng = np.random.default_rng(seed)
    n = 0
    for r in range(2):
        o = 1 - r
        for cls in range(3):
            k = 1 + 3 * cls
            g = jg._add(J, cls, jg._near(J, r, k, rng), [(r, k), (r, k + 1), (r, k + 2), (r, k + 3)], rng)
            J.move(cls, g, 2, TARGETS[n % 6])
            n += 1
            g = jg._add(J, cls, jg._near(J, r, k + 1, rng, 7.0), [(r, k), (r, k + 1), (r, k + 2), (o, k + 1), (o, k + 2)], rng)
            J.move(cls, g, 1, TARGETS[n % 6])
            J.move(cls, g, 4, TARGETS[(n + 3) % 6])          # (the other robot's second observation of it)
            n += 1
        g = J.point(jg._near(J, r, 9, rng), [(r, 8), (r, 9), (r, 10), (o, 9)])
        J.move(2, g, 3, 40.0)
    jg.background(J, rng, every=4)
    if extra is not None:
        extra(J)
    return J


def members_case(R, seed=55, P=10):
    """R robots of P poses (R = 1: a plain batched pass, no separator; R = 3: no dissection): per robot a point, a cube and a
    cylinder seen four times, with R > 1 once more from the next robot, the third observation moved (TARGETS in turn)."""
    return two_pass(lambda sig: _members(R, seed, P, sig))


def _members(R, seed, P, sig):
    J = ObsJoint([P] * R, seed=seed, cube_sigma=sig)
    rng = np.random.default_rng(seed)
    n = 0
    for r in range(R):
        for cls in range(3):
            k = 1 + 2 * cls
            obs = [(r, k), (r, k + 1), (r, k + 2), (r, k + 3)] + ([((r + 1) % R, k + 1)] if R > 1 else [])
            g = jg._add(J, cls, jg._near(J, r, k, rng), obs, rng)
            J.move(cls, g, 2, TARGETS[(n + 2) % 6])
            n += 1
    jg.background(J, rng, every=4)
    return J


# ---- (b) edges of the two regions of the linearisation launch, on one member ----------------------------------------------------------
EDGES = [(1, 1), (255, 7), (256, 8), (257, 9), (513, 17)]      # (bearing-range factors, cube / cylinder factors) of robot 0


def edge_case(n_br, n_nbr, seed=52):
    """Robot 0 (6 poses) holds exactly n_br bearing-range factors - one thread each in workgroups of 256 - and n_nbr cube /
    cylinder factors - 32 lanes each, eight per workgroup - interleaved landmark by landmark; the bearing-range factors first, last
    and on both sides of 256 and 512, and the cube / cylinder factors last and on both sides of 8 and 16 (where they create no
    landmark), are moved by 2 .. 3 sigma.  Robot 1 (3 poses) shares robot 0's first point and holds no cube or cylinder (n_nbr = 0);
    robot 2 (3 poses) holds no landmark factor at all; the grid, sized for robot 0, overruns both."""
    return two_pass(lambda sig: _edges(n_br, n_nbr, seed, sig))


def _edges(n_br, n_nbr, seed, sig):
    J = ObsJoint([6, 3, 3], seed=seed, step=0.5, cube_sigma=sig)
    rng = np.random.default_rng(seed)
    br_moved = {0, n_br - 1} | {q for b in (256, 512) for q in (b - 1, b) if q < n_br}
    nbr_moved = {n_nbr - 1} | {q for q in (7, 8, 15, 16) if q < n_nbr}
    g = J.point(jg._near(J, 0, 0, rng), [(0, 0), (1, 0), (1, 1), (1, 2)])
    if 0 in br_moved:
        J.move(2, g, 0, 2.0)
    q_br, q_nbr, j = 1, 0, 0
    while q_br < n_br or q_nbr < n_nbr:
        if q_br < n_br:
            m = min(6, n_br - q_br)
            g = J.point(jg._near(J, 0, j % 6, rng), [(0, (j + i) % 6) for i in range(m)])
            for i in range(m):
                if q_br + i in br_moved:
                    J.move(2, g, i, 2.0 + 0.2 * (i % 5))
            q_br += m
        if q_nbr < n_nbr:
            m = min(4, n_nbr - q_nbr)
            cls = j % 2
            g = jg._add(J, cls, jg._near(J, 0, j % 6, rng, 5.0), [(0, (j + i) % 6) for i in range(m)], rng)
            for i in range(1, m):
                if q_nbr + i in nbr_moved:
                    J.move(cls, g, i, 2.5)
            q_nbr += m
        j += 1
    return J


# ---- (c) both losses ----------------------------------------------------------------------------------------------------------------

def both_case(seed=53, P=12):
    """joint_robust_cases.kinds_case's displaced closures and inter-robot measurements on kinds_case's displaced observations."""
    def extra(J):
        n = 0
        for a, ka, b, kb in ((0, 2, 1, 2), (1, 6, 0, 9)):
            dt, dr = jr._disp(n)
            J.relative(a, ka, b, kb, dt=tuple(3.0 * v for v in dt), drot=tuple(4.0 * v for v in dr))
            n += 1
        for r in range(2):
            dt, dr = jr._disp(n)
            J.closure(r, 1, 7, dt=dt, drot=dr)
            n += 1
    return kinds_case(seed, P, extra)


# ---- (d) the planted scenario ---------------------------------------------------------------------------------------------------------
PLANTED_STEPS = 8
PLANTED_PARAM = {rc.GEMAN_MCCLURE: 3.0, rc.DCS: 9.0}
PLANTED_NOISE = 0.01          # gn_graphs.World's: the initial poses are off by 0.01 rad and 0.05 m
PLANTED_FALSE = 3             # false observations per robot


def planted_case(seed=54, P=20):
    """3 robots of P poses.  A private point near every second pose, seen from three poses.  Between neighbouring robots r and
    r + 1, six shared points in pairs about 2.4 m apart (at 6 m and a bearing sigma of 0.05 rad a
    neighbour one metre to the side stands at 3 sigma only, inside the quadratic part of both losses), each seen twice by either robot.  PLANTED_FALSE observations per robot
    measure the NEIGHBOURING shared point of the pair - the false match the association's gate lets through - in place of a third
    observation; every landmark keeps its true observations.  -> J, with J.false = [(cls, gid, call number)]."""
    J = ObsJoint([P] * 3, seed=seed, noise=PLANTED_NOISE)
    rng = np.random.default_rng(seed)
    J.false = []
    for r in range(3):
        o = (r + 1) % 3
        for i in range(PLANTED_FALSE):
            k = 2 + 6 * i
            a = jg._near(J, r, k, rng)
            b = a + np.array([1.5, -1.8, 0.6])
            obs = [(r, k), (r, k + 1), (o, k), (o, k + 1), (r, k + 2), (o, k + 2)]
            ga = J.point(a, obs)
            gb = J.point(b, obs[:4])
            # robot r's third observation of a measures b: the call's bearing and range are those of b from that pose
            R, t = J.T(r, k + 2)
            q = R.T @ (b - t)
            spec = J.lms[ga][2] if J.lms[ga][1] == ga and J.lms[ga][0] == 2 else None
            assert spec is not None
            call = spec["calls"][4]
            spec["calls"][4] = (call[0], call[1], q / np.linalg.norm(q), float(np.linalg.norm(q)))
            J.false.append((2, ga, 4))
    for r in range(3):
        for k in range(0, P - 2, 2):
            J.point(jg._near(J, r, k, rng, 5.0), [(r, k), (r, k + 1), (r, k + 2)])
    return J


def false_factors(J, ref):
    key = {k: int(f) for k, f in zip(oc.factor_keys(ref), oc.lf_index(ref))}
    out = []
    for cls, g, n in J.false:
        call = J.lms[g][2]["calls"][n]
        out.append(key[call[0], int(call[1]), cls, g])
    return np.array(out, int)


_PLANTED = {}


def planted_reference(kind, chart=0):
    """The numpy IRLS on the planted scenario (computed once per kind) -> dict(J, ref, sel, trace, values, w, plain, bad)."""
    if (kind, chart) not in _PLANTED:
        J = planted_case()
        ref = reference(J, chart)
        sel = oc.selected(ref)
        trace, vals = steps(ref, kind, PLANTED_PARAM.get(kind, 0.0), sel, PLANTED_STEPS)
        _, plain = steps(ref, 0, 0.0, sel, PLANTED_STEPS)
        _PLANTED[(kind, chart)] = dict(J=J, ref=ref, sel=sel, trace=trace, values=vals, w=trace[-1][3], plain=plain,
                                       bad=false_factors(J, ref))
    return _PLANTED[(kind, chart)]
