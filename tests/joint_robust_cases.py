"""Multi-robot graphs with in-robot loop closures and displaced (false) closures / inter-robot measurements, and the reweighted joint
Gauss-Newton step in numpy (test infrastructure for test_joint_robust_reference.py and test_gpu_joint_robust_loss.py).  No product
code is involved.

RobustJoint is joint_graphs.Joint plus add_loop_closure factors, emitted into the joint graph (robot r's as robot r) and into robot
r's shard (as robot 0) with the same measurement, so both hold the same factor.  The joint graph is emitted through
robust_cases.Fan, which notes the origin of every between factor in the export's order: with robust_cases.selected and robust_step
that gives the reweighted joint step on test_joint_reference.joint_reference — the reference of every pass of the GPU tests.

Every selected factor of the cases here carries a residual that no step removes (a displacement of decimetres or more against
sigmas of 1e-3 for closures and 0.1 |t| for inter-robot measurements, or noise of about 1.2 sigma per coordinate on the inter-robot
ones), so its whitened norm stays >= 1 at the points the tests linearise at: s^2 is then no difference of nearly equal numbers and
can be compared at 1e-12 (test_joint_robust_reference.py asserts the norms)."""
from __future__ import annotations

import numpy as np

import gn_graphs as gg
import joint_graphs as jg
import robust_cases as rc
from oracle import pyoracle as po

REL_SIGMA = 0.1            # noise_model_rel_meas_vec: add_relative_meas gives every coordinate 0.1 * max(|t|, noise floor)


class RobustJoint(jg.Joint):
    def __init__(self, sizes, seed=0, spacing=4.0, step=1.0, noise=0.02):
        self.noise = noise              # (gn_graphs.World's: the initial poses are off by noise rad and 5 noise m)
        super().__init__(sizes, seed, spacing, step)
        self.closures = []              # (robot, i, k, rel7)
        self.origin, self.keys = [], []
        self.bt_rel, self.bt_clo = [], []

    def _world(self, G, r, robot):
        return gg.World(G, self.sizes[r], seed=self.seed + 31 * r, step=self.step, origin=(1.0, 2.0 + self.spacing * r, 0.5),
                        robot=robot, noise=self.noise)

    def _rel(self, a, ka, b, kb, dt, drot):
        (Ra, ta), (Rb, tb) = self.T(a, ka), self.T(b, kb)
        R, t = Ra.T @ Rb, Ra.T @ (tb - ta)
        return gg.p7(R @ gg.rot(drot), t + R @ np.asarray(dt, float))

    def closure(self, r, i, k, dt=(0.0, 0.0, 0.0), drot=(0.0, 0.0, 0.0)):
        """Pose i of robot r re-observes pose k of robot r: exact for the ground truth, then moved by drot and dt in k's frame."""
        self.closures.append((r, i, k, self._rel(r, i, r, k, dt, drot)))

    def relative(self, a, ka, b, kb, dt=(0.0, 0.0, 0.0), drot=(0.0, 0.0, 0.0), noise=0.0):
        """Joint.relative, moved by drot and dt in kb's frame; noise: +- noise * sigma on every coordinate, signs alternating."""
        rel = self._rel(a, ka, b, kb, dt, drot)
        if noise:
            sg = noise * REL_SIGMA * np.linalg.norm(rel[:3])
            n = len(self.relmeas)
            sign = np.array([1.0 if (n + j) % 2 == 0 else -1.0 for j in range(6)])
            rel = self._rel(a, ka, b, kb, np.asarray(dt, float) + sg * sign[:3], np.asarray(drot, float) + sg * sign[3:])
        self.relmeas.append((ka, a, b, rel, kb))

    def emit_joint(self, G):
        fan = rc.Fan(G)
        super().emit_joint(fan)
        for r, i, k, rel in self.closures:
            fan.add_loop_closure(rel, i, r, k, r)
        self.origin, self.keys = list(fan.origin), list(fan.keys)
        self.bt_rel = [j for j, o in enumerate(self.origin) if o == 2]       # position among the export's between factors of relmeas[i]
        self.bt_clo = [j for j, o in enumerate(self.origin) if o == 1]       # ... of closures[c]
        assert len(self.bt_rel) == len(self.relmeas) and len(self.bt_clo) == len(self.closures)
        return G

    def emit_shard(self, G, r):
        super().emit_shard(G, r)
        for q, i, k, rel in self.closures:
            if q == r:
                G.add_loop_closure(rel, i, 0, k, 0)
        return G

    # ---- the reference's view -----------------------------------------------------------------------------------------------------
    def factor_rows(self, ref):
        """(export factor index of every relmeas entry, of every closure)."""
        bt = np.flatnonzero(ref.ftype == po.F_BETWEEN)
        return bt[self.bt_rel], bt[self.bt_clo]

    def expected_rows(self, ref):
        """What CholBatch.closure_weights lists: per slot the robot's closures in insertion order, then its ghost factors in the
        order PassDriver.setup_ghosts adds them -> [(slot, from_robot, from_idx, to_robot, to_idx, kind, ghost_id, export factor)];
        the other end of a ghost factor is robot -1 and its ghost slot."""
        rel_f, clo_f = self.factor_rows(ref)
        gkeys = sorted({(a, ka) for (ka, a, b, _, kb) in self.relmeas} | {(b, kb) for (ka, a, b, _, kb) in self.relmeas})
        slot = {key: i for i, key in enumerate(gkeys)}
        rows = []
        for r in range(self.R):
            for c, (q, i, k, _) in enumerate(self.closures):
                if q == r:
                    rows.append((r, 0, i, 0, k, 1, -1, int(clo_f[c])))
            for g, (ka, a, b, _, kb) in enumerate(self.relmeas):
                if a == r:
                    rows.append((r, 0, ka, -1, slot[(b, kb)], 2, g, int(rel_f[g])))
                if b == r:
                    rows.append((r, -1, slot[(a, ka)], 0, kb, 2, g, int(rel_f[g])))
        return rows


def selection(J, ref, mask=3):
    return rc.selected(ref, J.origin, mask)


def steps(J, ref, kind, param, mask, n, values=None):
    """n reweighted joint steps from `values` -> [(values the step starts from, dx, H, w, s2, floor)], final values."""
    sel = selection(J, ref, mask)
    vals = ref.values if values is None else values
    out = []
    for _ in range(n):
        dx, H, w, s2, floor = rc.robust_step(ref, vals, kind, param, sel)
        out.append((vals, dx, H, w, s2, floor))
        vals = ref.retract(vals, dx)
    return out, vals


# ---------------------------------------------------------------------------------------------------------------------------------
# cases.  Displacements: decimetres and tenths of a radian, different for every factor.

def _disp(n):
    return (0.3 + 0.07 * (n % 5), -0.2 + 0.05 * (n % 3), 0.1), (0.02, -0.03 * (n % 2), 0.08 + 0.02 * (n % 4))


def kinds_case(seed=31):
    """2 robots of 14 poses, 3 inter-robot measurements (both directions of first key), 2 in-robot closures per robot."""
    J = RobustJoint([14, 14], seed=seed)
    rng = np.random.default_rng(seed)
    n = 0
    for a, ka, b, kb in ((0, 2, 1, 2), (1, 6, 0, 9), (0, 11, 1, 8)):
        dt, dr = _disp(n)
        J.relative(a, ka, b, kb, dt=tuple(3.0 * v for v in dt), drot=tuple(4.0 * v for v in dr))
        n += 1
    for r in range(2):
        for i, k in ((1, 7), (4, 12)):
            dt, dr = _disp(n)
            J.closure(r, i, k, dt=dt, drot=dr)
            n += 1
    for r in range(2):
        for cls in range(3):
            jg._add(J, cls, jg._near(J, r, 3 + cls, rng), [(r, 3 + cls), (r, 4 + cls), ((r + 1) % 2, 5 + cls)], rng)
    jg.background(J, rng)
    return J


def mixed_case(R=3, seed=32):
    """R = 3: robot 0 holds ghost factors (as first and as second key, two of them on pose 5) and no closure; robot 1 holds closures
    and ghost factors; robot 2 holds closures only when `R` > 2 ... and with R = 1: closures, no ghosts at all."""
    J = RobustJoint([12] * R, seed=seed)
    rng = np.random.default_rng(seed)
    n = 0
    if R == 3:
        for a, ka, b, kb in ((0, 5, 1, 3), (1, 8, 0, 5), (0, 9, 1, 10)):
            dt, dr = _disp(n)
            J.relative(a, ka, b, kb, dt=tuple(3.0 * v for v in dt), drot=tuple(4.0 * v for v in dr))
            n += 1
    for r in ((1, 2) if R == 3 else (0,)):
        for i, k in ((0, 6), (3, 10)):
            dt, dr = _disp(n)
            J.closure(r, i, k, dt=dt, drot=dr)
            n += 1
    for r in range(R):
        for cls in range(3):
            obs = [(r, 2 + cls), (r, 3 + cls)] + ([((r + 1) % R, 4 + cls)] if R > 1 else [])
            jg._add(J, cls, jg._near(J, r, 2 + cls, rng), obs, rng)
    jg.background(J, rng)
    return J


def nothing_selected_case(seed=33):
    """Robots 0 and 1 share inter-robot measurements; robot 2 has neither a closure nor a ghost factor (a member with nothing
    selected), robot 1 has a closure."""
    J = RobustJoint([10, 10, 8], seed=seed)
    rng = np.random.default_rng(seed)
    for n, (a, ka, b, kb) in enumerate(((0, 1, 1, 4), (1, 7, 0, 6))):
        dt, dr = _disp(n)
        J.relative(a, ka, b, kb, dt=tuple(3.0 * v for v in dt), drot=tuple(4.0 * v for v in dr))
    dt, dr = _disp(5)
    J.closure(1, 2, 8, dt=dt, drot=dr)
    for r in range(3):
        for cls in range(3):
            jg._add(J, cls, jg._near(J, r, 1 + cls, rng), [(r, 1 + cls), (r, 2 + cls), ((r + 1) % 3, 3 + cls)], rng)
    jg.background(J, rng)
    return J


def edge_case(N, seed=34):
    """Robot 0 holds n_between + n_ghost = N factors of the 128-thread launch; robot 1 is small (7 poses), so the grid sized for
    robot 0 overruns it.  N == 1: one pose whose only factor is a ghost factor.  Otherwise two ghost factors (the local pose first
    key in one, second key in the other; on poses 0 and 1, next to the prior, where no step can take their residual away) on the last two thread indices, behind min(N - 2, 120 or 128) - 1 odometry factors and then
    closures up to the between / ghost boundary: N = 127 / 128 / 129 put a ghost factor on thread 126 / 127 / 127 and 128, N = 257
    puts closures on threads 127 and 128 and ghost factors on 255 and 256."""
    n_gh = 1 if N == 1 else 2
    n_bt = N - n_gh
    P0 = 1 if N == 1 else min(n_bt, 128 if N > 200 else 120)
    n_clo = n_bt - (P0 - 1)
    J = RobustJoint([P0, 7], seed=seed, step=0.3)
    rng = np.random.default_rng(seed)
    dt, dr = _disp(0)
    J.relative(0, 0, 1, 2, dt=tuple(3.0 * v for v in dt), drot=tuple(4.0 * v for v in dr))
    if n_gh == 2:
        dt, dr = _disp(1)
        J.relative(1, 1, 0, 1, dt=tuple(3.0 * v for v in dt), drot=tuple(4.0 * v for v in dr))
    for c in range(n_clo):
        dt, dr = _disp(c + 2)
        i = (5 * c) % (P0 - 6)
        J.closure(0, i, i + 3 + c % 3, dt=dt, drot=dr)
    dt, dr = _disp(9)
    J.closure(1, 0, 4, dt=dt, drot=dr)
    jg._add(J, 2, jg._near(J, 0, 0, rng), [(0, 0), (1, 1)] + ([(0, 1)] if P0 > 1 else []), rng)
    jg._add(J, 0, jg._near(J, 1, 3, rng), [(1, 3), (1, 4), (0, min(1, P0 - 1))], rng)
    jg.background(J, rng, every=7)
    return J


# ---- the planted scenario -----------------------------------------------------------------------------------------------------------
PLANTED_STEPS = 8
PLANTED_NOISE = 1e-4
PLANTED_PARAM = {rc.GEMAN_MCCLURE: 1.5, rc.DCS: 2.25}        # c and Phi = c^2, see planted_case
PLANTED_TRUE_REL = [(0, 2, 1, 3), (1, 9, 2, 8), (0, 15, 1, 14), (2, 17, 0, 16)]
PLANTED_FALSE_REL = [(0, 7, 2, 4), (1, 12, 0, 5)]
PLANTED_CLOSURES = [(1, 2, 16, False), (2, 3, 15, True)]      # (robot, i, k, false)


def planted_case(seed=41):
    """3 robots of 20 poses, some shared landmarks, four true inter-robot measurements (noise of 0.3 sigma per coordinate), two false
    ones about 3 m and 1 rad off, two in-robot closures of which one is true (1.2 sigma off per coordinate) and one false (3 m,
    1 rad).  The kernel's width is chosen as on one graph (robust_cases.planted_graph: as wide as what the true factors have to
    correct, in whitened units), and one width serves both classes: an inter-robot measurement's sigma is 0.1 |t| ~ 0.5 m, so a
    false one that is 3 m and 1 rad off stands at s ~ 4 only, while a closure's sigma is 1e-3.  The initial poses are therefore
    close (PLANTED_NOISE: 1e-4 rad, 5e-4 m — the true closure starts at s ~ 3.7, the true inter-robot measurements at s ~ 0.75),
    and c = 1.5 (Geman-McClure), Phi = c^2 = 2.25 (DCS) lies between them and the false measurements' s ~ 4."""
    J = RobustJoint([20, 20, 20], seed=seed, step=0.5, noise=PLANTED_NOISE)
    rng = np.random.default_rng(seed)
    for a, ka, b, kb in PLANTED_TRUE_REL:
        J.relative(a, ka, b, kb, noise=0.3)
    for n, (a, ka, b, kb) in enumerate(PLANTED_FALSE_REL):
        J.relative(a, ka, b, kb, dt=(3.0 - 0.5 * n, -1.0, 0.3), drot=(0.0, 0.1 * n, 1.0))
    for r, i, k, false in PLANTED_CLOSURES:
        if false:
            J.closure(r, i, k, dt=(2.5, 1.5, -0.4), drot=(0.1, 0.0, -1.0))
        else:
            J.closure(r, i, k, dt=(1.2e-3, -1.2e-3, 1.2e-3), drot=(-1.2e-3, 1.2e-3, 1.2e-3))
    for r in range(3):
        for cls in range(3):
            jg._add(J, cls, jg._near(J, r, 4 + cls, rng), [(r, 4 + cls), (r, 5 + cls), ((r + 1) % 3, 6 + cls)], rng)
    jg.background(J, rng, every=2)
    return J


def planted_truth_error(J, ref, values):
    """RMS position error of every robot's poses against the ground truth (metres)."""
    err = [np.linalg.norm(values[ref.pose_var(r, k), 9:12] - J.T(r, k)[1]) for r in range(J.R) for k in range(J.sizes[r])]
    return float(np.sqrt(np.mean(np.square(err))))


def planted_false_mask(J):
    """Per selected factor in export order (relmeas, then closures): True where planted false."""
    return np.array([False] * len(PLANTED_TRUE_REL) + [True] * len(PLANTED_FALSE_REL) + [f for *_, f in PLANTED_CLOSURES])


_PLANTED = {}


def planted_reference(kind, chart=0):
    """The numpy IRLS on the planted scenario (computed once per kind) -> dict(J, ref, sel, trace, values, w, plain)."""
    if (kind, chart) not in _PLANTED:
        from test_joint_reference import joint_reference
        J = planted_case()
        ref, _ = joint_reference(J, chart)
        sel = selection(J, ref)
        trace, vals = steps(J, ref, kind, PLANTED_PARAM[kind], 3, PLANTED_STEPS)
        _, plain = steps(J, ref, 0, 0.0, 3, PLANTED_STEPS)
        _PLANTED[(kind, chart)] = dict(J=J, ref=ref, sel=sel, trace=trace, values=vals, w=trace[-1][3][sel], plain=plain)
    return _PLANTED[(kind, chart)]
