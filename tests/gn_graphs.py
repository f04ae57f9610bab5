"""Graphs built through the SemanticFactorGraph seam (SlideGraph and OracleGraph take the same calls) at the shapes and values where
the solve's kernels switch code paths (test infrastructure for test_gn_reference.py and test_gpu_gn_step.py).

Measurements are exact for a ground-truth trajectory and map; the initial values are perturbed, so one Gauss-Newton step moves every
variable.  Every builder is deterministic (its own seeded generator)."""
from __future__ import annotations

import numpy as np


def quat(R):
    """Rotation matrix -> (x, y, z, w), w >= 0."""
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(R).as_quat()
    return q if q[3] >= 0 else -q


def rot(axis_angle):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(np.asarray(axis_angle, float)).as_matrix()


def p7(R, t, qscale=1.0, log=None):
    out = np.concatenate([t, qscale * quat(R)])
    if log is not None:
        log.append(out[3:].copy())
    return out


class World:
    """Ground-truth poses (R, t) of one robot (`robot`, default 0) and the calls that put a graph on them."""

    def __init__(self, G, P, seed=0, full3d=True, step=1.0, origin=(1.0, 2.0, 0.5), noise=0.02, qscale=1.0, rel_rots=None,
                 r0=(0.1, -0.2, 0.3), perturb=None, rperturb=None, robot=0):
        self.G, self.rng, self.robot = G, np.random.default_rng(seed), robot
        self.noise, self.qscale = noise, qscale
        self.quats = []          # every quaternion this world passes at the ABI (as passed)
        R = rot(r0 if full3d else [0, 0, 0.3])
        t = np.array(origin, float)
        self.T = [(R, t)]
        for k in range(1, P):
            w = (self.rng.normal(0, 0.15, 3) if full3d else np.array([0, 0, self.rng.normal(0, 0.15)]))
            if rel_rots is not None and k - 1 < len(rel_rots) and rel_rots[k - 1] is not None:
                w = rel_rots[k - 1]
            dR = rot(w)
            dt = np.array([step, 0.1 * self.rng.normal(), 0.05 * self.rng.normal() if full3d else 0.0])
            R, t = R @ dR, t + R @ dt
            self.T.append((R, t))
        self.est = []
        G.set_prior(robot, p7(*self.T[0], qscale, self.quats))
        self.est.append(p7(*self.T[0], qscale))
        for k in range(1, P):
            (Ra, ta), (Rb, tb) = self.T[k - 1], self.T[k]
            rel = p7(Ra.T @ Rb, Ra.T @ (tb - ta), qscale, self.quats)
            Re = Rb @ rot(self.rng.normal(0, noise, 3)) @ rot((rperturb or {}).get(k, np.zeros(3)))
            te = tb + self.rng.normal(0, noise * 5, 3) + np.asarray((perturb or {}).get(k, 0.0))
            e = p7(Re, te, qscale, self.quats)
            G.add_keypose_between(robot, k - 1, k, rel, e)
            self.est.append(e)

    def point(self, idx, xyz, observers):
        xyz = np.asarray(xyz, float)
        self.G.add_point_landmark(idx, xyz + self.rng.normal(0, self.noise, 3))
        for k in observers:
            R, t = self.T[k]
            q = R.T @ (xyz - t)
            self.G.add_range_bearing(self.robot, k, idx, q / np.linalg.norm(q), float(np.linalg.norm(q)))

    def cylinder(self, idx, root, ray, radius, observers):
        root, ray = np.asarray(root, float), np.asarray(ray, float)
        for n, k in enumerate(observers):
            rt = root + (self.rng.normal(0, self.noise, 3) if n == 0 else 0.0)
            self.G.add_cylinder(self.robot, k, idx, self.est[k], rt, ray, radius, n > 0)

    def cube(self, idx, R, t, scale, observers):
        for n, k in enumerate(observers):
            c7 = p7(R, np.asarray(t, float) + (self.rng.normal(0, self.noise, 3) if n == 0 else 0.0), self.qscale, self.quats)
            self.G.add_cube(self.robot, k, idx, self.est[k], c7, np.asarray(scale, float) + (0.01 if n == 0 else 0.0), n > 0)


def around(W, k, rng, r=6.0):
    """A point a few metres from pose k, in front of it."""
    R, t = W.T[k]
    return t + R @ np.array([r, rng.uniform(-3, 3), rng.uniform(-1, 2)])


def pose_list_graph(G, n_lm, seed=1):
    """Pose 2 of a 6-pose chain observes n_lm point landmarks; each is co-observed by one of poses 0, 1, 3, 4, 5 in turn, so the
    Schur strips of pose 2's column (rows 2..5) and of the other columns (row 2) read its list."""
    W = World(G, 6, seed=seed)
    rng = np.random.default_rng(seed + 100)
    others = [0, 1, 3, 4, 5]
    for l in range(n_lm):
        W.point(l, around(W, 2, rng), [2, others[l % len(others)]])
    return W


def landmark_count_graph(G, cls, nf, seed=2):
    """One landmark of class cls (0 cylinder, 1 cube, 2 point) observed by all nf poses of a chain, plus one point landmark seen from
    the first two poses."""
    W = World(G, nf, seed=seed, step=0.3)
    c = W.T[0][1] + W.T[0][0] @ np.array([5.0, 1.0, 0.5])
    if cls == 0:
        W.cylinder(0, c, [0.05, -0.02, 1.0] / np.linalg.norm([0.05, -0.02, 1.0]), 0.3, range(nf))
    elif cls == 1:
        W.cube(0, rot([0.2, 0.1, 0.9]), c, [1.0, 2.0, 0.5], range(nf))
    else:
        W.point(0, c, range(nf))
    W.point(1, c + np.array([1.0, -2.0, 0.3]), range(min(nf, 2)))
    return W


def pose_count_graph(G, P, seed=3):
    """A P-pose chain with a point, a cylinder and a cube landmark every few poses, each seen from up to four consecutive poses."""
    W = World(G, P, seed=seed)
    rng = np.random.default_rng(seed + 100)
    for k in range(0, P, 3):
        obs = list(range(k, min(P, k + 4)))
        W.point(k, around(W, k, rng), obs)
        if k % 2 == 0:
            W.cylinder(k, around(W, k, rng), [0.0, 0.05, 1.0] / np.linalg.norm([0.0, 0.05, 1.0]), 0.25, obs)
        else:
            W.cube(k, rot([0.1, 0.2, rng.uniform(-3, 3)]), around(W, k, rng), [0.8, 1.5, 0.6], obs)
    return W


def geometry_graph(G, kind, seed=4):
    """kind: 'full3d' (roll, pitch and yaw everywhere), 'rot3' / 'nearpi' (between factors with relative rotations of 3.0 rad and
    pi - 1e-3; nearpi also an initial value pi - 1e-3 away from its factors), 'quat' (quaternions with w < 0 and norm 1.7 at the ABI), 'far' (translations about 1e4 m), 'bearing' (bearings
    along an axis and with two equal smallest components at the linearisation point: sphere_basis's tie)."""
    if kind in ("rot3", "nearpi"):
        a = 3.0 if kind == "rot3" else np.pi - 1e-3
        # (nearpi: pose 2's initial rotation is also pi - 1e-3 away from where its factors put it, so the between factors' ERRORS —
        # the rotations Logmap sees — lie near pi too, not only their measurements)
        W = World(G, 5, seed=seed, rel_rots=[None, [0, 0, a], None, np.array([1.0, 1.0, 0.0]) / np.sqrt(2) * a],
                  rperturb={2: np.array([0.0, 0.6, 0.8]) * a} if kind == "nearpi" else None)
    elif kind == "quat":
        W = World(G, 5, seed=seed, qscale=-1.7)
    elif kind == "far":
        W = World(G, 5, seed=seed, origin=(1.0e4, -0.7e4, 30.0))
    elif kind == "bearing":
        W = World(G, 3, seed=seed, r0=(0.0, 0.0, 0.0), origin=(0.0, 0.0, 0.0))
        G2 = W.G
        # pose 0 (the prior) is the identity and these landmarks' initial values are exact: the predicted bearings are exactly these
        R, t = W.T[0]
        for l, b in enumerate(([0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [3.0, 1.0, 1.0], [1.0, -2.0, 1.0])):
            b = np.array(b) / np.linalg.norm(b)
            xyz = t + R @ (4.0 * b)
            G2.add_point_landmark(l, xyz)
            G2.add_range_bearing(0, 0, l, b, 4.0)
            for k in (1, 2):
                Rk, tk = W.T[k]
                q = Rk.T @ (xyz - tk)
                G2.add_range_bearing(0, k, l, q / np.linalg.norm(q) + 0.01, float(np.linalg.norm(q)) + 0.05)
        return W
    else:
        W = World(G, 5, seed=seed)
    rng = np.random.default_rng(seed + 100)
    for k in range(len(W.T)):
        W.point(k, around(W, k, rng), [k, (k + 1) % len(W.T)])
    W.cylinder(0, around(W, 1, rng), [0.1, 0.0, 1.0] / np.linalg.norm([0.1, 0.0, 1.0]), 0.3, [1, 2, 3])
    W.cube(0, rot([0.3, -0.2, 1.1]), around(W, 2, rng), [1.0, 2.0, 0.5], [2, 3, 4])
    return W
