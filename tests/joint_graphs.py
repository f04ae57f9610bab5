"""Multi-robot graphs described once, in global terms, and emitted into two targets (test infrastructure for test_joint_reference.py
and test_gpu_joint_step.py):

  joint   ONE graph (OracleGraph) holding robot r's factors as robot r and every landmark under its global id: the graph of the
          reference's full replica, whose Gauss-Newton step gn_reference.Reference computes;
  shards  one graph per robot (SlideGraph or OracleGraph) holding that robot's factors as robot 0 with local landmark ids, plus the
          id table gid[r][cls] (local id -> global id) that setup_local_shards(..., assoc=(gid, n_global)) takes.

Every shared landmark starts at a DIFFERENT value in every replica (each robot creates it from its own first observation); the joint
graph holds the owner's value (the lowest robot that observes it), the value setup_local_shards' broadcast (phases 10 / 11) installs.
A cylinder or cube's first observation in a replica is emitted in a frame moved by a small rigid transform (pose and landmark alike):
the factor's measurement is the same, the landmark's initial value is not.  The joint graph receives exactly the arguments each shard
receives, so the factors agree bit for bit.  Inter-robot relative-pose measurements are synth.relmeas_keys entries
(ka, a, b, rel7, kb): add_relative_meas Between factors in the joint graph, PassDriver.setup_ghosts in the shards.

Measurements are exact for the ground truth; the initial poses are perturbed (gn_graphs.World), so one step moves every variable.
Every builder is deterministic."""
from __future__ import annotations

import numpy as np

import gn_graphs as gg

SLOT_DIM = {0: 7, 1: 9, 2: 3}


class _Null:
    """Swallows the graph calls (World on it only computes a trajectory)."""

    def __getattr__(self, name):
        return lambda *a, **k: None


def _compose(G, R, t):
    """The rigid transform G = (Rg, tg) applied to the pose (R, t)."""
    Rg, tg = G
    return Rg @ R, Rg @ t + tg


class Joint:
    """One multi-robot graph.  sizes[r] = pose count of robot r; robots are laid side by side (origin r * spacing along y)."""

    def __init__(self, sizes, seed=0, spacing=4.0, step=1.0):
        self.sizes, self.seed, self.spacing, self.step = list(sizes), seed, spacing, step
        self.worlds = [self._world(_Null(), r, r) for r in range(len(sizes))]
        self.lms = []                   # (cls, gid, per-robot args, observers [(r, k)])
        self.n_global = [0, 0, 0]
        self.relmeas = []               # (ka, a, b, rel7, kb)
        self.rng = np.random.default_rng(seed + 1000)

    def _world(self, G, r, robot):
        return gg.World(G, self.sizes[r], seed=self.seed + 31 * r, step=self.step, origin=(1.0, 2.0 + self.spacing * r, 0.5),
                        robot=robot)

    @property
    def R(self):
        return len(self.sizes)

    def T(self, r, k):
        return self.worlds[r].T[k]

    def _offsets(self, robots):
        """Per observing robot, the rigid transform of its first observation (its replica's initial value)."""
        out = {}
        for r in robots:
            out[r] = (gg.rot(self.rng.normal(0, 0.02, 3)), self.rng.normal(0, 0.05, 3))
        return out

    def _gid(self, cls):
        g = self.n_global[cls]
        self.n_global[cls] += 1
        return g

    # ---- landmarks, in global terms; obs = [(robot, pose index)], a robot's observations in the order they are emitted ----
    def point(self, xyz, obs):
        xyz = np.asarray(xyz, float)
        init = {r: xyz + self.rng.normal(0, 0.05, 3) for r in sorted({r for r, _ in obs})}
        calls = []
        for r, k in obs:
            R, t = self.T(r, k)
            q = R.T @ (xyz - t)
            calls.append((r, k, q / np.linalg.norm(q), float(np.linalg.norm(q))))
        self.lms.append((2, self._gid(2), dict(init=init, calls=calls), list(obs)))
        return self.lms[-1][1]

    def cylinder(self, root, ray, radius, obs):
        root, ray = np.asarray(root, float), np.asarray(ray, float) / np.linalg.norm(ray)
        off = self._offsets(sorted({r for r, _ in obs}))
        calls, seen = [], set()
        for r, k in obs:
            Re, te = self._est(r, k)
            first = r not in seen
            seen.add(r)
            if first:
                Re, te = _compose(off[r], Re, te)
                rt, ry = off[r][0] @ root + off[r][1], off[r][0] @ ray
            else:
                rt, ry = root, ray
            calls.append((r, k, gg.p7(Re, te), rt, ry, radius, first))
        self.lms.append((0, self._gid(0), dict(calls=calls), list(obs)))
        return self.lms[-1][1]

    def cube(self, R, t, scale, obs):
        R, t = np.asarray(R, float), np.asarray(t, float)
        off = self._offsets(sorted({r for r, _ in obs}))
        calls, seen = [], set()
        for r, k in obs:
            Re, te = self._est(r, k)
            first = r not in seen
            seen.add(r)
            Rc, tc = R, t
            if first:
                Re, te = _compose(off[r], Re, te)
                Rc, tc = _compose(off[r], R, t)
            calls.append((r, k, gg.p7(Re, te), gg.p7(Rc, tc), np.asarray(scale, float), first))
        self.lms.append((1, self._gid(1), dict(calls=calls), list(obs)))
        return self.lms[-1][1]

    def relative(self, a, ka, b, kb):
        """Pose ka of robot a measures pose kb of robot b (exact for the ground truth)."""
        (Ra, ta), (Rb, tb) = self.T(a, ka), self.T(b, kb)
        self.relmeas.append((ka, a, b, gg.p7(Ra.T @ Rb, Ra.T @ (tb - ta)), kb))

    def _est(self, r, k):
        e = self.worlds[r].est[k]
        from scipy.spatial.transform import Rotation
        return Rotation.from_quat(e[3:7]).as_matrix(), e[:3].copy()

    # ---- emission ----
    def _emit_landmark(self, G, cls, idx, spec, robot_of, only=None):
        """The calls of one landmark, robot r's factors as robot_of(r); only: emit robot `only`'s calls alone (a shard)."""
        created = False
        if cls == 2:
            owner = min(spec["init"]) if only is None else only
            G.add_point_landmark(idx, spec["init"][owner])
            for r, k, b, rng in spec["calls"]:
                if only is None or r == only:
                    G.add_range_bearing(robot_of(r), k, idx, b, rng)
            return
        for c in spec["calls"]:
            r = c[0]
            if only is not None and r != only:
                continue
            if cls == 0:
                _, k, p7, rt, ry, radius, _ = c
                G.add_cylinder(robot_of(r), k, idx, p7, rt, ry, radius, created)
            else:
                _, k, p7, c7, scale, _ = c
                G.add_cube(robot_of(r), k, idx, p7, c7, scale, created)
            created = True

    def emit_joint(self, G):
        for r in range(self.R):
            W = self._world(G, r, r)
            assert all(np.array_equal(a, b) for a, b in zip(W.est, self.worlds[r].est))
        # a landmark's first call is its owner's first observation (calls are emitted robot by robot)
        for cls, g, spec, obs in self.lms:
            spec = dict(spec, calls=sorted(spec["calls"], key=lambda c: c[0]))
            self._emit_landmark(G, cls, g, spec, lambda r: r)
        for ka, a, b, rel, kb in self.relmeas:
            G.add_relative_meas(rel, ka, a, kb, b)
        return G

    def local_ids(self):
        """gid[r][cls]: the global ids of robot r's landmarks of class cls, in local id order."""
        gid = [[[] for _ in range(3)] for _ in range(self.R)]
        for cls, g, _, obs in self.lms:
            for r in sorted({r for r, _ in obs}):
                gid[r][cls].append(g)
        return [[np.array(x, np.int64) for x in row] for row in gid]

    def emit_shard(self, G, r):
        self._world(G, r, 0)
        gid = self.local_ids()
        loc = [{int(g): i for i, g in enumerate(gid[r][cls])} for cls in range(3)]
        for cls, g, spec, obs in self.lms:
            if g in loc[cls]:
                self._emit_landmark(G, cls, loc[cls][g], spec, lambda _: 0, only=r)
        return G

    def observers(self, cls, g):
        for c, gg_, _, obs in self.lms:
            if c == cls and gg_ == g:
                return obs
        raise KeyError((cls, g))


class Shard:
    """What setup_local_shards and PassDriver take: `.graph` and landmark_table(cls) (only the table's length matters when the
    association is given)."""

    def __init__(self, graph, gid_r):
        self.graph, self.gid = graph, gid_r

    def landmark_table(self, cls):
        n = len(self.gid[cls])
        return np.zeros((n, 3)), np.zeros(n, np.int32)


def build(J, make_graph):
    """Shards of J (make_graph() -> an empty SlideGraph or OracleGraph per robot) and the association to give setup_local_shards."""
    gid = J.local_ids()
    shards = []
    for r in range(J.R):
        G = J.emit_shard(make_graph(), r)
        if hasattr(G, "export"):
            G.export()          # (an OracleGraph merges its pending entries here; set_shared looks the landmarks up among the merged)
        shards.append(Shard(G, gid[r]))
    return shards, (gid, list(J.n_global))


# ---------------------------------------------------------------------------------------------------------------------------------
# cases


def _near(J, r, k, rng, d=6.0):
    R, t = J.T(r, k)
    return t + R @ np.array([d, rng.uniform(-3, 3), rng.uniform(-1, 2)])


def _add(J, cls, centre, obs, rng):
    if cls == 0:
        return J.cylinder(centre, [0.05, -0.02, 1.0], 0.3, obs)
    if cls == 1:
        return J.cube(gg.rot([0.2, 0.1, 0.9]), centre, [1.0, 2.0, 0.5], obs)
    return J.point(centre, obs)


def background(J, rng, every=3, shared_every=0):
    """A point, cylinder or cube near every `every`-th pose of every robot, seen from up to three consecutive poses; with
    shared_every > 0 every shared_every-th of them is also seen once from the next robot's same-index pose."""
    n = 0
    for r in range(J.R):
        P = J.sizes[r]
        for k in range(0, P, every):
            obs = [(r, j) for j in range(k, min(P, k + 3))]
            if shared_every and n % shared_every == 0 and J.R > 1:
                r2 = (r + 1) % J.R
                obs.append((r2, min(k, J.sizes[r2] - 1)))
            _add(J, n % 3, _near(J, r, k, rng), obs, rng)
            n += 1


def landmark_count_case(cls, nf, shared=False, seed=11):
    """Robot 0 observes one landmark of class cls from nf poses (k_landmark_b<3>'s factor count); shared: robot 1 sees it once more
    (a separator landmark, its sums go to the border) — else robot 1 shares a point with robot 0 so that the batch has a separator."""
    J = Joint([max(nf, 2), 8], seed=seed, step=0.3)
    rng = np.random.default_rng(seed)
    c = _near(J, 0, 0, rng, 5.0)
    obs = [(0, k) for k in range(nf)] + ([(1, 3)] if shared else [])
    _add(J, cls, c, obs, rng)
    J.point(c + np.array([1.0, -2.0, 0.3]), [(0, 0), (0, 1), (1, 0), (1, 1)])
    background(J, rng, every=4)
    return J


def shared_mix_case(R, seed=12, sizes=None):
    """R robots: landmarks seen by two robots, by every robot, and one seen many times by robot 0 and once by the last robot."""
    J = Joint(sizes or [12] * R, seed=seed)
    rng = np.random.default_rng(seed)
    for r in range(R):
        r2 = (r + 1) % R
        for cls in range(3):
            _add(J, cls, _near(J, r, 2 + cls, rng), [(r, 2 + cls), (r, 3 + cls), (r2, 4 + cls)], rng)
    for cls in range(3):
        _add(J, cls, _near(J, 0, 6, rng, 8.0), [(r, 6 + cls) for r in range(R)], rng)
    _add(J, 2, _near(J, 0, 1, rng), [(0, k) for k in range(10)] + [(R - 1, 9)], rng)
    background(J, rng)
    return J


def sizes_case(sizes, seed=13, private_only=()):
    """Robots of different sizes in one batch; robots in `private_only` observe no shared landmark (an empty border)."""
    J = Joint(sizes, seed=seed)
    rng = np.random.default_rng(seed)
    sharing = [r for r in range(J.R) if r not in private_only]
    for i, r in enumerate(sharing):
        r2 = sharing[(i + 1) % len(sharing)]
        for cls in range(3):
            if r2 != r:
                _add(J, cls, _near(J, r, 1 + cls, rng), [(r, 1 + cls), (r2, min(J.sizes[r2] - 1, 2 + cls))], rng)
    for r in range(J.R):
        P = J.sizes[r]
        for k in range(0, P, 2 + r % 3):
            _add(J, (k + r) % 3, _near(J, r, k, rng), [(r, j) for j in range(k, min(P, k + 3))], rng)
    return J


def border_case(border, R=2, P=24, seed=14):
    """Robot 0's border holds `border` = (cylinders, cubes, points) shared with robot 1 (7 / 9 / 3 coordinates each)."""
    J = Joint([P] * R, seed=seed)
    rng = np.random.default_rng(seed)
    n = 0
    for cls, cnt in enumerate(border):
        for _ in range(cnt):
            k = n % P
            _add(J, cls, _near(J, 0, k, rng), [(0, k), (0, (k + 1) % P), (1 + n % (R - 1), (k + 2) % P)], rng)
            n += 1
    background(J, rng, every=4)
    return J


def walk_case(seed=15, P=280):
    """Robot 0 re-observes a landmark 270 poses later (its Schur strip is wider than 256 poses: build_schur_pairs falls back to the
    walk), with robot 1 sharing points with it."""
    J = Joint([P, 10], seed=seed, step=0.2)
    rng = np.random.default_rng(seed)
    _add(J, 2, _near(J, 0, 2, rng), [(0, 2), (0, 272)], rng)
    _add(J, 0, _near(J, 0, 5, rng), [(0, 5), (0, 6), (0, 275)], rng)
    _add(J, 2, _near(J, 0, 0, rng), [(0, 0), (0, 1), (1, 0), (1, 1)], rng)
    _add(J, 1, _near(J, 0, 8, rng), [(0, 8), (1, 4)], rng)
    background(J, rng, every=6)
    return J


def column_cap_case(n_lm=270, seed=16):
    """Pose 2 of robot 0 observes n_lm points (> SCHUR_PJ_CAP = 256 landmark factors on one column), each co-observed by another
    pose; robot 1 shares two of them."""
    J = Joint([6, 6], seed=seed)
    rng = np.random.default_rng(seed)
    others = [0, 1, 3, 4, 5]
    for l in range(n_lm):
        obs = [(0, 2), (0, others[l % 5])] + ([(1, l % 6)] if l < 2 else [])
        J.point(_near(J, 0, 2, rng), obs)
    background(J, rng, every=3)
    return J


def relmeas_case(R=2, n_rel=3, P=14, seed=17, shared=True):
    """Inter-robot relative-pose factors: between equal and different key-frame indices, n_rel of them (11: 66 lambda
    coordinates, past one tile)."""
    J = Joint([P] * R, seed=seed)
    rng = np.random.default_rng(seed)
    for i in range(n_rel):
        a = i % R
        b = (a + 1) % R
        ka = (2 * i) % P
        kb = ka if i % 2 == 0 else (ka + 3) % P
        J.relative(a, ka, b, kb)
    if shared:          # (the batched pass exchanges the ghost poses through the slot buffers: 54 doubles per slot, 12 per ghost)
        for r in range(R):
            for cls in range(3):
                _add(J, cls, _near(J, r, 3 + cls, rng), [(r, 3 + cls), (r, 4 + cls), ((r + 1) % R, 5 + cls)], rng)
    background(J, rng)
    return J


def segments_case(R=2, P=150, seed=18):
    """Robots of about 150 poses (bands the nested dissection cuts into segments), sharing landmarks along the way.  Around each place
    where 2, 3 or 4 segments are cut, a point seen from poses 14 apart: the separator behind the cut spans more than a tile (a
    narrower one would leave the band uncut)."""
    J = Joint([P] * R, seed=seed, step=0.5)
    rng = np.random.default_rng(seed)
    for r in range(R):
        for q in sorted({P * i // n for n in (2, 3, 4) for i in range(1, n)}):
            J.point(_near(J, r, q, rng), [(r, q - 2), (r, q + 12)])
    for r in range(R):
        r2 = (r + 1) % R
        for k in range(5, P, 40):
            _add(J, (k // 40) % 3, _near(J, r, k, rng), [(r, k), (r, k + 1), (r2, k + 2)], rng)
    background(J, rng, every=5)
    return J


def separator_tiles_case(seed=19, per_leaf=10, top=8):
    """Four robots in two halves (0, 1 | 2, 3): per_leaf cubes shared inside each half (a leaf block of 90 coordinates, past one
    tile) and `top` cubes shared across the halves (the top block)."""
    J = Joint([16] * 4, seed=seed)
    rng = np.random.default_rng(seed)
    for a, b in ((0, 1), (2, 3)):
        for i in range(per_leaf):
            k = i % 16
            _add(J, 1, _near(J, a, k, rng), [(a, k), (b, (k + 1) % 16)], rng)
    for i in range(top):
        k = (3 * i) % 16
        _add(J, 1, _near(J, 1, k, rng), [(1, k), (2, (k + 2) % 16)], rng)
    background(J, rng, every=4)
    return J
