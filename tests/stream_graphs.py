"""Streaming graphs and a per-update referee for SlideGraph.solve() (test infrastructure for test_stream_reference.py and
test_gpu_stream_step.py).

With the wildfire bound off (the default) a streaming update is exactly one Gauss-Newton step of the full linearisation at the
per-variable linearisation points theta (oracle/graph.hpp, the update rule in its header).  theta is not exposed, so the Tracker
restates it from the solver's public outputs: a variable joins with theta = the value passed to add_*; at each solve() a variable
whose last delta (tangent from theta to its last read-back estimate) has |delta|_inf >= relinearize_threshold takes theta = that
estimate.  Every update is then checked against gn_reference's least-squares step at theta.

Stream describes a ground-truth trajectory and map (gn_graphs.World) and emits it frame by frame, plus the events the cases need
(re-observations, late observations, loop closures), into every graph it is given: a SlideGraph and an OracleGraph.  The oracle is
a recorder (its export() is the reference's factor list); only test_stream_reference.py calls its solve().  Every builder is
deterministic (seeded)."""
from __future__ import annotations

import numpy as np

import gn_graphs as gg
from gn_reference import EPS, Reference, local, scaled_error, tolerance
from oracle import pyoracle as po
from test_gn_reference import numdiff_floor, oracle_values

NB = 64                    # tangent coordinates per block column of the reduced pose system
RELIN_THR = 0.1            # relinearize_threshold of both default parameter sets
MARGIN = 1e-9              # no |delta|_inf may lie this close (relative) to the threshold: the decision must be unambiguous
CLS = {"cyl": 0, "cube": 1, "point": 2}


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a: self.calls.append((name, a))


class Stream:
    """A P-pose ground truth (gn_graphs.World, robot 0) and a landmark plan: landmark (cls, idx) is created at its first observer's
    frame and observed from each of its observers at theirs.  frame(k) emits pose k (prior or odometry between factor with its
    initial value) and the landmark calls of pose k.  yaw_bias: every odometry measurement turns by this much more than the ground
    truth, and the initial values are the dead-reckoned odometry chain (drift that a loop closure corrects)."""

    def __init__(self, graphs, P, seed=0, yaw_bias=0.0, every=1, **world_kw):
        rec = _Recorder()
        self.W = gg.World(rec, P, seed=seed, **world_kw)
        self.graphs = list(graphs)
        self.calls = rec.calls                 # [set_prior, between 0 -> 1, between 1 -> 2, ...]
        self.rng = np.random.default_rng(seed + 200)
        if yaw_bias:
            q = self.W.qscale
            est = [self.W.T[0]]
            for k in range(1, P):
                (Ra, ta), (Rb, tb) = self.W.T[k - 1], self.W.T[k]
                Rr, tr = Ra.T @ Rb @ gg.rot([0, 0, yaw_bias]), Ra.T @ (tb - ta)
                Re, te = est[-1]
                est.append((Re @ Rr, te + Re @ tr))
                self.calls[k] = ("add_keypose_between", (0, k - 1, k, gg.p7(Rr, tr, q), gg.p7(*est[-1], q)))
                self.W.est[k] = gg.p7(*est[-1], q)
        self.plan = {}                         # pose -> [(cls, idx, first observer?)]
        self.spec = {}                         # (cls, idx) -> its ground truth
        self.first = {}                        # (cls, idx) -> first observer
        for k in range(0, P, every):
            self.landmark(("point", "cube", "cyl")[(k // every) % 3], 1000 + k, range(k, min(P, k + 3)))

    def _emit(self, name, *a):
        for g in self.graphs:
            getattr(g, name)(*a)

    def landmark(self, cls, idx, observers):
        """Plans landmark (cls, idx) near its first observer, seen from `observers` (created at the first one's frame)."""
        obs = list(observers)
        k = obs[0]
        xyz = gg.around(self.W, k, self.rng)
        if cls == "point":
            self.spec[cls, idx] = (xyz,)
        elif cls == "cube":
            self.spec[cls, idx] = (gg.rot([0.1, 0.2, self.rng.uniform(-3, 3)]), xyz, np.array([0.8, 1.5, 0.6]))
        else:
            ray = np.array([0.0, 0.05, 1.0])
            self.spec[cls, idx] = (xyz, ray / np.linalg.norm(ray), 0.25)
        self.first[cls, idx] = k
        for n, j in enumerate(obs):
            self.plan.setdefault(j, []).append((cls, idx, n == 0))
        return cls, idx

    def frame(self, k):
        name, a = self.calls[k]
        self._emit(name, *a)
        for cls, idx, new in self.plan.get(k, []):
            self.observe(cls, idx, k, new)

    def observe(self, cls, idx, k, new=False, rng_offset=0.0):
        """Pose k observes landmark (cls, idx); new: the call that creates it (gn_graphs.World's conventions: the first observation
        carries the noisy initial value, the rest are exact).  rng_offset: a point's measured range is this much off."""
        W, sp = self.W, self.spec[cls, idx]
        R, t = W.T[k]
        noise = (lambda: W.rng.normal(0, W.noise, 3)) if new else (lambda: 0.0)
        if cls == "point":
            if new:
                self._emit("add_point_landmark", idx, sp[0] + noise())
            q = R.T @ (sp[0] - t)
            self._emit("add_range_bearing", 0, k, idx, q / np.linalg.norm(q), float(np.linalg.norm(q)) + rng_offset)
        elif cls == "cube":
            c7 = gg.p7(sp[0], sp[1] + noise(), W.qscale)
            self._emit("add_cube", 0, k, idx, W.est[k], c7, sp[2] + (0.01 if new else 0.0), not new)
        else:
            self._emit("add_cylinder", 0, k, idx, W.est[k], sp[0] + noise(), sp[1], sp[2], not new)

    def loop(self, i, k):
        """Loop closure between poses i and k (addLoopClosureFactor), measured on the ground truth."""
        (Ra, ta), (Rb, tb) = self.W.T[i], self.W.T[k]
        self._emit("add_loop_closure", gg.p7(Ra.T @ Rb, Ra.T @ (tb - ta), self.W.qscale), i, 0, k, 0)


# ---- the referee ----------------------------------------------------------------------------------------------------------------

class Structure:
    """Who touches whom in an export: pose index of each pose variable, between partners, observers of each landmark."""

    def __init__(self, ref):
        nv = len(ref.vtype)
        self.pidx = np.full(nv, -1)
        poses = np.flatnonzero(ref.vtype == po.V_POSE)
        self.pidx[poses] = np.arange(len(poses))
        self.P = len(poses)
        self.partners = [[] for _ in range(nv)]
        self.observes = [[] for _ in range(nv)]      # pose var -> landmark vars it observes
        self.first = np.full(nv, 1 << 30)            # landmark var -> lowest observing pose
        for f in range(len(ref.ftype)):
            t, a, b = int(ref.ftype[f]), int(ref.fv[f, 0]), int(ref.fv[f, 1])
            if t == po.F_BETWEEN:
                self.partners[a].append(b)
                self.partners[b].append(a)
            elif t in (po.F_BR, po.F_CUBE, po.F_CYL):
                self.observes[a].append(b)
                self.first[b] = min(self.first[b], self.pidx[a])

    def dirty_of_factor(self, ref, f):
        t, a, b = int(ref.ftype[f]), int(ref.fv[f, 0]), int(ref.fv[f, 1])
        p = self.pidx[a]
        if t == po.F_BETWEEN:
            return min(p, self.pidx[b])
        if t in (po.F_BR, po.F_CUBE, po.F_CYL):
            return min(p, self.first[b])
        return p

    def dirty_of_var(self, ref, v):
        if int(ref.vtype[v]) != po.V_POSE:
            return int(self.first[v])
        return min([self.pidx[v]] + [self.pidx[u] for u in self.partners[v]] + [self.first[l] for l in self.observes[v]])


class Tracker:
    """theta per variable key, restated from the solver's read-backs (see the module docstring)."""

    def __init__(self, chart, thr=RELIN_THR):
        self.chart, self.thr = chart, thr
        self.theta = {}            # key -> value row (15)
        self.est = {}              # key -> last read-back estimate
        self.vtype = {}
        self.nf = 0                # factors merged before this update

    def relinearise(self):
        """At solve(): theta := estimate where the last delta reached the threshold.  -> (relinearised keys, smallest relative
        distance of any |delta|_inf from the threshold)."""
        moved, margin = [], np.inf
        for key, est in self.est.items():
            th = self.theta[key]
            d = local(self.vtype[key], th, est, self.chart)
            mx = float(np.abs(d).max())
            margin = min(margin, abs(mx - self.thr) / self.thr)
            if mx >= self.thr:
                self.theta[key] = est.copy()
                moved.append(key)
        return moved, margin


def var_key(cls_or_pose, idx):
    """The key of pose idx of robot 0 (cls_or_pose = 'pose') or of landmark (cls, idx), as both graphs build it."""
    if cls_or_pose == "pose":
        return (ord("x") << 56) | int(idx)
    return (ord("lcu"[CLS[cls_or_pose]]) << 56) | int(idx)


class Update:
    """One update's record: what the referee expected and found."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "Update(" + ", ".join(f"{k}={v}" for k, v in self.__dict__.items() if k not in ("ref", "values", "got", "moved", "oracle_theta")) + ")"


class Run:
    """Drives one stream: frames and events go to every graph; solve() solves the solver under test (`solver`: a SlideGraph, or the
    recording OracleGraph itself) and checks the update against the reference step at the tracked theta.  check: False skips the
    least-squares comparison of an update (the CPU file's cases that only need the tracker)."""

    def __init__(self, og, solver, chart, read=None, stats=None):
        self.og, self.solver, self.chart = og, solver, chart
        self.read = read or (lambda ref: oracle_values(og, ref))
        self.stats = stats or (lambda: {})
        self.tr = Tracker(chart)
        self.updates = []

    def solve(self, check=True):
        og, tr = self.og, self.tr
        ref = Reference(og, self.chart)
        st = Structure(ref)
        nf = len(ref.ftype)
        # (1) relinearisation of what was there before; (2) new variables join at their initial values
        moved, margin = tr.relinearise()
        assert margin > MARGIN, f"|delta|_inf within {MARGIN} of the threshold: the builder's seed makes the decision ambiguous"
        for k, key in enumerate(ref.vkey):
            key = int(key)
            if key not in tr.theta:
                tr.theta[key] = ref.values[k].copy()
                tr.vtype[key] = int(ref.vtype[k])
        values = np.array([tr.theta[int(key)] for key in ref.vkey])
        # the dirty rule, restated: merged factors, then the relinearised variables
        key2var = {int(key): k for k, key in enumerate(ref.vkey)}
        pmin_fac = min([st.dirty_of_factor(ref, f) for f in range(tr.nf, nf)], default=1 << 30)
        pmin_rel = min([st.dirty_of_var(ref, key2var[key]) for key in moved], default=1 << 30)
        tr.nf = nf
        dx = H = None
        if check:
            dx, H = ref.step(values)
        assert self.solver.solve() == 0
        got = self.read(ref)
        for k, key in enumerate(ref.vkey):
            tr.est[int(key)] = got[k].copy()
        u = Update(P=st.P, T=-(-6 * st.P // NB), n_relin=len(moved), moved=moved, pmin_fac=int(pmin_fac), pmin_rel=int(pmin_rel),
                   pmin=int(min(pmin_fac, pmin_rel)), ratio=None, ref=ref, values=values, got=got, **self.stats())
        if check:
            u.ratio = check_step(ref, values, got, dx, H)
        self.updates.append(u)
        return u

    def delta(self, key):
        """|delta|_inf of a variable after the last update (what decides its relinearisation at the next)."""
        tr = self.tr
        return float(np.abs(local(tr.vtype[key], tr.theta[key], tr.est[key], self.chart)).max())


def check_step(ref, values, got, dx, H):
    """The update (`got`, read back) against the least-squares step dx at `values`: gn_reference's bound, as check_steps uses it.
    -> scaled_error / tolerance."""
    mag = ref.magnitude(values)
    step = ref.tangent(values, got)
    w = np.sqrt(np.diag(H))
    if not np.linalg.norm(w * dx) > 0.0:      # (a graph at its optimum: nothing to scale by; only the read-back's rounding remains)
        err, bound = float(np.linalg.norm(w * step)), 8 * EPS * float(np.linalg.norm(w * mag))
        assert err <= bound, (err, bound)
        return err / bound if bound else 0.0
    tol, kappa = tolerance(H, dx, mag, numdiff_floor(ref, dx, H, values))
    err = scaled_error(step, dx, H)
    assert err <= tol, (err, tol, kappa)
    return err / tol


def stream_pair(gpu, chart, P, seed=0, **kw):
    """(Stream over a SlideGraph and a recording OracleGraph, Run checking the SlideGraph)."""
    og = po.OracleGraph(po.OrcParams.default(pose_chart=chart))
    G = gpu.SlideGraph(gpu.default_params(pose_chart=chart))
    S = Stream([G, og], P, seed=seed, **kw)

    def read(ref):
        from test_gpu_gn_step import gpu_values
        return gpu_values(G, ref)

    def stats():
        return dict(gpu_relin=G.stats()["n_relin"], **G.incremental_stats())
    return S, Run(og, G, chart, read, stats), G


def oracle_stream(chart, P, seed=0, **kw):
    """(Stream over one OracleGraph, Run checking the oracle's own solve)."""
    og = po.OracleGraph(po.OrcParams.default(pose_chart=chart))
    S = Stream([og], P, seed=seed, **kw)

    def stats():
        return dict(oracle_relin=og.stats()["n_relin"], oracle_theta=og.export()["var_val"])
    return S, Run(og, og, chart, stats=stats)


# ---- the cases (shared by the CPU and the GPU file; each returns the updates its edge is asserted on) ----------------------------

def run_frames(S, R, ks):
    for k in ks:
        S.frame(k)
        R.solve()


def case_plain(S, R, P=50):
    """Plain stream, P = 1 .. 50: T <= 2, the first incremental updates, the band gaining block columns, T > 4."""
    run_frames(S, R, range(P))
    return {}


REOBS_FIRST = (42, 32, 31, 11, 10)       # pose 10: coordinates 60 .. 65 (columns 0 and 1), 11: starts column 1, 31: ends column 2,
                                         # 32: starts column 3, 42: column 3


def reobs_landmarks(S, cls):
    return {f: S.landmark(cls, 2000 + f, (f, f + 1, f + 2)) for f in REOBS_FIRST}


def case_reobserve(S, R, cls, P=45):
    """Frames 0 .. P-1, then each of frames P .. P+4 re-observes one old landmark of class cls, first observer 42, 32, 31, 11, 10."""
    lms = reobs_landmarks(S, cls)
    run_frames(S, R, range(P))
    marks = {}
    for n, f in enumerate(REOBS_FIRST):
        S.frame(P + n)
        S.observe(*lms[f], P + n)
        marks[f] = R.solve()
    return marks


def case_late(S, R, P=44):
    """A point landmark first seen from pose 30 is observed at frame 40 from pose 25 (an older pose: its first observer moves down),
    with a range 0.6 m off, so that the landmark's next update relinearises it: from the NEW first observer on."""
    lm = S.landmark("point", 3000, (30, 31, 32))
    run_frames(S, R, range(40))
    S.frame(40)
    S.observe(*lm, 25, rng_offset=0.6)
    late = R.solve()
    run_frames(S, R, range(41, P))
    return {"late": late, "after": R.updates[-(P - 41)], "key": var_key(*lm)}


LOOP_TO = ("P-2", 21, 11, 10, 0)


def case_loop(S, R, P=45):
    """Frames 0 .. P-1, then frames P .. P+4 each add a loop closure from the new (newest) pose to pose P-2 (with P the pose count
    after the frame: the newest pose's odometry partner), 21, 11, 10, 0."""
    run_frames(S, R, range(P))
    marks = {}
    for n, i in enumerate(LOOP_TO):
        k = P + n
        i = k - 1 if i == "P-2" else i         # (P poses after the frame: P - 2 is the newest one's predecessor)
        S.frame(k)
        S.loop(i, k)
        marks[i] = R.solve()
    return marks


def case_drift(S, R, P=36, after=4):
    """Drifting odometry (Stream yaw_bias) over P frames, then a loop closure from the newest pose to pose 0 (a large correction);
    the frame after it also closes a loop to a pose and re-observes a landmark that are predicted to relinearise (|delta| >= thr);
    then `after` plain frames."""
    run_frames(S, R, range(P))
    S.loop(0, P - 1)
    corr = R.solve()
    # predicted to relinearise at the next update: the variables whose delta reached the threshold
    poses = [k for k in range(2, P - 4) if R.delta(var_key("pose", k)) >= RELIN_THR]
    lms = [(c, i) for (c, i) in S.spec if i < 2000 and S.first[c, i] < P - 4 and R.delta(var_key(c, i)) >= RELIN_THR]
    assert poses and lms, (poses, lms)
    j, lm = poses[len(poses) // 2], lms[len(lms) // 2]
    S.frame(P)
    S.loop(j, P)
    S.observe(*lm, P)
    nxt = R.solve()
    run_frames(S, R, range(P + 1, P + 1 + after))
    return {"correction": corr, "next": nxt, "pose": j, "lm": var_key(*lm)}


def case_repeat(S, R, P1=26, P2=45):
    """solve() with no new factors: four times at T = 3 (P1 poses: the last two relinearise nothing), twice at T = 5 (P2 poses)."""
    run_frames(S, R, range(P1))
    small = [R.solve() for _ in range(4)]
    run_frames(S, R, range(P1, P2))
    big = [R.solve(), R.solve()]
    return {"small": small, "big": big}


def case_toggle(S, R, P=45, off=(30, 36), set_incremental=None):
    """set_incremental(False) before frame off[0], back on before frame off[1] (the SlideGraph only: the oracle has one branch)."""
    for k in range(P):
        if set_incremental is not None and k in off:
            set_incremental(k != off[0])
        S.frame(k)
        R.solve()
    return {}
