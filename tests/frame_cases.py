"""Frame sequences for the per-frame association kernel (k_assoc_frame) and a plain numpy restatement of one frame.

A case is a list of backend calls (process_frame in HOST / HOST_DEFERRED / FOREIGN mode, ingest_solve, end_frame) on a seeded world
of upright cylinders, cubes and ellipsoids.  `run_case` feeds it to any backend with the SlideBackend / OracleBackend interface;
`numpy_frame_reference` restates the decision rule of one frame (float32 K-NN gate, double-precision nearest-neighbour match) from
the documented rule alone, without the product and without oracle/.  tests/test_frame_reference.py proves the cases and the
reference on the CPU, tests/test_gpu_frame_assoc.py runs them on the device.  No GPU and no compiled code is needed here.
"""
from __future__ import annotations

import functools
import math

import numpy as np

CLS = ("cyl", "cube", "ell")
COUNT_KEY = ("cyl", "cube", "point")
FRAME_HOST, FRAME_HOST_DEFERRED, FRAME_FOREIGN = 0, 1, 2
K_DEFAULT = (50, 30, 1000)
THRESH = dict(cyl=2.0, cube=2.0, ell=0.75)           # cylinder / cuboid / ellipsoid match thresholds (the defaults of both sides)
BEST_INIT = dict(cyl=THRESH["cyl"] + 100, cube=30.0, ell=1000.0)
LABEL_GATE = dict(cyl=True, cube=False, ell=True)
MARGIN = 1e-9                                        # the numpy reference is asserted on detections with a margin above this
SPACING = dict(cyl=5.0, cube=6.0, ell=1.5)           # grid spacing per class: above the class's match threshold with the jitter off
JITTER = dict(cyl=0.5, cube=0.5, ell=0.25)           # (closest pair: 4.0 / 5.0 / 1.0 m against thresholds 2.0 / 2.0 / 0.75)
LABELS = dict(cyl=(10, 11), cube=(20, 21, 22), ell=(30, 31, 32, 33, 34, 35))
NO_SUCH_LABEL = 99
N_POOL = 8                                           # objects per class outside the grids, never in a seeding frame: "far" detections
IDENT7 = np.array([0, 0, 0, 0, 0, 0, 1.0])


# ---- small SE(3) helpers -------------------------------------------------------------------------------------------------------
def rpy_R(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def quat_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_quat(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    q = np.array(q)
    return -q if q[3] < 0 else q


def pose7(R, t):
    return np.concatenate([np.asarray(t, np.float64), R_quat(np.asarray(R, np.float64))])


def pose7_Rt(p):
    p = np.asarray(p, np.float64)
    return quat_R(p[3:7]), p[0:3].copy()


def rel7(a7, b7):
    """a^-1 * b"""
    Ra, ta = pose7_Rt(a7)
    Rb, tb = pose7_Rt(b7)
    return pose7(Ra.T @ Rb, Ra.T @ (tb - ta))


# ---- world ---------------------------------------------------------------------------------------------------------------------
def _grid(rng, n, spacing, jitter, centre):
    """n points on distinct cells of a square grid around `centre`, each jittered by at most `jitter` per axis."""
    if n == 0:
        return np.zeros((0, 2))
    side = int(math.ceil(math.sqrt(n)))
    cells = rng.permutation(side * side)[:n]
    ij = np.stack([cells // side, cells % side], axis=1).astype(np.float64) - 0.5 * (side - 1)
    return np.asarray(centre)[None, :2] + spacing * ij + rng.uniform(-jitter, jitter, (n, 2))


@functools.lru_cache(maxsize=None)
def make_world(seed, n_cyl, n_cube, n_ell, centre=(40.0, -25.0)):
    """A seeded world: n objects per class on jittered grids (spacing above the class's match threshold) and N_POOL more per class in
    a row beyond every grid, at least 6 m from anything.  Cylinders are upright with a small tilt, cubes carry roll, pitch and yaw."""
    rng = np.random.default_rng(seed)
    n = dict(cyl=n_cyl, cube=n_cube, ell=n_ell)
    half = max(SPACING[c] * (math.ceil(math.sqrt(max(n[c], 1))) + 1) / 2 for c in CLS)
    w = dict(n=n, centre=np.array([centre[0], centre[1], 1.5]))
    for ci, c in enumerate(CLS):
        xy = _grid(rng, n[c], SPACING[c], JITTER[c], centre)
        pool = np.stack([centre[0] - half + 6.0 * np.arange(N_POOL), np.full(N_POOL, centre[1] + half + 8.0 + 6.0 * ci)], axis=1)
        xy = np.concatenate([xy, pool + rng.uniform(-0.5, 0.5, (N_POOL, 2))])
        m = len(xy)
        if c == "cyl":
            z = rng.uniform(-0.2, 0.2, m)
            ray = np.concatenate([rng.uniform(-0.05, 0.05, (m, 2)), np.ones((m, 1))], axis=1)
            w[c] = dict(pos=np.column_stack([xy, z]), ray=ray / np.linalg.norm(ray, axis=1)[:, None], radius=rng.uniform(0.1, 0.4, m))
        elif c == "cube":
            z = rng.uniform(0.5, 1.5, m)
            Rw = np.array([rpy_R(*a) for a in np.column_stack([rng.uniform(-0.2, 0.2, (m, 2)), rng.uniform(-math.pi, math.pi, m)])])
            w[c] = dict(pos=np.column_stack([xy, z]), R=Rw.reshape(m, 3, 3), scale=rng.uniform(0.5, 2.0, (m, 3)))
        else:
            z = rng.uniform(0.0, 3.0, m)
            w[c] = dict(pos=np.column_stack([xy, z]), scale=rng.uniform(0.2, 1.0, (m, 3)))
        w[c]["label"] = rng.choice(LABELS[c], m).astype(np.int32)
    return w


def empty_det():
    return dict(cyl_root=np.zeros((0, 3)), cyl_ray=np.zeros((0, 3)), cyl_radius=np.zeros(0), cyl_label=np.zeros(0, np.int32),
                cube_pose7=np.zeros((0, 7)), cube_scale=np.zeros((0, 3)), cube_label=np.zeros(0, np.int32),
                ell_pose7=np.zeros((0, 7)), ell_scale=np.zeros((0, 3)), ell_label=np.zeros(0, np.int32))


def detect(world, p7, pick, rng, noise=0.02, relabel=None):
    """Body-frame detections, at the pose p7, of the objects pick[cls] (indices into the world's tables, in that order) with
    Gaussian position noise; relabel[cls] = {position in pick[cls]: label} overrides labels.  The dict process_frame takes."""
    R, t = pose7_Rt(p7)
    relabel = relabel or {}
    d = empty_det()
    for c in CLS:
        idx = np.asarray(pick.get(c, []), np.int64)
        m = len(idx)
        if m == 0:
            continue
        o = world[c]
        pb = (o["pos"][idx] - t) @ R + rng.normal(0, noise, (m, 3))          # rows: R^T (p - t)
        lab = o["label"][idx].copy()
        for k, v in relabel.get(c, {}).items():
            lab[k] = v
        d[c + "_label"] = lab.astype(np.int32)
        if c == "cyl":
            d["cyl_root"] = pb
            d["cyl_ray"] = o["ray"][idx] @ R + rng.normal(0, 0.1 * noise, (m, 3))
            d["cyl_radius"] = o["radius"][idx] + rng.normal(0, 0.01, m)
        elif c == "cube":
            d["cube_pose7"] = np.array([pose7(R.T @ o["R"][i], pb[k]) for k, i in enumerate(idx)])
            d["cube_scale"] = o["scale"][idx] + rng.normal(0, 0.02, (m, 3))
        else:
            d["ell_pose7"] = np.column_stack([pb, np.tile(R_quat(R.T), (m, 1))])
            d["ell_scale"] = o["scale"][idx] + rng.normal(0, 0.02, (m, 3))
    return d


def det_exact(cyl=(), cube=(), ell=()):
    """Detections at GIVEN body positions (cylinders: root, ray (0, 0, 1)); items are (xyz, label).  With an identity rotation and
    dyadic coordinates the projection to the world frame is exact, which is what the tie cases need."""
    d = empty_det()
    if cyl:
        d["cyl_root"] = np.array([p for p, _ in cyl], np.float64)
        d["cyl_ray"] = np.tile([0.0, 0.0, 1.0], (len(cyl), 1))
        d["cyl_radius"] = np.full(len(cyl), 0.25)
        d["cyl_label"] = np.array([l for _, l in cyl], np.int32)
    for c, items in (("cube", cube), ("ell", ell)):
        if items:
            d[c + "_pose7"] = np.array([np.concatenate([np.asarray(p, np.float64), [0, 0, 0, 1.0]]) for p, _ in items])
            d[c + "_scale"] = np.full((len(items), 3), 0.5)
            d[c + "_label"] = np.array([l for _, l in items], np.int32)
    return d


# ---- the plain reference -------------------------------------------------------------------------------------------------------
def project(p7, det):
    """projectModels in numpy (double): world-frame cylinders (n, 7) [root ray radius], cube and ellipsoid positions (n, 3)."""
    R, t = pose7_Rt(p7)
    nc = len(det["cyl_label"])
    cyl = np.zeros((nc, 7))
    if nc:
        root, ray = np.asarray(det["cyl_root"], np.float64), np.asarray(det["cyl_ray"], np.float64)
        cyl[:, 0:3] = root @ R.T + t
        cyl[:, 3:6] = ray @ R.T
        cyl[:, 6] = det["cyl_radius"]
    out = dict(cyl=cyl)
    for c in ("cube", "ell"):
        p = np.asarray(det[c + "_pose7"], np.float64).reshape(-1, 7)
        out[c] = p[:, 0:3] @ R.T + t
    return out


def cylinder_distance(models, tgt):
    """Cylinder::distance of every map cylinder (m, 7) to one detection (7,): the smallest distance between the two axes' points at the
    heights 0, 3 and 6 m (labels are the caller's business)."""
    best = np.full(len(models), 10000.0)
    for h in (0.0, 3.0, 6.0):
        st = (h - models[:, 2]) / models[:, 5]
        tt = (h - tgt[2]) / tgt[5]
        d = (models[:, 0:3] + st[:, None] * models[:, 3:6]) - (tgt[0:3] + tt * tgt[3:6])
        best = np.minimum(best, np.sqrt((d * d).sum(axis=1)))
    return best


def gate(cloud_f32, t, K):
    """The submap: map indices of the min(K, n) cloud points nearest to the pose translation, float32 arithmetic
    (r = dx*dx; r += dy*dy; r += dz*dz), nearest first, equal distances by index."""
    n = len(cloud_f32)
    if n == 0:
        return np.zeros(0, np.int64)
    q = np.asarray(t, np.float64).astype(np.float32)
    d = cloud_f32.astype(np.float32) - q[None, :]
    r = d[:, 0] * d[:, 0]
    r = r + d[:, 1] * d[:, 1]
    r = r + d[:, 2] * d[:, 2]
    assert r.dtype == np.float32
    return np.lexsort((np.arange(n), r))[: min(K, n)]


def numpy_frame_reference(maps, p7, det, K3=K_DEFAULT, thresholds=None, first_host=False):
    """One frame: maps[cls] = dict(model=(n, 7) or (n, 3+), label=(n,)) as the backend holds them BEFORE the frame (the cloud is
    float32 of the model position: true while nothing has refreshed the map), p7 the pose estimate.  Returns per class
    dict(match, id, margin): the match's position in the nearest-first submap or -1, its map index or -1, and the smaller of the
    relative gaps best / second-best admissible distance and best / threshold (inf when nothing is admissible).
    first_host: the first HOST frame of a backend is never matched."""
    thr = dict(THRESH, **(thresholds or {}))
    _, t = pose7_Rt(p7)
    world = project(p7, det)
    out = {}
    for ci, c in enumerate(CLS):
        nd = len(det[c + "_label"])
        match, mid, margin = np.full(nd, -1, np.int32), np.full(nd, -1, np.int32), np.full(nd, np.inf)
        model = np.asarray(maps[c]["model"], np.float64).reshape(len(maps[c]["label"]), 7 if c == "cyl" else 3)
        sub = gate(model[:, 0:3].astype(np.float32), t, K3[ci])
        if not first_host and len(sub) and nd:
            sm, sl = model[sub], np.asarray(maps[c]["label"])[sub]
            for o in range(nd):
                if c == "cyl":
                    d = cylinder_distance(sm, world[c][o])
                else:
                    e = sm[:, 0:3] - world[c][o][None, :]
                    d = np.sqrt((e * e).sum(axis=1))
                adm = d < BEST_INIT[c]
                if LABEL_GATE[c]:
                    adm &= sl == det[c + "_label"][o]
                if not adm.any():
                    continue
                d = np.where(adm, d, np.inf)
                j = int(np.argmin(d))                                  # the first of equal distances: the earlier submap position
                d1 = d[j]
                margin[o] = abs(d1 - thr[c]) / thr[c]
                if d1 < thr[c]:
                    match[o], mid[o] = j, sub[j]
                    d2 = np.partition(d, 1)[1] if len(d) > 1 else np.inf
                    gap = 1.0 if np.isinf(d2) else (0.0 if d2 == 0 else (d2 - d1) / d2)
                    margin[o] = min(margin[o], gap)
        out[c] = dict(match=match, id=mid, margin=margin)
    return out


# ---- running a case ------------------------------------------------------------------------------------------------------------
class Case:
    """ops: dicts op='frame' (mode, robot, rel7, prev7 or None = the backend's own last pose of that robot, det, pose7 = the pose
    estimate when the case knows it), op='ingest_solve', op='end_frame' (robot).  ties: {(op index, cls, detection)} built to tie."""

    def __init__(self, name, ops, knn=K_DEFAULT, n_robots=1, ties=(), world=None):
        self.name, self.ops, self.knn, self.n_robots, self.ties, self.world = name, ops, tuple(knn), n_robots, set(ties), world
        self.foreign_only = all(o["op"] == "frame" and o["mode"] == FRAME_FOREIGN for o in ops)


def frame_op(mode, robot, rel, prev, det):
    return dict(op="frame", mode=mode, robot=robot, rel7=np.asarray(rel, np.float64), prev7=None if prev is None else np.asarray(prev, np.float64), det=det)


def foreign_ops(poses7, dets, robot=0):
    ops = []
    for k, (p, d) in enumerate(zip(poses7, dets)):
        ops.append(frame_op(FRAME_FOREIGN, robot, p if k == 0 else rel7(poses7[k - 1], p), p, d))
    return ops


def read_new_models(backend, maps):
    """Extend maps[cls] (model, label, hits lists) by the landmarks the backend has and the mirror has not, through map_model."""
    cnt = backend.counts()
    for ci, c in enumerate(CLS):
        for i in range(len(maps[c]["label"]), cnt[COUNT_KEY[ci]]):
            st, m, hits, label = backend.map_model(ci, i)
            assert st == 0, (c, i, st)
            maps[c]["model"].append(np.array(m[: 7 if ci == 0 else 3], np.float64))
            maps[c]["label"].append(label)
    return maps


def empty_maps():
    return {c: dict(model=[], label=[]) for c in CLS}


def run_case(backend, case, before_frame=None, after_op=None):
    """Feed the case's calls to a backend.  Returns one dict per op: a frame's result dict (+ 'counts'), or dict(status, pose7).
    before_frame(k, op, prev7) runs before a frame is processed, after_op(k, op, result) after every call."""
    last = {}
    out = []
    for k, op in enumerate(case.ops):
        if op["op"] == "frame":
            prev = op["prev7"] if op["prev7"] is not None else last.get(op["robot"], IDENT7)
            if before_frame:
                before_frame(k, op, prev)
            r = backend.process_frame(op["robot"], op["rel7"], prev, op["det"], op["mode"])
            if op["mode"] != FRAME_FOREIGN:
                last[op["robot"]] = np.array(r["pose7"], np.float64)
            r = dict(r, counts=backend.counts())
        elif op["op"] == "ingest_solve":
            r = dict(status=int(backend.ingest_solve()))
        else:
            st, p = backend.end_frame(op["robot"])
            last[op["robot"]] = np.array(p, np.float64)
            r = dict(status=int(st), pose7=last[op["robot"]])
        if after_op:
            after_op(k, op, r)
        out.append(r)
    return out


def check_against_numpy(backend, case, results=None):
    """FOREIGN-only cases: run the case on `backend` and compare every frame with numpy_frame_reference on the map read back from
    that backend before the frame (margin rule: only detections with margin > MARGIN; the case's named ties are exempt from it,
    every other detection must be above it), and the models of the landmarks a frame created with R b + t from numpy (1e-12
    relative: a handful of double operations on values of size <= 100).  Returns (results, number of detections under the margin)."""
    assert case.foreign_only
    maps = empty_maps()
    state = {}
    under = []

    def before(k, op, prev):
        read_new_models(backend, maps)
        state["ref"] = numpy_frame_reference(maps, prev, op["det"], case.knn)
        state["n0"] = {c: len(maps[c]["label"]) for c in CLS}

    def after(k, op, r):
        ref = state["ref"]
        world = project(op["prev7"], op["det"])
        read_new_models(backend, maps)
        for c in CLS:
            low = ref[c]["margin"] <= MARGIN
            for o in np.nonzero(low)[0]:
                if (k, c, int(o)) not in case.ties:
                    under.append((k, c, int(o), float(ref[c]["margin"][o])))
            named = [o for (kk, cc, o) in case.ties if kk == k and cc == c]
            assert all(low[o] for o in named), (case.name, k, c, "a detection named as a tie does not tie", ref[c]["margin"][named])
            ok = ~low
            assert np.array_equal(r[c + "_match"][ok], ref[c]["match"][ok]), (case.name, k, c, "match", r[c + "_match"], ref[c]["match"])
            exp_id = ref[c]["id"].copy()
            new = np.nonzero(r[c + "_match"] == -1)[0]
            exp_id[new] = state["n0"][c] + np.arange(len(new))         # a new landmark's id is the next free map index
            assert np.array_equal(r[c + "_id"][ok], exp_id[ok]), (case.name, k, c, "id", r[c + "_id"], exp_id)
            assert len(maps[c]["label"]) == state["n0"][c] + len(new), (case.name, k, c, "map growth")
            for j, o in enumerate(new):
                got, want = maps[c]["model"][state["n0"][c] + j], world[c][o]
                assert maps[c]["label"][state["n0"][c] + j] == op["det"][c + "_label"][o]
                if c == "cyl":
                    assert np.linalg.norm(got[0:3] - want[0:3]) <= 1e-12 * np.linalg.norm(want[0:3]), (case.name, k, c, o, "root")
                    assert np.linalg.norm(got[3:6] - want[3:6]) <= 1e-12 * np.linalg.norm(want[3:6]), (case.name, k, c, o, "ray")
                    assert got[6] == want[6]
                else:
                    assert np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want), (case.name, k, c, o, "position")

    res = run_case(backend, case, before, after)
    return res, under


def compare_results(case, got, ref, what=("match", "id")):
    """Per op and per detection: *_match, *_id, counts and status of two runs of a case are identical."""
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g["status"] == 0 and r["status"] == 0, (case.name, k, g["status"], r["status"])
        if case.ops[k]["op"] != "frame":
            continue
        for c in CLS:
            for f in what:
                assert np.array_equal(g[f"{c}_{f}"], r[f"{c}_{f}"]), (case.name, k, f"{c}_{f}", g[f"{c}_{f}"], r[f"{c}_{f}"])
        for key in COUNT_KEY + ("factors",):
            assert g["counts"][key] == r["counts"][key], (case.name, k, key, g["counts"][key], r["counts"][key])
        assert np.array_equal(g["counts"]["poses"][: case.n_robots], r["counts"]["poses"][: case.n_robots]), (case.name, k, "poses")


def ranks_off_distance_order(maps, p7, result):
    """How many matches of a frame have a submap position (nearest-first by the first-seen float32 cloud) that is NOT the number of
    landmarks whose current MODEL lies nearer to the pose: the refreshed models have moved off the cloud."""
    t = np.asarray(p7[0:3], np.float64)
    off = 0
    for c in CLS:
        if not len(maps[c]["label"]):
            continue
        d = np.linalg.norm(np.array([m[0:3] for m in maps[c]["model"]]) - t, axis=1)
        for rank, i in zip(result[c + "_match"], result[c + "_id"]):
            if rank >= 0:
                off += int((d < d[i]).sum() != rank)
    return off


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _pose(world, dx, dy, yaw, roll=0.3, pitch=-0.3):
    return pose7(rpy_R(roll, pitch, yaw), world["centre"] + np.array([dx, dy, 0.0]))


def _nearest(world, c, p7, n=None):
    """The grid objects of a class (not the pool), nearest to the pose first."""
    t = np.asarray(p7[0:3])
    d = np.linalg.norm(world[c]["pos"][: world["n"][c]] - t, axis=1)
    return np.argsort(d, kind="stable")[:n]


def _seed_det(world, p7, rng):
    return detect(world, p7, {c: np.arange(world["n"][c]) for c in CLS}, rng)


def _other_label(c, lab):
    return next(l for l in LABELS[c] if l != lab)


def _counted_det(world, p7, n3, rng, pool_from=0):
    """A frame of exactly n3 = (cylinders, cubes, ellipsoids) detections: mostly the nearest objects, a fifth of them the FARTHEST
    (beyond the gate when K < n: they become second landmarks of their objects), up to 3 pool objects (far from every landmark: new
    landmarks), up to 3 with a label no landmark has, and up to 2 cylinders with the right place and the other cylinder label."""
    pick, relabel = {}, {}
    for c, n in zip(CLS, n3):
        n_pool = min(n // 8, 3)
        n_bad = min(n // 8, 3)
        n_wrong = min(n // 8, 2) if c == "cyl" else 0
        n_real = min(n - n_pool, world["n"][c])
        n_pool = n - n_real
        assert n_pool <= N_POOL - pool_from
        order = _nearest(world, c, p7)
        n_farthest = n_real // 5
        idx = np.concatenate([order[: n_real - n_farthest], order[len(order) - n_farthest:] if n_farthest else order[:0],
                              world["n"][c] + pool_from + np.arange(n_pool)]).astype(np.int64)
        rl = {k: NO_SUCH_LABEL for k in range(n_bad)}
        rl.update({n_bad + k: _other_label(c, world[c]["label"][idx[n_bad + k]]) for k in range(n_wrong)})
        perm = rng.permutation(n)
        inv = np.argsort(perm)
        pick[c] = idx[perm]
        relabel[c] = {int(inv[k]): v for k, v in rl.items()}
    return detect(world, p7, pick, rng, relabel=relabel)


def _followup_det(world, p7, rng, pool_seen=3, again=None):
    """A small normal frame: the five nearest objects of each class, the pool objects an earlier frame turned into landmarks, one new,
    and — again = (pose, counts) of an earlier _counted_det frame — that frame's unknown-label detections once more: they match the
    landmarks that frame created, inside the gate."""
    pick, relabel = {}, {}
    for ci, c in enumerate(CLS):
        parts = [_nearest(world, c, p7, 5), world["n"][c] + np.arange(min(pool_seen + 1, N_POOL))]
        if again is not None:
            n_bad = min(min(again[1][ci] // 8, 3), world["n"][c])
            relabel[c] = {len(parts[0]) + len(parts[1]) + k: NO_SUCH_LABEL for k in range(n_bad)}
            parts.append(_nearest(world, c, again[0], n_bad))
        pick[c] = np.concatenate(parts).astype(np.int64)
    return detect(world, p7, pick, rng, relabel=relabel)


DET_COUNTS = [(0, 0, 0), (1, 1, 1), (16, 16, 16), (17, 17, 17), (32, 33, 49), (33, 48, 64), (40, 49, 65), (40, 65, 100)]


def case_det_counts(i):
    """Seed 120 / 80 / 1500 landmarks in one FOREIGN frame, then a frame of DET_COUNTS[i] detections, then a small normal frame."""
    w = make_world(11, 120, 80, 1500)
    rng = np.random.default_rng(100 + i)
    poses = [_pose(w, 0, 0, 0.4), _pose(w, 3.0, -2.0, 1.1), _pose(w, -4.0, 1.0, -2.0, roll=-0.3, pitch=0.2)]
    dets = [_seed_det(w, poses[0], rng), _counted_det(w, poses[1], DET_COUNTS[i], rng),
            _followup_det(w, poses[2], rng, again=(poses[1], DET_COUNTS[i]))]
    return Case(f"det_counts_{'_'.join(map(str, DET_COUNTS[i]))}", foreign_ops(poses, dets), world=w)


KNN_K = (1, 2, 63, 64, 65, 128, 129)


def knn_sizes(K):
    return (K - 1, K, K + 1, 3 * K)


def case_knn(K, n):
    """K for all three gates against maps of n landmarks per class: seed, a frame of 17 / 17 / 17 or fewer, a small normal frame."""
    w = make_world(1000 * K + n, n, n, n)
    rng = np.random.default_rng(7 * K + n)
    poses = [_pose(w, 0, 0, -0.7), _pose(w, 2.0, 1.5, 2.2), _pose(w, -1.0, -3.0, 0.3, roll=0.2, pitch=0.3)]
    m = min(17, n + 2)
    dets = [_seed_det(w, poses[0], rng), _counted_det(w, poses[1], (m, m, m), rng),
            _followup_det(w, poses[2], rng, pool_seen=2, again=(poses[1], (m, m, m)))]
    if n == 0:
        poses, dets = poses[1:], dets[1:]
    return Case(f"knn_K{K}_n{n}", foreign_ops(poses, dets), knn=(K, K, K), world=w)


def case_ell_k5000():
    """K = 5000 ellipsoid neighbours of a map of 6000 (cylinders and cubes: small maps at the default K)."""
    w = make_world(5000, 20, 20, 6000)
    rng = np.random.default_rng(5000)
    poses = [_pose(w, 0, 0, 0.1), _pose(w, 5.0, 5.0, 1.9)]
    dets = [_seed_det(w, poses[0], rng), _counted_det(w, poses[1], (9, 9, 40), rng)]
    return Case("ell_K5000_n6000", foreign_ops(poses, dets), knn=(50, 30, 5000), world=w)


BEYOND_CACHE_N = 33537


def case_beyond_cache():
    """Ellipsoids only, a map one landmark beyond the LDS distance cache, frames of 20 and 70 detections."""
    w = make_world(33, 0, 0, BEYOND_CACHE_N)
    rng = np.random.default_rng(33)
    poses = [_pose(w, 0, 0, 0.0), _pose(w, 10.0, -6.0, 0.8), _pose(w, -20.0, 15.0, -1.4)]
    dets = [detect(w, poses[0], dict(ell=np.arange(BEYOND_CACHE_N)), rng),
            _counted_det(w, poses[1], (0, 0, 20), rng), _counted_det(w, poses[2], (0, 0, 70), rng, pool_from=3)]
    return Case("beyond_cache", foreign_ops(poses, dets), world=w)


def case_empty_maps(which):
    """which = 'all': detections of every class on empty maps (the first FOREIGN frame), then a frame that matches them;
    'cyl' / 'cube' / 'ell': that class's map stays empty through the seeding and meets detections in the second frame;
    'no_dets_first': the first frame has no detections at all (empty maps, nothing to do), then a normal one."""
    n = {c: (0 if c == which else 30) for c in CLS}
    w = make_world(50 + len(which), n["cyl"], n["cube"], n["ell"])
    rng = np.random.default_rng(len(which))
    poses = [_pose(w, 0, 0, 0.5), _pose(w, 1.0, 2.0, -0.9), _pose(w, -2.0, 0.5, 2.8)]
    if which == "all":
        dets = [_counted_det(w, poses[0], (12, 12, 12), rng), _counted_det(w, poses[1], (12, 12, 12), rng), _followup_det(w, poses[2], rng, 1)]
    elif which == "no_dets_first":
        dets = [empty_det(), _seed_det(w, poses[1], rng), _followup_det(w, poses[2], rng, 0)]
    else:
        n3 = tuple(6 if c == which else 10 for c in CLS)          # (the empty class: pool objects only)
        dets = [_seed_det(w, poses[0], rng), _counted_det(w, poses[1], n3, rng), _followup_det(w, poses[2], rng, 1)]
    return Case(f"empty_maps_{which}", foreign_ops(poses, dets), world=w)


T0 = np.array([32.0, -16.0, 2.0])       # the tie cases' pose: identity rotation, dyadic coordinates (every sum below is exact)


def case_ties():
    """Identity rotation and dyadic coordinates, so that equal distances are EXACTLY equal on every side.
    Frame 0 creates, per class: two landmarks at P1 and five at P2 (equal cloud keys up to the index), two landmarks 2 d apart around
    P3 (the FARTHER from the robot first, so the lowest map index is not the earlier submap position), and — cubes and ellipsoids —
    two coincident landmarks of different labels at P4.  Frames 1 and 2 (another pose: other ranks) detect exactly P1, P2, P3 and P4."""
    P1, P2, P3, P4 = np.array([4.0, 3.0, 1.0]), np.array([-6.0, 2.0, 0.5]), np.array([8.0, -5.0, 1.0]), np.array([2.0, 8.0, 1.5])
    ex = np.array([1.0, 0.0, 0.0])

    def z0(p):
        return np.array([p[0], p[1], 0.0])

    def create(shift):
        cyl = [(z0(P1) - shift, 10)] * 2 + [(z0(P2) - shift, 11)] * 5 + [(z0(P3) + ex - shift, 10), (z0(P3) - ex - shift, 10)]
        cube = [(P1 - shift, 20)] * 2 + [(P2 - shift, 21)] * 5 + [(P3 + 0.5 * ex - shift, 20), (P3 - 0.5 * ex - shift, 20),
                                                                 (P4 - shift, 20), (P4 - shift, 21)]
        ell = [(P1 - shift, 30)] * 2 + [(P2 - shift, 31)] * 5 + [(P3 + 0.25 * ex - shift, 32), (P3 - 0.25 * ex - shift, 32),
                                                                 (P4 - shift, 33), (P4 - shift, 34)]
        return det_exact(cyl, cube, ell)

    def look(shift):
        cyl = [(z0(P1) - shift, 10), (z0(P2) - shift, 11), (z0(P3) - shift, 10)]
        cube = [(P1 - shift, 20), (P2 - shift, 21), (P3 - shift, 20), (P4 - shift, 21), (P4 - shift, 20)]
        ell = [(P1 - shift, 30), (P2 - shift, 31), (P3 - shift, 32), (P4 - shift, 34), (P4 - shift, 33)]
        return det_exact(cyl, cube, ell)

    s2 = np.array([1.0, 0.5, 0.0])
    poses = [np.concatenate([T0, [0, 0, 0, 1.0]]), np.concatenate([T0, [0, 0, 0, 1.0]]), np.concatenate([T0 + s2, [0, 0, 0, 1.0]])]
    dets = [create(0 * s2), look(0 * s2), look(s2)]
    # built to tie: every cylinder detection, cubes P1 P2 P3 and both at P4 (no label gate), ellipsoids P1 P2 P3 (not P4: one admissible)
    ties = {(k, "cyl", o) for k in (1, 2) for o in range(3)} | {(k, "cube", o) for k in (1, 2) for o in range(5)} \
        | {(k, "ell", o) for k in (1, 2) for o in range(3)}
    # what the rule says, for the test to pin: (id per detection) cyl, cube, ell
    expect = dict(cyl=[0, 2, 8], cube=[0, 2, 8, 9, 9], ell=[0, 2, 8, 10, 9])
    c = Case("ties", foreign_ops(poses, dets), ties=ties)
    c.expect_id = expect
    return c


TIES_MANY = 130


def case_ties_many():
    """K = 200 / 200 / 1000.  Frame 0 creates three landmarks next to the robot and then TIES_MANY = 130 coincident landmarks of one
    label per class: more than a wavefront has lanes, so one lane meets two or three exactly tied candidates (in an order the
    select's compaction does not fix) and has to keep the lowest key itself before the lanes are reduced.  Frames 1 and 2 detect that
    spot: landmark 3, the first of the 130, at position 3 of the submap."""
    near = [np.array([0.5, 0.0, 0.0]), np.array([0.0, -0.75, 0.0]), np.array([-1.0, 0.0, 0.25])]
    P = np.array([6.0, 4.0, 0.5])
    Pc = np.array([6.0, 4.0, 0.0])

    def frame(shift, create):
        m = TIES_MANY if create else 1
        return det_exact([(p * [1, 1, 0] - shift, 10) for p in near] + [(Pc - shift, 11)] * m,
                         [(p - shift, 20) for p in near] + [(P - shift, 21)] * m, [(p - shift, 30) for p in near] + [(P - shift, 31)] * m)

    s2 = np.array([0.25, -0.5, 0.0])
    I = [0, 0, 0, 1.0]
    poses = [np.concatenate([T0, I]), np.concatenate([T0, I]), np.concatenate([T0 + s2, I])]
    c = Case("ties_many", foreign_ops(poses, [frame(0 * s2, True), frame(0 * s2, False), frame(s2, False)]), knn=(200, 200, 1000),
             ties={(k, cl, 3) for k in (1, 2) for cl in CLS})
    c.expect_id, c.expect_match = [0, 1, 2, 3], {1: [0, 1, 2, 3], 2: None}
    return c


def case_gate_tie():
    """K = 2: landmark 0 next to the robot, landmarks 1 and 2 EQUIDISTANT from it (r = 4 exactly): the gate keeps the lower index.
    A detection exactly at landmark 1 matches (position 1 in the submap), one at landmark 2 finds only 0 and 1 — both beyond the
    threshold — and becomes a new landmark, in frame 1 and again in frame 2 (then three cloud points tie behind the cut)."""
    pts = [np.array([0.5, 0.0, 0.0]), np.array([2.0, 0.0, 0.0]), np.array([0.0, 2.0, 0.0])]
    d = det_exact([(p, 10) for p in pts], [(p, 20) for p in pts], [(p, 30) for p in pts])
    p = np.concatenate([T0, [0, 0, 0, 1.0]])
    c = Case("gate_tie", foreign_ops([p, p, p], [d, d, d]), knn=(2, 2, 2))
    c.expect_id = [[0, 1, 3], [0, 1, 4]]           # frames 1 and 2, the same for every class
    c.expect_match = [0, 1, -1]
    return c


def _host_frame(mode, gt_prev, gt, det, rng, first=False):
    if first:
        return frame_op(mode, 0, gt, IDENT7, det)                  # prevKeyPose = identity for the first key frame
    R, t = pose7_Rt(rel7(gt_prev, gt))
    noisy = pose7(R @ rpy_R(*rng.normal(0, 0.003, 3)), t + rng.normal(0, 0.02, 3))
    return frame_op(mode, 0, noisy, None, det)


def case_host_rank():
    """HOST-mode frames with 0.04 m detection noise and gates of K = 20 / 10 / 100 on maps of 40 / 30 / 300: the first frame (never
    matched) seeds every landmark, every solve then moves the models off the first-seen cloud, so the nearest-first order of the
    submap (cloud, float32) and the order of the model distances differ.  The third frame is HOST_DEFERRED + end_frame."""
    w = make_world(77, 40, 30, 300)
    rng = np.random.default_rng(77)
    gts = [_pose(w, 0, 0, 0.2, 0.1, -0.1), _pose(w, 1.5, 0.5, 0.35, 0.3, -0.3), _pose(w, 3.0, 1.5, 0.5, -0.3, 0.3), _pose(w, 4.0, 3.0, 0.7, 0.3, 0.3)]
    ops = [_host_frame(FRAME_HOST, None, gts[0], detect(w, gts[0], {c: np.arange(w["n"][c]) for c in CLS}, rng, noise=0.04), rng, first=True)]
    for k in (1, 2, 3):
        pick = {c: np.concatenate([_nearest(w, c, gts[k], m), w["n"][c] + np.arange(k)]) for c, m in zip(CLS, (18, 12, 60))}
        ops.append(_host_frame(FRAME_HOST_DEFERRED if k == 2 else FRAME_HOST, gts[k - 1], gts[k], detect(w, gts[k], pick, rng, noise=0.04), rng))
        if k == 2:
            ops.append(dict(op="end_frame", robot=0))
    return Case("host_rank", ops, knn=(20, 10, 100), world=w)


def case_multi_robot():
    """The order replay_multi uses on one map: a HOST_DEFERRED frame of robot 0, three FOREIGN frames of robot 1 that add landmarks,
    ingest_solve, end_frame, one more HOST frame."""
    w = make_world(88, 30, 20, 100)
    rng = np.random.default_rng(88)
    g0, g1 = _pose(w, -3.0, 0, 0.0, 0.1, 0.1), _pose(w, -1.5, 0.5, 0.2, 0.3, -0.3)
    f = [_pose(w, 6.0, 4.0, 2.0, -0.3, 0.3), _pose(w, 7.5, 3.0, 2.2, 0.3, 0.3), _pose(w, 9.0, 2.5, 2.5, 0.2, -0.3)]

    def near(p, k):
        return {c: np.concatenate([_nearest(w, c, p, m), w["n"][c] + np.arange(k)]) for c, m in zip(CLS, (12, 9, 35))}

    ops = [_host_frame(FRAME_HOST_DEFERRED, None, g0, detect(w, g0, near(g0, 0), rng, noise=0.03), rng, first=True)]
    for k, p in enumerate(f):
        ops.append(frame_op(FRAME_FOREIGN, 1, p if k == 0 else rel7(f[k - 1], p), p, detect(w, p, near(p, k + 1), rng, noise=0.03)))
    ops += [dict(op="ingest_solve"), dict(op="end_frame", robot=0)]
    ops.append(_host_frame(FRAME_HOST, g0, g1, detect(w, g1, near(g1, 4), rng, noise=0.03), rng))
    return Case("multi_robot", ops, n_robots=2, world=w)


FOREIGN_CASES = {}
for _i in range(len(DET_COUNTS)):
    FOREIGN_CASES["det_counts_" + "_".join(map(str, DET_COUNTS[_i]))] = functools.partial(case_det_counts, _i)
for _K in KNN_K:
    for _n in knn_sizes(_K):
        FOREIGN_CASES[f"knn_K{_K}_n{_n}"] = functools.partial(case_knn, _K, _n)
for _w in ("all", "cyl", "cube", "ell", "no_dets_first"):
    FOREIGN_CASES["empty_maps_" + _w] = functools.partial(case_empty_maps, _w)
FOREIGN_CASES["ell_K5000_n6000"] = case_ell_k5000
FOREIGN_CASES["beyond_cache"] = case_beyond_cache
FOREIGN_CASES["ties"] = case_ties
FOREIGN_CASES["ties_many"] = case_ties_many
FOREIGN_CASES["gate_tie"] = case_gate_tie
HOST_CASES = {"host_rank": case_host_rank, "multi_robot": case_multi_robot}


@functools.lru_cache(maxsize=None)
def get_case(name):
    return (FOREIGN_CASES.get(name) or HOST_CASES[name])()
