"""Cases and plain references for the same-robot half of place recognition over a LIST of candidate key poses
(SLOAMNode::intraLoopClosureThread_, sloamNode.cpp:355-486): the submaps around the candidates (getkeyPoseSubmap of the three map
managers, cylinderMapManager.cpp:186-211, cubeMapManager.cpp:77-101, ellipsoidMapManager.cpp:82-107, then prepareLCInput,
sloamNode.cpp:544-576) and findIntraLoopClosure (place_recognition.cpp:389-496) per candidate.  Plain numpy on top of place_cases: no
GPU, no product import; the oracle is loaded only by intra_case() for the conditions the case must meet.  One elementary operation per
numpy call in source order, so nothing is contracted or re-associated.

The per-candidate sweep reference is built from the primitives slidematch_list_cases.list_reference is built from (place_cases'
lattice, sweep_counts and first_argmax) without its centring step: intra maps are swept as they are, over the fixed intra window."""
import ctypes as C
import math

import numpy as np

import place_cases as pc
import slidematch_list_cases as lc

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 600]      # chunk (256) and wave (64) edges of k_keypose_submap
RADIUS, MAX_DZ = 20.0, 1.5
MARGIN = 1e-9
F32 = np.float32


# ---- getkeyPoseSubmap x 3 + prepareLCInput ----------------------------------------------------------------------------------------------
def submap_distances(t, pose, float32_pose=True):
    """(distance(p) per object of the concatenated table, |model_z - pose_z| per object) for one pose.  float32_pose: the pose position
    goes through pcl's PointT (float32) for the distance, as the reference does; the height test always uses the double z."""
    p = [float(F32(v)) if float32_pose else float(v) for v in pose]
    px, py, pz = p
    r, a, rad = t["cyl_root"], t["cyl_ray"], t["cyl_radius"]
    ex, ey, ez = np.subtract(px, r[:, 0]), np.subtract(py, r[:, 1]), np.subtract(pz, r[:, 2])
    num = np.add(np.add(np.multiply(ex, a[:, 0]), np.multiply(ey, a[:, 1])), np.multiply(ez, a[:, 2]))
    den = np.add(np.add(np.multiply(a[:, 0], a[:, 0]), np.multiply(a[:, 1], a[:, 1])), np.multiply(a[:, 2], a[:, 2]))
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = np.divide(num, den)
    qx, qy, qz = (np.add(r[:, k], np.multiply(tt, a[:, k])) for k in range(3))
    dx, dy, dz = np.subtract(px, qx), np.subtract(py, qy), np.subtract(pz, qz)
    d_cyl = np.subtract(np.sqrt(np.add(np.add(np.multiply(dx, dx), np.multiply(dy, dy)), np.multiply(dz, dz))), rad)
    out_d, out_z = [d_cyl], [np.abs(np.subtract(r[:, 2], float(pose[2])))]
    for c in (t["cube_xyz"], t["ell_xyz"]):
        dx, dy, dz = np.subtract(c[:, 0], px), np.subtract(c[:, 1], py), np.subtract(c[:, 2], pz)
        out_d.append(np.sqrt(np.add(np.add(np.multiply(dx, dx), np.multiply(dy, dy)), np.multiply(dz, dz))))
        out_z.append(np.abs(np.subtract(c[:, 2], float(pose[2]))))
    return np.concatenate(out_d), np.concatenate(out_z)


def all_rows(t):
    """prepareLCInput of the WHOLE map: cylinders [label, root, radius, 0, 0], cubes and ellipsoids [label, centre, scale]"""
    n = len(t["cyl_label"])
    cyl = np.zeros((n, 7))
    cyl[:, 0], cyl[:, 1:4], cyl[:, 4] = t["cyl_label"], t["cyl_root"], t["cyl_radius"]
    rest = [np.concatenate([np.asarray(t[c + "_label"], np.float64)[:, None], t[c + "_xyz"], t[c + "_scale"]], axis=1) for c in ("cube", "ell")]
    return np.concatenate([cyl] + rest)


def submaps_reference(t, poses, radius=RADIUS, max_dz=MAX_DZ, float32_pose=True):
    """dict(sub_off, rows, src_idx, keep (n_poses, N), dist, dzs) — the rule of getkeyPoseSubmap, inclusive radius, strict height."""
    rows7 = all_rows(t)
    keep, dist, dzs = [], [], []
    for pose in poses:
        d, z = submap_distances(t, pose, float32_pose)
        keep.append(np.logical_and(np.less_equal(d, radius), np.less(z, max_dz)))
        dist.append(d)
        dzs.append(z)
    keep = np.array(keep, bool).reshape(len(poses), len(rows7))
    src = [np.nonzero(k)[0].astype(np.int32) for k in keep]
    off = np.zeros(len(poses) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in src])
    cat = np.concatenate(src) if src else np.zeros(0, np.int32)
    return dict(sub_off=off, rows=rows7[cat], src_idx=cat.astype(np.int32), keep=keep, dist=np.array(dist).reshape(keep.shape),
                dzs=np.array(dzs).reshape(keep.shape))


def tables_args(t):
    """the three table tuples of slide_slam_amd.keypose_submaps / intra_loop_closure_attempt"""
    return ((t["cyl_root"], t["cyl_ray"], t["cyl_radius"], t["cyl_label"]), (t["cube_xyz"], t["cube_scale"], t["cube_label"]),
            (t["ell_xyz"], t["ell_scale"], t["ell_label"]))


BOUNDARY_POSE = (0.0, 0.0, 0.0)                  # float-exact
WITNESS_POSE = (0.1, 7.3, 0.3)                   # none of these is a float32
BOX_BOUNDARIES = [                                # (offset from BOUNDARY_POSE, kept?) — exact in any evaluation order
    ("at_radius_kept", (20.0, 0.0, 0.0), True),
    ("next_above_radius_dropped", (math.nextafter(20.0, math.inf), 0.0, 0.0), False),
    ("dz_exactly_max_dropped", (1.0, 0.0, 1.5), False),
    ("dz_just_below_max_kept", (1.0, 0.0, math.nextafter(1.5, 0.0)), True),
]


def _random_map(rng, n_cyl, n_cube, n_ell, extent=45.0):
    def xyz(n):
        out = np.zeros((n, 3))
        out[:, :2] = rng.uniform(-extent, extent, (n, 2))
        out[:, 2] = rng.choice([0.0, 3.0], n) + rng.normal(0, 0.5, n)       # two floors: the height test drops the other one
        return out
    ray = np.column_stack([rng.normal(0, 0.1, n_cyl), rng.normal(0, 0.1, n_cyl), np.ones(n_cyl)]) * rng.uniform(0.5, 2.0, (n_cyl, 1))
    return dict(cyl_root=xyz(n_cyl), cyl_ray=ray, cyl_radius=rng.uniform(0.1, 0.5, n_cyl), cyl_label=rng.integers(1, 5, n_cyl).astype(np.int32),
                cube_xyz=xyz(n_cube), cube_scale=rng.uniform(0.3, 2.0, (n_cube, 3)), cube_label=rng.integers(1, 5, n_cube).astype(np.int32),
                ell_xyz=xyz(n_ell), ell_scale=rng.uniform(0.3, 2.0, (n_ell, 3)), ell_label=rng.integers(1, 5, n_ell).astype(np.int32))


def submap_case(i):
    """Case i of 10: class sizes (SIZES[i], SIZES[i + 3], SIZES[i + 6]) (indices mod 9), so that over cases 0..8 every class takes every
    size; case 9 has all three classes empty.  33 poses: the float-exact boundary pose, the witness pose (twice: second and last), a
    pose far from everything, random poses whose coordinates are no float32.  Conditions asserted here, on the CPU: the boundary
    objects are what they claim under the numpy restatement, every OTHER (pose, object) lies more than MARGIN from both thresholds
    (so a fused multiply-add on the device cannot flip it), and a restatement that skips the float32 step disagrees on an object."""
    if i == 9:
        sizes = (0, 0, 0)
    else:
        sizes = (SIZES[i], SIZES[(i + 3) % 9], SIZES[(i + 6) % 9])
    rng = np.random.default_rng(1000 + i)
    t = _random_map(rng, *sizes)
    n_cyl, n_cube, n_ell = sizes
    poses = np.zeros((33, 3))
    poses[:, :2] = rng.uniform(-30.0, 30.0, (33, 2))
    poses[:, 2] = rng.uniform(-0.5, 0.9, 33)
    poses[0], poses[1], poses[2], poses[32] = BOUNDARY_POSE, WITNESS_POSE, (500.1, 500.3, 0.7), WITNESS_POSE
    special = np.zeros((33, sum(sizes)), bool)          # (pose, object) pairs built to sit ON a threshold
    edges = dict(sizes=sizes, boundaries=[], witness=None)
    first = dict(cyl=0, cube=n_cyl, ell=n_cyl + n_cube)
    # boundary objects: the first objects of the first box class with room for them (and for the witness behind them)
    for c, n in (("cube", n_cube), ("ell", n_ell)):
        if n >= len(BOX_BOUNDARIES) + 1:
            for k, (name, off, _) in enumerate(BOX_BOUNDARIES):
                t[c + "_xyz"][k] = np.add(BOUNDARY_POSE, off)
                special[0, first[c] + k] = True
                edges["boundaries"].append((name, first[c] + k))
            break
    if n_cyl >= 2:                                       # ray (0, 0, 1), root offset (20.25, 0, 0.25), radius 0.25: distance exactly 20
        t["cyl_root"][0], t["cyl_ray"][0], t["cyl_radius"][0] = (20.25, 0.0, 0.25), (0.0, 0.0, 1.0), 0.25
        special[0, 0] = True
        edges["boundaries"].append(("cylinder_at_radius_kept", 0))
    # the float32 witness: 1e-8 inside the radius seen from the float32 pose, outside seen from the double pose (float32(7.3) - 7.3 = 1.9e-7)
    w32 = [float(F32(v)) for v in WITNESS_POSE]
    assert w32[1] - WITNESS_POSE[1] > 1e-7
    if max(n_cube, n_ell) >= 1:
        c = "cube" if n_cube >= n_ell else "ell"
        k = len(t[c + "_label"]) - 1
        t[c + "_xyz"][k] = (w32[0], w32[1] + 20.0 - 1e-8, w32[2])
        edges["witness"] = first[c] + k
    elif n_cyl >= 1:
        k = n_cyl - 1
        t["cyl_root"][k], t["cyl_ray"][k], t["cyl_radius"][k] = (w32[0], w32[1] + 20.25 - 1e-8, w32[2]), (0.0, 0.0, 1.0), 0.25
        edges["witness"] = k
    ref = submaps_reference(t, poses)
    for name, idx in edges["boundaries"]:
        want = dict((n, k) for n, _, k in BOX_BOUNDARIES).get(name, True)
        assert bool(ref["keep"][0, idx]) == want, (i, name)
    if sum(sizes):
        away = np.logical_and(np.abs(np.subtract(ref["dist"], RADIUS)) > MARGIN, np.abs(np.subtract(ref["dzs"], MAX_DZ)) > MARGIN)
        assert np.all(np.logical_or(away, special)), (i, "an ordinary object sits within MARGIN of a threshold")
        plain = submaps_reference(t, poses, float32_pose=False)
        assert edges["witness"] is not None and ref["keep"][1, edges["witness"]] and not plain["keep"][1, edges["witness"]], i
        assert not np.array_equal(ref["keep"], plain["keep"])
        assert ref["sub_off"][3] == ref["sub_off"][2], "the far pose has an empty submap"
    return dict(name=f"submaps_{i}", tables=t, poses=poses, radius=RADIUS, max_dz=MAX_DZ, ref=ref, edges=edges)


_SUBMAP_CACHE = {}


def submap_cases():
    if not _SUBMAP_CACHE:
        for i in range(10):
            _SUBMAP_CACHE[i] = submap_case(i)
        names = {n for c in _SUBMAP_CACHE.values() for n, _ in c["edges"]["boundaries"]}
        assert names == {n for n, _, _ in BOX_BOUNDARIES} | {"cylinder_at_radius_kept"}
        for cls in range(3):
            assert sorted(c["edges"]["sizes"][cls] for k, c in _SUBMAP_CACHE.items() if k < 9) == SIZES
    return _SUBMAP_CACHE


# ---- findIntraLoopClosure over a list of candidates ----------------------------------------------------------------------------------
X_HALF, Y_HALF, YAW_HALF = 5.0, 5.0, 10.0 * math.pi / 180.0      # match_{x,y,yaw}_half_range_intra, place_recognition.cpp:53-63


def quat_z(yaw):
    return np.array([0, 0, np.sin(yaw / 2), np.cos(yaw / 2)])


def to_map_frame(meas7, pose7):
    """the detections in the map frame: R(q) v + t with the library's quaternion-to-rotation text (sl_math.hpp quat_to_R, mul,
    transform_from) in Python floats, operation by operation"""
    x, y, z, w = (float(v) for v in pose7[3:7])
    n = math.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    R = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
         2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
    out = np.array(meas7, np.float64).reshape(-1, 7)
    for row in out:
        vx, vy, vz = float(row[1]), float(row[2]), float(row[3])
        row[1] = (R[0] * vx + R[1] * vy + R[2] * vz) + float(pose7[0])
        row[2] = (R[3] * vx + R[4] * vy + R[5] * vz) + float(pose7[1])
        row[3] = (R[6] * vx + R[7] * vy + R[8] * vz) + float(pose7[2])
    return out


def intra_lattice(params, nq, x_half=X_HALF, y_half=Y_HALF, yaw_half=YAW_HALF):
    """place_cases.lattice over the fixed intra window (findTransformation :801-816): its half ranges come from the maps' extents times
    the dilation factor, so it is handed a one-object map AT the half ranges and a dilation factor of exactly 1."""
    assert params["disable_yaw_search"] or x_half == y_half
    P = dict(params, dilation_factor=1.0, match_yaw_half_range=yaw_half)
    return pc.lattice(np.array([[0.0, x_half, y_half, 0, 0, 0, 0]]), np.zeros((nq, 7)), P)


_SWEEP_CACHE = {}


def intra_sweep_reference(case, k, x_half=X_HALF, y_half=Y_HALF, yaw_half=YAW_HALF):
    """dict(candidates, best_index, max_count) of candidate k by itself: numpy first-of-maximum over the lattice, maps not centred."""
    key = (case["name"], id(case["submaps"][k]), x_half, y_half, yaw_half)
    if key not in _SWEEP_CACHE:
        mw = to_map_frame(case["meas"], case["query_pose"])
        lat = intra_lattice(case["params"], len(mw), x_half, y_half, yaw_half)
        sub = case["submaps"][k]
        assert lat["n"] * len(sub) * len(mw) <= lc.MAX_PAIR_TESTS
        counts = pc.sweep_counts(sub, mw, lat, case["params"])
        bi = pc.first_argmax(counts)
        _SWEEP_CACHE[key] = dict(candidates=lat["n"], best_index=bi, max_count=int(counts[bi]) if bi >= 0 else None)
    return _SWEEP_CACHE[key]


class OPlace(C.Structure):                     # the oracle's parameter block (tests/test_gpu_place.py)
    _fields_ = [("dilation_factor", C.c_double), ("xy_step", C.c_double), ("yaw_half_range", C.c_double),
                ("yaw_step", C.c_double), ("match_threshold", C.c_double), ("match_threshold_dimension", C.c_double),
                ("disable_yaw_search", C.c_int), ("ignore_dimension", C.c_int), ("min_num_inliers", C.c_int),
                ("use_lsq", C.c_int), ("min_num_map_objects_to_start", C.c_int), ("max_rings", C.c_int)]


def oracle_intra(meas, submap, query_pose, cand_pose, params, x_half=X_HALF, y_half=Y_HALF, yaw_half=YAW_HALF):
    """orc_find_intra_loop_closure on the CPU: dict(found, inliers, tf (4, 4), xyzyaw)"""
    from oracle import pyoracle as po
    P = params
    op = OPlace(P["dilation_factor"], P["search_xy_step_size"], P["match_yaw_half_range"], P["search_yaw_step_size"], P["match_threshold_position"],
                P["match_threshold_dimension"], P["disable_yaw_search"], P["ignore_dimension"], P["min_num_inliers"], P["use_nonlinear_least_squares"],
                P["min_num_map_objects_to_start"], P["max_rings"])

    def p(a):
        return a.ctypes.data_as(C.c_void_p)
    m, sm = np.ascontiguousarray(meas, np.float64), np.ascontiguousarray(submap, np.float64)
    if len(sm) == 0:
        sm = np.zeros((1, 7))
    tf, inl, xyz = np.zeros(16), C.c_int(0), np.zeros(4)
    q, c = np.ascontiguousarray(query_pose, np.float64), np.ascontiguousarray(cand_pose, np.float64)
    ok = po.lib().orc_find_intra_loop_closure(p(m), C.c_int(len(meas)), p(sm), C.c_int(len(submap)), p(q), p(c), C.byref(op), C.c_double(x_half),
                                              C.c_double(y_half), C.c_double(yaw_half), p(tf), C.byref(inl), p(xyz))
    return dict(found=bool(ok), inliers=int(inl.value), tf=tf.reshape(4, 4), xyzyaw=xyz)


def smallest_refused_rows(nq, ignore_dimension):
    """the smallest submap the bucketed sweep's 150 KiB image refuses beside nq detections"""
    n = pc.bucketed_max_nr(nq, ignore_dimension) + 1
    assert lc.lds_image_bytes(n, nq, ignore_dimension) > pc.LDS_BYTES >= lc.lds_image_bytes(n - 1, nq, ignore_dimension)
    return n


_INTRA_CACHE = {}


def intra_case():
    """One query of 20 detections seen from a query pose that has drifted by (0.8, -0.6) m and 4 deg (the construction of
    test_find_intra_loop_closure_matches_oracle) against 12 candidates at the reference's default intra window and steps: 4840 lattice
    poses each.  `kinds[k]` names what candidate k is.  The oracle's verdict per candidate that can reach the sweep is computed once,
    here, and the case asserts that it finds at least 3 and rejects at least 2 whose submap is non-empty and fits the 150 KiB image."""
    if _INTRA_CACHE:
        return _INTRA_CACHE["case"]
    rng = np.random.default_rng(5)
    n = 45
    base = np.zeros((n, 7))
    base[:, 0] = rng.integers(1, 4, n)
    base[:, 1:3] = rng.uniform(-12, 12, (n, 2)) + np.array([30.0, 10.0])
    base[:, 3] = rng.normal(0, 0.2, n)
    base[:, 4:7] = rng.uniform(0.3, 2.0, (n, 3))
    base[rng.integers(0, 3, n) == 0, 5:7] = 0.0               # some take the one-dimension branch
    true_q = np.concatenate([[31.0, 9.0, 1.0], quat_z(0.6)])
    drift_q = np.concatenate([[31.8, 8.4, 1.0], quat_z(0.6 + np.deg2rad(4.0))])
    c, s_ = np.cos(0.6), np.sin(0.6)
    Rq = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1.0]])
    seen = rng.permutation(n)[:20]
    meas = base[seen].copy()
    meas[:, 1:4] = (base[seen, 1:4] - true_q[:3]) @ Rq + rng.normal(0, 0.03, (20, 3))

    def extras(m):
        e = np.zeros((m, 7))
        e[:, 0] = rng.integers(1, 4, m)
        e[:, 1:3] = rng.uniform(-14, 14, (m, 2)) + np.array([30.0, 10.0])
        e[:, 4:7] = rng.uniform(0.3, 2.0, (m, 3))
        return e
    params = pc.place_params()
    with_extras = np.concatenate([extras(15), base[np.sort(np.concatenate([seen, rng.permutation(n)[:10]]))]])
    shuffled = np.ascontiguousarray(base[rng.permutation(n)])
    far = base.copy()
    far[:, 1:3] += 200.0
    other_labels = base.copy()
    other_labels[:, 0] += 10.0
    half_gone = np.ascontiguousarray(np.delete(base, seen[::2], axis=0))
    over = extras(smallest_refused_rows(20, params["ignore_dimension"]))
    poses = [np.concatenate([[29.0, 11.0, 1.0], quat_z(-0.2)]), np.concatenate([[33.5, 7.25, 0.8], quat_z(1.1)]),
             np.concatenate([[26.0, 14.0, 1.2], quat_z(2.9)])]
    cands = [("revisit", base, 0), ("revisit_other_pose", base, 1), ("revisit_with_extras", with_extras, 2), ("far_away", far, 0),
             ("no_common_label", other_labels, 1), ("empty", np.zeros((0, 7)), 0), ("oversized", over, 2), ("revisit_again", base, 0),
             ("revisit_shuffled", shuffled, 1), ("unrelated", extras(40), 2), ("half_gone", half_gone, 0), ("revisit_with_extras_again", with_extras, 1)]
    case = dict(name="intra_list", meas=meas, query_pose=drift_q, params=params, kinds=[k for k, _, _ in cands],
                submaps=[np.ascontiguousarray(m) for _, m, _ in cands], cand_poses=np.array([poses[p] for _, _, p in cands]))
    case["oracle"] = [None if kind == "oversized" else oracle_intra(meas, m, drift_q, poses[p], params) for kind, m, p in cands]
    live = [o for kind, o in zip(case["kinds"], case["oracle"]) if kind not in ("oversized", "empty")]
    assert sum(o["found"] for o in live) >= 3 and sum(not o["found"] for o in live) >= 2, [(k, o and o["found"]) for k, o in zip(case["kinds"], case["oracle"])]
    lat = intra_lattice(params, 20)      # 440 cells (21 x 21 less the centre) x 11 yaws: ten steps of 2 deg added up from -10 deg stop just short of +10 deg
    assert (lat["n_cells"], lat["n_yaw"], lat["n"]) == (440, 11, 4840)
    _INTRA_CACHE["case"] = case
    return case


# ---- the map and the attempt of the timing tool and tests/test_gpu_intra_attempt.py ------------------------------------------------
def attempt_case(n_objects=600, seed=77, extent=40.0, n_pose=120, turns=1.02):
    """A map of the three classes (half cylinders, a quarter cubes, a quarter ellipsoids) around a loop of key poses, 20 detections of
    the objects near the last key pose seen from a drifted query pose, and the key-pose cloud (float32) from which the candidates are
    drawn."""
    rng = np.random.default_rng(seed)
    n_cyl, n_cube = n_objects // 2, n_objects // 4
    t = _random_map(rng, n_cyl, n_cube, n_objects - n_cyl - n_cube, extent=extent)
    for c in ("cyl_root", "cube_xyz", "ell_xyz"):
        t[c][:, 2] = rng.normal(0.0, 0.3, len(t[c]))
    ang = np.linspace(0, 2 * np.pi * turns, n_pose)
    cloud = np.column_stack([25 * np.cos(ang), 25 * np.sin(ang), 0.05 * np.ones(n_pose)]) + rng.normal(0, 0.2, (n_pose, 3))
    cloud = cloud.astype(np.float32)
    true_xyz = cloud[-1].astype(np.float64)
    yaw = 0.6
    true_q = np.concatenate([true_xyz, quat_z(yaw)])
    drift_q = np.concatenate([true_xyz + np.array([0.8, -0.6, 0.0]), quat_z(yaw + np.deg2rad(4.0))])
    rows = all_rows(t)
    near = np.argsort(np.hypot(rows[:, 1] - true_xyz[0], rows[:, 2] - true_xyz[1]))[:20]
    c, s_ = np.cos(yaw), np.sin(yaw)
    Rq = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1.0]])
    meas = rows[near].copy()
    meas[:, 1:4] = (rows[near, 1:4] - true_q[:3]) @ Rq + rng.normal(0, 0.03, (20, 3))
    return dict(tables=t, cloud=cloud, meas=meas, query_pose=drift_q, radius=RADIUS, max_dz=MAX_DZ, params=pc.place_params())


def key_pose7(cloud, idx):
    """candidate key poses from the cloud: position of key pose idx (as doubles), a yaw that depends on idx"""
    return np.array([np.concatenate([cloud[i].astype(np.float64), quat_z(0.1 * (int(i) % 7))]) for i in idx]).reshape(-1, 7)
