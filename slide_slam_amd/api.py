"""ctypes binding of include/slide_gpu.h (the C-ABI drop-in boundary of the sloam backend hot path).

The shared library carries gfx950 HIP kernels only.  There is no CPU fallback: importing works
anywhere (so that symbol/ABI tests run without a GPU), but every compute call fails loudly with
``SlideError`` when the library or a gfx950 device is missing.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libslide_gpu.so")
_LIB = None

SLIDE_OK, SLIDE_MISSING = 0, 1
SLIDE_ERR_CAPACITY = -3
ERR = {-1: "SLIDE_ERR_INVALID", -2: "SLIDE_ERR_NOT_SPD", -3: "SLIDE_ERR_CAPACITY", -4: "SLIDE_ERR_HIP", -5: "SLIDE_ERR_RUNTIME"}
CHART_CAYLEY, CHART_EXPMAP = 0, 1
CLS_CYLINDER, CLS_CUBE, CLS_ELLIPSOID = 0, 1, 2
FRAME_HOST, FRAME_HOST_DEFERRED, FRAME_FOREIGN = 0, 1, 2
GATE_DROP, GATE_NEW = 0, 1      # SLIDE_GATE_*: what SlideBackend.set_association_gate does with a rejected match
MATCH_GATED = -2                # SLIDE_MATCH_GATED: *_match of a detection whose match the association gate rejected

# every symbol include/slide_gpu.h declares (checked by tests/test_abi.py against the header text)
EXPORTS = [
    "slide_default_params", "slide_device_check", "slide_last_error", "slide_version",
    "slide_graph_create", "slide_graph_destroy", "slide_graph_set_prior", "slide_graph_add_keypose_between",
    "slide_graph_add_loop_closure", "slide_graph_add_relative_meas", "slide_graph_add_point_landmark",
    "slide_graph_add_range_bearing", "slide_graph_add_cube", "slide_graph_add_cylinder", "slide_graph_solve",
    "slide_graph_gauss_newton", "slide_graph_get_pose", "slide_graph_get_pose12", "slide_graph_get_all_poses",
    "slide_graph_get_landmark", "slide_graph_get_pose_covariance", "slide_graph_get_pose_covariances", "slide_graph_get_landmark_covariances", "slide_graph_marginal_traces", "slide_graph_closure_info_gain", "slide_graph_closure_info_gain_batch", "slide_graph_stats", "slide_graph_rejected_count", "slide_graph_set_shared", "slide_graph_dist_phase", "slide_chol_batch_create", "slide_chol_batch_destroy", "slide_graph_join_chol_batch", "slide_graph_dist_pass_local", "slide_chol_batch_pass", "slide_chol_batch_get_pose_covariances", "slide_chol_batch_get_landmark_covariances", "slide_chol_batch_marginal_traces", "slide_chol_batch_closure_info_gain", "slide_chol_batch_closure_info_gain_batch", "slide_chol_batch_pass_part", "slide_chol_batch_stream", "slide_chol_batch_set_pcg", "slide_graph_set_pcg", "slide_chol_batch_set_pcg_tolerance", "slide_graph_set_pcg_tolerance", "slide_graph_set_separator", "slide_chol_batch_set_exact_joint", "slide_chol_batch_sep_buffer_len", "slide_chol_batch_sep_exchange_len", "slide_chol_batch_profile_exact_joint", "slide_graph_get_border_profile", "slide_graph_get_incremental_stats", "slide_graph_set_wildfire", "slide_graph_get_wildfire_stats", "slide_graph_get_segments", "slide_graph_get_segment_table", "slide_chol_batch_set_segments", "slide_clipper_dense_clique_batch", "slide_clipper_last_solve_info", "slide_last_device_ms", "slide_chol_batch_set_separator_profile", "slide_chol_batch_set_separator_blocks", "slide_chol_batch_set_separator_owner", "slide_chol_batch_sep_segment", "slide_graph_set_incremental", "slide_graph_set_ghost_ids", "slide_graph_get_pcg_stats", "slide_graph_get_tile_profile", "slide_graph_set_dense_profile", "slide_graph_chi2", "slide_chol_batch_profile", "slide_graph_set_ghosts", "slide_graph_add_relative_meas_ghost",
    "slide_backend_landmark_table", "slide_graph_set_profiling", "slide_graph_get_profile",
    "slide_dense_spd_solve", "slide_dense_spd_solve_ex", "slide_debug_chol_bordered", "slide_debug_chol_batch", "slide_debug_chol_plan", "slide_debug_pair_timeouts", "slide_debug_border_product", "slide_debug_border_apply", "slide_debug_selected_inverse", "slide_debug_multi_solve", "slide_debug_gram", "slide_debug_pose_covariance", "slide_debug_joint_selected_inverse", "slide_submap_knn", "slide_assoc_match_cylinders", "slide_assoc_match_boxes", "slide_assoc_sweep_batch_device", "slide_assoc_sweep_batch",
    "slide_backend_create", "slide_backend_destroy", "slide_backend_process_frame", "slide_backend_ingest_solve",
    "slide_backend_end_frame", "slide_backend_graph", "slide_backend_counts", "slide_backend_map_model",
    "slide_place_default_params", "slide_match_maps", "slide_match_maps_sweep", "slide_find_inter_loop_closure", "slide_find_inter_loop_closures",
    "slide_find_intra_loop_closure", "slide_keypose_submaps", "slide_find_intra_loop_closures", "slide_intra_loop_closure_attempt",
    "slide_loop_candidate_idx", "slide_loop_candidate_list", "slide_clipper_affinity", "slide_clipper_affinity_csr", "slide_clipper_dense_clique_csr", "slide_clipper_match",
    "slide_closest_stamp", "slide_clipper_default_params", "slide_clipper_dense_clique", "slide_match_triangles",
    "slide_estimate_tf2d", "slide_semantic_clipper", "slide_find_relative_meas_match", "slide_delaunay_2d", "slide_run_semantic_clipper",
    "slide_pick_next_measurement", "slide_in_loop_closure_region",
    "slide_slidegraph_default_params", "slide_find_inter_loop_closure_clipper", "slide_find_inter_loop_closures_clipper",
    "slide_closure_default_params", "slide_closure_canonicalize", "slide_closure_consistency_csr", "slide_select_consistent_closures",
    "slide_graph_select_closures", "slide_graph_get_pose_pair_covariances", "slide_graph_closure_mahalanobis",
    "slide_graph_observation_mahalanobis", "slide_graph_observation_joint_compatibility", "slide_chi2_quantile",
    "slide_graph_set_robust_loss", "slide_graph_get_closure_weights",
    "slide_graph_set_observation_loss", "slide_graph_get_observation_weights",
    "slide_chol_batch_set_robust_loss", "slide_chol_batch_get_closure_weights", "slide_chol_batch_profile_robust_reweight",
    "slide_chol_batch_get_pose_pair_covariances", "slide_chol_batch_closure_mahalanobis", "slide_chol_batch_observation_mahalanobis",
    "slide_chol_batch_set_observation_loss", "slide_chol_batch_get_observation_weights", "slide_chol_batch_profile_linearize",
    "slide_chol_batch_observation_joint_compatibility",
    "slide_graph_landmark_pair_mahalanobis", "slide_graph_get_landmark_pair_covariances", "slide_pairs_within",
    "slide_graph_landmark_pairs_within", "slide_graph_merge_landmarks", "slide_graph_landmark_alias", "slide_graph_merge_timing",
    "slide_chol_batch_landmark_pair_mahalanobis", "slide_chol_batch_get_landmark_pair_covariances", "slide_chol_batch_landmark_pairs_within",
    "slide_graph_predicted_observation_mahalanobis", "slide_backend_set_association_gate", "slide_backend_gate_stats",
]


class SlideError(RuntimeError):
    pass


# the 0.99 quantiles of chi-square by degrees of freedom: what SlideGraph.observation_mahalanobis's d2 is compared with (points 3,
# cylinders 7, cubes 9)
OBSERVATION_GATE_CHI2_99 = {3: 11.345, 7: 18.475, 9: 21.666}
_OBS_CLASSES = {"cylinder": 0, "cube": 1, "point": 2}      # SLIDE_CLS_*
_OBS_NARGS = {"point": 4, "cube": 17, "cylinder": 14}
_OBS_NPARTS = {"point": 2, "cube": 3, "cylinder": 4}      # measurement arguments of a candidate tuple


def _observation_arrays(candidates, with_lm_slot):
    """The candidate tuples of observation_mahalanobis as the C call's arrays (one spare row for an empty list).  with_lm_slot: a
    tuple may carry one more trailing value, the landmark's slot (CholBatch); the last array is then the landmarks' slots."""
    rows = [tuple(c) for c in candidates]
    n = len(rows)
    k = max(n, 1)
    robot, cls, lslot = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
    pidx, lidx, meas = np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros((k, 17))
    for i, c in enumerate(rows):
        if c[0] not in _OBS_CLASSES:
            raise SlideError(f"observation_mahalanobis: unknown candidate kind {c[0]!r}")
        cls[i], robot[i], pidx[i], lidx[i] = _OBS_CLASSES[c[0]], c[1], c[2], c[3]
        rest = c[4:]
        lslot[i] = robot[i]
        if with_lm_slot and len(rest) == _OBS_NPARTS[c[0]] + 1:
            lslot[i], rest = int(rest[-1]), rest[:-1]
        parts = [np.atleast_1d(_d(x)).ravel() for x in rest]
        v = np.concatenate(parts)
        if len(v) != _OBS_NARGS[c[0]]:
            raise SlideError(f"observation_mahalanobis: a {c[0]} candidate takes {_OBS_NARGS[c[0]]} measurement values, got {len(v)}")
        meas[i, :len(v)] = v
    return n, k, robot, pidx, cls, lidx, meas, lslot


class Params(C.Structure):
    _fields_ = [("pose_chart", C.c_int), ("relinearize_threshold", C.c_double), ("noise_floor", C.c_double),
                ("noise_model_prior_first_pose_vec", C.c_double * 6), ("noise_model_odom_vec", C.c_double * 6),
                ("noise_model_cube_vec", C.c_double * 9), ("noise_model_rel_meas_vec", C.c_double * 6),
                ("cylinder_sigma", C.c_double), ("bearing_range_sigma", C.c_double), ("numdiff_delta", C.c_double),
                ("cylinder_match_thresh", C.c_double), ("cuboid_match_thresh", C.c_double),
                ("ellipsoid_match_thresh", C.c_double), ("knn_cylinder", C.c_int), ("knn_cube", C.c_int),
                ("knn_ellipsoid", C.c_int), ("number_of_robots", C.c_int), ("device", C.c_int)]


class Detections(C.Structure):
    _fields_ = [("n_cyl", C.c_int), ("cyl_root", C.c_void_p), ("cyl_ray", C.c_void_p), ("cyl_radius", C.c_void_p),
                ("cyl_label", C.c_void_p), ("n_cube", C.c_int), ("cube_pose7", C.c_void_p), ("cube_scale", C.c_void_p),
                ("cube_label", C.c_void_p), ("n_ell", C.c_int), ("ell_pose7", C.c_void_p), ("ell_scale", C.c_void_p),
                ("ell_label", C.c_void_p)]


class FrameResult(C.Structure):
    _fields_ = [("out_pose7", C.c_double * 7), ("cyl_match", C.c_void_p), ("cube_match", C.c_void_p),
                ("ell_match", C.c_void_p), ("cyl_id", C.c_void_p), ("cube_id", C.c_void_p), ("ell_id", C.c_void_p),
                ("optimized", C.c_int), ("ms_association", C.c_double), ("ms_graph", C.c_double)]


class PlaceParams(C.Structure):
    _fields_ = [("dilation_factor", C.c_double), ("search_xy_step_size", C.c_double), ("match_yaw_half_range", C.c_double),
                ("search_yaw_step_size", C.c_double), ("match_threshold_position", C.c_double),
                ("match_threshold_dimension", C.c_double), ("disable_yaw_search", C.c_int), ("ignore_dimension", C.c_int),
                ("min_num_inliers", C.c_int), ("use_nonlinear_least_squares", C.c_int),
                ("min_num_map_objects_to_start", C.c_int), ("max_rings", C.c_int)]


def lib():
    """Load libslide_gpu.so (built by slide_slam_amd.build / __graft_entry__.build)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise SlideError(f"{LIB_PATH} is missing: run `python -m slide_slam_amd.build` (hipcc, gfx950). "
                             "There is no CPU fallback.")
        # (SLIDE_LIB_VARIANT=<name>: an experiment build _lib/<name>.so of the SAME sources with other compile-time constants,
        # tools/build_variant.py — kernel tuning only; it is a build of this library, not another path)
        var = os.environ.get("SLIDE_LIB_VARIANT")
        path = os.path.join(_HERE, "_lib", var + ".so") if var else LIB_PATH
        if var and not os.path.exists(path):
            raise SlideError(f"{path} is missing (SLIDE_LIB_VARIANT)")
        L = C.CDLL(path)
        L.slide_last_error.restype = C.c_char_p
        L.slide_version.restype = C.c_char_p
        L.slide_graph_create.restype = C.c_void_p
        L.slide_backend_create.restype = C.c_void_p
        L.slide_backend_graph.restype = C.c_void_p
        L.slide_chol_batch_create.restype = C.c_void_p
        L.slide_graph_rejected_count.restype = C.c_int64
        L.slide_graph_rejected_count.argtypes = [C.c_void_p]
        L.slide_chol_batch_destroy.argtypes = [C.c_void_p]
        L.slide_chol_batch_destroy.restype = None
        L.slide_chol_batch_stream.restype = C.c_void_p
        L.slide_chol_batch_stream.argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


def last_error() -> str:
    return lib().slide_last_error().decode()


def _check(rc, allow_missing=False):
    if rc == SLIDE_OK or (allow_missing and rc == SLIDE_MISSING):
        return rc
    raise SlideError(f"{ERR.get(rc, rc)}: {last_error()}")


def default_params(**kw) -> Params:
    p = Params()
    lib().slide_default_params(C.byref(p))
    for k, v in kw.items():
        if isinstance(v, (list, tuple, np.ndarray)):
            arr = getattr(p, k)
            for i, x in enumerate(v):
                arr[i] = float(x)
        else:
            setattr(p, k, v)
    return p


def chi2_quantile(prob: float, dof: int) -> float:
    """slide_chi2_quantile: the prob quantile of chi-square with dof degrees of freedom (host code, no device needed): what
    SlideGraph.observation_joint_compatibility compares d2_single and d2_joint with."""
    q = C.c_double(0.0)
    _check(lib().slide_chi2_quantile(C.c_double(prob), C.c_int(dof), C.byref(q)))
    return q.value


def merge_clusters(idx_a, idx_b):
    """The clusters of the pairs (idx_a[k], idx_b[k]) — duplicate_landmarks' output — as the (keep, drop) rows merge_landmarks takes:
    union-find over the pairs, one row (survivor, member) per member, the survivor being the cluster's smallest key.  Rows sorted by
    (survivor, member): the result does not depend on the order, the orientation or the repetition of the pairs.  Pure Python."""
    a = np.asarray(idx_a).reshape(-1)
    b = np.asarray(idx_b).reshape(-1)
    if len(a) != len(b):
        raise SlideError("merge_clusters: idx_a and idx_b differ in length")
    parent = {}

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for x, y in zip(a.tolist(), b.tolist()):
        x, y = int(x), int(y)
        if x < 0 or y < 0:
            raise SlideError("merge_clusters: a negative landmark index")
        parent.setdefault(x, x)
        parent.setdefault(y, y)
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)      # (the smaller root survives: a cluster's root is its smallest key)
    rows = sorted((find(x), x) for x in parent if find(x) != x)
    return np.array(rows, dtype=np.uint64).reshape(-1, 2)


def device_check(device: int = -1) -> None:
    _check(lib().slide_device_check(C.c_int(device)))


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class _Ptr(C.c_void_p):
    """A pointer argument that holds the array it points into (a slot: no per-call attribute dictionary)."""
    __slots__ = ("keep",)


def _p(a):
    # (ndarray.ctypes.data_as costs 2.9 us a call, this 1.1: a streaming frame passes eighteen pointers.)  The pointer carries the
    # array: _p(_d(list)) converts into a temporary that nothing else holds, and freed memory would be passed otherwise.
    v = _Ptr(a.ctypes.data)
    v.keep = a
    return v


def _candidate_list(trajs, travels, traj_slots=None):
    """The flat arguments of the *_closure_info_gain_batch calls: off (n + 1), traj, travel (parallel to traj: a candidate's last
    entry is padding) and, when given, traj_slots."""
    if len(trajs) != len(travels) or (traj_slots is not None and len(traj_slots) != len(trajs)):
        raise ValueError("one list of travel distances (and of slots) per trajectory")
    off = np.zeros(len(trajs) + 1, dtype=np.int32)
    for k, t in enumerate(trajs):
        off[k + 1] = off[k] + len(t)
    traj = np.zeros(int(off[-1]), dtype=np.uint64)
    travel = np.zeros(int(off[-1]), dtype=np.float64)
    slots = np.zeros(int(off[-1]), dtype=np.int32) if traj_slots is not None else None
    for k, (t, d) in enumerate(zip(trajs, travels)):
        if len(d) != max(len(t) - 1, 0):
            raise ValueError("travel needs one distance per step of traj")
        traj[off[k]:off[k + 1]] = np.asarray(t, dtype=np.uint64).reshape(-1)
        travel[off[k]:off[k] + len(d)] = np.asarray(d, dtype=np.float64).reshape(-1)
        if slots is not None:
            if len(traj_slots[k]) != len(t):
                raise ValueError("traj_slots needs one slot per pose of traj")
            slots[off[k]:off[k + 1]] = np.asarray(traj_slots[k], dtype=np.int32).reshape(-1)
    return off, traj, travel, slots


def _sigma6(sigma_per_m):
    if sigma_per_m is None:
        return None
    sg = _d(sigma_per_m).reshape(-1)
    if len(sg) != 6:
        raise ValueError("sigma_per_m has six entries")
    return sg


ROBUST_KINDS = {None: 0, "none": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3, "dcs": 4}
# the columns of the weight read-backs, in the C ABI's argument order
_I32, _U64, _F64 = np.int32, np.uint64, np.float64
_CLOSURE_COLS = [("from_robot", _I32), ("from_idx", _U64), ("to_robot", _I32), ("to_idx", _U64), ("kind", _I32)]
_OBSERVATION_COLS = [("pose_idx", _U64), ("cls", _I32), ("lm_idx", _U64)]
_WEIGHT_COLS = [("weight", _F64), ("s2", _F64)]


def _loss_kind(kind, what):
    """The kind of a loss (`what`: "robust" / "observation") as the C ABI takes it: a name of ROBUST_KINDS resolved, a number passed on."""
    if kind is None or isinstance(kind, str):
        if kind not in ROBUST_KINDS:
            raise ValueError(f"{what} loss {kind!r}: one of huber, cauchy, geman_mcclure, dcs, None")
        kind = ROBUST_KINDS[kind]
    return C.c_int(int(kind))


def _weights(fn, handle, columns, cap=None):
    """The read-back of a *_get_*_weights call: the count first (cap None), then one array per (name, dtype) column filled up to
    cap rows.  Returns the columns cut to the rows written, and n, the full count."""
    n = C.c_int(0)
    if cap is None:
        _check(fn(handle, C.c_int(0), *[None] * len(columns), C.byref(n)))
        cap = n.value
    cols = {name: np.zeros(max(int(cap), 1), dt) for name, dt in columns}
    _check(fn(handle, C.c_int(int(cap)), *[_p(a) for a in cols.values()], C.byref(n)))
    k = min(int(cap), n.value)
    return {**{name: a[:k].copy() for name, a in cols.items()}, "n": n.value}


class SlideGraph:
    """SemanticFactorGraph seam (reference include/factorgraph/graph.h:70-121) on the MI355X."""

    def __init__(self, params: Params | None = None, handle=None):
        self.L = lib()
        self.own = handle is None
        if handle is None:
            h = self.L.slide_graph_create(C.byref(params) if params is not None else None)
            if not h:
                raise SlideError(f"slide_graph_create failed: {last_error()}")
            handle = C.c_void_p(h)
        self.h = handle

    def __del__(self):
        if getattr(self, "own", False) and getattr(self, "h", None):
            self.L.slide_graph_destroy(self.h)
            self.h = None

    def set_prior(self, robot, pose7):
        _check(self.L.slide_graph_set_prior(self.h, C.c_int(robot), _p(_d(pose7))))

    def add_keypose_between(self, robot, frm, to, rel7, est7):
        _check(self.L.slide_graph_add_keypose_between(self.h, C.c_int(robot), C.c_uint64(frm), C.c_uint64(to), _p(_d(rel7)),
                                                      _p(_d(est7))))

    def add_loop_closure(self, rel7, i1, r1, i2, r2):
        _check(self.L.slide_graph_add_loop_closure(self.h, _p(_d(rel7)), C.c_uint64(i1), C.c_int(r1), C.c_uint64(i2),
                                                   C.c_int(r2)))

    def add_relative_meas(self, rel7, i1, r1, i2, r2):
        _check(self.L.slide_graph_add_relative_meas(self.h, _p(_d(rel7)), C.c_uint64(i1), C.c_int(r1), C.c_uint64(i2),
                                                    C.c_int(r2)))

    def add_point_landmark(self, idx, xyz):
        _check(self.L.slide_graph_add_point_landmark(self.h, C.c_uint64(idx), _p(_d(xyz))))

    def add_range_bearing(self, robot, pose_idx, lm_idx, bearing, rng):
        _check(self.L.slide_graph_add_range_bearing(self.h, C.c_int(robot), C.c_uint64(pose_idx), C.c_uint64(lm_idx),
                                                    _p(_d(bearing)), C.c_double(rng)))

    def add_cube(self, robot, pose_idx, cube_idx, pose7, cube7, scale, exists):
        _check(self.L.slide_graph_add_cube(self.h, C.c_int(robot), C.c_uint64(pose_idx), C.c_uint64(cube_idx), _p(_d(pose7)),
                                           _p(_d(cube7)), _p(_d(scale)), C.c_int(int(exists))))

    def add_cylinder(self, robot, pose_idx, cyl_idx, pose7, root, ray, radius, exists):
        _check(self.L.slide_graph_add_cylinder(self.h, C.c_int(robot), C.c_uint64(pose_idx), C.c_uint64(cyl_idx),
                                               _p(_d(pose7)), _p(_d(root)), _p(_d(ray)), C.c_double(radius),
                                               C.c_int(int(exists))))

    def solve(self):
        return _check(self.L.slide_graph_solve(self.h))

    def gauss_newton(self, iterations=1):
        return _check(self.L.slide_graph_gauss_newton(self.h, C.c_int(iterations)))

    def get_pose(self, robot, idx):
        out = np.zeros(7)
        st = _check(self.L.slide_graph_get_pose(self.h, C.c_int(robot), C.c_uint64(idx), _p(out)), True)
        return st, out

    def get_pose12(self, robot, idx):
        out = np.zeros(12)
        st = _check(self.L.slide_graph_get_pose12(self.h, C.c_int(robot), C.c_uint64(idx), _p(out)), True)
        return st, out

    def get_all_poses(self, robot, cap):
        out = np.zeros((cap, 7))
        n = C.c_uint64(0)
        _check(self.L.slide_graph_get_all_poses(self.h, C.c_int(robot), _p(out), C.c_uint64(cap), C.byref(n)))
        return out[: n.value]

    def get_landmark(self, cls, idx):
        out = np.zeros(15)
        st = _check(self.L.slide_graph_get_landmark(self.h, C.c_int(cls), C.c_uint64(idx), _p(out)), True)
        return st, out[: (7, 15, 3)[cls]]

    def stats(self):
        out = np.zeros(5, np.int64)
        _check(self.L.slide_graph_stats(self.h, _p(out)))
        return dict(n_pose=int(out[0]), n_lm=int(out[1]), n_factors=int(out[2]), n_relin=int(out[3]), chol_dim=int(out[4]))

    def rejected_count(self):
        """Entries (factors on unknown keys, values inserted twice) refused since creation; the reference's isam->update throws there."""
        return int(self.L.slide_graph_rejected_count(self.h))

    def set_shared(self, cls, idx, owner):
        cls, owner = _i(cls), _i(owner)
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        _check(self.L.slide_graph_set_shared(self.h, _p(cls), _p(idx), _p(owner), C.c_int(len(cls))))

    def get_pose_covariance(self, robot, idx):
        """getPoseCovariance (graph.cpp:314-323).  Returns (status, 6x6)."""
        out = np.zeros(36)
        st = self.L.slide_graph_get_pose_covariance(self.h, C.c_int(robot), C.c_uint64(idx), _p(out))
        if st < 0:
            _check(st)
        return st, out.reshape(6, 6)

    def get_pose_covariances(self, robot, idx):
        """isam->marginalCovariance(X(i)) for every pose index in `idx` of `robot`: (n, 6, 6), tangent order [rot, trans].  One
        selected inversion of the resident factor per factorisation serves every later call.  KeyError for an unknown pose."""
        ids = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        out = np.zeros(36 * len(ids))
        st = self.L.slide_graph_get_pose_covariances(self.h, C.c_int(robot), _p(ids), C.c_int(len(ids)), _p(out))
        if st == SLIDE_MISSING:
            raise KeyError(f"pose of robot {robot} not in the graph")
        _check(st)
        return out.reshape(-1, 6, 6)

    def get_landmark_covariances(self, cls, idx):
        """Marginal covariances of landmarks of class `cls` (CLS_*): (n, d, d), d = 7 / 9 / 3 for cylinder / cube / point, tangent
        order cylinder [ray, root, radius], cube pose (6) then scale (3), point xyz.  KeyError for an unknown landmark."""
        d = {CLS_CYLINDER: 7, CLS_CUBE: 9}.get(cls, 3)
        ids = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        out = np.zeros(d * d * len(ids))
        st = self.L.slide_graph_get_landmark_covariances(self.h, C.c_int(cls), _p(ids), C.c_int(len(ids)), _p(out))
        if st == SLIDE_MISSING:
            raise KeyError(f"landmark of class {cls} not in the graph")
        _check(st)
        return out.reshape(-1, d, d)

    def marginal_traces(self, robot=0):
        """logEntropy (graph.cpp:423-466): [pose trace sum, point-landmark trace sum, #poses, #point landmarks]."""
        out = np.zeros(4)
        _check(self.L.slide_graph_marginal_traces(self.h, C.c_int(robot), _p(out)))
        return out

    def closure_info_gain(self, robot, traj, travel, sigma_per_m=None):
        """estimateClosureInfoGain (graph.cpp:469-623): [10 pose + landmark, pose, landmark] information gain of Between factors
        (traj[i+1], traj[i]) with noise sigma_per_m * travel[i] (None: the graph's own noise_model_odom_vec), at the resident factor."""
        t = np.ascontiguousarray(traj, dtype=np.uint64).reshape(-1)
        tr = _d(travel).reshape(-1)
        if len(tr) != max(len(t) - 1, 0):
            raise ValueError("travel needs one distance per step of traj")
        sg = None
        if sigma_per_m is not None:
            sg = _d(sigma_per_m).reshape(-1)
            if len(sg) != 6:
                raise ValueError("sigma_per_m has six entries")
        out = np.zeros(3)
        st = self.L.slide_graph_closure_info_gain(self.h, C.c_int(robot), _p(t), C.c_int(len(t)), _p(tr),
                                                  _p(sg) if sg is not None else None, _p(out))
        if st == SLIDE_MISSING:
            raise KeyError(f"trajectory pose of robot {robot} not in the graph")
        _check(st)
        return out

    def closure_info_gain_batch(self, robot, trajs, travels, sigma_per_m=None):
        """closure_info_gain for a list of candidates in one call (slide_graph_closure_info_gain_batch): trajs[k] / travels[k] as the
        single call's arguments.  Returns ((n, 3) gains, (n,) int32 status): row k is what closure_info_gain gives for candidate k
        alone; a candidate with a fault of its own (SLIDE_MISSING, SLIDE_ERR_INVALID, _CAPACITY, _NOT_SPD) has zeros and its code."""
        off, traj, travel, _ = _candidate_list(trajs, travels)
        sg = _sigma6(sigma_per_m)
        out = np.zeros((len(trajs), 3))
        status = np.zeros(len(trajs), dtype=np.int32)
        vp = C.c_void_p
        _check(self.L.slide_graph_closure_info_gain_batch(
            self.h, C.c_int(robot), C.c_int(len(trajs)), off.ctypes.data_as(vp), traj.ctypes.data_as(vp), travel.ctypes.data_as(vp),
            sg.ctypes.data_as(vp) if sg is not None else None, out.ctypes.data_as(vp), status.ctypes.data_as(vp)))
        return out, status

    def select_closures(self, closures, params=None, clipper=None):
        """slide_graph_select_closures: the mutually consistent subset of a list of loop closures, their endpoints resolved against
        the graph's current estimate (call it after a solve and before the closures are added; the graph is only read).  closures:
        dicts or tuples (from_robot, from_idx, to_robot, to_idx, rel7, sigma6) — the arguments of add_loop_closure plus the closure's
        own six sigmas [rot, trans].  Returns a dict: keep (bool per closure), group, status (SLIDE_MISSING: an endpoint the graph
        does not hold), n_selected / score per group."""
        fr, fi, tr, ti, rel, sg = _closure_arrays(closures)
        L = len(fr)
        p = params or closure_params()
        cp = clipper or clipper_params()
        keep, group, status = np.zeros(max(L, 1), np.int32), np.full(max(L, 1), -1, np.int32), np.zeros(max(L, 1), np.int32)
        nsel, score, ng = np.zeros(max(L, 1), np.int32), np.zeros(max(L, 1)), C.c_int(0)
        _check(self.L.slide_graph_select_closures(self.h, C.c_int(L), _p(fr), _p(fi), _p(tr), _p(ti), _p(rel), _p(sg), C.byref(p),
                                                  C.byref(cp), _p(keep), _p(group), _p(status), _p(nsel), _p(score), C.byref(ng)))
        return {"keep": keep[:L].astype(bool), "group": group[:L].copy(), "status": status[:L].copy(),
                "n_selected": nsel[:ng.value].copy(), "score": score[:ng.value].copy()}

    def get_pose_pair_covariances(self, pairs):
        """slide_graph_get_pose_pair_covariances (Marginals::jointMarginalCovariance): pairs = tuples (robot_a, idx_a, robot_b, idx_b).
        Returns ((n, 12, 12), (n,) int32 status): block k = [[Saa, Sab], [Sba, Sbb]], pose a's six coordinates then pose b's, tangent
        order [rot, trans]; a pair naming a pose the graph does not hold (SLIDE_MISSING) or one pose twice (SLIDE_ERR_INVALID) has
        zeros and its code.  The graph is only read."""
        rows = [tuple(p) for p in pairs]
        n = len(rows)
        ra, rb = (np.array([r[j] for r in rows] + [0], np.int32) for j in (0, 2))
        ia, ib = (np.array([r[j] for r in rows] + [0], np.uint64) for j in (1, 3))
        out, status = np.zeros((max(n, 1), 12, 12)), np.zeros(max(n, 1), np.int32)
        _check(self.L.slide_graph_get_pose_pair_covariances(self.h, C.c_int(n), _p(ra), _p(ia), _p(rb), _p(ib), _p(out), _p(status)))
        return out[:n], status[:n]

    def closure_mahalanobis(self, closures):
        """slide_graph_closure_mahalanobis: the individual-compatibility test of every closure of a list against the graph as it
        stands (call it after a solve and before the closures are added; the graph is only read).  closures: what select_closures
        takes.  Returns a dict: d2 (L) = r^T C^-1 r, chi-square with 6 degrees of freedom for a true closure — compare it with 16.81,
        no threshold is applied here; status (SLIDE_MISSING, SLIDE_ERR_INVALID for from == to, SLIDE_ERR_NOT_SPD; zeros then);
        C (L, 6, 6) = I + A Sigma A^T and r (L, 6), the whitened innovation covariance and residual."""
        fr, fi, tr, ti, rel, sg = _closure_arrays(closures)
        L = len(fr)
        n = max(L, 1)
        d2, Cm, r, status = np.zeros(n), np.zeros((n, 6, 6)), np.zeros((n, 6)), np.zeros(n, np.int32)
        _check(self.L.slide_graph_closure_mahalanobis(self.h, C.c_int(L), _p(fr), _p(fi), _p(tr), _p(ti), _p(rel), _p(sg), _p(d2), _p(Cm),
                                                      _p(r), _p(status)))
        return {"d2": d2[:L], "status": status[:L], "C": Cm[:L], "r": r[:L]}

    def observation_mahalanobis(self, candidates):
        """slide_graph_observation_mahalanobis: the individual-compatibility test of candidate landmark observations against the
        graph as it stands (call it after a solve and before the observations are added; the graph is only read).  candidates: tuples
        ("point", robot, pose_idx, lm_idx, bearing, range), ("cube", robot, pose_idx, idx, pose7, cube7, scale) or
        ("cylinder", robot, pose_idx, idx, pose7, root, ray, radius): the arguments of add_range_bearing / add_cube / add_cylinder
        for an existing landmark.  Returns a dict: d2 (n) = r^T C^-1 r, chi-square with dof (n) = 3 / 9 / 7 degrees of freedom for a
        true match — compare it with OBSERVATION_GATE_CHI2_99[dof], no threshold is applied here; status (SLIDE_MISSING,
        SLIDE_ERR_NOT_SPD; zeros then); C (n, 9, 9) = I + A H^-1 A^T, zero outside the dof x dof block, and r (n, 9), the whitened
        innovation covariance and residual."""
        n, k, robot, pidx, cls, lidx, meas, _ = _observation_arrays(candidates, False)
        d2, dof, Cm, r, status = np.zeros(k), np.zeros(k, np.int32), np.zeros((k, 9, 9)), np.zeros((k, 9)), np.zeros(k, np.int32)
        _check(self.L.slide_graph_observation_mahalanobis(self.h, C.c_int(n), _p(robot), _p(pidx), _p(cls), _p(lidx), _p(meas), _p(d2),
                                                          _p(dof), _p(Cm), _p(r), _p(status)))
        return {"d2": d2[:n], "dof": dof[:n], "status": status[:n], "C": Cm[:n], "r": r[:n]}

    def predicted_observation_mahalanobis(self, robot, from_idx, rel7, est7, candidates):
        """slide_graph_predicted_observation_mahalanobis: observation_mahalanobis at a PREDICTED pose — est7, the value
        add_keypose_between(robot, from_idx, ., rel7, est7) would give a new pose — before that pose or anything else is added: the
        gate that call would compute on the graph extended by the pose and its Between factor.  candidates: the tuples
        observation_mahalanobis takes; their robot and pose_idx fields are IGNORED (every candidate sits at the predicted pose), so
        a frame's list can be passed to either call.  Returns that call's dict.  Raises SlideError("SLIDE_MISSING...") when the
        graph does not hold the from pose."""
        n, k, _, _, cls, lidx, meas, _ = _observation_arrays(candidates, False)
        d2, dof, Cm, r, status = np.zeros(k), np.zeros(k, np.int32), np.zeros((k, 9, 9)), np.zeros((k, 9)), np.zeros(k, np.int32)
        rc = self.L.slide_graph_predicted_observation_mahalanobis(self.h, C.c_int(robot), C.c_uint64(from_idx), _p(_d(rel7)), _p(_d(est7)),
                                                                  C.c_int(n), _p(cls), _p(lidx), _p(meas), _p(d2), _p(dof), _p(Cm), _p(r),
                                                                  _p(status))
        if rc == SLIDE_MISSING:
            raise SlideError(f"SLIDE_MISSING: {last_error()}")
        _check(rc)
        return {"d2": d2[:n], "dof": dof[:n], "status": status[:n], "C": Cm[:n], "r": r[:n]}

    @staticmethod
    def _landmark_pair_arrays(cls, pairs):
        rows = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1, 2)
        n = len(rows)
        k = max(n, 1)
        ia, ib = np.zeros(k, np.uint64), np.zeros(k, np.uint64)
        ia[:n], ib[:n] = rows[:, 0], rows[:, 1]
        return n, k, np.full(k, cls, np.int32), ia, ib

    def landmark_pair_mahalanobis(self, cls, pairs, sigma):
        """slide_graph_landmark_pair_mahalanobis: are landmarks a and b of class `cls` (CLS_ELLIPSOID or CLS_CYLINDER; cubes are
        refused) one object mapped twice?  pairs: (idx_a, idx_b) rows; sigma: the model noise of the hypothesis in the class's tangent
        order (3 or 7 entries, > 0, or one scalar for all).  Returns a dict: d2 (n) = r^T C^-1 r with r = (est_b - est_a) / sigma and
        C = I + diag(1 / sigma) (Sig_aa + Sig_bb - Sig_ab - Sig_ba) diag(1 / sigma), chi-square with dof (n) = 3 / 7 degrees of freedom
        for one object — compare it with chi2_quantile(0.99, dof), no threshold is applied here; status (SLIDE_MISSING, SLIDE_ERR_INVALID
        for a == b, SLIDE_ERR_NOT_SPD; zeros then); route (0: read off the selected inverse, 1: forward substitution); C (n, 9, 9), zero
        outside the dof x dof block, and r (n, 9).  Call it after a solve; the graph is only read."""
        n, k, c, ia, ib = self._landmark_pair_arrays(cls, pairs)
        D = 7 if cls == CLS_CYLINDER else 3
        sg = np.ascontiguousarray(np.broadcast_to(_d(sigma).reshape(-1), (D,)) if np.size(sigma) == 1 else _d(sigma).reshape(-1))
        if len(sg) != D:
            raise SlideError(f"landmark_pair_mahalanobis: sigma takes {D} entries for this class, got {len(sg)}")
        d2, dof, Cm, r = np.zeros(k), np.zeros(k, np.int32), np.zeros((k, 9, 9)), np.zeros((k, 9))
        route, status = np.zeros(k, np.int32), np.zeros(k, np.int32)
        _check(self.L.slide_graph_landmark_pair_mahalanobis(self.h, C.c_int(n), _p(c), _p(ia), _p(ib), _p(sg), _p(sg), _p(d2), _p(dof), _p(Cm),
                                                            _p(r), _p(route), _p(status)))
        return {"d2": d2[:n], "dof": dof[:n], "status": status[:n], "route": route[:n], "C": Cm[:n], "r": r[:n]}

    def get_landmark_pair_covariances(self, cls, pairs):
        """slide_graph_get_landmark_pair_covariances (Marginals::jointMarginalCovariance({L(a), L(b)})): pairs = (idx_a, idx_b) rows of
        landmarks of class `cls`, any of the three.  Returns ((n, 2 d, 2 d) blocks [[Saa, Sab], [Sba, Sbb]], d = 7 / 9 / 3, in the
        tangent order of get_landmark_covariances, (n,) int32 status, (n,) int32 route); a pair naming a landmark the graph does not
        hold (SLIDE_MISSING) or one landmark twice (SLIDE_ERR_INVALID) has zeros and its code.  The graph is only read."""
        n, k, c, ia, ib = self._landmark_pair_arrays(cls, pairs)
        d = {CLS_CYLINDER: 7, CLS_CUBE: 9}.get(cls, 3)
        out, route, status = np.zeros((k, 18, 18)), np.zeros(k, np.int32), np.zeros(k, np.int32)
        _check(self.L.slide_graph_get_landmark_pair_covariances(self.h, C.c_int(n), _p(c), _p(ia), _p(ib), _p(out), _p(route), _p(status)))
        return out[:n, :2 * d, :2 * d].copy(), status[:n], route[:n]

    def landmark_pairs_within(self, cls, radius, idx=None, labels=None):
        """slide_graph_landmark_pairs_within: every pair of landmarks of class `cls` whose anchors (point xyz, cube translation,
        cylinder root of the current estimate) lie within `radius`, searched on the device.  idx: the landmark keys to search among
        (None: every landmark of the class, in the graph's order); labels: one per searched landmark, only equal labels pair.  Returns
        (idx_a, idx_b, dist), sorted by the positions in the selection.  KeyError for a selected landmark the graph does not hold."""
        sel = None if idx is None else np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        lab = None if labels is None else _i(labels).reshape(-1)
        if sel is not None and lab is not None and len(lab) != len(sel):
            raise SlideError("landmark_pairs_within: one label per selected landmark")
        nsel = 0 if sel is None else len(sel)
        total, cap = C.c_int64(0), 0
        for _ in range(2):      # (the first call counts, the second has room)
            ia, ib, dist = np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1), np.uint64), np.zeros(max(cap, 1))
            st = self.L.slide_graph_landmark_pairs_within(self.h, C.c_int(cls), C.c_double(radius), C.c_int(nsel), _p(sel) if sel is not None else None,
                                                          _p(lab) if lab is not None else None, C.c_int64(cap), _p(ia), _p(ib), _p(dist),
                                                          C.byref(total))
            if st == SLIDE_MISSING:
                raise KeyError(f"landmark of class {cls} not in the graph")
            if st != -3:      # SLIDE_ERR_CAPACITY: now the total is known
                _check(st)
                break
            cap = total.value
        return ia[:total.value], ib[:total.value], dist[:total.value]

    def duplicate_landmarks(self, cls, radius, sigma, prob=0.99, idx=None, labels=None):
        """The landmarks of class `cls` (CLS_ELLIPSOID or CLS_CYLINDER) that are one object mapped twice: landmark_pairs_within
        proposes the pairs within `radius`, landmark_pair_mahalanobis tests them under the model noise `sigma`, and the pairs with
        status 0 and d2 <= chi2_quantile(prob, D) are kept.  Returns (idx_a, idx_b, d2, dist) of the kept pairs.  The graph is only
        read; merging the pairs: `merge_landmarks` (merge_duplicates does both)."""
        ia, ib, dist = self.landmark_pairs_within(cls, radius, idx, labels)
        res = self.landmark_pair_mahalanobis(cls, np.stack([ia, ib], axis=1), sigma)
        keep = (res["status"] == 0) & (res["d2"] <= chi2_quantile(prob, 7 if cls == CLS_CYLINDER else 3))
        return ia[keep], ib[keep], res["d2"][keep], dist[keep]

    def merge_landmarks(self, cls, pairs, fuse=True):
        """slide_graph_merge_landmarks: pairs = (keep, drop) rows of landmarks of class `cls` that are one object mapped twice.  Every
        factor of `drop` becomes a factor of `keep`, the dropped key stays as an alias of the survivor (get_landmark, later
        observations), its slot as a tombstone no walk visits.  Pairs are applied in order and a dropped key stands for its survivor,
        so chains and triangles are legal.  fuse (points and cylinders): the survivor takes (sum H_i)^-1 sum H_i est_i over its
        cluster, H_i each member's own H_ll at the last linearisation — call it after a solve then; fuse=False keeps the survivor's
        estimate and has no such requirement.  Returns a dict: into (the key each pair resolves to), moved (factors re-pointed by
        the pair), status (SLIDE_MISSING, SLIDE_ERR_INVALID for keep == drop, SLIDE_ERR_NOT_SPD for a failed fusion).  The next
        update is a full one at the current estimate; the marginal queries refuse until it ran."""
        if cls not in (CLS_CYLINDER, CLS_CUBE, CLS_ELLIPSOID):
            raise SlideError(f"merge_landmarks: {cls!r} is not a landmark class")
        rows = np.asarray(pairs)
        if rows.size and (rows.ndim != 2 or rows.shape[1] != 2):
            raise SlideError("merge_landmarks: pairs are rows of (keep, drop)")
        if rows.size and np.any(rows < 0):
            raise SlideError("merge_landmarks: a negative landmark index")
        n, k, c, keep, drop = self._landmark_pair_arrays(cls, rows)
        into, moved, status = np.zeros(k, np.uint64), np.zeros(k, np.int32), np.zeros(k, np.int32)
        _check(self.L.slide_graph_merge_landmarks(self.h, C.c_int(n), _p(c), _p(keep), _p(drop), C.c_int(1 if fuse else 0), _p(into), _p(moved),
                                                  _p(status)))
        return {"into": into[:n], "moved": moved[:n], "status": status[:n]}

    def landmark_alias(self, cls, idx):
        """slide_graph_landmark_alias: the key landmark (cls, idx) resolves to — itself unless merge_landmarks dropped it, then its
        survivor's.  KeyError for a landmark the graph does not know."""
        out = C.c_uint64(0)
        st = self.L.slide_graph_landmark_alias(self.h, C.c_int(cls), C.c_uint64(idx), C.byref(out))
        if st == SLIDE_MISSING:
            raise KeyError(f"landmark {idx} of class {cls} not in the graph")
        _check(st)
        return int(out.value)

    def merge_timing(self):
        """slide_graph_merge_timing: ms of the last merge_landmarks call — host restructure, upload, fusion with its read-back (wall),
        k_lm_merge_fuse alone (HIP events)."""
        out = np.zeros(4)
        _check(self.L.slide_graph_merge_timing(self.h, _p(out)))
        return {"host_ms": out[0], "upload_ms": out[1], "fuse_ms": out[2], "fuse_kernel_ms": out[3]}

    def merge_duplicates(self, cls, radius, sigma, prob=0.99, idx=None, labels=None, fuse=True):
        """duplicate_landmarks, then merge_clusters, then merge_landmarks: finds the landmarks of class `cls` mapped twice and merges
        each cluster into its smallest key.  Returns (idx_a, idx_b, d2 of the kept pairs, merge_landmarks' dict with `pairs`, the
        (survivor, member) rows it was given)."""
        ia, ib, d2, _ = self.duplicate_landmarks(cls, radius, sigma, prob, idx, labels)
        rows = merge_clusters(ia, ib)
        res = self.merge_landmarks(cls, rows, fuse)
        res["pairs"] = rows
        return ia, ib, d2, res

    def observation_joint_compatibility(self, groups, prob=0.99):
        """slide_graph_observation_joint_compatibility: the joint compatibility of a key frame's landmark matches, tested together
        (Neira and Tardos' test in its greedy sequential form).  groups: a list of hypotheses, each a list of the candidate tuples
        observation_mahalanobis takes, tried in the given order.  A candidate is accepted iff it passes alone (d2_single against the
        prob quantile of its own rows) and stacked on the candidates accepted before it (d2_joint against the quantile of dof_joint);
        prob=0 evaluates only: every served candidate is accepted and d2_joint is the prefix sequence of the stacked test.  Returns a
        dict: per candidate, in the groups' order, accepted, d2_single, d2_joint, dof_joint, status (SLIDE_MISSING: skipped, the rest
        of its group served without it; SLIDE_ERR_NOT_SPD: rejected); per group group_d2, group_dof, group_count (the accepted set's
        stacked d2, rows and size) and group_status (SLIDE_ERR_INVALID: a landmark named twice, SLIDE_ERR_CAPACITY: more than 384
        rows; zeros in the group then); group_ptr, the groups' offsets into the candidate arrays."""
        groups = [list(g) for g in groups]
        ng = len(groups)
        ptr = np.zeros(ng + 1, np.int32)
        ptr[1:] = np.cumsum([len(g) for g in groups])
        n, k, robot, pidx, cls, lidx, meas, _ = _observation_arrays([c for g in groups for c in g], False)
        acc, dofj, status = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        d2s, d2j = np.zeros(k), np.zeros(k)
        kg = max(ng, 1)
        gd2, gdof, gcnt, gst = np.zeros(kg), np.zeros(kg, np.int32), np.zeros(kg, np.int32), np.zeros(kg, np.int32)
        _check(self.L.slide_graph_observation_joint_compatibility(
            self.h, C.c_int(ng), _p(ptr), _p(robot), _p(pidx), _p(cls), _p(lidx), _p(meas), C.c_double(prob), _p(acc), _p(d2s), _p(d2j), _p(dofj),
            _p(status), _p(gd2), _p(gdof), _p(gcnt), _p(gst)))
        return {"accepted": acc[:n].astype(bool), "d2_single": d2s[:n], "d2_joint": d2j[:n], "dof_joint": dofj[:n], "status": status[:n],
                "group_d2": gd2[:ng], "group_dof": gdof[:ng], "group_count": gcnt[:ng], "group_status": gst[:ng], "group_ptr": ptr}

    def set_ghosts(self, own_robot, own_idx):
        r = _i(own_robot)
        i = np.ascontiguousarray(own_idx, dtype=np.int64)
        _check(self.L.slide_graph_set_ghosts(self.h, _p(r), _p(i), C.c_int(len(r))))

    def add_relative_meas_ghost(self, rel7, idx, robot, slot, local_first):
        _check(self.L.slide_graph_add_relative_meas_ghost(self.h, _p(_d(rel7)), C.c_uint64(idx), C.c_int(robot), C.c_int(slot),
                                                          C.c_int(int(local_first))))

    def join_chol_batch(self, batch, slot=0):
        """Share the dense factor + solve of phase 1 with the other graphs of `batch` (CholBatch; None leaves it)."""
        _check(self.L.slide_graph_join_chol_batch(self.h, C.c_void_p(batch.h if batch is not None else None), C.c_int(slot)))

    def set_pcg(self, iterations, tol=0.0):
        """Un-batched passes: PCG iterations of the joint solve (dist_phase 31 / 32 / 33 between phases 1 and 2); 0 = block solves only.
        tol > 0: iterations past a relative reduction of sqrt(r^T M^-1 r) by tol are no-ops."""
        _check(self.L.slide_graph_set_pcg_tolerance(self.h, C.c_double(float(tol))))
        _check(self.L.slide_graph_set_pcg(self.h, C.c_int(iterations)))

    def set_ghost_ids(self, ids, n_total):
        """Exact joint step: ids[i] = index of this graph's i-th ghost factor in the job's list of n_total relative-pose measurements."""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        _check(self.L.slide_graph_set_ghost_ids(self.h, _p(a), C.c_int(len(a)), C.c_int(int(n_total))))

    def set_separator(self, offsets):
        """Exact joint step: offsets of the shared slots' tangent coordinates in the separator system (n_slots + 1 ints)."""
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        _check(self.L.slide_graph_set_separator(self.h, _p(off), C.c_int(len(off))))

    ROBUST_KINDS = ROBUST_KINDS

    def set_robust_loss(self, kind, param=0.0, closures=True, relative_meas=True):
        """slide_graph_set_robust_loss (GTSAM's noiseModel::Robust on the loop-closure / relative-measurement factors, iteratively
        reweighted): kind = 0 / None (off), 1 / "huber", 2 / "cauchy", 3 / "geman_mcclure", 4 / "dcs"; param <= 0: the loss's default
        (1.345, 0.1, 1.0, 1.0).  Covers factors already added and added later; the next solve relinearises everything."""
        mask = (1 if closures else 0) | (2 if relative_meas else 0)
        _check(self.L.slide_graph_set_robust_loss(self.h, _loss_kind(kind, "robust"), C.c_double(float(param)), C.c_int(mask)))

    def closure_weights(self, cap=None):
        """slide_graph_get_closure_weights: every loop-closure (kind 1) and relative-measurement (kind 2) factor in insertion order.
        Returns a dict of arrays: from_robot, from_idx, to_robot, to_idx, kind, weight, s2 (weight and squared whitened norm of the
        factor's last linearisation; weight 1 where no loss applied) and n, the full count (cap: write at most that many)."""
        return _weights(self.L.slide_graph_get_closure_weights, self.h, _CLOSURE_COLS + _WEIGHT_COLS, cap)

    def set_observation_loss(self, kind, param=0.0, points=True, cubes=True, cylinders=True):
        """slide_graph_set_observation_loss (GTSAM's noiseModel::Robust on the bearing-range / cube / cylinder factors, iteratively
        reweighted inside the linearisation kernel): kinds, names and defaults as set_robust_loss; independent of it.  Covers
        factors already added and added later; the next solve relinearises everything."""
        mask = (1 if points else 0) | (2 if cubes else 0) | (4 if cylinders else 0)
        _check(self.L.slide_graph_set_observation_loss(self.h, _loss_kind(kind, "observation"), C.c_double(float(param)), C.c_int(mask)))

    def observation_weights(self, cap=None):
        """slide_graph_get_observation_weights: every landmark factor in insertion order.  Returns a dict of arrays: robot, pose_idx,
        cls (SLIDE_CLS_*), lm_idx, weight, s2 (weight and unscaled squared whitened norm of the factor's last linearisation; weight 1
        where no loss applied) and n, the full count (cap: write at most that many)."""
        return _weights(self.L.slide_graph_get_observation_weights, self.h, [("robot", _I32)] + _OBSERVATION_COLS + _WEIGHT_COLS, cap)

    def chi2(self):
        """Sum of squared whitened residuals at the current estimate: dict(total, prior, between, landmark).  While a robust loss
        is set (on the closures or on the observations): of the reweighted system."""
        out = np.zeros(4)
        _check(self.L.slide_graph_chi2(self.h, _p(out)))
        return dict(total=out[0], prior=out[1], between=out[2], landmark=out[3])

    def tile_profile(self):
        """Tile-level profile of the reduced pose system: prof[c] = last tile row of block column c inside it (64 x 64 tiles)."""
        T = self.L.slide_graph_get_tile_profile(self.h, None, C.c_int(0))
        if T < 0:
            _check(T)
        out = np.zeros(max(T, 1), np.int32)
        T = self.L.slide_graph_get_tile_profile(self.h, _p(out), C.c_int(T))
        if T < 0:
            _check(T)
        return out[:T]

    def set_incremental(self, on=True):
        """False: every update re-factors all block columns (the reference behaviour of round 2; same result to rounding)."""
        _check(self.L.slide_graph_set_incremental(self.h, C.c_int(int(on))))

    def set_wildfire(self, threshold):
        """iSAM2's wildfire threshold on the back-substitution of incremental updates (0: off, the default; the reference's GTSAM: 1e-3)."""
        _check(self.L.slide_graph_set_wildfire(self.h, C.c_double(threshold)))

    def wildfire_stats(self):
        out = np.zeros(2, np.int64)
        _check(self.L.slide_graph_get_wildfire_stats(self.h, _p(out)))
        return dict(kept_total=int(out[0]), kept_last=int(out[1]))

    def incremental_stats(self):
        """Updates that re-factored a suffix of the block columns only / everything, first re-factored column of the last, block columns."""
        out = np.zeros(4, np.int64)
        _check(self.L.slide_graph_get_incremental_stats(self.h, _p(out)))
        return dict(incremental=int(out[0]), full=int(out[1]), last_first_column=int(out[2]), block_columns=int(out[3]))

    def segments(self):
        """Exact joint passes: (tile ranges of the band's segments, separator poses); ([], 0) when the band is not cut."""
        out = np.zeros(32, np.int32)
        n = self.L.slide_graph_get_segments(self.h, _p(out), C.c_int(32))
        if n < 0:
            _check(-n)
        if n <= 1:
            return [], 0
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)], int(out[2 * n])

    def segment_table(self):
        """Exact joint passes over a cut band: (ends, first) — ends[s] = last block column + 1 of segment s, first[s][i] = first block
        column of segment s in which border tile row i is non-zero (i = nbr: the right-hand side; 1 << 30: never) — or None."""
        n = self.L.slide_graph_get_segment_table(self.h, None, C.c_int(0))
        if n < 0:
            _check(-n)
        if n == 0:
            return None
        out = np.zeros(n, np.int32)
        self.L.slide_graph_get_segment_table(self.h, _p(out), C.c_int(n))
        ns = int(out[0])
        w = (n - 1 - ns) // ns
        return [int(v) for v in out[1:1 + ns]], out[1 + ns:].reshape(ns, w).astype(np.int64)

    def border_profile(self):
        """Exact joint step: first[i] = first block column of the band in which border tile row i can be non-zero (len = border row tiles)."""
        n = self.L.slide_graph_get_border_profile(self.h, None, C.c_int(0))
        if n < 0:
            _check(-n)
        out = np.zeros(max(n, 1), np.int32)
        n = self.L.slide_graph_get_border_profile(self.h, _p(out), C.c_int(n))
        if n < 0:
            _check(-n)
        return out[:n]

    def set_dense_profile(self, on=True):
        """Measurement aid: make the solver ignore the structure (every tile of the lower triangle)."""
        _check(self.L.slide_graph_set_dense_profile(self.h, C.c_int(1 if on else 0)))

    def pcg_stats(self):
        out = np.zeros(8)
        _check(self.L.slide_graph_get_pcg_stats(self.h, _p(out)))
        return dict(alpha=out[2], beta=out[3], gamma_first=out[4], gamma_last=out[5])

    def dist_pass_local(self, d_buf_ptr):
        """One distributed pass with device-side exchanges: every robot of the job must be in this graph's CholBatch."""
        return _check(self.L.slide_graph_dist_pass_local(self.h, C.c_void_p(d_buf_ptr)))

    def dist_phase(self, phase, d_buf_ptr):
        """d_buf_ptr: integer DEVICE address of the exchange buffer (e.g. torch_tensor.data_ptr())."""
        return _check(self.L.slide_graph_dist_phase(self.h, C.c_int(phase), C.c_void_p(d_buf_ptr)))

    def set_profiling(self, on=True):
        _check(self.L.slide_graph_set_profiling(self.h, C.c_int(int(on))))

    def get_profile(self):
        names = C.create_string_buffer(32 * 32)
        ms = np.zeros(32)
        cnt = np.zeros(32, np.int64)
        n = self.L.slide_graph_get_profile(self.h, names, _p(ms), _p(cnt), C.c_int(32))
        out = {}
        for i in range(n):
            nm = names.raw[32 * i: 32 * i + 32].split(b"\0")[0].decode()
            out[nm] = dict(ms=float(ms[i]), launches=int(cnt[i]))
        return out


class CholBatch:
    """slide_chol_batch_t: the graphs of several robots on one GPU factor and solve their pose systems in one launch sequence."""

    def __init__(self, n_graphs):
        self.L = lib()
        self.h = self.L.slide_chol_batch_create(C.c_int(n_graphs))
        if not self.h:
            raise ValueError("CholBatch: 1 .. 8 graphs")

    def pass_all(self, buf_ptrs):
        """One distributed pass of all joined graphs from this thread; buf_ptrs[i] = device address of slot i's exchange buffer."""
        arr = (C.c_void_p * len(buf_ptrs))(*[int(p) for p in buf_ptrs])
        return _check(self.L.slide_chol_batch_pass(C.c_void_p(self.h), arr))

    def get_pose_covariances(self, slot, idx):
        """Marginal covariances on the JOINT graph (exact joint passes; slide_gpu.h) of the poses `idx` of the robot whose graph is in
        `slot`: (n, 6, 6), tangent order [rot, trans].  KeyError for an unknown pose."""
        ids = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        out = np.zeros(36 * len(ids))
        st = self.L.slide_chol_batch_get_pose_covariances(C.c_void_p(self.h), C.c_int(slot), _p(ids), C.c_int(len(ids)), _p(out))
        if st == SLIDE_MISSING:
            raise KeyError(f"pose of slot {slot} not in the graph")
        _check(st)
        return out.reshape(-1, 6, 6)

    def get_landmark_covariances(self, slot, cls, idx):
        """Joint-graph marginal covariances of the landmarks `idx` (that graph's ids) of class `cls` of the graph in `slot`: (n, d, d)."""
        d = {CLS_CYLINDER: 7, CLS_CUBE: 9}.get(cls, 3)
        ids = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        out = np.zeros(d * d * len(ids))
        st = self.L.slide_chol_batch_get_landmark_covariances(C.c_void_p(self.h), C.c_int(slot), C.c_int(cls), _p(ids), C.c_int(len(ids)), _p(out))
        if st == SLIDE_MISSING:
            raise KeyError(f"landmark of class {cls} not in slot {slot}")
        _check(st)
        return out.reshape(-1, d, d)

    def marginal_traces(self, slot):
        """logEntropy on the joint graph: [pose trace sum of the robot in `slot`, the job's point-landmark trace sum, #poses, #points]."""
        out = np.zeros(4)
        _check(self.L.slide_chol_batch_marginal_traces(C.c_void_p(self.h), C.c_int(slot), _p(out)))
        return out

    def closure_info_gain(self, slot, traj, travel, sigma_per_m=None, traj_slots=None):
        """estimateClosureInfoGain on the JOINT graph (slide_gpu.h): [10 pose + landmark, pose drop of the robot in `slot`, the job's
        point-landmark drop, pose drop of every robot] of Between factors (traj[i+1], traj[i]) with noise sigma_per_m * travel[i] (None:
        the noise_model_odom_vec of the graph in `slot`).  traj_slots[q]: the slot whose robot owns pose traj[q] (None: all `slot`)."""
        t = np.ascontiguousarray(traj, dtype=np.uint64).reshape(-1)
        tr = _d(travel).reshape(-1)
        if len(tr) != max(len(t) - 1, 0):
            raise ValueError("travel needs one distance per step of traj")
        sg = None
        if sigma_per_m is not None:
            sg = _d(sigma_per_m).reshape(-1)
            if len(sg) != 6:
                raise ValueError("sigma_per_m has six entries")
        ts = None
        if traj_slots is not None:
            ts = np.ascontiguousarray(traj_slots, dtype=np.int32).reshape(-1)
            if len(ts) != len(t):
                raise ValueError("traj_slots needs one slot per pose of traj")
        out = np.zeros(4)
        st = self.L.slide_chol_batch_closure_info_gain(C.c_void_p(self.h), C.c_int(slot), _p(ts) if ts is not None else None, _p(t),
                                                       C.c_int(len(t)), _p(tr), _p(sg) if sg is not None else None, _p(out))
        if st == SLIDE_MISSING:
            raise KeyError(f"trajectory pose not in the joint graph (slot {slot})")
        _check(st)
        return out

    def closure_info_gain_batch(self, slot, trajs, travels, sigma_per_m=None, traj_slots=None):
        """closure_info_gain on the JOINT graph for a list of candidates in one call (slide_chol_batch_closure_info_gain_batch):
        trajs[k] / travels[k] / traj_slots[k] as the single call's arguments (traj_slots None: every pose in `slot`).  Returns
        ((n, 4) gains, (n,) int32 status): row k is what closure_info_gain gives for candidate k alone; a candidate with a fault of
        its own has zeros and its code."""
        off, traj, travel, slots = _candidate_list(trajs, travels, traj_slots)
        sg = _sigma6(sigma_per_m)
        out = np.zeros((len(trajs), 4))
        status = np.zeros(len(trajs), dtype=np.int32)
        vp = C.c_void_p
        _check(self.L.slide_chol_batch_closure_info_gain_batch(
            C.c_void_p(self.h), C.c_int(slot), C.c_int(len(trajs)), off.ctypes.data_as(vp),
            slots.ctypes.data_as(vp) if slots is not None else None, traj.ctypes.data_as(vp), travel.ctypes.data_as(vp),
            sg.ctypes.data_as(vp) if sg is not None else None, out.ctypes.data_as(vp), status.ctypes.data_as(vp)))
        return out, status

    def get_pose_pair_covariances(self, pairs):
        """slide_chol_batch_get_pose_pair_covariances (Marginals::jointMarginalCovariance on the JOINT graph): pairs = tuples
        (slot_a, idx_a, slot_b, idx_b); the two poses may belong to different slots.  Returns ((n, 12, 12), (n,) int32 status) as
        SlideGraph.get_pose_pair_covariances: a pair naming a slot the batch does not have or a pose its graph does not hold
        (SLIDE_MISSING) or one pose twice (SLIDE_ERR_INVALID) has zeros and its code.  The batch is only read."""
        rows = [tuple(p) for p in pairs]
        n = len(rows)
        sa, sb = (np.array([r[j] for r in rows] + [0], np.int32) for j in (0, 2))
        ia, ib = (np.array([r[j] for r in rows] + [0], np.uint64) for j in (1, 3))
        out, status = np.zeros((max(n, 1), 12, 12)), np.zeros(max(n, 1), np.int32)
        _check(self.L.slide_chol_batch_get_pose_pair_covariances(C.c_void_p(self.h), C.c_int(n), _p(sa), _p(ia), _p(sb), _p(ib), _p(out),
                                                                 _p(status)))
        return out[:n], status[:n]

    def closure_mahalanobis(self, closures):
        """slide_chol_batch_closure_mahalanobis: SlideGraph.closure_mahalanobis on the JOINT graph, for closures whose two ends may sit
        in different robots' graphs.  closures: what select_closures takes, with from_robot / to_robot read as slots of the batch.
        Returns the same dict: d2 (L) to compare with 16.81 (no threshold is applied), status (SLIDE_MISSING, SLIDE_ERR_INVALID for
        from == to, SLIDE_ERR_NOT_SPD; zeros then), C (L, 6, 6) = I + A Sigma A^T and r (L, 6)."""
        fs, fi, ts, ti, rel, sg = _closure_arrays(closures)
        L = len(fs)
        n = max(L, 1)
        d2, Cm, r, status = np.zeros(n), np.zeros((n, 6, 6)), np.zeros((n, 6)), np.zeros(n, np.int32)
        _check(self.L.slide_chol_batch_closure_mahalanobis(C.c_void_p(self.h), C.c_int(L), _p(fs), _p(fi), _p(ts), _p(ti), _p(rel), _p(sg),
                                                           _p(d2), _p(Cm), _p(r), _p(status)))
        return {"d2": d2[:L], "status": status[:L], "C": Cm[:L], "r": r[:L]}

    def observation_mahalanobis(self, candidates):
        """slide_chol_batch_observation_mahalanobis: SlideGraph.observation_mahalanobis on the JOINT graph.  candidates: that call's
        tuples with a slot of the batch where they name a robot — ("point", slot, pose_idx, lm_idx, bearing, range), ("cube", slot,
        pose_idx, idx, pose7, cube7, scale), ("cylinder", slot, pose_idx, idx, pose7, root, ray, radius) — and optionally one more
        trailing value, lm_slot: the slot whose graph holds the landmark (idx is then its index THERE), for robot a's pose against a
        landmark of robot b.  Returns the same dict: d2 to compare with OBSERVATION_GATE_CHI2_99[dof] (no threshold is applied), dof,
        status (SLIDE_MISSING, SLIDE_ERR_NOT_SPD; zeros then), C (n, 9, 9) and r (n, 9).  The batch is only read."""
        n, k, slot, pidx, cls, lidx, meas, lslot = _observation_arrays(candidates, True)
        d2, dof, Cm, r, status = np.zeros(k), np.zeros(k, np.int32), np.zeros((k, 9, 9)), np.zeros((k, 9)), np.zeros(k, np.int32)
        _check(self.L.slide_chol_batch_observation_mahalanobis(C.c_void_p(self.h), C.c_int(n), _p(slot), _p(pidx), _p(lslot), _p(cls), _p(lidx),
                                                               _p(meas), _p(d2), _p(dof), _p(Cm), _p(r), _p(status)))
        return {"d2": d2[:n], "dof": dof[:n], "status": status[:n], "C": Cm[:n], "r": r[:n]}

    def observation_joint_compatibility(self, groups, prob=0.99):
        """slide_chol_batch_observation_joint_compatibility: SlideGraph.observation_joint_compatibility on the JOINT graph — a frame's
        landmark matches tested together on the factor of the last exact pass.  groups: a list of hypotheses, each a list of the
        candidate tuples observation_mahalanobis takes here (slots for robots, an optional trailing lm_slot), tried in the given
        order; prob=0 evaluates only.  A private landmark may be named once per group (SLIDE_ERR_INVALID for the group otherwise), a
        shared one as often as the caller likes, through any replica.  Returns SlideGraph.observation_joint_compatibility's dict:
        accepted, d2_single, d2_joint, dof_joint, status per candidate; group_d2, group_dof, group_count, group_status per group;
        group_ptr.  The batch is only read."""
        groups = [list(g) for g in groups]
        ng = len(groups)
        ptr = np.zeros(ng + 1, np.int32)
        ptr[1:] = np.cumsum([len(g) for g in groups])
        n, k, slot, pidx, cls, lidx, meas, lslot = _observation_arrays([c for g in groups for c in g], True)
        acc, dofj, status = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        d2s, d2j = np.zeros(k), np.zeros(k)
        kg = max(ng, 1)
        gd2, gdof, gcnt, gst = np.zeros(kg), np.zeros(kg, np.int32), np.zeros(kg, np.int32), np.zeros(kg, np.int32)
        _check(self.L.slide_chol_batch_observation_joint_compatibility(
            C.c_void_p(self.h), C.c_int(ng), _p(ptr), _p(slot), _p(pidx), _p(lslot), _p(cls), _p(lidx), _p(meas), C.c_double(prob), _p(acc), _p(d2s),
            _p(d2j), _p(dofj), _p(status), _p(gd2), _p(gdof), _p(gcnt), _p(gst)))
        return {"accepted": acc[:n].astype(bool), "d2_single": d2s[:n], "d2_joint": d2j[:n], "dof_joint": dofj[:n], "status": status[:n],
                "group_d2": gd2[:ng], "group_dof": gdof[:ng], "group_count": gcnt[:ng], "group_status": gst[:ng], "group_ptr": ptr}

    @staticmethod
    def _landmark_pair_arrays(cls, pairs):
        rows = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 4)
        n = len(rows)
        k = max(n, 1)
        sa, sb, ia, ib = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.uint64), np.zeros(k, np.uint64)
        sa[:n], ia[:n], sb[:n], ib[:n] = rows[:, 0], rows[:, 1].astype(np.uint64), rows[:, 2], rows[:, 3].astype(np.uint64)
        return n, k, np.full(k, cls, np.int32), sa, ia, sb, ib

    def landmark_pair_mahalanobis(self, cls, pairs, sigma):
        """slide_chol_batch_landmark_pair_mahalanobis: SlideGraph.landmark_pair_mahalanobis on the JOINT graph — are two landmarks of
        class `cls` (CLS_ELLIPSOID or CLS_CYLINDER; cubes are refused), of one robot or of two, one object?  pairs: rows
        (slot_a, idx_a, slot_b, idx_b), idx the landmark's index in the graph of its slot; a shared landmark may be named through any
        replica.  sigma: the hypothesis' model noise as there.  Returns that call's dict without `route` (every pair takes the
        forward substitution): d2 to compare with chi2_quantile(0.99, dof) (no threshold is applied), dof, status (SLIDE_MISSING,
        SLIDE_ERR_INVALID for two names of one variable, SLIDE_ERR_NOT_SPD; zeros then), C (n, 9, 9) and r (n, 9).  Call it after an
        exact joint pass; the batch is only read."""
        n, k, c, sa, ia, sb, ib = self._landmark_pair_arrays(cls, pairs)
        D = 7 if cls == CLS_CYLINDER else 3
        sg = np.ascontiguousarray(np.broadcast_to(_d(sigma).reshape(-1), (D,)) if np.size(sigma) == 1 else _d(sigma).reshape(-1))
        if len(sg) != D:
            raise SlideError(f"landmark_pair_mahalanobis: sigma takes {D} entries for this class, got {len(sg)}")
        d2, dof, Cm, r, status = np.zeros(k), np.zeros(k, np.int32), np.zeros((k, 9, 9)), np.zeros((k, 9)), np.zeros(k, np.int32)
        _check(self.L.slide_chol_batch_landmark_pair_mahalanobis(C.c_void_p(self.h), C.c_int(n), _p(c), _p(sa), _p(ia), _p(sb), _p(ib), _p(sg),
                                                                 _p(sg), _p(d2), _p(dof), _p(Cm), _p(r), _p(status)))
        return {"d2": d2[:n], "dof": dof[:n], "status": status[:n], "C": Cm[:n], "r": r[:n]}

    def get_landmark_pair_covariances(self, cls, pairs):
        """slide_chol_batch_get_landmark_pair_covariances: the joint marginal [[Saa, Sab], [Sba, Sbb]] of landmark pairs of class
        `cls` (any of the three) on the JOINT graph, the block between two robots' landmarks included.  pairs as
        landmark_pair_mahalanobis takes them.  Returns ((n, 2 d, 2 d), (n,) int32 status); SLIDE_MISSING / SLIDE_ERR_INVALID pairs
        have zeros and their code.  The batch is only read."""
        n, k, c, sa, ia, sb, ib = self._landmark_pair_arrays(cls, pairs)
        d = {CLS_CYLINDER: 7, CLS_CUBE: 9}.get(cls, 3)
        out, status = np.zeros((k, 18, 18)), np.zeros(k, np.int32)
        _check(self.L.slide_chol_batch_get_landmark_pair_covariances(C.c_void_p(self.h), C.c_int(n), _p(c), _p(sa), _p(ia), _p(sb), _p(ib),
                                                                     _p(out), _p(status)))
        return out[:n, :2 * d, :2 * d].copy(), status[:n]

    def landmark_pairs_within(self, cls, radius, cross_only=False):
        """slide_chol_batch_landmark_pairs_within: every pair of the JOB's landmarks of class `cls` — each member's private ones and
        every shared slot once, through its lowest replica — whose anchors (point xyz, cube translation, cylinder root of the current
        estimates) lie within `radius`.  cross_only: drop the pairs of two private landmarks of one member.  Returns
        (slot_a, idx_a, slot_b, idx_b, dist), sorted by position in (slot, index) order."""
        total, cap = C.c_int64(0), 0
        for _ in range(2):      # (the first call counts, the second has room)
            m = max(cap, 1)
            sa, sb, ia, ib, dist = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m)
            st = self.L.slide_chol_batch_landmark_pairs_within(C.c_void_p(self.h), C.c_int(cls), C.c_double(radius), C.c_int(1 if cross_only else 0),
                                                               C.c_int64(cap), _p(sa), _p(ia), _p(sb), _p(ib), _p(dist), C.byref(total))
            if st != -3:      # SLIDE_ERR_CAPACITY: now the total is known
                _check(st)
                break
            cap = total.value
        t = total.value
        return sa[:t], ia[:t], sb[:t], ib[:t], dist[:t]

    def duplicate_landmarks(self, cls, radius, sigma, prob=0.99, cross_only=False):
        """The job's landmarks of class `cls` (CLS_ELLIPSOID or CLS_CYLINDER) that are one object mapped twice, by one robot or by two:
        landmark_pairs_within proposes the pairs within `radius` (cross_only: not those of two private landmarks of one member),
        landmark_pair_mahalanobis tests them under the model noise `sigma`, and the pairs with status 0 and
        d2 <= chi2_quantile(prob, D) are kept.  Returns (slot_a, idx_a, slot_b, idx_b, d2, dist) of the kept pairs.  The batch is
        only read; making a kept cross-robot pair a shared slot (set_shared / set_separator) is the caller's."""
        sa, ia, sb, ib, dist = self.landmark_pairs_within(cls, radius, cross_only)
        res = self.landmark_pair_mahalanobis(cls, np.stack([sa, ia.astype(np.int64), sb, ib.astype(np.int64)], axis=1), sigma)
        keep = (res["status"] == 0) & (res["d2"] <= chi2_quantile(prob, 7 if cls == CLS_CYLINDER else 3))
        return sa[keep], ia[keep], sb[keep], ib[keep], res["d2"][keep], dist[keep]

    def set_robust_loss(self, kind, param=0.0, closures=True, relative_meas=True):
        """slide_chol_batch_set_robust_loss: SlideGraph.set_robust_loss's loss (same kinds, names and defaults) on the exact joint
        pass, uniform over the member graphs: their loop closures (closures) and relative measurements, the inter-robot relative-pose
        factors included (relative_meas).  kind 0 / None clears it.  Not with PCG passes."""
        mask = (1 if closures else 0) | (2 if relative_meas else 0)
        _check(self.L.slide_chol_batch_set_robust_loss(C.c_void_p(self.h), _loss_kind(kind, "robust"), C.c_double(float(param)), C.c_int(mask)))

    def closure_weights(self, cap=None):
        """slide_chol_batch_get_closure_weights after a pass: slot by slot the member's loop-closure / relative-measurement between
        factors in insertion order (ghost_id -1), then its ghost factors (the inter-robot relative-pose factors: ghost_id = index in
        the job's list, the other end as robot -1 / idx = ghost slot).  Returns a dict of arrays: slot, from_robot, from_idx,
        to_robot, to_idx, kind, ghost_id, weight, s2, and n, the full count (cap: write at most that many rows)."""
        cols = [("slot", _I32)] + _CLOSURE_COLS + [("ghost_id", _I32)] + _WEIGHT_COLS
        return _weights(self.L.slide_chol_batch_get_closure_weights, C.c_void_p(self.h), cols, cap)

    def profile_robust_reweight(self, buf_ptrs):
        """slide_chol_batch_profile_robust_reweight: milliseconds of the loss's reweighting launch alone, between two events (closure_weights then
        wants a pass first)."""
        arr = (C.c_void_p * len(buf_ptrs))(*[int(p) for p in buf_ptrs])
        ms = C.c_double(0.0)
        _check(self.L.slide_chol_batch_profile_robust_reweight(C.c_void_p(self.h), arr, C.byref(ms)))
        return ms.value

    def set_observation_loss(self, kind, param=0.0, points=True, cubes=True, cylinders=True):
        """slide_chol_batch_set_observation_loss: SlideGraph.set_observation_loss's loss (same kinds, names and defaults) on the
        batched passes, uniform over the member graphs: their bearing-range (points), cube and cylinder factors, the observations
        of the shared landmarks included.  Fused into the passes' linearisation launch; independent of set_robust_loss.  kind 0 /
        None clears it.  Not with PCG passes."""
        mask = (1 if points else 0) | (2 if cubes else 0) | (4 if cylinders else 0)
        _check(self.L.slide_chol_batch_set_observation_loss(C.c_void_p(self.h), _loss_kind(kind, "observation"), C.c_double(float(param)),
                                                            C.c_int(mask)))

    def observation_weights(self, cap=None):
        """slide_chol_batch_get_observation_weights after a pass: slot by slot the member's landmark factors in insertion order.
        Returns a dict of arrays: slot, pose_idx, cls (SLIDE_CLS_*), lm_idx (the member's own landmark index), weight, s2 (weight and
        unscaled squared whitened norm of the factor's linearisation in the last pass; weight 1 where no loss applied) and n, the
        full count (cap: write at most that many rows).  The per-graph SlideGraph.observation_weights of a member does not know
        the batch's loss (weight 1, s2 of the scaled record): use this one."""
        cols = [("slot", _I32)] + _OBSERVATION_COLS + _WEIGHT_COLS
        return _weights(self.L.slide_chol_batch_get_observation_weights, C.c_void_p(self.h), cols, cap)

    def profile_linearize(self, buf_ptrs):
        """slide_chol_batch_profile_linearize: milliseconds of the passes' linearisation launch alone, between two events, under the
        batch's current observation loss (the read-backs and joint queries then want a pass first)."""
        arr = (C.c_void_p * len(buf_ptrs))(*[int(p) for p in buf_ptrs])
        ms = C.c_double(0.0)
        _check(self.L.slide_chol_batch_profile_linearize(C.c_void_p(self.h), arr, C.byref(ms)))
        return ms.value

    def set_pcg(self, iterations, tol=0.0):
        """PCG iterations of the joint solve after the factorisations (0 = every robot's own block solve only); tol > 0: iterations
        past a relative reduction of sqrt(r^T M^-1 r) by tol are no-ops."""
        _check(self.L.slide_chol_batch_set_pcg_tolerance(C.c_void_p(self.h), C.c_double(float(tol))))
        _check(self.L.slide_chol_batch_set_pcg(C.c_void_p(self.h), C.c_int(iterations)))

    def set_exact_joint(self, on=True, sep_ptr=0, sep_len=0):
        """Passes take the EXACT joint Gauss-Newton step (shared landmarks as the separator of the joint graph, slide_gpu.h);
        sep_ptr / sep_len: the caller's device buffer for the separator system (sep_buffer_len(m) doubles) or 0."""
        _check(self.L.slide_chol_batch_set_exact_joint(C.c_void_p(self.h), C.c_int(int(on)), C.c_void_p(int(sep_ptr) or None), C.c_longlong(int(sep_len))))

    def set_segments(self, n_seg):
        """Exact joint passes: cut every robot's pose chain into n_seg segments factored side by side (nested dissection; 1 = off)."""
        _check(self.L.slide_chol_batch_set_segments(C.c_void_p(self.h), C.c_int(int(n_seg))))

    def set_separator_profile(self, prof):
        """Tile profile of the separator system's landmark part (distributed.separator_offsets)."""
        a = np.ascontiguousarray(prof, dtype=np.int32)
        _check(self.L.slide_chol_batch_set_separator_profile(C.c_void_p(self.h), _p(a), C.c_int(len(a))))

    def set_separator_blocks(self, Ta, Tb, used_a, used_b):
        """Nested dissection of the separator system (distributed.separator_offsets: two leaf blocks + the top block); zeros: off."""
        _check(self.L.slide_chol_batch_set_separator_blocks(C.c_void_p(self.h), C.c_int(int(Ta)), C.c_int(int(Tb)), C.c_int(int(used_a)), C.c_int(int(used_b))))

    @staticmethod
    def sep_buffer_len(m, n_relmeas=0):
        L = lib()
        L.slide_chol_batch_sep_buffer_len.restype = C.c_longlong
        return int(L.slide_chol_batch_sep_buffer_len(C.c_int(int(m)), C.c_int(int(n_relmeas))))

    def set_separator_owner(self, leaf, leader=True):
        """Cut passes of a job whose ranks split in two halves along the separator's dissection: this rank factors leaf `leaf` only
        (-1: off); `leader`: the one rank of its half that adds the leaf's Schur complement to the top block's sum."""
        _check(self.L.slide_chol_batch_set_separator_owner(C.c_void_p(self.h), C.c_int(int(leaf)), C.c_int(1 if leader else 0)))

    @staticmethod
    def sep_segment(m, n_relmeas, Ta, Tb, which):
        """(offset, length) in doubles of leaf a (0), leaf b (1) or the top block + lambdas (2) inside the packed exchange buffer."""
        out = (C.c_longlong * 2)()
        _check(lib().slide_chol_batch_sep_segment(C.c_int(int(m)), C.c_int(int(n_relmeas)), C.c_int(int(Ta)), C.c_int(int(Tb)), C.c_int(int(which)), out))
        return int(out[0]), int(out[1])

    @staticmethod
    def sep_exchange_len(m, n_relmeas=0, Ta=0, Tb=0):
        L = lib()
        L.slide_chol_batch_sep_exchange_len.restype = C.c_longlong
        return int(L.slide_chol_batch_sep_exchange_len(C.c_int(int(m)), C.c_int(int(n_relmeas)), C.c_int(int(Ta)), C.c_int(int(Tb))))

    def pass_part(self, buf_ptrs, part):
        """Part 0 / 1 / 2 of the pass cut at its two exchanges (jobs that span GPUs): the caller's all-reduce of buffer 0 goes onto
        stream() between the parts; only part 2 synchronises with the host."""
        arr = (C.c_void_p * len(buf_ptrs))(*[int(p) for p in buf_ptrs])
        return _check(self.L.slide_chol_batch_pass_part(C.c_void_p(self.h), arr, C.c_int(part)))

    def stream(self):
        """hipStream_t (integer) the passes run on."""
        return int(self.L.slide_chol_batch_stream(C.c_void_p(self.h)) or 0)

    def profile(self, buf_ptrs):
        """(ms of the batched step kernels of one un-captured pass, number of step launches)."""
        arr = (C.c_void_p * len(buf_ptrs))(*[int(p) for p in buf_ptrs])
        ms, nl = C.c_double(0), C.c_int(0)
        _check(self.L.slide_chol_batch_profile(C.c_void_p(self.h), arr, C.byref(ms), C.byref(nl)))
        return ms.value, nl.value

    def profile_exact_joint(self, buf_ptrs):
        """Stage times (ms) of one un-captured exact joint pass + block columns of the separator system."""
        arr = (C.c_void_p * len(buf_ptrs))(*[int(p) for p in buf_ptrs])
        out = np.zeros(6)
        ns = C.c_int(0)
        _check(self.L.slide_chol_batch_profile_exact_joint(C.c_void_p(self.h), arr, _p(out), C.byref(ns)))
        names = ("assembly", "band_factorisations", "border_products", "separator_gather", "separator_solve", "back_substitution")
        return dict(zip(names, [float(v) for v in out])), ns.value

    def close(self):
        if self.h:
            self.L.slide_chol_batch_destroy(C.c_void_p(self.h))
            self.h = None

    def __del__(self):
        self.close()


class SlideBackend:
    """runSLOAMNode seam (reference src/core/sloamNode.cpp:762-1036) on the MI355X."""

    def __init__(self, params: Params | None = None, num_robots: int = 1):
        self.L = lib()
        self.n_robots = num_robots
        h = self.L.slide_backend_create(C.byref(params) if params is not None else None)
        if not h:
            raise SlideError(f"slide_backend_create failed: {last_error()}")
        self.h = C.c_void_p(h)
        self.graph = SlideGraph(handle=C.c_void_p(self.L.slide_backend_graph(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.slide_backend_destroy(self.h)
            self.h = None

    def process_frame(self, robot, rel7, prev7, det, mode=FRAME_HOST):
        nc, nb, ne = len(det["cyl_label"]), len(det["cube_label"]), len(det["ell_label"])
        a = [_d(det["cyl_root"]), _d(det["cyl_ray"]), _d(det["cyl_radius"]), _i(det["cyl_label"]),
             _d(det["cube_pose7"]), _d(det["cube_scale"]), _i(det["cube_label"]),
             _d(det["ell_pose7"]), _d(det["ell_scale"]), _i(det["ell_label"])]
        D = Detections(nc, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), nb, _p(a[4]), _p(a[5]), _p(a[6]), ne, _p(a[7]),
                       _p(a[8]), _p(a[9]))
        cm, bm, em = np.full(nc, -1, np.int32), np.full(nb, -1, np.int32), np.full(ne, -1, np.int32)
        cid, bid, eid = np.full(nc, -1, np.int32), np.full(nb, -1, np.int32), np.full(ne, -1, np.int32)
        R = FrameResult()
        R.cyl_match, R.cube_match, R.ell_match = _p(cm), _p(bm), _p(em)
        R.cyl_id, R.cube_id, R.ell_id = _p(cid), _p(bid), _p(eid)
        rc = self.L.slide_backend_process_frame(self.h, C.c_int(mode), C.c_int(robot), _p(_d(rel7)), _p(_d(prev7)),
                                                C.byref(D), C.byref(R))
        if rc not in (SLIDE_OK, -2):
            _check(rc)
        return dict(status=int(rc), pose7=np.array(R.out_pose7[:]), cyl_match=cm, cube_match=bm, ell_match=em,
                    cyl_id=cid, cube_id=bid, ell_id=eid, t_assoc=R.ms_association * 1e-3, t_graph=R.ms_graph * 1e-3)

    def set_association_gate(self, prob, on_reject="drop"):
        """slide_backend_set_association_gate: with 0 < prob < 1, process_frame tests every match of a host frame at the predicted
        pose (SlideGraph.predicted_observation_mahalanobis) before it is added and rejects those with d2 above chi2_quantile(prob,
        dof): on_reject "drop" leaves the detection out (its *_match MATCH_GATED, its *_id -1), "new" makes it a new landmark (its
        *_match MATCH_GATED).  prob 0 (the default state) turns the gate off."""
        if on_reject not in ("drop", "new"):
            raise SlideError(f"set_association_gate: on_reject is {on_reject!r}, not 'drop' or 'new'")
        _check(self.L.slide_backend_set_association_gate(self.h, C.c_double(prob), C.c_int(GATE_NEW if on_reject == "new" else GATE_DROP)))

    def gate_stats(self):
        """slide_backend_gate_stats: dict(frames_gated, frames_skipped, tested, rejected)."""
        out = np.zeros(4, np.int64)
        _check(self.L.slide_backend_gate_stats(self.h, _p(out)))
        return dict(frames_gated=int(out[0]), frames_skipped=int(out[1]), tested=int(out[2]), rejected=int(out[3]))

    def ingest_solve(self):
        return self.L.slide_backend_ingest_solve(self.h)

    def end_frame(self, robot):
        out = np.zeros(7)
        st = self.L.slide_backend_end_frame(self.h, C.c_int(robot), _p(out))
        return int(st), out

    def counts(self):
        out = np.zeros(4, np.uint64)
        pc = np.zeros(13, np.uint64)
        _check(self.L.slide_backend_counts(self.h, _p(out), _p(pc), C.c_int(13)))
        return dict(cyl=int(out[0]), cube=int(out[1]), point=int(out[2]), factors=int(out[3]),
                    poses=pc[: self.n_robots].astype(np.int64))

    def landmark_table(self, cls):
        n = self.counts()[("cyl", "cube", "point")[cls]]
        xyz = np.zeros((max(n, 1), 3))
        lab = np.zeros(max(n, 1), np.int32)
        k = self.L.slide_backend_landmark_table(self.h, C.c_int(cls), _p(xyz), _p(lab), C.c_int(n))
        if k < 0:
            _check(k)
        return xyz[:k], lab[:k]

    def map_model(self, cls, idx):
        out = np.zeros(7)
        hits, label = C.c_int(0), C.c_int(0)
        st = _check(self.L.slide_backend_map_model(self.h, C.c_int(cls), C.c_int(idx), _p(out), C.byref(hits), C.byref(label)),
                    True)
        return int(st), out[: 7 if cls == 0 else 6], hits.value, label.value


def pair_timeouts():
    """Flag waits of the pair kernel (two block columns per launch) that gave up since the library was loaded; 0 on a healthy run."""
    f = lib().slide_debug_pair_timeouts
    f.restype = C.c_int
    return int(f())


def dense_spd_solve(A, b, repeats=1, method=0):
    """x = A^-1 b on the GPU (blocked FP64-MFMA Cholesky); returns (x, device ms over `repeats` passes).  method 0: one step launch
    per 64-column block; 1: the left-looking persistent factorisation (one launch, flags between workgroups); 2: two block columns
    per launch (k_chol_pair_batched)."""
    A = np.asfortranarray(np.asarray(A, dtype=np.float64))
    n = A.shape[0]
    x = np.zeros(n)
    ms = C.c_double(0)
    _check(lib().slide_dense_spd_solve_ex(A.ctypes.data_as(C.c_void_p), C.c_int(n), _p(_d(b)), _p(x), C.c_int(repeats),
                                          C.byref(ms), C.c_int(method)))
    return x, ms.value


def debug_chol_bordered(S, ld, T, nbr, prof=None, bfirst=None, ord=None, b0=0, kofs=0, n_copies=1, method=0):
    """slide_debug_chol_bordered: factor one bordered system with a profile (S: flat column-major ld x T*64) n_copies times side by side.
    Returns dict(S, Ld, Winv, status, copy_diff)."""
    S = np.ascontiguousarray(S, dtype=np.float64).ravel()
    assert S.size == ld * T * 64
    So = np.zeros_like(S)
    Ld = np.zeros(T * 64 * 64)
    Wi = np.zeros(T * 1024)
    st = np.zeros(8, np.int32)
    diff = C.c_double(0)
    ia = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    pr, bf, od = ia(prof), ia(bfirst), ia(ord)
    pp = lambda a: None if a is None else _p(a)
    _check(lib().slide_debug_chol_bordered(_p(S), C.c_int(ld), C.c_int(T), C.c_int(nbr), pp(pr), pp(bf), pp(od), C.c_int(b0), C.c_int(kofs),
                                           C.c_int(n_copies), C.c_int(method), _p(So), _p(Ld), _p(Wi), _p(st), C.byref(diff)))
    return dict(S=So, Ld=Ld, Winv=Wi, status=st, copy_diff=diff.value)


def _chol_batch_tables(systems):
    """The descriptors of debug_chol_batch / debug_chol_plan as the C calls' flat arrays.  systems: dicts with T, nbr and optionally
    ld, prof, bfirst, ord, b0, kofs (as debug_chol_bordered takes them)."""
    n = len(systems)
    k = max(n, 1)
    col = lambda key: np.array([int(s.get(key) or 0) for s in systems] + [0] * (k - n), np.int32)
    flat, off = {}, {}
    for key in ("prof", "bfirst", "ord"):
        vals, o = [], np.full(k, -1, np.int32)
        for i, s in enumerate(systems):
            if s.get(key) is not None:
                o[i] = len(vals)
                vals += [int(x) for x in s[key]]
                assert len(vals) - o[i] == (s["T"] if key == "prof" else s["nbr"]), key
        flat[key], off[key] = np.array(vals + [0], np.int32), o
    return n, col("ld"), col("T"), col("nbr"), col("b0"), col("kofs"), flat, off


def debug_chol_plan(systems, method=0, cu_share=100, assumed_cus=256):
    """slide_debug_chol_plan: the launches debug_chol_batch would issue for these systems on a device with assumed_cus compute units, by
    the planning code of the real launches; no device needed.  Returns an (launches, 5) int array: k, a_split, a_joins, nAw, nB."""
    n, _, T, nbr, b0, kofs, flat, off = _chol_batch_tables(systems)
    cap = 2 * int(T.max()) + 2
    trace = np.zeros((cap, 5), np.int32)
    rc = lib().slide_debug_chol_plan(C.c_int(n), _p(T), _p(nbr), _p(flat["prof"]), _p(off["prof"]), _p(flat["bfirst"]), _p(off["bfirst"]),
                                     _p(b0), _p(kofs), C.c_int(method), C.c_int(cu_share), C.c_int(assumed_cus), _p(trace), C.c_int(cap))
    if rc < 0:
        _check(rc)
    assert rc <= cap
    return trace[:rc].copy()


def debug_chol_batch(systems, method=0, cu_share=100, assumed_cus=0, want_l32=False):
    """slide_debug_chol_batch: factor n DIFFERENT bordered systems (dicts with S, ld, T, nbr and optionally prof, bfirst, ord, b0, kofs) in
    one launch sequence, planned for assumed_cus compute units (0: the device's own).  Returns dict(systems=[dict(S, Ld, Winv, status,
    L32 or None)], trace=(launches, 5) int array of k, a_split, a_joins, nAw, nB, n_cu)."""
    n, ld, T, nbr, b0, kofs, flat, off = _chol_batch_tables(systems)
    S = np.concatenate([np.ascontiguousarray(s["S"], dtype=np.float64).ravel() for s in systems]) if n else np.zeros(1)
    sizes = [int(s["ld"]) * int(s["T"]) * 64 for s in systems]
    assert all(np.size(s["S"]) == z for s, z in zip(systems, sizes))
    l32_sizes = [t * (t - 1) // 2 * 4096 + 4 if (want_l32 and not b) else 0 for t, b in zip(T[:n].tolist(), b0[:n].tolist())]
    Tt = int(T[:n].sum())
    So, Ld, Wi, st = np.zeros_like(S), np.zeros(max(Tt, 1) * 4096), np.zeros(max(Tt, 1) * 1024), np.zeros(8 * max(n, 1), np.int32)
    L32 = np.zeros(max(sum(l32_sizes), 1), np.float32)
    cap = 2 * int(T.max()) + 2
    trace = np.zeros((cap, 5), np.int32)
    nl, ncu = C.c_int(0), C.c_int(0)
    rc = lib().slide_debug_chol_batch(C.c_int(n), _p(S), _p(ld), _p(T), _p(nbr), _p(flat["prof"]), _p(off["prof"]), _p(flat["bfirst"]),
                                      _p(off["bfirst"]), _p(flat["ord"]), _p(off["ord"]), _p(b0), _p(kofs), C.c_int(method),
                                      C.c_int(cu_share), C.c_int(assumed_cus), C.c_int(1 if want_l32 else 0), _p(So), _p(Ld), _p(Wi),
                                      _p(st), _p(L32), _p(trace), C.c_int(cap), C.byref(nl), C.byref(ncu))
    if rc != SLIDE_OK:
        err = SlideError(f"{ERR.get(rc, rc)}: {last_error()}")
        err.code, err.n_launches = rc, nl.value
        raise err
    assert nl.value <= cap
    out, so, to, lo = [], 0, 0, 0
    for i in range(n):
        t = int(T[i])
        out.append(dict(S=So[so:so + sizes[i]], Ld=Ld[to * 4096:(to + t) * 4096], Winv=Wi[to * 1024:(to + t) * 1024], status=st[8 * i:8 * i + 8],
                        L32=L32[lo:lo + l32_sizes[i]] if l32_sizes[i] else None))
        so, to, lo = so + sizes[i], to + t, lo + l32_sizes[i]
    return dict(systems=out, trace=trace[:nl.value].copy(), n_cu=ncu.value)


def _border_tables(systems, key, count):
    """One optional int table per system, end to end, with the offsets (-1: none) and lengths the C calls take."""
    vals, off, ln = [], np.full(max(len(systems), 1), -1, np.int32), np.zeros(max(len(systems), 1), np.int32)
    for i, s in enumerate(systems):
        if s.get(key) is not None:
            t = [int(x) for x in s[key]]
            assert count is None or len(t) == count(s), key
            off[i], ln[i] = len(vals), len(t)
            vals += t
    # (values above 2^31 are the high mask words: the same bits as int32)
    return np.array(vals + [0], np.int64).astype(np.uint32).view(np.int32), off, ln


def debug_border_product(systems, jobs=None, lds_pad=0, ks=1, ks_sys=None, jb_end=-1, fuse_add=False, prefill=None):
    """slide_debug_border_product: the border product of n systems after their steps (dicts with S, ld, T, nbr, bord, ldb and optionally
    b0, bord_cols (columns of the bord buffer, default nbr * 64), bfirst (nbr + 1 ints), segtab (HostGraph::seg_tab's flat layout),
    bord_src) through launch_border_syrk (jobs None) or launch_border_syrk_jobs (jobs: codes system << 20 | ib << 10 | jb).  prefill: the
    value the split-K scratch holds in place of zero.  Returns [dict(bord, S)], flat as given.  Raises SlideError (code -1) for a
    combination the launchers do not define."""
    n = len(systems)
    col = lambda key, dflt=None: np.array([int(s[key] if s.get(key) is not None else dflt(s)) for s in systems] or [0], np.int32)
    ld, T, nbr, b0, ldb = col("ld"), col("T"), col("nbr"), col("b0", lambda s: 0), col("ldb")
    cols = col("bord_cols", lambda s: s["nbr"] * 64)
    S = np.concatenate([np.ascontiguousarray(s["S"], dtype=np.float64).ravel() for s in systems])
    bord = np.concatenate([np.ascontiguousarray(s["bord"], dtype=np.float64).ravel() for s in systems])
    s_sz = [int(ld[i]) * int(T[i]) * 64 for i in range(n)]
    b_sz = [int(ldb[i]) * int(cols[i]) for i in range(n)]
    assert all(np.size(s["S"]) == z for s, z in zip(systems, s_sz)) and all(np.size(s["bord"]) == z for s, z in zip(systems, b_sz))
    bf, bf_off, _ = _border_tables(systems, "bfirst", lambda s: s["nbr"] + 1)
    sg, sg_off, sg_len = _border_tables(systems, "segtab", None)
    has_src = np.array([1 if s.get("bord_src") is not None else 0 for s in systems], np.int32)
    src = None
    if has_src.any():
        src = np.concatenate([np.ascontiguousarray(s["bord_src"] if s.get("bord_src") is not None else np.zeros(z), dtype=np.float64).ravel()
                              for s, z in zip(systems, b_sz)])
        assert src.size == bord.size
    jb = None if jobs is None else np.ascontiguousarray(jobs, dtype=np.int32)
    kk = None if ks_sys is None else np.ascontiguousarray(ks_sys, dtype=np.int32)
    assert kk is None or kk.size == 2
    pp = lambda a: None if a is None else _p(a)
    bo, So = np.zeros_like(bord), np.zeros_like(S)
    rc = lib().slide_debug_border_product(C.c_int(n), _p(S), _p(ld), _p(T), _p(nbr), _p(b0), _p(bord), _p(ldb), _p(cols), _p(bf), _p(bf_off),
                                          _p(sg), _p(sg_off), _p(sg_len), pp(src), _p(has_src), pp(jb), C.c_int(0 if jb is None else jb.size),
                                          C.c_int(lds_pad), C.c_int(ks), pp(kk), C.c_int(jb_end), C.c_int(1 if fuse_add else 0),
                                          C.c_int(0 if prefill is None else 1), C.c_double(0.0 if prefill is None else prefill), _p(bo), _p(So))
    if rc != SLIDE_OK:
        err = SlideError(f"{ERR.get(rc, rc)}: {last_error()}")
        err.code = rc
        raise err
    out, so, bo_ = [], 0, 0
    for i in range(n):
        out.append(dict(bord=bo[bo_:bo_ + b_sz[i]], S=So[so:so + s_sz[i]]))
        so, bo_ = so + s_sz[i], bo_ + b_sz[i]
    return out


def debug_border_apply(systems):
    """slide_debug_border_apply: yv -= W x_loc of n systems (dicts with S, ld, T, nbr, yv (T * 64), x_loc (nbr * 64) and optionally b0,
    segtab) in one launch_border_apply.  Returns the systems' yv."""
    n = len(systems)
    col = lambda key: np.array([int(s.get(key) or 0) for s in systems] or [0], np.int32)
    ld, T, nbr, b0 = col("ld"), col("T"), col("nbr"), col("b0")
    cat = lambda key: np.concatenate([np.ascontiguousarray(s[key], dtype=np.float64).ravel() for s in systems])
    S, yv, x = cat("S"), cat("yv"), cat("x_loc")
    assert S.size == int((ld.astype(np.int64) * T * 64)[:n].sum()) and yv.size == int(T[:n].sum()) * 64 and x.size == int(nbr[:n].sum()) * 64
    sg, sg_off, sg_len = _border_tables(systems, "segtab", None)
    out = np.zeros_like(yv)
    rc = lib().slide_debug_border_apply(C.c_int(n), _p(S), _p(ld), _p(T), _p(nbr), _p(b0), _p(yv), _p(x), _p(sg), _p(sg_off), _p(sg_len), _p(out))
    if rc != SLIDE_OK:
        err = SlideError(f"{ERR.get(rc, rc)}: {last_error()}")
        err.code = rc
        raise err
    offs = np.concatenate([[0], np.cumsum(T[:n].astype(np.int64) * 64)])
    return [out[offs[i]:offs[i + 1]] for i in range(n)]


def _debug_rc(rc):
    if rc != SLIDE_OK:
        err = SlideError(f"{ERR.get(rc, rc)}: {last_error()}")
        err.code = rc
        raise err


def _debug_factor(f):
    """S, ld, T, Ld, Winv, prof pointer (and the array it points into) of a caller-given factor (dict with S, ld, T, Ld, Winv, prof)."""
    ld, T = int(f["ld"]), int(f["T"])
    S, Ld, Wi = _d(f["S"]).ravel(), _d(f["Ld"]).ravel(), _d(f["Winv"]).ravel()
    assert S.size == max(ld * T * 64, 0) and Ld.size == max(T, 0) * 4096 and Wi.size == max(T, 0) * 1024
    pr = None if f.get("prof") is None else _i(f["prof"])
    assert pr is None or pr.size == T
    return S, ld, T, Ld, Wi, (None if pr is None else _p(pr))


def debug_selected_inverse(f, Sg, Z, stage=1):
    """slide_debug_selected_inverse: launch_selected_inverse (stage 1) or k_sinv_prep alone (stage 0) on the caller-given factor f (dict
    with S, ld, T, Ld, Winv, prof or None) with Sg / Z (ld * T * 64 each) as the pre-filled output buffers.  Returns dict(Sg, Z, S, Ld,
    Winv), the last three as the device held them afterwards.  Raises SlideError (code -1) for what the launcher does not define."""
    S, ld, T, Ld, Wi, pr = _debug_factor(f)
    Sg, Z = _d(Sg).ravel().copy(), _d(Z).ravel().copy()
    assert Sg.size == S.size and Z.size == S.size
    So, Lo, Wo = np.zeros_like(S), np.zeros_like(Ld), np.zeros_like(Wi)
    _debug_rc(lib().slide_debug_selected_inverse(_p(S), C.c_int(ld), C.c_int(T), _p(Ld), _p(Wi), pr, C.c_int(stage), _p(Sg), _p(Z), _p(So),
                                                 _p(Lo), _p(Wo)))
    return dict(Sg=Sg, Z=Z, S=So, Ld=Lo, Winv=Wo)


def debug_multi_solve(f, B, X, nrhs, mode=0, k0=0):
    """slide_debug_multi_solve: launch_multi_solve (mode 0) or launch_multi_fwd from block column k0 (mode 1) on the factor f; B and X:
    (ncol_alloc, T * 64) arrays (a row = one column of the device's buffer).  Returns (B, X) afterwards, same shape."""
    S, ld, T, Ld, Wi, pr = _debug_factor(f)
    B, X = _d(B).copy(), _d(X).copy()
    assert B.ndim == 2 and B.shape == X.shape and B.shape[1] == max(T, 0) * 64
    _debug_rc(lib().slide_debug_multi_solve(_p(S), C.c_int(ld), C.c_int(T), _p(Ld), _p(Wi), pr, _p(B), _p(X), C.c_int(B.shape[0]),
                                            C.c_int(nrhs), C.c_int(mode), C.c_int(k0)))
    return B, X


def debug_gram(X, rows, nrows, M):
    """slide_debug_gram: launch_gram on X ((ncol, ldx): a row = one column of the device's buffer) over `rows` (or None: 0 .. nrows - 1)
    into M ((ncol + 1, ncol), pre-filled; the last row is the guard).  Returns M afterwards."""
    X, M = _d(X), _d(M).copy()
    ncol, ldx = X.shape
    assert M.shape == (ncol + 1, ncol)
    rw = None if rows is None else _i(rows)
    assert rw is None or rw.size == nrows
    _debug_rc(lib().slide_debug_gram(_p(X), C.c_longlong(ldx), C.c_int(ncol), None if rw is None else _p(rw), C.c_int(nrows), _p(M)))
    return M


def debug_pose_covariance(f, row0):
    """slide_debug_pose_covariance: launch_pose_covariance for the six rows from row0 on the factor f.  Returns (cov (6, 6), Y (6, T * 64))."""
    S, ld, T, Ld, Wi, _ = _debug_factor(f)
    cov, Y = np.zeros(36), np.zeros((6, max(T, 1) * 64))
    _debug_rc(lib().slide_debug_pose_covariance(_p(S), C.c_int(ld), C.c_int(T), _p(Ld), _p(Wi), C.c_int(row0), _p(cov), _p(Y)))
    return cov.reshape(6, 6), Y


def debug_joint_selected_inverse(systems, rp, rows, jobs, step_off, stage=1):
    """slide_debug_joint_selected_inverse: systems = dicts with S (ld x Tb * 64), ld, Tb, B (ldb x (Tc - Tb) * 64), ldb, Tc, Ld, Winv (all
    Tc columns), neg0, col0, lds, Trow and the pre-filled Sg, Z (lds x Trow * 64 each); rp / rows the flat row lists; jobs a list of
    (system, column); step_off the steps' first jobs and the end.  Returns [dict(Sg, Z)], flat as given."""
    n = len(systems)
    col = lambda key: np.array([int(s[key]) for s in systems] or [0], np.int32)
    cat = lambda key: np.concatenate([_d(s[key]).ravel() for s in systems] + [np.zeros(1)])
    ld, Tb, ldb, Tc, neg0, col0, lds, Trow = (col(k) for k in ("ld", "Tb", "ldb", "Tc", "neg0", "col0", "lds", "Trow"))
    S, B, Ld, Wi, Sg, Z = (cat(k) for k in ("S", "B", "Ld", "Winv", "Sg", "Z"))
    g_sz = [int(s["lds"]) * int(s["Trow"]) * 64 for s in systems]
    for s, z in zip(systems, g_sz):
        assert np.size(s["S"]) == s["ld"] * s["Tb"] * 64 and np.size(s["B"]) == s["ldb"] * (s["Tc"] - s["Tb"]) * 64
        assert np.size(s["Ld"]) == s["Tc"] * 4096 and np.size(s["Winv"]) == s["Tc"] * 1024 and np.size(s["Sg"]) == z and np.size(s["Z"]) == z
    rp_, rows_ = _i(rp), _i(list(rows) + [0])
    jb, so = _i(np.asarray(jobs, np.int32).reshape(-1, 2)), _i(step_off)
    _debug_rc(lib().slide_debug_joint_selected_inverse(C.c_int(n), _p(S), _p(ld), _p(Tb), _p(B), _p(ldb), _p(Tc), _p(Ld), _p(Wi), _p(neg0),
                                                       _p(col0), _p(lds), _p(Trow), _p(rp_), C.c_int(rp_.size), _p(rows_), C.c_int(len(rows)),
                                                       _p(jb), C.c_int(jb.shape[0]), _p(so), C.c_int(so.size - 1), C.c_int(stage), _p(Sg), _p(Z)))
    out, o = [], 0
    for z in g_sz:
        out.append(dict(Sg=Sg[o:o + z], Z=Z[o:o + z]))
        o += z
    return out


# ---- stand-alone association / place recognition ---------------------------------------------------------
def pairs_within(xyz, radius, labels=None):
    """slide_pairs_within: every pair i < j of the points xyz (n, 3) at most `radius` apart (and of one label, where labels are
    given), found on the device; sorted by (i, j).  Returns (i, j, dist)."""
    pts = _d(xyz).reshape(-1, 3)
    lab = None if labels is None else _i(labels).reshape(-1)
    if lab is not None and len(lab) != len(pts):
        raise SlideError("pairs_within: one label per point")
    total, cap = C.c_int64(0), 0
    for _ in range(2):      # (the first call counts, the second has room)
        oi, oj, dist = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1))
        st = lib().slide_pairs_within(_p(pts), _p(lab) if lab is not None else None, C.c_int(len(pts)), C.c_double(radius), C.c_int64(cap),
                                      _p(oi), _p(oj), _p(dist), C.byref(total))
        if st != -3:      # SLIDE_ERR_CAPACITY: now the total is known
            _check(st)
            break
        cap = total.value
    return oi[:total.value], oj[:total.value], dist[:total.value]


def submap_knn(cloud_xyz_f32, query_xyz, K):
    cloud = np.ascontiguousarray(cloud_xyz_f32, dtype=np.float32)
    n = cloud.shape[0]
    out = np.zeros(max(min(K, n), 1), np.int32)
    k = C.c_int(0)
    _check(lib().slide_submap_knn(_p(cloud), C.c_uint64(n), _p(_d(query_xyz)), C.c_int(K), _p(out), C.byref(k)))
    return out[: k.value]


def match_cylinders(root, ray, label, map_root, map_ray, map_label, thresh):
    n, m = len(label), len(map_label)
    out = np.full(max(n, 1), -1, np.int32)
    _check(lib().slide_assoc_match_cylinders(C.c_int(n), _p(_d(root)), _p(_d(ray)), _p(_i(label)), C.c_int(m), _p(_d(map_root)),
                                             _p(_d(map_ray)), _p(_i(map_label)), C.c_double(thresh), _p(out)))
    return out[:n]


def match_boxes(cls, xyz, label, map_xyz, map_label, thresh):
    n, m = len(label), len(map_label)
    out = np.full(max(n, 1), -1, np.int32)
    _check(lib().slide_assoc_match_boxes(C.c_int(cls), C.c_int(n), _p(_d(xyz)), _p(_i(label)), C.c_int(m), _p(_d(map_xyz)),
                                         _p(_i(map_label)), C.c_double(thresh), _p(out)))
    return out[:n]


def assoc_sweep_batch(cloud_xyz_f32, model_xyz, label, query_pos, obs_xyz, obs_label, K, thresh, repeats=1):
    """Batched association sweep (getSubmap K-NN gate + matchEllipsoidModels) of n_query frames against one resident map.
    obs_xyz: (n_query, n_obs, 3), obs_label: (n_query, n_obs).  Returns (map index or -1 per observation, device ms of `repeats`
    launches on resident inputs)."""
    cloud = np.ascontiguousarray(cloud_xyz_f32, dtype=np.float32).reshape(-1, 3)
    model = _d(model_xyz).reshape(-1, 3)
    lab = _i(label)
    qp = _d(query_pos).reshape(-1, 3)
    ox = _d(obs_xyz)
    ol = _i(obs_label)
    nq = qp.shape[0]
    n_obs = ol.shape[1] if ol.ndim == 2 else 0
    out = np.full((nq, max(n_obs, 1)), -1, np.int32)
    ms = C.c_double(0)
    _check(lib().slide_assoc_sweep_batch(_p(cloud), _p(model), _p(lab), C.c_int(len(lab)), _p(qp), _p(ox), _p(ol), C.c_int(nq),
                                         C.c_int(n_obs), C.c_int(K), C.c_double(thresh), _p(out), C.c_int(repeats), C.byref(ms)))
    return out[:, :n_obs], ms.value


def place_default_params(**kw) -> PlaceParams:
    p = PlaceParams()
    lib().slide_place_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def match_maps(ref7, qry7, params: PlaceParams):
    ref7, qry7 = _d(ref7), _d(qry7)
    nr, nq = ref7.shape[0], qry7.shape[0]
    best = np.zeros(3)
    pr, pq = np.full(max(nq, 1), -1, np.int32), np.full(max(nq, 1), -1, np.int32)
    nc = C.c_int64(0)
    inl = lib().slide_match_maps(_p(ref7), C.c_int(nr), _p(qry7), C.c_int(nq), C.byref(params), _p(best), _p(pr), _p(pq),
                                 C.byref(nc))
    if inl < 0 and inl != -10000:
        _check(inl)
    k = max(inl, 0)
    return dict(inliers=int(inl), xyyaw=best, ref_idx=pr[:k], qry_idx=pq[:k], candidates=int(nc.value))


def match_maps_sweep(ref7, qry7, params: PlaceParams, capacity=None):
    """slide_match_maps_sweep: the whole sweep of match_maps read back.  Returns dict(status, candidates, xyyaw (n, 3), inliers (n,),
    best_index); status SLIDE_ERR_CAPACITY (candidates still filled) when the lattice exceeds `capacity` or the maps the on-chip image.
    capacity=None: sized by a first call that launches nothing."""
    ref7, qry7 = _d(ref7), _d(qry7)
    nr, nq = ref7.shape[0], qry7.shape[0]
    nc, bi = C.c_int64(0), C.c_int64(-1)

    def call(cap):
        xy, inl = np.zeros((max(cap, 1), 3)), np.zeros(max(cap, 1), np.int32)
        rc = lib().slide_match_maps_sweep(_p(ref7), C.c_int(nr), _p(qry7), C.c_int(nq), C.byref(params), _p(xy), _p(inl),
                                          C.c_int64(cap), C.byref(nc), C.byref(bi))
        return rc, xy, inl
    if capacity is None:
        rc, xy, inl = call(0)
        if rc == SLIDE_ERR_CAPACITY and nc.value > 0:
            rc, xy, inl = call(nc.value)
    else:
        rc, xy, inl = call(int(capacity))
    if rc not in (SLIDE_OK, SLIDE_ERR_CAPACITY):
        _check(rc)
    n = nc.value if rc == SLIDE_OK else 0
    return dict(status=int(rc), candidates=int(nc.value), xyyaw=xy[:n], inliers=inl[:n], best_index=int(bi.value))


def find_inter_loop_closure(ref7, qry7, params: PlaceParams):
    ref7, qry7 = _d(ref7), _d(qry7)
    tf = np.zeros(16)
    inl = C.c_int(0)
    xyzyaw = np.zeros(4)
    rc = lib().slide_find_inter_loop_closure(_p(ref7), C.c_int(ref7.shape[0]), _p(qry7), C.c_int(qry7.shape[0]),
                                             C.byref(params), _p(tf), C.byref(inl), _p(xyzyaw))
    if rc < 0:
        _check(rc)
    return dict(found=bool(rc), tf=tf.reshape(4, 4), inliers=inl.value, xyzyaw=xyzyaw)


def find_inter_loop_closures(maps, pairs, params: PlaceParams):
    """The SlideMatch branch of SLOAMNode::interLoopClosureThread_ (sloamNode.cpp:600-694) in one call: maps = list of (n_i, 7) object
    maps, pairs = list of (reference map, query map) indices.  Every pair is evaluated by itself and gets exactly
    find_inter_loop_closure's result for that pair alone (tf = identity when it is not found).  Returns one dict per pair with the
    single call's keys plus `status` (0 or the pair's own SLIDE_ERR_CAPACITY), `best_index` (the winning candidate in lattice order, -1
    for none) and `candidates` (the pair's lattice size)."""
    ms = [_d(m).reshape(-1, 7) for m in maps]
    off = np.zeros(len(ms) + 1, np.int32)
    off[1:] = np.cumsum([len(m) for m in ms])
    flat = np.ascontiguousarray(np.concatenate(ms, axis=0)) if ms else np.zeros((0, 7))
    if len(flat) == 0:
        flat = np.zeros((1, 7))
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    n = len(pr)
    tf = np.zeros((max(n, 1), 16))
    xyzyaw = np.zeros((max(n, 1), 4))
    inl, found, status = (np.zeros(max(n, 1), np.int32) for _ in range(3))
    best, cand = np.full(max(n, 1), -1, np.int64), np.zeros(max(n, 1), np.int64)
    _check(lib().slide_find_inter_loop_closures(_p(flat), _p(off), C.c_int(len(ms)), _p(pr if n else np.zeros((1, 2), np.int32)), C.c_int(n),
                                                C.byref(params), _p(tf), _p(inl), _p(xyzyaw), _p(found), _p(best), _p(cand), _p(status)))
    return [dict(found=bool(found[k]), tf=tf[k].reshape(4, 4).copy(), inliers=int(inl[k]), xyzyaw=xyzyaw[k].copy(), status=int(status[k]),
                 best_index=int(best[k]), candidates=int(cand[k])) for k in range(n)]


def find_intra_loop_closure(meas7, submap7, query_pose7, candidate_pose7, params: PlaceParams, x_half=5.0, y_half=5.0,
                            yaw_half=10.0 * np.pi / 180.0):
    """PlaceRecognition::findIntraLoopClosure (place_recognition.cpp:389-496); intra half ranges default as :53-63."""
    m, sm = _d(meas7).reshape(-1, 7), _d(submap7).reshape(-1, 7)
    tf = np.zeros(16)
    inl = C.c_int(0)
    xyzyaw = np.zeros(4)
    rc = lib().slide_find_intra_loop_closure(_p(m), C.c_int(len(m)), _p(sm), C.c_int(len(sm)), _p(_d(query_pose7)),
                                             _p(_d(candidate_pose7)), C.byref(params), C.c_double(x_half), C.c_double(y_half),
                                             C.c_double(yaw_half), _p(tf), C.byref(inl), _p(xyzyaw))
    if rc < 0:
        _check(rc)
    return dict(found=bool(rc), tf=tf.reshape(4, 4), inliers=inl.value, xyzyaw=xyzyaw)


def loop_candidate_idx(cloud_xyz, max_dist, pose_idx, at_least_num_of_poses_old):
    """CylinderMapManager::getLoopCandidateIdx (cylinderMapManager.cpp:160-184).  Returns the candidate index or None."""
    cloud = np.ascontiguousarray(cloud_xyz, dtype=np.float32).reshape(-1, 3)
    cand, found = C.c_uint64(0), C.c_int(0)
    _check(lib().slide_loop_candidate_idx(_p(cloud), C.c_int(len(cloud)), C.c_double(max_dist), C.c_uint64(pose_idx),
                                          C.c_uint64(at_least_num_of_poses_old), C.byref(cand), C.byref(found)))
    return int(cand.value) if found.value else None


def loop_candidate_list(cloud_xyz, max_dist, pose_idx, at_least_num_of_poses_old, cap=None):
    """slide_loop_candidate_list: EVERY key pose that passes getLoopCandidateIdx's test, in loop_candidate_idx's order (entry 0 is its
    result).  Returns (indices as an int64 array of at most `cap` entries — all of them when cap is None —, the full count)."""
    cloud = np.ascontiguousarray(cloud_xyz, dtype=np.float32).reshape(-1, 3)
    size = len(cloud) if cap is None else int(cap)
    out, n = np.zeros(max(size, 1), np.uint64), C.c_int(0)
    _check(lib().slide_loop_candidate_list(_p(cloud), C.c_int(len(cloud)), C.c_double(max_dist), C.c_uint64(pose_idx),
                                           C.c_uint64(at_least_num_of_poses_old), _p(out), C.c_int(size), C.byref(n)))
    return out[:min(n.value, size)].astype(np.int64), int(n.value)


def _map_tables(cylinders, cubes, ellipsoids):
    """The three map tables as the C arguments of slide_keypose_submaps.  cylinders: (root (n, 3), ray (n, 3), radius (n,), label (n,)),
    cubes / ellipsoids: (centre (n, 3), scale (n, 3), label (n,)); None: an empty class."""
    keep, args = [], []
    for cls, widths in ((cylinders, (3, 3, 1)), (cubes, (3, 3)), (ellipsoids, (3, 3))):
        if cls is None:
            cls = [np.zeros((0, w)) for w in widths] + [np.zeros(0, np.int32)]
        arrs = [_d(a).reshape(-1, w) if w > 1 else _d(a).reshape(-1) for a, w in zip(cls[:-1], widths)] + [_i(cls[-1]).reshape(-1)]
        n = len(arrs[-1])
        assert all(len(a) == n for a in arrs), "a map table's columns differ in length"
        keep += arrs
        args += [_p(a) if n else None for a in arrs] + [C.c_int(n)]
    return keep, args


def keypose_submaps(cylinders, cubes, ellipsoids, pose_xyz, submap_radius, max_dz=1.5, capacity=None, with_src=True):
    """slide_keypose_submaps: getkeyPoseSubmap of the three map managers + prepareLCInput around a list of key-pose positions, on the
    device.  Returns dict(status, n_rows, sub_off (n_poses + 1), rows (n_rows, 7), src_idx (n_rows,)); status SLIDE_ERR_CAPACITY
    (n_rows and sub_off still filled, no rows) when `capacity` is too small.  capacity=None: sized by a first call that writes
    nothing.  max_dz: the reference hard-codes 1.5."""
    keep, targs = _map_tables(cylinders, cubes, ellipsoids)
    pos = _d(pose_xyz).reshape(-1, 3)
    n = len(pos)
    off, nr = np.zeros(n + 1, np.int32), C.c_int64(0)

    def call(cap):
        rows, src = np.zeros((max(cap, 1), 7)), np.full(max(cap, 1), -1, np.int32)
        rc = lib().slide_keypose_submaps(*targs, _p(pos) if n else None, C.c_int(n), C.c_double(submap_radius), C.c_double(max_dz), _p(off),
                                         _p(rows), _p(src) if with_src else None, C.c_int64(cap), C.byref(nr))
        return rc, rows, src
    if capacity is None:
        rc, rows, src = call(0)
        if rc == SLIDE_ERR_CAPACITY and nr.value > 0:
            rc, rows, src = call(nr.value)
    else:
        rc, rows, src = call(int(capacity))
    if rc not in (SLIDE_OK, SLIDE_ERR_CAPACITY):
        _check(rc)
    k = nr.value if rc == SLIDE_OK else 0
    return dict(status=int(rc), n_rows=int(nr.value), sub_off=off, rows=rows[:k], src_idx=src[:k] if with_src else None)


def _intra_outputs(n):
    tf, xyzyaw = np.zeros((max(n, 1), 16)), np.zeros((max(n, 1), 4))
    inl, found, status = (np.zeros(max(n, 1), np.int32) for _ in range(3))
    best, cand = np.full(max(n, 1), -1, np.int64), np.zeros(max(n, 1), np.int64)
    return tf, inl, xyzyaw, found, best, cand, status


def _intra_dicts(n, tf, inl, xyzyaw, found, best, cand, status):
    return [dict(found=bool(found[k]), tf=tf[k].reshape(4, 4).copy(), inliers=int(inl[k]), xyzyaw=xyzyaw[k].copy(), status=int(status[k]),
                 best_index=int(best[k]), candidates=int(cand[k])) for k in range(n)]


def find_intra_loop_closures(meas7, query_pose7, submaps, candidate_poses7, params: PlaceParams, x_half=5.0, y_half=5.0,
                             yaw_half=10.0 * np.pi / 180.0):
    """slide_find_intra_loop_closures: one set of detections (local frame of the query pose) against a LIST of candidate key poses in
    one call; submaps = list of (n_k, 7) submaps, candidate_poses7 = (n, 7).  Every candidate gets exactly find_intra_loop_closure's
    result for that candidate alone (tf = identity when it is not found).  Returns one dict per candidate in the shape
    find_inter_loop_closures returns."""
    m = _d(meas7).reshape(-1, 7)
    sm = [_d(x).reshape(-1, 7) for x in submaps]
    n = len(sm)
    cp = _d(candidate_poses7).reshape(-1, 7)
    assert len(cp) == n, "one candidate pose per submap"
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in sm])
    flat = np.ascontiguousarray(np.concatenate(sm, axis=0)) if sm else np.zeros((0, 7))
    if len(flat) == 0:
        flat = np.zeros((1, 7))
    out = _intra_outputs(n)
    _check(lib().slide_find_intra_loop_closures(_p(m) if len(m) else None, C.c_int(len(m)), _p(_d(query_pose7)), _p(flat), _p(off), C.c_int(n),
                                                _p(cp if n else np.zeros((1, 7))), C.byref(params), C.c_double(x_half), C.c_double(y_half),
                                                C.c_double(yaw_half), *[_p(a) for a in out]))
    return _intra_dicts(n, *out)


def intra_loop_closure_attempt(cylinders, cubes, ellipsoids, meas7, query_pose7, candidate_poses7, submap_radius, params: PlaceParams,
                               max_dz=1.5, x_half=5.0, y_half=5.0, yaw_half=10.0 * np.pi / 180.0):
    """slide_intra_loop_closure_attempt: keypose_submaps around the candidates' positions followed by find_intra_loop_closures on what
    it produced, in one call.  Returns find_intra_loop_closures' dicts, each with `submap_size` added."""
    keep, targs = _map_tables(cylinders, cubes, ellipsoids)
    m = _d(meas7).reshape(-1, 7)
    cp = _d(candidate_poses7).reshape(-1, 7)
    n = len(cp)
    out = _intra_outputs(n)
    sizes = np.zeros(max(n, 1), np.int32)
    _check(lib().slide_intra_loop_closure_attempt(*targs, _p(m) if len(m) else None, C.c_int(len(m)), _p(_d(query_pose7)),
                                                  _p(cp if n else np.zeros((1, 7))), C.c_int(n), C.c_double(submap_radius), C.c_double(max_dz),
                                                  C.byref(params), C.c_double(x_half), C.c_double(y_half), C.c_double(yaw_half),
                                                  *[_p(a) for a in out], _p(sizes)))
    res = _intra_dicts(n, *out)
    for k, r in enumerate(res):
        r["submap_size"] = int(sizes[k])
    return res


def clipper_affinity(D1, D2, A, sigma=0.01, epsilon=0.06, mindist=0.0, affinityeps=1e-4):
    D1, D2 = _d(D1), _d(D2)
    A = _i(A)
    m = A.shape[0]
    M = np.zeros((m, m))
    _check(lib().slide_clipper_affinity(_p(D1), C.c_int(D1.shape[0]), _p(D2), C.c_int(D2.shape[0]), C.c_int(D1.shape[1]), _p(A),
                                        C.c_int(m), C.c_double(sigma), C.c_double(epsilon), C.c_double(mindist),
                                        C.c_double(affinityeps), _p(M)))
    return M


class ClipperParams(C.Structure):
    """slide_clipper_params_t (clipper.h:27-60, euclidean_distance.h:24-29)."""
    _fields_ = [("tol_u", C.c_double), ("tol_F", C.c_double), ("maxiniters", C.c_int), ("maxoliters", C.c_int),
                ("beta", C.c_double), ("maxlsiters", C.c_int), ("eps", C.c_double), ("affinityeps", C.c_double),
                ("rescale_u0", C.c_int), ("sigma", C.c_double), ("epsilon", C.c_double), ("mindist", C.c_double)]


def clipper_params(**kw):
    p = ClipperParams()
    lib().slide_clipper_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def clipper_dense_clique(M_upper, u0=None, params=None):
    """CLIPPER::findDenseClique (clipper.cpp:172-323, DSD_HEU).  Returns (nodes, u, score)."""
    M = _d(M_upper)
    n = M.shape[0]
    p = params or clipper_params()
    nodes = np.zeros(max(n, 1), np.int32)
    u = np.zeros(max(n, 1))
    nn, sc = C.c_int(0), C.c_double(0)
    u0a = _d(u0) if u0 is not None else None
    _check(lib().slide_clipper_dense_clique(_p(M), C.c_int(n), _p(u0a) if u0a is not None else None, C.byref(p), _p(nodes),
                                            C.byref(nn), _p(u), C.byref(sc)))
    return nodes[:nn.value].copy(), u[:n].copy(), sc.value


def clipper_affinity_csr(D1, D2, A, sigma=0.01, epsilon=0.06, mindist=0.0, affinityeps=1e-4):
    """scorePairwiseConsistency (clipper.cpp:21-65) ending in M_ = M.sparseView(): the symmetric affinity matrix without its diagonal
    as CSR, built on the device without the dense m x m form.  Returns (rowptr (m + 1), col, val), columns ascending; the values
    are clipper_affinity's bit for bit.  (The two-call protocol of slide_clipper_affinity_csr: sizes first, then the arrays.)"""
    D1, D2 = _d(D1), _d(D2)
    A = _i(A).reshape(-1, 2)
    m = A.shape[0]
    rowptr = np.zeros(m + 1, np.int32)
    nnz = C.c_longlong(0)

    def call(col, val, cap):
        return lib().slide_clipper_affinity_csr(_p(D1), C.c_int(D1.shape[0]), _p(D2), C.c_int(D2.shape[0]), C.c_int(D1.shape[1]), _p(A),
                                                C.c_int(m), C.c_double(sigma), C.c_double(epsilon), C.c_double(mindist),
                                                C.c_double(affinityeps), _p(rowptr), col, val, C.c_longlong(cap), C.byref(nnz))
    rc = call(None, None, 0)
    if rc == SLIDE_OK:                       # nothing to fetch
        return rowptr, np.zeros(0, np.int32), np.zeros(0)
    if rc != SLIDE_ERR_CAPACITY or nnz.value <= 0:
        _check(rc)
    col, val = np.zeros(nnz.value, np.int32), np.zeros(nnz.value)
    _check(call(_p(col), _p(val), nnz.value))
    return rowptr, col, val


def clipper_dense_clique_csr(rowptr, col, val, u0=None, params=None):
    """CLIPPER::findDenseClique (clipper.cpp:172-323, DSD_HEU) from the CSR of the symmetric affinity matrix without its diagonal
    (clipper_affinity_csr's output).  Returns (nodes, u, score) — clipper_dense_clique's for the same matrix, bit for bit."""
    rowptr, col, val = _i(rowptr), _i(col), _d(val)
    n = len(rowptr) - 1
    if n < 0 or len(col) != len(val) or (n >= 0 and len(rowptr) and rowptr[-1] != len(col)):
        raise SlideError(f"SLIDE_ERR_INVALID: clipper CSR, row {max(n - 1, 0)}: rowptr[n] = {rowptr[-1] if len(rowptr) else None} "
                         f"is not the length of col ({len(col)}) / val ({len(val)})")
    p = params or clipper_params()
    nodes = np.zeros(max(n, 1), np.int32)
    u = np.zeros(max(n, 1))
    nn, sc = C.c_int(0), C.c_double(0)
    u0a = _d(u0) if u0 is not None else None
    _check(lib().slide_clipper_dense_clique_csr(_p(rowptr), _p(col), _p(val), C.c_int(n), _p(u0a) if u0a is not None else None,
                                                C.byref(p), _p(nodes), C.byref(nn), _p(u), C.byref(sc)))
    return nodes[:nn.value].copy(), u[:n].copy(), sc.value


def clipper_match(D1, D2, A, u0=None, params=None):
    """scorePairwiseConsistency + findDenseClique + getSelectedAssociations in one call (slide_clipper_match): from the associations
    to the clique with nothing of size m^2 anywhere.  sigma / epsilon / mindist / affinityeps come from params.
    Returns (nodes, u, score) = clipper_dense_clique_csr(*clipper_affinity_csr(...)), bit for bit."""
    D1, D2 = _d(D1), _d(D2)
    A = _i(A).reshape(-1, 2)
    m = A.shape[0]
    p = params or clipper_params()
    nodes = np.zeros(max(m, 1), np.int32)
    u = np.zeros(max(m, 1))
    nn, sc = C.c_int(0), C.c_double(0)
    u0a = _d(u0) if u0 is not None else None
    _check(lib().slide_clipper_match(_p(D1), C.c_int(D1.shape[0]), _p(D2), C.c_int(D2.shape[0]), C.c_int(D1.shape[1]), _p(A), C.c_int(m),
                                     _p(u0a) if u0a is not None else None, C.byref(p), _p(nodes), C.byref(nn), _p(u), C.byref(sc)))
    return nodes[:nn.value].copy(), u[:m].copy(), sc.value


class ClosureParams(C.Structure):
    """slide_closure_params_t: the gate, the score's width and the odometry sigmas of the loop-closure consistency test."""
    _fields_ = [("gate", C.c_double), ("sigma", C.c_double), ("affinityeps", C.c_double), ("odom_sigma6", C.c_double * 6),
                ("min_set", C.c_int)]


def closure_params(**kw) -> ClosureParams:
    p = ClosureParams()
    lib().slide_closure_default_params(C.byref(p))
    for k, v in kw.items():
        if k == "odom_sigma6":
            for i, x in enumerate(np.broadcast_to(np.asarray(v, float), (6,))):
                p.odom_sigma6[i] = float(x)
        else:
            setattr(p, k, v)
    return p


def _closure_arrays(closures):
    """closures: dicts with from_robot, from_idx, to_robot, to_idx, rel7, sigma6 (or tuples in that order) -> the flat arrays."""
    rows = [(c["from_robot"], c["from_idx"], c["to_robot"], c["to_idx"], c["rel7"], c["sigma6"]) if isinstance(c, dict) else tuple(c)
            for c in closures]
    L = len(rows)
    fr = np.array([r[0] for r in rows] + [0], np.int32)
    fi = np.array([r[1] for r in rows] + [0], np.uint64)
    tr = np.array([r[2] for r in rows] + [0], np.int32)
    ti = np.array([r[3] for r in rows] + [0], np.uint64)
    rel = np.zeros((L + 1, 7))
    sg = np.ones((L + 1, 6))
    for k, r in enumerate(rows):
        rel[k] = np.asarray(r[4], float).reshape(7)
        sg[k] = np.broadcast_to(np.asarray(r[5], float), (6,))
    return fr[:L], fi[:L], tr[:L], ti[:L], rel[:L], sg[:L]


def closure_canonicalize(closures):
    """slide_closure_canonicalize (host bookkeeping, no device): closures with from_robot > to_robot get their ends swapped and rel
    inverted; groups by ascending (from_robot, to_robot), filled stably.  Returns a dict of arrays: from_robot, from_idx, to_robot,
    to_idx, rel7, flipped, group, order (row in the grouped list) and n_groups."""
    fr, fi, tr, ti, rel, _ = _closure_arrays(closures)
    L = len(fr)
    n = max(L, 1)
    o = {"from_robot": np.zeros(n, np.int32), "from_idx": np.zeros(n, np.uint64), "to_robot": np.zeros(n, np.int32),
         "to_idx": np.zeros(n, np.uint64), "rel7": np.zeros((n, 7)), "flipped": np.zeros(n, np.int32), "group": np.zeros(n, np.int32),
         "order": np.zeros(n, np.int32)}
    ng = C.c_int(0)
    _check(lib().slide_closure_canonicalize(C.c_int(L), _p(fr), _p(fi), _p(tr), _p(ti), _p(rel), _p(o["from_robot"]), _p(o["from_idx"]),
                                            _p(o["to_robot"]), _p(o["to_idx"]), _p(o["rel7"]), _p(o["flipped"]), _p(o["group"]),
                                            _p(o["order"]), C.byref(ng)))
    o = {k: v[:L] for k, v in o.items()}
    o["n_groups"] = ng.value
    return o


def closure_consistency_csr(from_pose7, to_pose7, rel7, sigma6, from_idx, to_idx, params=None):
    """slide_closure_consistency_csr: the loop-closure consistency matrix of ONE group (the closures as given), poses per closure, as
    the symmetric CSR without its diagonal, built on the device.  Returns (rowptr (L + 1), col, val), columns ascending."""
    fp, tp, rel, sg = _d(from_pose7).reshape(-1, 7), _d(to_pose7).reshape(-1, 7), _d(rel7).reshape(-1, 7), _d(sigma6).reshape(-1, 6)
    fi, ti = np.ascontiguousarray(from_idx, np.uint64), np.ascontiguousarray(to_idx, np.uint64)
    L = rel.shape[0]
    if not (len(fp) == len(tp) == len(sg) == len(fi) == len(ti) == L):
        raise ValueError("one pose pair, sigma6 and index pair per closure")
    p = params or closure_params()
    rowptr = np.zeros(L + 1, np.int32)
    nnz = C.c_longlong(0)

    def call(col, val, cap):
        return lib().slide_closure_consistency_csr(_p(fp), _p(tp), _p(rel), _p(sg), _p(fi), _p(ti), C.c_int(L), C.byref(p), _p(rowptr),
                                                   col, val, C.c_longlong(cap), C.byref(nnz))
    rc = call(None, None, 0)
    if rc == SLIDE_OK:                       # nothing to fetch
        return rowptr, np.zeros(0, np.int32), np.zeros(0)
    if rc != SLIDE_ERR_CAPACITY or nnz.value <= 0:
        _check(rc)
    col, val = np.zeros(nnz.value, np.int32), np.zeros(nnz.value)
    _check(call(_p(col), _p(val), nnz.value))
    return rowptr, col, val


def select_consistent_closures(closures, from_pose7, to_pose7, params=None, clipper=None, u0=None, with_csr=False):
    """slide_select_consistent_closures: the mutually consistent subset of a list of loop closures over any robot pairs
    (pairwise-consistency maximisation on the clique solver), the endpoints' poses given per closure.  closures as in
    SlideGraph.select_closures; u0: None, or a dict {group: start weights in the group's row order}.  Returns a dict: keep (bool),
    group, status, u per closure; n_selected, score per group; with_csr: also csr = one (rowptr, col, val) per group (None for a
    group of one closure)."""
    fr, fi, tr, ti, rel, sg = _closure_arrays(closures)
    L = len(fr)
    fp, tp = _d(from_pose7).reshape(-1, 7), _d(to_pose7).reshape(-1, 7)
    if len(fp) != L or len(tp) != L:
        raise ValueError("one pose pair per closure")
    p = params or closure_params()
    cp = clipper or clipper_params()
    n = max(L, 1)
    keep, group, status = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    nsel, score, ng, u = np.zeros(n, np.int32), np.zeros(n), C.c_int(0), np.zeros(n)
    u0p, held = None, []
    if u0:
        arr = (C.c_void_p * n)()
        for g, w in u0.items():
            held.append(_d(w))
            arr[int(g)] = held[-1].ctypes.data
        u0p = arr
    rowcnt = col = val = None
    cap, nnz = 0, C.c_longlong(0)
    if with_csr:
        cap = L * max(L - 1, 0)
        rowcnt, col, val = np.zeros(n, np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1))
    _check(lib().slide_select_consistent_closures(C.c_int(L), _p(fr), _p(fi), _p(tr), _p(ti), _p(rel), _p(sg), _p(fp), _p(tp), C.byref(p),
                                                  C.byref(cp), u0p, _p(keep), _p(group), _p(status), _p(nsel), _p(score), C.byref(ng),
                                                  _p(u), _p(rowcnt) if with_csr else None, _p(col) if with_csr else None,
                                                  _p(val) if with_csr else None, C.c_longlong(cap), C.byref(nnz)))
    out = {"keep": keep[:L].astype(bool), "group": group[:L].copy(), "status": status[:L].copy(), "u": u[:L].copy(),
           "n_selected": nsel[:ng.value].copy(), "score": score[:ng.value].copy()}
    if with_csr:
        # rows of a group in list order (the stable grouping), its slice of col / val behind the groups of two or more before it
        csr, at = [], 0
        for g in range(ng.value):
            rows = np.nonzero(group[:L] == g)[0]
            if len(rows) < 2:
                csr.append(None)
                continue
            rp = np.concatenate([[0], np.cumsum(rowcnt[rows])]).astype(np.int32)
            csr.append((rp, col[at:at + rp[-1]].copy(), val[at:at + rp[-1]].copy()))
            at += int(rp[-1])
        assert at == nnz.value
        out["csr"] = csr
    return out


def clipper_last_solve_info():
    """(workgroups, gradient evaluations) of this process's last clipper_dense_clique / _csr / clipper_match call: > 1 workgroup = the cooperative solve of
    one large problem (n >= 1024, or SLIDE_CLIPPER_WGS)."""
    w, e = C.c_int(0), C.c_double(0)
    lib().slide_clipper_last_solve_info(C.byref(w), C.byref(e))
    return w.value, e.value


MS_PLACE_SWEEP, MS_TRI_MATCH, MS_CLQ_CSR, MS_CLQ_SOLVE, MS_AFFINITY, MS_CLQ_NNZ, MS_PLACE_PAIR_TESTS, MS_TRI_PAIRS, MS_PLACE_DIST_TESTS = range(9)
MS_AFFINITY_CSR = 9


def last_device_ms(what):
    """slide_last_device_ms: kernel time (ms) or work count of the last stand-alone SlideMatch / SlideGraph / CLIPPER call."""
    v = C.c_double(0)
    _check(lib().slide_last_device_ms(C.c_int(what), C.byref(v)))
    return v.value


def clipper_dense_clique_batch(Ms, u0s=None, params=None):
    """Several CLIPPER dense-clique problems in one launch (one persistent workgroup per problem).  Ms: list of (n_j, n_j) affinity
    matrices; u0s: list of start vectors or None.  Returns [(nodes, u, score), ...] — what clipper_dense_clique gives for each."""
    J = len(Ms)
    Ma = [_d(M) for M in Ms]
    ns = np.array([M.shape[0] for M in Ma], np.int32)
    p = params or clipper_params()
    nodes = [np.zeros(max(int(k), 1), np.int32) for k in ns]
    us = [np.zeros(max(int(k), 1)) for k in ns]
    u0a = [(_d(u) if u is not None else None) for u in (u0s or [None] * J)]
    PP = C.POINTER(C.c_double)
    Mp = (C.c_void_p * J)(*[M.ctypes.data for M in Ma])
    Up = (C.c_void_p * J)(*[(u.ctypes.data if u is not None else None) for u in u0a])
    Np = (C.c_void_p * J)(*[x.ctypes.data for x in nodes])
    Op = (C.c_void_p * J)(*[x.ctypes.data for x in us])
    nn = np.zeros(max(J, 1), np.int32)
    sc = np.zeros(max(J, 1))
    _check(lib().slide_clipper_dense_clique_batch(C.c_int(J), Mp, _p(ns), Up, C.byref(p), Np, _p(nn), Op, _p(sc)))
    return [(nodes[j][:nn[j]].copy(), us[j][:ns[j]].copy(), float(sc[j])) for j in range(J)]


def match_triangles(tri_model, tri_data, threshold=0.1):
    """semantic_clipper::match_triangles (semantic_clipper.cpp:49-118).  tri_*: (n, 3, 2).  Returns (pts (n_pairs, 3, 4) with
    rows [model x, model y, data x, data y], diffs (n_pairs,))."""
    tm, td = _d(tri_model).reshape(-1, 6), _d(tri_data).reshape(-1, 6)
    n = C.c_int(0)
    _check(lib().slide_match_triangles(_p(tm), C.c_int(len(tm)), _p(td), C.c_int(len(td)), C.c_double(threshold), None, None,
                                       C.c_int(0), C.byref(n)))
    pts = np.zeros((max(n.value, 1), 3, 4))
    diffs = np.zeros(max(n.value, 1))
    _check(lib().slide_match_triangles(_p(tm), C.c_int(len(tm)), _p(td), C.c_int(len(td)), C.c_double(threshold), _p(pts), _p(diffs),
                                       C.c_int(n.value), C.byref(n)))
    return pts[:n.value], diffs[:n.value]


def estimate_tf2d(a_xy, b_xy):
    a, b = _d(a_xy), _d(b_xy)
    tf = np.zeros(9)
    _check(lib().slide_estimate_tf2d(_p(a), _p(b), C.c_int(len(a)), _p(tf)))
    return tf.reshape(3, 3)


def semantic_clipper(tri_model, tri_data, params=None, min_num_pairs=4, matching_threshold=0.1, u0=None):
    """semantic_clipper::run_semantic_clipper (semantic_clipper.cpp:140-274) from the triangle lists on.
    Returns dict(found, tf (4x4 query -> reference), n_putative, n_inliers, inliers)."""
    tm, td = _d(tri_model).reshape(-1, 6), _d(tri_data).reshape(-1, 6)
    p = params or clipper_params()
    tf = np.zeros(16)
    counts = np.zeros(2, np.int32)
    cap = 3 * len(tm) * max(len(td), 1)
    cap = min(cap, 1 << 22)
    inl = np.zeros(max(cap, 1), np.int32)
    found = C.c_int(0)
    u0a = _d(u0) if u0 is not None else None
    _check(lib().slide_semantic_clipper(_p(tm), C.c_int(len(tm)), _p(td), C.c_int(len(td)), C.byref(p), C.c_int(min_num_pairs),
                                        C.c_double(matching_threshold), _p(u0a) if u0a is not None else None,
                                        C.c_int(len(u0a) if u0a is not None else 0), _p(tf), _p(counts), _p(inl), C.c_int(len(inl)),
                                        C.byref(found)))
    return dict(found=bool(found.value), tf=tf.reshape(4, 4), n_putative=int(counts[0]), n_inliers=int(counts[1]),
                inliers=inl[:counts[1]].copy())


def closest_stamp(sec, nsec, qsec, qnsec):
    sec = np.ascontiguousarray(sec, dtype=np.int64)
    nsec = np.ascontiguousarray(nsec, dtype=np.int64)
    idx, diff = C.c_int(0), C.c_double(0)
    lib().slide_closest_stamp(_p(sec), _p(nsec), C.c_int(len(sec)), C.c_int64(qsec), C.c_int64(qnsec), C.byref(idx),
                              C.byref(diff))
    return idx.value, diff.value


def find_relative_meas_match(packets, counters, host, pending):
    """sloam::FindRelativeMeasurementMatch (sloam.cpp:321-412).  packets: per robot list of (sec, nsec); pending: list of
    ((sec, nsec), robot, only_use_odom).  Returns (matches (n, 4) = [tag, index, host idx, other idx], tags of the
    measurements still pending); raises SlideError where the reference throws."""
    sec, ns, off = [], [], [0]
    for pk in packets:
        for (a, b) in pk:
            sec.append(a); ns.append(b)
        off.append(len(sec))
    sec = np.array(sec + [0], np.int64); ns = np.array(ns + [0], np.int64); off = np.array(off, np.int32)
    pc = np.array(counters, np.uint64)
    npend = C.c_int(len(pending))
    m_sec = np.array([p[0][0] for p in pending] + [0], np.int64)
    m_ns = np.array([p[0][1] for p in pending] + [0], np.int64)
    m_rob = np.array([p[1] for p in pending] + [0], np.int32)
    m_odo = np.array([int(p[2]) for p in pending] + [0], np.int32)
    m_tag = np.arange(len(pending) + 1, dtype=np.int32)
    out = np.zeros(4 * max(len(pending), 1), np.int32)
    nm = C.c_int(0)
    _check(lib().slide_find_relative_meas_match(C.c_int(len(packets)), _p(sec), _p(ns), _p(off), _p(pc), C.c_int(host), C.byref(npend),
                                                _p(m_sec), _p(m_ns), _p(m_rob), _p(m_odo), _p(m_tag), _p(out), C.byref(nm)))
    return out.reshape(-1, 4)[:nm.value].copy(), m_tag[:npend.value].copy()


def delaunay_2d(points_xy):
    """Triangle index triples (ascending ids, lexicographic order) of the 2-D Delaunay triangulation (host code)."""
    xy = _d(points_xy)
    n = len(xy)
    cap = max(2 * n, 1)
    tri = np.zeros((cap, 3), np.int32)
    nt = C.c_int(0)
    _check(lib().slide_delaunay_2d(_p(xy), C.c_int(n), _p(tri), C.c_int(cap), C.byref(nt)))
    return tri[:nt.value].copy()


def run_semantic_clipper(ref7, qry7, sigma=0.01, epsilon=0.06, min_num_pairs=4, matching_threshold=0.1, u0=None):
    """semantic_clipper::run_semantic_clipper (semantic_clipper.cpp:140-274) on two object maps (rows [label, x, y, z, d1, d2, d3])."""
    r, q = _d(ref7), _d(qry7)
    tf = np.zeros(16)
    counts = np.zeros(2, np.int32)
    found = C.c_int(0)
    u0a = _d(u0) if u0 is not None else None
    _check(lib().slide_run_semantic_clipper(_p(r), C.c_int(len(r)), _p(q), C.c_int(len(q)), C.c_double(sigma), C.c_double(epsilon),
                                            C.c_int(min_num_pairs), C.c_double(matching_threshold),
                                            _p(u0a) if u0a is not None else None, C.c_int(len(u0a) if u0a is not None else 0),
                                            _p(tf), _p(counts), C.byref(found)))
    return dict(found=bool(found.value), tf=tf.reshape(4, 4), n_putative=int(counts[0]), n_inliers=int(counts[1]))


class SlidegraphParams(C.Structure):
    _fields_ = [("sigma", C.c_double), ("epsilon", C.c_double), ("num_inliers_threshold", C.c_int), ("matching_threshold", C.c_double),
                ("min_num_map_objects_to_start", C.c_int)]


def slidegraph_params(**kw) -> SlidegraphParams:
    """PlaceRecognition's SlideGraph parameters with the reference's defaults (place_recognition.cpp:65-75)."""
    p = SlidegraphParams()
    lib().slide_slidegraph_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"slidegraph_params: no field {k!r}")
        setattr(p, k, v)
    return p


def _closure_dict(tf, counts, found):
    return dict(found=bool(found), tf=np.array(tf, dtype=np.float64).reshape(4, 4), n_putative=int(counts[2]), n_inliers=int(counts[3]),
                n_ref_used=int(counts[0]), n_qry_used=int(counts[1]))


def find_inter_loop_closure_clipper(ref7, qry7, params=None, u0=None):
    """PlaceRecognition::findInterLoopClosureWithClipper (place_recognition.cpp:541-629) on two object maps (rows [label, x, y, z, d1,
    d2, d3]): rows with x == y == 0 dropped, the gate on the kept counts, run_semantic_clipper, and tf = the INVERSE of its estimate
    (identity when nothing is found).  Returns dict(found, tf, n_putative, n_inliers, n_ref_used, n_qry_used)."""
    r, q = _d(ref7).reshape(-1, 7), _d(qry7).reshape(-1, 7)
    p = params or slidegraph_params()
    tf = np.zeros(16)
    counts = np.zeros(4, np.int32)
    found = C.c_int(0)
    u0a = _d(u0) if u0 is not None else None
    _check(lib().slide_find_inter_loop_closure_clipper(_p(r), C.c_int(len(r)), _p(q), C.c_int(len(q)), C.byref(p),
                                                       _p(u0a) if u0a is not None else None, C.c_int(len(u0a) if u0a is not None else 0),
                                                       _p(tf), _p(counts), C.byref(found)))
    return _closure_dict(tf, counts, found.value)


def find_inter_loop_closures_clipper(maps, pairs, params=None, u0s=None):
    """The loop of SLOAMNode::interLoopClosureThread_ (sloamNode.cpp:587-694) in one call: maps = list of (n_i, 7) object maps, pairs =
    list of (reference map, query map) indices, u0s = None or a list with None / start weights per pair.  Every pair is evaluated by
    itself and gets exactly find_inter_loop_closure_clipper's result for that pair alone.  Returns a list of dicts as the single call's,
    each with `status` added (0, or the pair's own SLIDE_ERR_INVALID / SLIDE_ERR_CAPACITY)."""
    ms = [_d(m).reshape(-1, 7) for m in maps]
    off = np.zeros(len(ms) + 1, np.int32)
    off[1:] = np.cumsum([len(m) for m in ms])
    flat = np.ascontiguousarray(np.concatenate(ms, axis=0)) if ms else np.zeros((0, 7))
    if len(flat) == 0:
        flat = np.zeros((1, 7))
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    n = len(pr)
    p = params or slidegraph_params()
    tf = np.zeros((max(n, 1), 16))
    counts = np.zeros((max(n, 1), 4), np.int32)
    found = np.zeros(max(n, 1), np.int32)
    status = np.zeros(max(n, 1), np.int32)
    u0_ptrs = n_u0 = None
    keep = []
    if u0s is not None:
        if len(u0s) != n:
            raise ValueError("u0s needs one entry (or None) per pair")
        u0_ptrs = (C.c_void_p * max(n, 1))()
        n_u0 = np.zeros(max(n, 1), np.int32)
        for k, u in enumerate(u0s):
            if u is not None:
                a = _d(u).reshape(-1)
                keep.append(a)
                u0_ptrs[k] = a.ctypes.data
                n_u0[k] = len(a)
    _check(lib().slide_find_inter_loop_closures_clipper(_p(flat), _p(off), C.c_int(len(ms)), _p(pr if n else np.zeros((1, 2), np.int32)), C.c_int(n),
                                                        C.byref(p), u0_ptrs, _p(n_u0) if n_u0 is not None else None, _p(tf), _p(counts),
                                                        _p(found), _p(status)))
    out = []
    for k in range(n):
        d = _closure_dict(tf[k], counts[k], found[k])
        d["status"] = int(status[k])
        out.append(d)
    return out


def pick_next_measurement(odom, obs, rel, latest, current_time, msg_delay_tolerance, min_odom_distance):
    """Input::PickNextMeasurementToAdd (input.cpp:26-108).  odom: list of ((sec, nsec), pose7); obs / rel: lists of (sec, nsec);
    latest: ((sec, nsec), pose7).  Returns (meas_to_add, pop_odom, pop_obs, pop_rel)."""
    def stamps(lst):
        a = np.array([[x[0], x[1]] for x in lst] + [[0, 0]], np.int64)
        return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])
    os_, on_ = stamps([o[0] for o in odom])
    op = _d(np.array([o[1] for o in odom] + [[0, 0, 0, 0, 0, 0, 1.0]]))
    bs, bn = stamps(obs)
    rs, rn = stamps(rel)
    out = np.zeros(4, np.int32)
    _check(lib().slide_pick_next_measurement(_p(os_), _p(on_), _p(op), C.c_int(len(odom)), _p(bs), _p(bn), C.c_int(len(obs)), _p(rs), _p(rn),
                                             C.c_int(len(rel)), C.c_int64(latest[0][0]), C.c_int64(latest[0][1]), _p(_d(latest[1])),
                                             C.c_double(current_time), C.c_double(msg_delay_tolerance), C.c_float(min_odom_distance),
                                             _p(out)))
    return tuple(int(v) for v in out)


def in_loop_closure_region(cloud_xyz, pose_xyz, max_dist_xy=10.0, max_dist_z=2.0, at_least_num_of_poses_old=30):
    cloud = np.ascontiguousarray(cloud_xyz, dtype=np.float32).reshape(-1, 3)
    inside = C.c_int(0)
    _check(lib().slide_in_loop_closure_region(_p(cloud), C.c_int(len(cloud)), _p(_d(pose_xyz)), C.c_double(max_dist_xy),
                                              C.c_double(max_dist_z), C.c_uint64(at_least_num_of_poses_old), C.byref(inside)))
    return bool(inside.value)
