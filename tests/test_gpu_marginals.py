"""Batched marginal covariances and loop-closure information gain (slide_graph_get_pose_covariances / _get_landmark_covariances /
_marginal_traces / _closure_info_gain: the dormant logEntropy / estimateClosureInfoGain of graph.cpp:421-625) against the dense
inverse of the full, unreduced H = J^T J of tests/gn_reference.py (every factor linearised by the oracle's orc_linearize: no Schur
complement, no tile profile, no product library), and against the product's own single-pose getter.

After gauss_newton(1) the resident factor is the one of the initial values, which is where the reference linearises.  Blocks are
compared Jacobi-scaled by diag(H)^1/2; the tolerance comes from the case as in gn_reference.tolerance (8 n eps kappa_s, plus ten
times the central-difference noise floor for cubes and cylinders)."""
import ctypes as C

import numpy as np
import pytest

import gn_graphs as gg
from gn_reference import EPS, Reference
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

ROBOT_CH = "xyzmnopqrstvw"


def build_pair(gpu, build, chart, dense=False):
    og = po.OracleGraph(po.OrcParams.default(pose_chart=chart))
    build(og)
    G = gpu.SlideGraph(gpu.default_params(pose_chart=chart))
    if dense:
        G.set_dense_profile(True)
    build(G)
    assert G.gauss_newton(1) == 0
    return Reference(og, chart), G


def var_kind(ref, k):
    key = int(ref.vkey[k])
    c, idx = chr(key >> 56), key & ((1 << 56) - 1)
    if int(ref.vtype[k]) == po.V_POSE:
        return "pose", ROBOT_CH.index(c), idx
    return "lm", "lcu".index(c), idx


def dense_inverse(ref):
    """inv(H) at the initial values, its Jacobi scaling w, and the tolerance of a scaled entry relative to max |W inv(H) W|."""
    _, H = ref.step()
    w = np.sqrt(np.diag(H))
    Hs = H / np.outer(w, w)
    kappa = float(np.linalg.cond(Hs))
    Sig = np.linalg.inv(H)
    nd = 0.0
    if np.isin(ref.ftype, (po.F_CUBE, po.F_CYL)).any():
        _, H2 = ref.step(delta=1.00001e-6)
        nd = float(np.abs((np.linalg.inv(H2) - Sig) * np.outer(w, w)).max() / np.abs(Sig * np.outer(w, w)).max())
    return H, Sig, w, 8 * H.shape[0] * EPS * kappa + 10 * nd, kappa


def gpu_marginals(ref, G):
    """{variable: its marginal block} from the batched getters, one call per robot / landmark class."""
    groups = {}
    for k in range(len(ref.vtype)):
        kind, a, idx = var_kind(ref, k)
        groups.setdefault((kind, a), []).append((k, idx))
    out = {}
    for (kind, a), items in groups.items():
        idx = [i for _, i in items]
        blocks = G.get_pose_covariances(a, idx) if kind == "pose" else G.get_landmark_covariances(a, idx)
        for (k, _), b in zip(items, blocks):
            out[k] = b
    return out


def check_marginals(ref, G):
    H, Sig, w, tol, kappa = dense_inverse(ref)
    scale = np.abs(Sig * np.outer(w, w)).max()
    got = gpu_marginals(ref, G)
    worst = 0.0
    for k, b in got.items():
        o0, o1 = ref.off[k], ref.off[k + 1]
        ws = np.outer(w[o0:o1], w[o0:o1])
        worst = max(worst, float(np.abs((b - Sig[o0:o1, o0:o1]) * ws).max() / scale))
    assert len(got) == len(ref.vtype)
    assert worst <= tol, (worst, tol, kappa)
    return got


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def chain40(g):
    return gg.pose_count_graph(g, 40)


def loop36(g):
    """A 36-pose chain closed from its last pose back to its first: the profile becomes the full triangle."""
    W = gg.pose_count_graph(g, 36, seed=5)
    (Ra, ta), (Rb, tb) = W.T[35], W.T[0]
    g.add_loop_closure(gg.p7(Ra.T @ Rb, Ra.T @ (tb - ta)), 35, 0, 0, 0)
    return W


def two_robots(g):
    """Robot 0's 24-pose chain and robot 1's 16-pose chain, joined by one relative-pose factor; a point seen by both."""
    W = gg.pose_count_graph(g, 24, seed=6)
    T1 = [(gg.rot([0.0, 0.0, 0.1 * k]), np.array([1.0 * k, 6.0, 0.2])) for k in range(16)]
    g.set_prior(1, gg.p7(*T1[0]))
    rng = np.random.default_rng(7)
    for k in range(1, 16):
        (Ra, ta), (Rb, tb) = T1[k - 1], T1[k]
        g.add_keypose_between(1, k - 1, k, gg.p7(Ra.T @ Rb, Ra.T @ (tb - ta)), gg.p7(Rb, tb + rng.normal(0, 0.05, 3)))
    (Ra, ta), (Rb, tb) = W.T[10], T1[4]
    g.add_relative_meas(gg.p7(Ra.T @ Rb, Ra.T @ (tb - ta)), 10, 0, 4, 1)
    return W


CASES = [("chain40", chain40), ("loop36", loop36), ("two_robots", two_robots)]


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("name,build", CASES, ids=[c[0] for c in CASES])
def test_marginals_vs_dense_inverse(gpu, chart, name, build):
    ref, G = build_pair(gpu, build, chart)
    prof = G.tile_profile()
    if name == "chain40":
        assert len(prof) >= 4                                            # four tile columns or more
        assert any((6 * p) // 64 != (6 * p + 5) // 64 for p in range(40))   # pose blocks straddling a tile boundary
    if name == "loop36":
        assert prof[0] == len(prof) - 1                                  # the full triangle
    # the resident factor is the one of the initial values: the single-pose getter agrees with inv(H)
    H, Sig, w, tol, kappa = dense_inverse(ref)
    k = ref.pose_var(0, 5)
    st, c = G.get_pose_covariance(0, 5)
    o = ref.off[k]
    assert st == 0
    ws = np.outer(w[o:o + 6], w[o:o + 6])
    assert np.abs((c - Sig[o:o + 6, o:o + 6]) * ws).max() <= tol * np.abs(Sig * np.outer(w, w)).max()
    check_marginals(ref, G)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("cls", [0, 1, 2], ids=["cyl", "cube", "point"])
@pytest.mark.parametrize("nf", [1, 64, 65, 130])
def test_landmark_factor_count(gpu, chart, cls, nf):
    """One landmark with 1 .. 130 factors (k_lm_cov's pair sum over them) next to a point seen from two poses."""
    ref, G = build_pair(gpu, lambda g: gg.landmark_count_graph(g, cls, nf), chart)
    _, per_lm = ref.list_lengths()
    assert per_lm[ref.lm_var(cls, 0)] == nf
    check_marginals(ref, G)


@pytest.mark.parametrize("chart", [0, 1])
def test_dense_profile_same_result(gpu, chart):
    ref, G = build_pair(gpu, chain40, chart)
    _, Gd = build_pair(gpu, chain40, chart, dense=True)
    a = check_marginals(ref, G)
    b = check_marginals(ref, Gd)
    for k in a:
        assert np.abs(a[k] - b[k]).max() <= 1e-9 * np.abs(a[k]).max(), k


# ---- the 625-pose robot graph of the synthetic worlds, incremental updates ------------------------------------------------------------
def _replay(backend, log, k0, k1, prev):
    from slide_slam_amd.synth import frame_detections
    for k in range(k0, k1):
        r = backend.process_frame(0, log["rel7"][k], prev, frame_detections(log, k), 0)
        assert r["status"] == 0
        prev = r["pose7"].copy()
    return prev


def _against_single(G, P):
    batch = G.get_pose_covariances(0, np.arange(P))
    worst = 0.0
    for p in range(P):
        st, c = G.get_pose_covariance(0, p)
        assert st == 0
        worst = max(worst, float(np.abs(batch[p] - c).max() / np.abs(c).max()))
    return worst


def test_batched_poses_625_and_incremental(gpu):
    from slide_slam_amd.synth import SynthConfig, make_robot_log, make_world
    cfg = SynthConfig.preset("C4shard")
    assert cfg.poses_per_robot == 625
    log = make_robot_log(cfg, make_world(cfg), 0)
    b = gpu.SlideBackend(gpu.default_params(), 1)
    G = b.graph
    G.set_incremental(True)
    from slide_slam_amd.replay import IDENT7
    prev = _replay(b, log, 0, 620, IDENT7.copy())
    w0 = _against_single(G, 620)
    assert w0 <= 1e-9, w0
    _replay(b, log, 620, 625, prev)
    st = G.incremental_stats()
    assert st["last_first_column"] > 0, st                        # the last update kept block columns of the factor
    w1 = _against_single(G, 625)
    assert w1 <= 1e-9, w1
    print(f"625 poses: batched vs single max rel {w0:.2e}, after an incremental update {w1:.2e}")


# ---- information gain -------------------------------------------------------------------------------------------------------------------
def rel12(a12, b12):
    """a^-1 b as R row-major (9) + t (3)."""
    Ra, ta = a12[:9].reshape(3, 3), a12[9:12]
    Rb, tb = b12[:9].reshape(3, 3), b12[9:12]
    return np.concatenate([(Ra.T @ Rb).ravel(), Ra.T @ (tb - ta)])


def ref_gain(ref, H, robot, traj, travel, sigma):
    """The trace drops of inv(H) -> inv(H + J_f^T J_f), J_f: the Between rows (traj[i+1], traj[i]) linearised by orc_linearize."""
    L = po.lib()
    vals = ref.values
    Jf = np.zeros((6 * len(travel), ref.n))
    r, J0, J1 = np.zeros(9), np.zeros(81), np.zeros(81)
    for i, d in enumerate(travel):
        a, b = ref.pose_var(robot, traj[i + 1]), ref.pose_var(robot, traj[i])
        xa, xb = np.ascontiguousarray(vals[a][:12]), np.ascontiguousarray(vals[b][:12])
        z = rel12(xa, xb)
        sg = np.ascontiguousarray(np.asarray(sigma, float) * d)
        m = L.orc_linearize(C.c_int(po.F_BETWEEN), xa.ctypes.data_as(C.c_void_p), C.c_int(po.V_POSE), xb.ctypes.data_as(C.c_void_p),
                            z.ctypes.data_as(C.c_void_p), sg.ctypes.data_as(C.c_void_p), C.c_int(ref.chart), C.c_double(1e-6),
                            r.ctypes.data_as(C.c_void_p), J0.ctypes.data_as(C.c_void_p), J1.ctypes.data_as(C.c_void_p), C.c_int(1))
        assert m == 6 and np.abs(r[:6]).max() < 1e-9
        Jf[6 * i:6 * i + 6, ref.off[a]:ref.off[a] + 6] += J0[:36].reshape(6, 6)
        Jf[6 * i:6 * i + 6, ref.off[b]:ref.off[b] + 6] += J1[:36].reshape(6, 6)
    S0, S1 = np.linalg.inv(H), np.linalg.inv(H + Jf.T @ Jf)
    gp = gl = tp = tl = 0.0
    for k in range(len(ref.vtype)):
        kind, a, _ = var_kind(ref, k)
        o0, o1 = ref.off[k], ref.off[k + 1]
        d0, d1 = np.trace(S0[o0:o1, o0:o1]), np.trace(S1[o0:o1, o0:o1])
        if kind == "pose" and a == robot:
            gp += d0 - d1; tp += d0
        elif int(ref.vtype[k]) == po.V_POINT:
            gl += d0 - d1; tl += d0
    return np.array([10 * gp + gl, gp, gl]), np.array([10 * tp + tl, tp, tl])


SIGMA = np.array([0.02, 0.02, 0.02, 0.05, 0.05, 0.05])


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("name,build", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("m", [1, 3])
def test_info_gain_vs_dense(gpu, chart, name, build, m):
    ref, G = build_pair(gpu, build, chart)
    H, _, _, tol, kappa = dense_inverse(ref)
    traj = [30 if name != "two_robots" else 20, 22, 12, 2][: m + 1] if m == 3 else [33 if name != "two_robots" else 22, 1]
    travel = [4.0 + i for i in range(m)]
    got = G.closure_info_gain(0, traj, travel, SIGMA)
    want, traces = ref_gain(ref, H, 0, traj, travel, SIGMA)
    assert want[1] > 0 and want[2] >= 0
    # relative to the gains themselves; only a gain below a thousandth of its trace sum is measured against that instead (the dense
    # reference forms it as a difference of two traces and loses those digits)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-3 * traces)
    assert (err <= max(tol, 1e-12)).all(), (got, want, err, tol, kappa)
    if name == "chain40" and m == 1:
        pts = [k for k in range(len(ref.vtype)) if int(ref.vtype[k]) == po.V_POINT]
        assert pts and want[2] > 0
    # the same distance across a long stretch of the chain gains more than between neighbouring poses
    near = G.closure_info_gain(0, [1, 0], [4.0], SIGMA)
    far = G.closure_info_gain(0, [traj[0], 0], [4.0], SIGMA)
    assert far[0] > near[0] > 0


def test_info_gain_default_sigma_and_traces(gpu):
    ref, G = build_pair(gpu, chain40, 0)
    g1 = G.closure_info_gain(0, [39, 0], [5.0])
    g2 = G.closure_info_gain(0, [39, 0], [5.0], list(gpu.default_params().noise_model_odom_vec))
    assert np.array_equal(g1, g2) and g1[0] > 0
    t = G.marginal_traces(0)
    H, Sig, _, tol, _ = dense_inverse(ref)
    tp = sum(np.trace(Sig[ref.off[k]:ref.off[k + 1], ref.off[k]:ref.off[k + 1]]) for k in range(len(ref.vtype)) if int(ref.vtype[k]) == po.V_POSE)
    pts = [k for k in range(len(ref.vtype)) if int(ref.vtype[k]) == po.V_POINT]
    tl = sum(np.trace(Sig[ref.off[k]:ref.off[k + 1], ref.off[k]:ref.off[k + 1]]) for k in pts)
    assert t[2] == 40 and t[3] == len(pts)
    assert abs(t[0] - tp) <= max(tol, 1e-12) * tp and abs(t[1] - tl) <= max(tol, 1e-12) * tl, (t, tp, tl)


def test_default_sigma_is_the_graphs_own(gpu):
    """sigma_per_m omitted: the odometry noise of the graph the query runs on, also for a graph reached through its backend."""
    from slide_slam_amd.synth import SynthConfig, frame_detections, make_robot_log, make_world
    from slide_slam_amd.replay import IDENT7
    p = gpu.default_params()
    odom = [0.03, 0.04, 0.05, 0.2, 0.3, 0.4]
    for i, v in enumerate(odom):
        p.noise_model_odom_vec[i] = v
    cfg = SynthConfig.preset("tiny")
    log = make_robot_log(cfg, make_world(cfg), 0)
    b = gpu.SlideBackend(p, 1)
    _replay(b, log, 0, 12, IDENT7.copy())
    G = b.graph
    own = G.closure_info_gain(0, [11, 0], [5.0])
    assert np.array_equal(own, G.closure_info_gain(0, [11, 0], [5.0], odom))
    assert not np.array_equal(own, G.closure_info_gain(0, [11, 0], [5.0], list(gpu.default_params().noise_model_odom_vec)))


def test_graph_changed_since_the_solve(gpu):
    """A call that merges pending additions after the solve (tile_profile) leaves the resident factor describing an older system — and
    poses past the tile capacity re-allocate S, Ld and Winv and grow ld.  The queries refuse until the next solve."""
    G = gpu.SlideGraph(gpu.default_params())
    W = chain40(G)
    assert G.gauss_newton(1) == 0
    T0 = len(G.tile_profile())
    before = G.get_pose_covariances(0, range(40))
    G.get_landmark_covariances(2, [0])
    # one more landmark factor on existing poses, merged by tile_profile(): same geometry, other system
    W.point(1000, gg.around(W, 5, np.random.default_rng(3)), [5, 6])
    assert len(G.tile_profile()) == T0
    for call in ((G.get_pose_covariances, 0, [1]), (G.get_landmark_covariances, 2, [0]), (G.marginal_traces, 0),
                 (G.closure_info_gain, 0, [39, 0], [2.0], SIGMA)):
        _raises("SLIDE_ERR_INVALID", *call)
    assert G.gauss_newton(1) == 0
    assert G.get_pose_covariances(0, [1]).shape == (1, 6, 6)
    # ten more poses: T 4 -> 5 past the capacity (S re-allocated, ld 320 -> 512), merged by tile_profile()
    R, t = W.T[-1]
    for k in range(40, 50):
        G.add_keypose_between(0, k - 1, k, gg.p7(np.eye(3), np.array([1.0, 0.0, 0.0])), gg.p7(R, t + np.array([k - 39.0, 0.0, 0.0])))
    assert len(G.tile_profile()) == 5
    for call in ((G.get_pose_covariances, 0, [1, 45]), (G.get_pose_covariances, 0, [1]), (G.get_landmark_covariances, 2, [0]),
                 (G.marginal_traces, 0), (G.closure_info_gain, 0, [49, 0], [2.0], SIGMA)):
        _raises("SLIDE_ERR_INVALID", *call)
    assert G.gauss_newton(1) == 0
    after = G.get_pose_covariances(0, range(50))
    for p in (0, 20, 45, 49):
        assert np.array_equal(after[p], G.get_pose_covariance(0, p)[1]) or \
            np.abs(after[p] - G.get_pose_covariance(0, p)[1]).max() <= 1e-9 * np.abs(after[p]).max()
    assert before.shape == (40, 6, 6)


# ---- nothing moved, status paths ------------------------------------------------------------------------------------------------------
def test_queries_leave_the_graph_as_it_was(gpu):
    A = gpu.SlideGraph(gpu.default_params())
    B = gpu.SlideGraph(gpu.default_params())
    for g in (A, B):
        loop36(g)
        g.set_incremental(True)
        assert g.gauss_newton(1) == 0
    A.closure_info_gain(0, [35, 20, 10, 0], [3.0, 2.0, 2.5], SIGMA)
    A.get_pose_covariances(0, range(36))
    A.get_landmark_covariances(2, [0, 3])
    A.get_landmark_covariances(0, [0])
    A.marginal_traces(0)
    A.closure_info_gain(0, [30, 1], [3.0], SIGMA)
    for p in (0, 17, 35):
        assert np.array_equal(A.get_pose_covariance(0, p)[1], B.get_pose_covariance(0, p)[1])
    for g in (A, B):
        assert g.gauss_newton(1) == 0
    for p in range(36):
        assert np.array_equal(A.get_pose12(0, p)[1], B.get_pose12(0, p)[1]), p
    assert np.array_equal(A.get_pose_covariance(0, 7)[1], B.get_pose_covariance(0, 7)[1])
    assert np.array_equal(A.get_pose_covariances(0, [7])[0], B.get_pose_covariances(0, [7])[0])


def _raises(code, fn, *a):
    with pytest.raises(Exception) as e:
        fn(*a)
    assert code in str(e.value), str(e.value)


def test_status_paths(gpu):
    G = gpu.SlideGraph(gpu.default_params())
    gg.pose_count_graph(G, 10)
    _raises("SLIDE_ERR_INVALID", G.get_pose_covariances, 0, [1])           # before the first solve
    _raises("SLIDE_ERR_INVALID", G.get_landmark_covariances, 2, [0])
    _raises("SLIDE_ERR_INVALID", G.marginal_traces, 0)
    _raises("SLIDE_ERR_INVALID", G.closure_info_gain, 0, [9, 0], [2.0], SIGMA)
    assert G.gauss_newton(1) == 0
    assert G.get_pose_covariances(0, [1, 2]).shape == (2, 6, 6)
    with pytest.raises(KeyError):
        G.get_pose_covariances(0, [1, 99])
    with pytest.raises(KeyError):
        G.get_pose_covariances(1, [0])
    with pytest.raises(KeyError):
        G.get_landmark_covariances(2, [777])
    with pytest.raises(KeyError):
        G.closure_info_gain(0, [99, 0], [2.0], SIGMA)
    _raises("SLIDE_ERR_INVALID", G.closure_info_gain, 0, [3], [], SIGMA)                 # m = 0
    _raises("SLIDE_ERR_INVALID", G.closure_info_gain, 0, [9, 0], [0.0], SIGMA)           # zero travel distance
    _raises("SLIDE_ERR_INVALID", G.closure_info_gain, 0, [9, 5, 0], [1.0, -1.0], SIGMA)
    G.closure_info_gain(0, list(range(9, -1, -1)) * 6 + [9, 8, 7, 6, 5], [1.0] * 64, SIGMA)     # 6m = 384: the cap itself
    _raises("SLIDE_ERR_CAPACITY", G.closure_info_gain, 0, list(range(9, -1, -1)) * 6 + [9, 8, 7, 6, 5, 4], [1.0] * 65, SIGMA)
    G.chi2()
    _raises("SLIDE_ERR_INVALID", G.get_pose_covariances, 0, [1])           # chi2() clears the factorisation
    _raises("SLIDE_ERR_INVALID", G.closure_info_gain, 0, [9, 0], [2.0], SIGMA)
    assert G.gauss_newton(1) == 0
    assert G.get_pose_covariances(0, [1]).shape == (1, 6, 6)
    G.set_ghosts([0], [0])                                                 # a shard of a distributed solve
    _raises("SLIDE_ERR_INVALID", G.get_pose_covariances, 0, [1])
    _raises("SLIDE_ERR_INVALID", G.marginal_traces, 0)
    _raises("SLIDE_ERR_INVALID", G.closure_info_gain, 0, [9, 0], [2.0], SIGMA)
