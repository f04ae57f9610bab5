"""Each Gauss-Newton step of the product (slide_graph_gauss_newton(1): relinearise everything, one plain step) against an independent
least-squares solve of the same linearisation (tests/gn_reference.py: the full whitened Jacobian by QR, cross-checked against the
oracle's first solve in test_gn_reference.py), at the shapes where the assembly kernels switch code paths.

A wrong Jacobian or Schur block need not move the optimum, only the path to it: parity after N passes would not see it, one step
does.  Tolerances: gn_reference.tolerance, computed from the case (scaled condition number, numdiff noise floor, value size)."""
import numpy as np
import pytest

import gn_graphs as gg
from gn_reference import Reference, scaled_error, tolerance
from oracle import pyoracle as po
from test_gn_reference import numdiff_floor

pytestmark = pytest.mark.gpu


def gpu_values(G, ref):
    """The product's estimate in the reference's variable layout."""
    out = ref.values.copy()
    for k, key in enumerate(ref.vkey):
        c, idx = int(key) >> 56, int(key) & ((1 << 56) - 1)
        if int(ref.vtype[k]) == po.V_POSE:
            st, v = G.get_pose12("xyzmnopqrstvw".index(chr(c)), idx)
        else:
            st, v = G.get_landmark("lcu".index(chr(c)), idx)
        assert st == 0
        out[k, : len(v)] = v
    return out


def build_pair(gpu, build, chart):
    og = po.OracleGraph(po.OrcParams.default(pose_chart=chart))
    build(og)
    G = gpu.SlideGraph(gpu.default_params(pose_chart=chart))
    W = build(G)
    return Reference(og, chart), G, W


def check_steps(ref, G, steps=2, values=None):
    """`steps` plain steps of G, each against the reference rebuilt at G's point before it."""
    vals = ref.values if values is None else values
    for s in range(steps):
        dx, H = ref.step(vals)
        assert G.gauss_newton(1) == 0
        new = gpu_values(G, ref)
        got = ref.tangent(vals, new)
        tol, kappa = tolerance(H, dx, ref.magnitude(vals), numdiff_floor(ref, dx, H, vals))
        err = scaled_error(got, dx, H)
        assert err <= tol, (s, err, tol, kappa)
        vals = new
    return vals


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("n_lm", [255, 256, 257, 300])
def test_pose_list_cap(gpu, chart, n_lm):
    """k_schur keeps a column pose's landmark-factor list in LDS up to SCHUR_PJ_CAP = 256 entries and reads longer lists from global
    memory: pose 2 with 255 .. 300 landmark factors, co-observed by the other poses."""
    ref, G, _ = build_pair(gpu, lambda g: gg.pose_list_graph(g, n_lm), chart)
    per_pose, _ = ref.list_lengths()
    assert per_pose[ref.pose_var(0, 2)] == n_lm
    check_steps(ref, G)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("cls", [0, 1, 2], ids=["cyl", "cube", "point"])
@pytest.mark.parametrize("nf", [1, 24, 25, 63, 64, 65, 130])
def test_landmark_factor_count(gpu, chart, cls, nf):
    """k_landmark<0>, the landmark pass of gauss_newton's path: lane q owns factors q, q + 64, ... and the lanes' partial sums meet in
    an xor-shuffle tree.  One landmark of each size (D = 7, 9, 3) with 1 .. 130 factors: one lane, part of a wave, a full wave, two
    and three factors on a lane.  (The batched path's k_landmark_b<3>, which reduces through LDS in rounds of LM_RED_MAX = 24
    lanes, is not reached by gauss_newton and not by these cases.)"""
    ref, G, _ = build_pair(gpu, lambda g: gg.landmark_count_graph(g, cls, nf), chart)
    _, per_lm = ref.list_lengths()
    assert per_lm[ref.lm_var(cls, 0)] == nf
    check_steps(ref, G)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("P", [1, 10, 11, 32, 33, 64, 65, 150])
def test_pose_count(gpu, chart, P):
    """6P straddles the 64-wide tiles of the reduced system and the Schur strip's 32-pose chunks; k_pose gives one lane per incident
    factor."""
    ref, G, _ = build_pair(gpu, lambda g: gg.pose_count_graph(g, P), chart)
    assert int((ref.vtype == po.V_POSE).sum()) == P
    check_steps(ref, G, steps=3 if P in (33, 65) else 2)


GEOMETRY = [(k, c) for k in ("full3d", "rot3", "quat", "far", "bearing") for c in (0, 1)] + [("nearpi", 1)]


@pytest.mark.parametrize("kind,chart", GEOMETRY)
def test_geometry(gpu, kind, chart):
    """Device Lie math beyond yaw-only poses: full 3-D orientations, relative rotations of 3.0 rad and (Expmap only: Cayley is
    singular there) pi - 1e-3, quaternions with w < 0 and norm 1.7, translations about 1e4 m, bearings at sphere_basis's tie."""
    ref, G, W = build_pair(gpu, lambda g: gg.geometry_graph(g, kind), chart)
    poses = ref.values[ref.vtype == po.V_POSE]
    if kind == "full3d":         # roll and pitch: R[2, 0] = -sin(pitch), R[2, 1] = cos(pitch) sin(roll)
        assert np.abs(poses[:, 6]).max() > 0.1 and np.abs(poses[:, 7]).max() > 0.1
    if kind == "quat":           # every quaternion at the ABI has w < 0 and norm 1.7
        q = np.array(W.quats)
        assert len(q) >= 9 and (q[:, 3] < 0).all() and np.allclose(np.linalg.norm(q, axis=1), 1.7)
    if kind == "bearing":        # measured bearings along an axis and with two equal smallest |components|, at pose 0 exact
        b = np.sort(np.abs(ref.fz[ref.ftype == po.F_BR, :3]), axis=1)
        assert ((b[:, 0] == 0) & (b[:, 1] == 0)).sum() >= 2 and ((b[:, 0] == b[:, 1]) & (b[:, 0] > 0)).sum() >= 1
    if kind in ("rot3", "nearpi"):
        a = 3.0 if kind == "rot3" else np.pi - 1e-3
        z = ref.fz[ref.ftype == po.F_BETWEEN]
        ang = np.arccos(np.clip((z[:, 0] + z[:, 4] + z[:, 8] - 1) / 2, -1, 1))
        assert np.isclose(ang.max(), a, atol=1e-9)
    if kind == "far":
        assert np.abs(ref.values[ref.vtype == po.V_POSE, 9:12]).max() > 9e3
    check_steps(ref, G)


def test_list_inputs_give_the_ndarray_graph(gpu):
    """Lists at the ABI (each converted into a temporary by the binding) build the same graph as float64 ndarrays."""
    class Lists:
        def __init__(self, G):
            self.G = G

        def __getattr__(self, name):
            f = getattr(self.G, name)
            return lambda *a: f(*[x.tolist() if isinstance(x, np.ndarray) else x for x in a])
    A = gpu.SlideGraph(gpu.default_params())
    B = gpu.SlideGraph(gpu.default_params())
    gg.geometry_graph(A, "full3d")
    gg.geometry_graph(Lists(B), "full3d")
    assert A.gauss_newton(1) == 0 and B.gauss_newton(1) == 0
    for k in range(5):
        assert np.array_equal(A.get_pose12(0, k)[1], B.get_pose12(0, k)[1])
    for cls, idx in ((0, 0), (1, 0), (2, 3)):
        assert np.array_equal(A.get_landmark(cls, idx)[1], B.get_landmark(cls, idx)[1])


def _two_pose_graph(G, split, n_lm, seed=5):
    """Two exact poses; landmark l is seen from pose 0 (l < split or split < 0: every landmark from both poses) and/or pose 1; the
    landmarks' initial values are perturbed."""
    W = gg.World(G, 2, seed=seed, noise=0.0)
    rng = np.random.default_rng(seed)
    xyz = W.T[0][1] + rng.uniform([3, -20, -5], [40, 20, 5], (n_lm, 3))
    noise = rng.normal(0, 0.05, (n_lm, 3))
    for l in range(n_lm):
        G.add_point_landmark(l, xyz[l] + noise[l])
        obs = (0, 1) if split < 0 else ((0,) if l < split else (1,))
        for k in obs:
            R, t = W.T[k]
            q = R.T @ (xyz[l] - t)
            G.add_range_bearing(0, k, l, q / np.linalg.norm(q), float(np.linalg.norm(q)))
    return W


def _lds_landmarks(P):
    """k_schur's dynamic LDS (host_graph.hip, upload_new): a short per landmark, rounded up to 8, plus (P + 31) / 32 + 1 words of
    the pose bitmap, within 120 KiB.  The largest landmark count it admits."""
    words = ((P + 31) // 32 + 1) * 4
    return (120 * 1024 - words) // 2 // 8 * 8


def test_schur_lds_capacity_boundary(gpu):
    """The largest landmark count the Schur LDS check admits is solved; one tile (8 landmarks) more is refused with
    SLIDE_ERR_CAPACITY.  Each landmark is seen once (from one of two exact poses), so its least-squares step is the exact solution of
    its own 3 x 3 whitened system and the poses do not move — a reference that needs no solve of the whole graph."""
    L = _lds_landmarks(2)
    assert L == 61432
    og = po.OracleGraph(po.OrcParams.default())
    _two_pose_graph(og, L // 2, L)
    ref = Reference(og, 0)
    G = gpu.SlideGraph(gpu.default_params())
    _two_pose_graph(G, L // 2, L)
    per_pose, _ = ref.list_lengths()
    assert per_pose.max() <= 32768 and len(ref.vtype) == L + 2
    assert G.gauss_newton(1) == 0
    i, j, v, r = ref.linearize()
    new = gpu_values(G, ref)
    # per landmark: rows 3f .. 3f + 2 of its factor (the priors and the between factor come first: 6 + 6 rows)
    f_of = {int(ref.fv[f, 1]): f for f in range(len(ref.ftype)) if ref.ftype[f] == po.F_BR}
    worst, bound = 0.0, 0.0
    rows0 = 12
    J = np.zeros((len(r), 3))
    sel = j >= 12
    J[i[sel], (j[sel] - 12) % 3] = v[sel]
    for k in range(2, len(ref.vtype)):
        f = f_of[k]
        rr = slice(rows0 + 3 * (f - 2), rows0 + 3 * (f - 2) + 3)
        A = J[rr]
        dx = np.linalg.solve(A, -r[rr])
        got = new[k, :3] - ref.values[k, :3]
        worst = max(worst, np.abs(got - dx).max() / np.abs(dx).max())
        # 3 x 3 solve through the normal equations: 8 * 3 eps cond(A)^2, plus reading the step as a difference of values of size |x|
        bound = max(bound, 8 * 3 * np.finfo(float).eps * np.linalg.cond(A) ** 2
                    + 8 * np.finfo(float).eps * np.abs(ref.values[k, :3]).max() / np.abs(dx).max())
    assert worst <= bound, (worst, bound)
    for k in range(2):
        assert np.abs(new[k] - ref.values[k]).max() <= 1e-12 * max(1.0, np.abs(ref.values[k]).max())
    # one tile more
    G2 = gpu.SlideGraph(gpu.default_params())
    _two_pose_graph(G2, (L + 8) // 2, L + 8)
    with pytest.raises(gpu.SlideError, match="CAPACITY"):
        G2.gauss_newton(1)


def test_schur_slot_table_overflow(gpu):
    """k_schur's landmark -> list position table holds shorts: a position past 32767 wraps negative and that landmark's Schur terms
    were dropped without an error.  Two poses that both observe the same 32769 landmarks (one more than the longest list whose
    positions fit) are refused with SLIDE_ERR_CAPACITY, before any launch."""
    n = 32769
    G = gpu.SlideGraph(gpu.default_params())
    _two_pose_graph(G, -1, n)
    with pytest.raises(gpu.SlideError, match="CAPACITY.*32768 landmark factors"):
        G.gauss_newton(1)


@pytest.mark.parametrize("chart", [0, 1])
def test_wildfire_after_chi2(gpu, chart):
    """chi2() folds delta into theta and zeroes it; a solve after it with the wildfire bound on must not keep the previous solve's dp
    for quiet blocks (that dp was applied already).  Solve, chi2, add a key frame, solve: the same poses as with the bound off, to
    within the threshold.  And gauss_newton(1) after chi2() is the reference's step at the point chi2 left."""
    thr = 1e-3
    P = 30
    runs = []
    for wf in (0.0, thr):
        G = gpu.SlideGraph(gpu.default_params(pose_chart=chart))
        G.set_wildfire(wf)
        W = gg.World(G, P, seed=6, noise=0.0, perturb={3: [0.05, -0.03, 0.02]})
        assert G.solve() == 0
        G.chi2()
        (Ra, ta) = W.T[-1]
        rel = gg.p7(gg.rot([0, 0, 0.1]), np.array([1.0, 0.0, 0.0]))
        Rb, tb = Ra @ gg.rot([0, 0, 0.1]), ta + Ra @ np.array([1.0, 0.0, 0.0])
        G.add_keypose_between(0, P - 1, P, rel, gg.p7(Rb, tb))
        assert G.solve() == 0
        runs.append(np.array([G.get_pose12(0, k)[1] for k in range(P + 1)]))
    assert np.abs(runs[1] - runs[0]).max() <= thr, np.abs(runs[1] - runs[0]).max()
    # gauss_newton(1) after chi2()
    og = po.OracleGraph(po.OrcParams.default(pose_chart=chart))
    gg.World(og, P, seed=6, noise=0.0, perturb={3: [0.05, -0.03, 0.02]})
    ref = Reference(og, chart)
    G = gpu.SlideGraph(gpu.default_params(pose_chart=chart))
    G.set_wildfire(thr)
    gg.World(G, P, seed=6, noise=0.0, perturb={3: [0.05, -0.03, 0.02]})
    assert G.solve() == 0
    G.chi2()
    check_steps(ref, G, steps=1, values=gpu_values(G, ref))
