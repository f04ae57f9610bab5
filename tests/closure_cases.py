"""Loop-closure consistency (slide_closure_consistency_csr / slide_select_consistent_closures / slide_graph_select_closures): a numpy
restatement of the invariant and the score, written from the formulas of include/slide_gpu.h and not from the kernel, and the case
generators (test infrastructure for test_closure_select.py and test_gpu_closure_select.py; not a test).

The restatement: closure k measures z_k = X(from_k)^-1 X(to_k); with F_k = X(from_k), T_k = X(to_k)
    e_ij = Log(z_i T_i^-1 T_j z_j^-1 F_j^-1 F_i)                     tangent order [rot(3), trans(3)]
    s2[c] = sigma_i[c]^2 + sigma_j[c]^2 + (|from_idx_i - from_idx_j| + |to_idx_i - to_idx_j|) odom_sigma[c]^2
    d = sqrt(sum_c e[c]^2 / s2[c]),   score = exp(-0.5 d^2 / sigma^2) if d < gate else 0, kept if > affinityeps.
Log: theta = atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2), w = theta / (2 sin theta) vee(R - R^T), u = V(w)^-1 t with
V^-1 = I - W / 2 + (1 - theta / (2 tan(theta / 2))) / theta^2 W^2 — every operation elementwise numpy, so the same text runs in
float64 and in np.longdouble (the measured tolerance of the GPU test).

Every generator asserts on its own output: no pair has |d - gate| < 1e-6 gate, no kept score lies within 1e-6 of affinityeps, and (the
planted cases) the oracle's orc_clipper_solve on the restatement's matrix selects exactly the planted true set — so rounding cannot
flip the pattern and the heuristic solver cannot excuse a miss."""
from __future__ import annotations

import ctypes as C

import numpy as np

GATE = 4.1
SIGMA = GATE / 2
AFFINITYEPS = 1e-4
CLOSURE_SIGMA6 = np.array([0.01] * 3 + [0.05] * 3)       # rad, m
ODOM_SIGMA6 = np.array([0.004] * 3 + [0.02] * 3)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _pose(p7, dt):
    p = np.asarray(p7, dt)
    x, y, z, w = p[3:] / np.sqrt((p[3:] * p[3:]).sum())
    one, two = dt(1), dt(2)
    R = np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                  [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                  [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dt)
    return R, p[:3].copy()


def _mul(A, B):
    return A[0] @ B[0], A[0] @ B[1] + A[1]


def _inv(A):
    return A[0].T, -(A[0].T @ A[1])


def _log(A, dt):
    R, t = A
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dt)
    s = np.sqrt((v * v).sum()) / dt(2)
    c = (R[0, 0] + R[1, 1] + R[2, 2] - dt(1)) / dt(2)
    th = np.arctan2(s, c)
    if th < dt(1e-7):                       # first order: w = vee / 2, V^-1 = I
        return np.concatenate([v / dt(2), t])
    w = th / (dt(2) * s) * v
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dt)
    k = (dt(1) - th / (dt(2) * np.tan(th / dt(2)))) / (th * th)
    return np.concatenate([w, t - (W @ t) / dt(2) + k * (W @ (W @ t))])


def restate(from_pose7, to_pose7, rel7, sigma6, from_idx, to_idx, gate=GATE, sigma=SIGMA, affinityeps=AFFINITYEPS, odom_sigma6=ODOM_SIGMA6,
            dtype=np.float64, smaller_first=True):
    """(d, M): the pairwise distances and the score matrix (zero diagonal) of one group, both L x L.  smaller_first: entry (i, j) is
    evaluated with min(i, j) as i (the rule of the library); False evaluates it as written, row index first."""
    dt = dtype
    L = len(rel7)
    F = [_pose(p, dt) for p in from_pose7]
    T = [_pose(p, dt) for p in to_pose7]
    Z = [_pose(p, dt) for p in rel7]
    sg2 = np.asarray(sigma6, dt).reshape(L, 6) ** 2
    od2 = np.asarray(odom_sigma6, dt) ** 2
    d = np.zeros((L, L), dt)
    M = np.zeros((L, L), dt)
    for a in range(L):
        for b in range(L):
            if a == b:
                continue
            i, j = (min(a, b), max(a, b)) if smaller_first else (a, b)
            E = _mul(_mul(_mul(_mul(_mul(Z[i], _inv(T[i])), T[j]), _inv(Z[j])), _inv(F[j])), F[i])
            e = _log(E, dt)
            legs = dt(abs(int(from_idx[i]) - int(from_idx[j])) + abs(int(to_idx[i]) - int(to_idx[j])))
            s2 = sg2[i] + sg2[j] + legs * od2
            d[a, b] = np.sqrt((e * e / s2).sum())
            sc = np.exp(dt(-0.5) * d[a, b] * d[a, b] / (dt(sigma) * dt(sigma))) if d[a, b] < dt(gate) else dt(0)
            M[a, b] = sc if sc > dt(affinityeps) else dt(0)
    return d, M


def dense_to_csr(S):
    S = np.asarray(S, np.float64)
    mask = S != 0
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    r, c = np.nonzero(mask)
    return rowptr, c.astype(np.int32), S[r, c]


def csr_to_dense(rowptr, col, val):
    n = len(rowptr) - 1
    S = np.zeros((n, n))
    for i in range(n):
        S[i, col[rowptr[i]:rowptr[i + 1]]] = val[rowptr[i]:rowptr[i + 1]]
    return S


def oracle_select(M, seed=7):
    """orc_clipper_solve (the oracle's CLIPPER, DSD_HEU rounding) on a symmetric score matrix: the sorted selected nodes."""
    from oracle import pyoracle as po
    n = len(M)
    Mup = np.ascontiguousarray(np.triu(np.asarray(M, np.float64), 1))
    u0 = np.ascontiguousarray(np.random.default_rng(seed).uniform(0.0, 1.0, n))
    nodes = np.zeros(n, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    k = po.lib().orc_clipper_solve(P(Mup), C.c_int(n), P(u0), None, P(nodes), None, None)
    return sorted(nodes[:k].tolist())


# ---- generators -------------------------------------------------------------------------------------------------------------------
def _rotvec(w):
    w = np.asarray(w, float)
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * (W @ W)


def _quat(R):
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(R).as_quat()
    return q if q[3] >= 0 else -q


def p7(A):
    return np.concatenate([A[1], _quat(A[0])])


PERIOD = 30


def random_walk(N, rng, start=None):
    """N ground-truth poses around a loop of PERIOD poses: steps of about 1 m, a turn of 2 pi / PERIOD about z plus about 0.02 rad of
    wobble — pose k + PERIOD comes back to within a few metres of pose k, where a loop closure is found."""
    A = start if start is not None else (_rotvec([0.1, -0.2, 0.3]), np.array([1.0, 2.0, 0.5]))
    out = [A]
    for _ in range(N - 1):
        A = _mul(A, (_rotvec(np.array([0, 0, 2 * np.pi / PERIOD]) + rng.normal(0, 0.02, 3)), np.array([1.0, 0.1 * rng.normal(), 0.05 * rng.normal()])))
        out.append(A)
    return out


def drift(truth, rng, scale=1.0, world=None):
    """The estimate of a chain: its first pose (moved into `world`, any frame), then the true steps, each times odometry noise of
    scale x ODOM_SIGMA6."""
    A = truth[0] if world is None else _mul(world, truth[0])
    out = [A]
    for k in range(1, len(truth)):
        step = _mul(_inv(truth[k - 1]), truth[k])
        A = _mul(A, _mul(step, (_rotvec(scale * rng.normal(0, 1, 3) * ODOM_SIGMA6[:3]), scale * rng.normal(0, 1, 3) * ODOM_SIGMA6[3:])))
        out.append(A)
    return out


def measure(A, B, rng, false=False, scale=1.0):
    """A^-1 B times a small noise (scale x the closure's sigmas), or, false, times a rotation of about 0.3 rad and a translation of
    about 3 m."""
    if false:
        ax, tr = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
        N = (_rotvec(0.3 * ax / np.linalg.norm(ax)), 3.0 * tr / np.linalg.norm(tr))
    else:
        N = (_rotvec(scale * rng.normal(0, 1, 3) * CLOSURE_SIGMA6[:3]), scale * rng.normal(0, 1, 3) * CLOSURE_SIGMA6[3:])
    return _mul(_mul(_inv(A), B), N)


def _ends(N, rng):
    """a late pose and the early pose it comes back to (one loop earlier, give or take a pose)"""
    i = int(rng.integers(PERIOD, N))
    return i, max(i - PERIOD + int(rng.integers(-1, 2)), 0)


class Case:
    """One group's closures with the poses of their endpoints: closures (tuples for the library), from_pose7 / to_pose7 / rel7 / sigma6
    / from_idx / to_idx arrays, truth (bool per closure) and the restatement's d / M."""

    def __init__(self, rows, truth, robots=(0, 0), restated=True):
        self.robots = robots
        self.from_idx = np.array([r[0] for r in rows], np.uint64)
        self.to_idx = np.array([r[1] for r in rows], np.uint64)
        self.from_pose7 = np.array([p7(r[2]) for r in rows]).reshape(-1, 7)
        self.to_pose7 = np.array([p7(r[3]) for r in rows]).reshape(-1, 7)
        self.rel7 = np.array([p7(r[4]) for r in rows]).reshape(-1, 7)
        self.sigma6 = np.tile(CLOSURE_SIGMA6, (len(rows), 1))
        self.truth = np.array(truth, bool)
        if restated:          # (a large case skips the O(L^2) restatement: it is compared against the library's own single-problem route)
            self.d, self.M = restate(*self.arrays())
            self.self_check()

    def __len__(self):
        return len(self.rel7)

    def arrays(self):
        return self.from_pose7, self.to_pose7, self.rel7, self.sigma6, self.from_idx, self.to_idx

    def closures(self, robots=None):
        a, b = robots or self.robots
        return [(a, int(self.from_idx[k]), b, int(self.to_idx[k]), self.rel7[k], self.sigma6[k]) for k in range(len(self))]

    def self_check(self):
        off = ~np.eye(len(self), dtype=bool)
        assert not np.any(np.abs(self.d[off] - GATE) < 1e-6 * GATE)
        kept = self.M[self.M != 0]
        assert not np.any(np.abs(kept - AFFINITYEPS) < 1e-6)


# The planted cases draw their noise at PLANTED_SCALE x the sigmas the closures and the odometry state.  The clique solver rounds to
# round(F) closures (DSD_HEU), F = 1 + (k - 1) x the mean score inside a k-clique, so it returns ALL k planted closures only while
# their mean score stays above 1 - 1 / (2 (k - 1)): 0.93 for k = 8, that is d below about 0.8 at sigma = gate / 2.  Noise at the full
# stated sigmas gives d^2 around 6 (chi-square, 6 degrees of freedom), scores around 0.5 and a selected set of about half the true one;
# such closures pass the gate but are not all returned.  DESIGN.md 7 says so.
PLANTED_SCALE = 0.15


def planted_case(seed, N=60, n_true=8, n_false=4, inter=False, check_oracle=True, restated=True):
    """A looping random-walk chain of N poses and a drifted estimate of it; closures from late poses (from) to the early poses they
    revisit (to) — n_true of the true relative pose times a small noise, n_false of it times a gross error, shuffled.  inter: the early
    poses belong to a second robot on the same loop whose estimate lives in an unrelated world frame (closures robot 0 -> robot 1)."""
    rng = np.random.default_rng(seed)
    truth = random_walk(N, rng)
    est = drift(truth, rng, PLANTED_SCALE)
    other, oest = truth, est
    if inter:
        other = random_walk(N, rng, start=truth[0])
        oest = drift(other, rng, PLANTED_SCALE, world=(_rotvec([0.7, -1.1, 2.0]), np.array([-40.0, 25.0, 3.0])))
    flags = np.array([True] * n_true + [False] * n_false)
    rng.shuffle(flags)
    rows = []
    for ok in flags:
        i, j = _ends(N, rng)
        rows.append((i, j, est[i], oest[j], measure(truth[i], other[j], rng, false=not ok, scale=PLANTED_SCALE)))
    case = Case(rows, flags, robots=(0, 1) if inter else (0, 0), restated=restated)
    assert len(case) == n_true + n_false
    if check_oracle and restated:
        assert oracle_select(case.M) == np.nonzero(flags)[0].tolist()
    return case


def csr_case(L, seed=11, inter=False):
    """L closures for the CSR checks, noise at the full stated sigmas (distances on both sides of the gate): closure 0 is a false one,
    closure L - 1 its exact duplicate (d at rounding level, score 1) and — asserted for L = 65 — its only partner, in the last
    column; closure 2 shares both endpoints with closure 1 (zero odometry legs); every fourth other closure is false.  inter: the
    to-poses belong to a second robot in an unrelated world frame."""
    rng = np.random.default_rng(seed + L)
    N = 60
    truth = random_walk(N, rng)
    est = drift(truth, rng)
    other, oest = truth, est
    if inter:
        other = random_walk(N, rng, start=truth[0])
        oest = drift(other, rng, world=(_rotvec([-2.0, 0.4, 0.9]), np.array([300.0, -120.0, 8.0])))
    rows, flags = [], []
    for k in range(L):
        ok = k != 0 and k % 4 != 3
        i, j = _ends(N, rng)
        if k == 2:
            i, j = rows[1][0], rows[1][1]
        rows.append((i, j, est[i], oest[j], measure(truth[i], other[j], rng, false=not ok)))
        flags.append(ok)
    if L >= 2:
        rows[L - 1] = rows[0]
        flags[L - 1] = False
    case = Case(rows, flags, robots=(0, 1) if inter else (0, 0))
    if L >= 2:
        assert case.M[0, L - 1] == 1.0 and case.d[0, L - 1] < 1e-9
    if L >= 4:
        assert case.from_idx[1] == case.from_idx[2] and case.to_idx[1] == case.to_idx[2]
    if L == 65:
        assert np.nonzero(case.M[0])[0].tolist() == [64]
    return case


CSR_SHAPES = (1, 2, 4, 5, 63, 64, 65)


def precision_spread(cases):
    """The largest relative difference between the restatement in float64 and in np.longdouble over the non-zero scores of the cases:
    what the choice of acos / exp / sqrt implementation and the rounding of the SE(3) products can move a value by."""
    worst = 0.0
    for c in cases:
        if len(c) < 2:
            continue
        _, Ml = restate(*c.arrays(), dtype=np.longdouble)
        nz = c.M != 0
        assert np.array_equal(nz, Ml != 0)
        if nz.any():
            worst = max(worst, float(np.max(np.abs(c.M[nz] - Ml[nz]) / np.abs(Ml[nz]))))
    return worst
