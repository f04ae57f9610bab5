"""The Mahalanobis gate of loop closures and the joint marginal of pose pairs on the JOINT multi-robot graph
(slide_chol_batch_closure_mahalanobis / slide_chol_batch_get_pose_pair_covariances): the dense reference and the list generators (test
infrastructure for test_joint_closure_gate.py and test_gpu_joint_closure_gate.py; not a test).

The reference side is the single-graph gate's (tests/closure_gate_cases.py: measured, ref_gate's arithmetic, gate_bound) on the joint
graph of tests/joint_graphs.py: Sigma the dense inverse of the joint Gauss-Newton H at the values before the pass
(test_gpu_joint_marginals.dense_inverse, with its Jacobi weights, `tol` and `kappa`), r and A from the oracle's
orc_linearize(F_BETWEEN, ..) at the poses a caller passes in, C_ref = I + A Sigma_pair A^T and d2_ref in numpy.  Poses are named
(robot, index) as the joint reference names them; robot r's graph sits in slot r of the batch, so the same tuples go to the device.
Everything here runs without a device: the estimate a generator needs on the CPU is the reference's own joint Gauss-Newton step."""
from __future__ import annotations

import numpy as np

import closure_cases as cc
import closure_gate_cases as gc
from test_gpu_joint_marginals import dense_inverse
from test_joint_reference import joint_reference

GATE2 = gc.GATE2
SIGMA6 = gc.SIGMA6


class JointGateCase:
    """One Joint under one chart: the reference; at() fixes the linearisation point (default: the reference's initial values, the
    point the first pass linearises at) and with it H's inverse, the Jacobi weights, tol, kappa and the reference's own one-step
    estimate.  Has what closure_gate_cases.ref_gate and gate_bound read of a GateCase."""

    def __init__(self, J, chart, ref=None, vals=None):
        self.J, self.chart = J, chart
        self.ref = ref if ref is not None else joint_reference(J, chart)[0]
        self.at(self.ref.values if vals is None else vals)

    def at(self, vals):
        self.vals = vals
        self.Sig, self.w, self.tol, self.kappa = dense_inverse(self.ref, vals)
        self.scale = float(np.abs(self.Sig * np.outer(self.w, self.w)).max())
        dx, _ = self.ref.step(vals)
        self.est = self.ref.retract(vals, dx)
        return self

    def off(self, robot, idx):
        return int(self.ref.off[self.ref.pose_var(robot, idx)])

    def cpu_pose12(self, robot, idx):
        return np.ascontiguousarray(self.est[self.ref.pose_var(robot, idx)][:12])

    def pair_sigma(self, ra, ia, rb, ib):
        """(12 x 12 joint marginal of the reference, the Jacobi weights of its twelve coordinates)"""
        sel = np.concatenate([np.arange(6) + self.off(ra, ia), np.arange(6) + self.off(rb, ib)])
        return self.Sig[np.ix_(sel, sel)], self.w[sel]

    def cross_ratio(self, ra, ia, rb, ib):
        """|Sab| / sqrt(|Saa| |Sbb|) of the Jacobi-scaled reference block (Frobenius norms)"""
        S, w = self.pair_sigma(ra, ia, rb, ib)
        S = S * np.outer(w, w)
        n = np.linalg.norm
        return float(n(S[:6, 6:]) / np.sqrt(n(S[:6, :6]) * n(S[6:, 6:])))


# ---- the lists ------------------------------------------------------------------------------------------------------------------------
def pair_list(J):
    """Pairs inside one robot (first with last, neighbours, both orders) and across robots (both orders; the last robot too)."""
    P, Z = J.sizes, J.R - 1
    out = [(0, 0, 0, P[0] - 1), (0, P[0] - 1, 0, 0), (0, 4, 0, 5), (1, P[1] - 1, 1, 1),
           (0, 1, 1, 2), (1, 2, 0, 1), (0, P[0] // 2, Z, P[Z] - 1), (Z, P[Z] - 1, 0, P[0] // 2), (Z, 3, 0, 5), (1, 6, 0, 7)]
    return out


def end_list(J):
    """Closure ends (from_robot, from_idx, to_robot, to_idx): inside one robot and across robots, both senses."""
    P, Z = J.sizes, J.R - 1
    return [(0, P[0] - 1, 0, 1), (1, 2, 1, P[1] - 2), (0, P[0] - 1, 1, 3), (1, 3, 0, P[0] - 1), (Z, P[Z] // 2, 0, 3), (0, 5, Z, 6)]


def inter(rows):
    return [x for x in rows if x[0] != x[2]]


def perturbed_list(J, pose12, seed=3):
    """closure_gate_cases.perturbed_list over end_list(J): per pair of ends three closures measured at the estimate's own relative pose
    times a fixed-seed tangent vector of 0.5 x, 2 x and 10 x the closure's stated sigmas, the sigmas varied per closure."""
    rng = np.random.default_rng(seed)
    out = []
    for e in end_list(J):
        for sc in gc.SCALES:
            sg = SIGMA6 * rng.uniform(0.5, 4.0, 6)
            u = rng.normal(0, 1, 6)
            out.append(gc.measured(pose12, *e, sc * sg * u / np.linalg.norm(u) * np.sqrt(6.0), sg))
    return out


FALSE_ROT, FALSE_TRANS = 0.6, 20.0      # rad, m: a false closure's displacement from the true relative pose


def displaced(A, B, rng):
    """A^-1 B times a rotation of FALSE_ROT about a random axis and a translation of FALSE_TRANS in a random direction.  The joint
    marginal of two robots' poses tied only through shared landmarks is metres wide in these cases (cond(C_ref) reaches 10^3 at the
    closures' sigmas), so closure_cases.measure's 3 m stay inside the gate; 20 m do not."""
    ax, tr = rng.normal(0, 1, 3), rng.normal(0, 1, 3)
    N = (cc._rotvec(FALSE_ROT * ax / np.linalg.norm(ax)), FALSE_TRANS * tr / np.linalg.norm(tr))
    return cc._mul(cc._mul(cc._inv(A), B), N)


def planted_list(c, pose12=None, seed=1, n_true=6, n_false=4):
    """Inter-robot closures, robot a -> robot b != a: true ones measure the GROUND TRUTH's relative pose (Joint.T) times noise drawn at
    their stated sigmas, false ones the true relative pose displaced by 0.6 rad and 20 m (displaced).  Asserted here, under d2_ref
    alone: every true one lies below 16.81 / 2, every false one above 4 x 16.81.  Returns (closures, truth flags, d2_ref)."""
    J = c.J
    rng = np.random.default_rng(seed)
    flags = np.array([True] * n_true + [False] * n_false)
    rng.shuffle(flags)
    out = []
    for ok in flags:
        a = int(rng.integers(J.R))
        b = (a + 1 + int(rng.integers(J.R - 1))) % J.R
        i, j = int(rng.integers(1, J.sizes[a])), int(rng.integers(1, J.sizes[b]))
        z = cc.measure(J.T(a, i), J.T(b, j), rng) if ok else displaced(J.T(a, i), J.T(b, j), rng)
        out.append((a, i, b, j, cc.p7(z), SIGMA6.copy()))
    _, _, _, d2 = gc.ref_gate(c, out, pose12 or c.cpu_pose12)
    assert d2[flags].max() < GATE2 / 2 and d2[~flags].min() > 4 * GATE2, (d2[flags].max(), d2[~flags].min())
    return out, flags, d2


def random_ends(J, n, rng):
    """n pairs of distinct poses, about half of them across robots"""
    out = []
    while len(out) < n:
        a, b = int(rng.integers(J.R)), int(rng.integers(J.R))
        i, j = int(rng.integers(J.sizes[a])), int(rng.integers(J.sizes[b]))
        if (a, i) != (b, j):
            out.append((a, i, b, j))
    return out


def long_closure_list(J, pose12, seed=9):
    """65 closures (a second sweep of one) with two exact duplicates, two candidates sharing a pose, and one whose from is another's to"""
    rng = np.random.default_rng(seed)
    ends = random_ends(J, 61, rng)
    a, i = ends[3][0], ends[3][1]
    ends += [ends[0], ends[7], (a, i, a, (i + 1) % J.sizes[a]), (ends[5][2], ends[5][3], ends[5][0], ends[5][1])]
    out = [gc.measured(pose12, *e, rng.normal(0, 1, 6) * SIGMA6 * 2, SIGMA6 * rng.uniform(0.5, 2.0, 6)) for e in ends]
    out[61], out[62] = out[0], out[7]
    assert len(out) == 65
    return out


def long_pair_list(J, seed=10):
    """33 pairs (a second sweep of one) with a duplicate, a swapped twin and two pairs sharing a pose"""
    rng = np.random.default_rng(seed)
    pairs = random_ends(J, 30, rng)
    a, i = pairs[2][0], pairs[2][1]
    pairs += [pairs[0], (pairs[4][2], pairs[4][3], pairs[4][0], pairs[4][1]), (a, i, a, (i + 1) % J.sizes[a])]
    assert len(pairs) == 33
    return pairs
