"""estimateClosureInfoGain on the JOINT multi-robot graph (CholBatch.closure_info_gain / PassDriver.closure_info_gain,
joint_cov_kernels.hip's k_jms_*, host side in host_marginals.hip) against the dense joint Gauss-Newton H of gn_reference, which shares no code with the kernels.

Per case: the shards of tests/test_gpu_joint_step.py's Run, H at the values read before one exact joint pass (the point the pass
linearises at), the candidate Between rows J_f from orc_linearize(F_BETWEEN, ..) at those values with (robot, index) endpoints, and the
trace drops of inv(H) -> inv(H + J_f^T J_f): the robot of the slot's poses, the job's point landmarks, every robot's poses.  Errors are
measured against max(|want|, 1e-3 trace) with test_gpu_joint_marginals.dense_inverse's tolerance, as test_gpu_marginals'
test_info_gain_vs_dense.  Every case asserts the structural edge it exists for."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_graphs as jg                                                      # noqa: E402
from oracle import pyoracle as po                                              # noqa: E402
from test_gpu_joint_marginals import dense_inverse                             # noqa: E402
from test_gpu_joint_step import NB, Run                                        # noqa: E402
from test_gpu_marginals import rel12, var_kind                                 # noqa: E402

pytestmark = pytest.mark.gpu

SIGMA = np.array([0.02, 0.02, 0.02, 0.05, 0.05, 0.05])


def ref_gain(ref, H, vals, slot, ends, travel, sigma):
    """The drops of inv(H) -> inv(H + J_f^T J_f), J_f: Between rows (ends[i+1], ends[i]), ends = (robot, index), at vals.  Returns
    (want, traces) as out4: [10 pose + landmark, pose drop of `slot`'s robot, point landmarks, poses of every robot]."""
    L = po.lib()
    Jf = np.zeros((6 * len(travel), ref.n))
    r, J0, J1 = np.zeros(9), np.zeros(81), np.zeros(81)
    for i, d in enumerate(travel):
        a, b = ref.pose_var(*ends[i + 1]), ref.pose_var(*ends[i])
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
    g = np.zeros(4)
    t = np.zeros(4)
    for k in range(len(ref.vtype)):
        kind, rob, _ = var_kind(ref, k)
        o0, o1 = ref.off[k], ref.off[k + 1]
        d0, d1 = np.trace(S0[o0:o1, o0:o1]), np.trace(S1[o0:o1, o0:o1])
        if kind == "pose":
            g[3] += d0 - d1; t[3] += d0
            if rob == slot:
                g[1] += d0 - d1; t[1] += d0
        elif int(ref.vtype[k]) == po.V_POINT:
            g[2] += d0 - d1; t[2] += d0
    g[0], t[0] = 10 * g[1] + g[2], 10 * t[1] + t[2]
    return g, t


class GainRun:
    """One Run, H and the tolerance at the values the pass linearises at, then one exact joint pass."""

    def __init__(self, gpu, J, chart=0, evidence=None):
        import torch
        self.r = Run(gpu, J, chart)
        if evidence is not None:
            evidence(self.r)
        self.vals = self.r.values()
        _, self.H = self.r.ref.step(self.vals)
        _, _, self.tol, self.kappa = dense_inverse(self.r.ref, self.vals)
        self.r.drv.one_pass()
        torch.cuda.synchronize()
        if evidence is not None:
            evidence(self.r)

    def check(self, slot, ends, travel=None, sigma=SIGMA):
        """The query against the dense reference; ends = [(robot, index)]."""
        travel = [4.0 + i for i in range(len(ends) - 1)] if travel is None else travel
        idx = [e[1] for e in ends]
        slots = [e[0] for e in ends] if any(e[0] != slot for e in ends) else None
        got = self.r.batch.closure_info_gain(slot, idx, travel, sigma, slots)
        want, traces = ref_gain(self.r.ref, self.H, self.vals, slot, ends, travel, sigma)
        assert want[1] > 0 and want[2] >= 0 and want[3] >= want[1]
        err = np.abs(got - want) / np.maximum(np.abs(want), 1e-3 * traces)
        assert (err <= max(self.tol, 1e-12)).all(), (got, want, err, self.tol, self.kappa)
        print(f"[joint-info-gain] worst {err.max():.3e} (tol {self.tol:.2e}, kappa {self.kappa:.2e})")
        return got

    def close(self):
        self.r.close()


def run_gain(gpu, J, queries, chart=0, evidence=None):
    g = GainRun(gpu, J, chart, evidence)
    try:
        for slot, ends in queries:
            g.check(slot, ends)
    finally:
        g.close()


def chain(robot, idx):
    return [(robot, i) for i in idx]


# ---- the structural cases of the pass ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [2, 4])
def test_shared_mix(gpu, R):
    J = jg.shared_mix_case(R)
    P = J.sizes[0]

    def ev(r):
        assert r.info["n_slots"] > 0 and r.drv.arrow
    run_gain(gpu, J, [(0, chain(0, [P - 1, 0])), (R - 1, chain(R - 1, [J.sizes[R - 1] - 2, J.sizes[R - 1] // 2, 3, 1]))], 0, ev)


@pytest.mark.parametrize("coords", [64, 129])
def test_border_rows(gpu, coords):
    """Robot 0's border of 64 / 129 coordinates (one tile, past two tiles) from cylinders, cubes and points."""
    J = jg.border_case({64: (1, 5, 4), 129: (3, 10, 6)}[coords])

    def ev(r):
        assert r.info["sep_dim"] == coords
    run_gain(gpu, J, [(0, chain(0, [J.sizes[0] - 1, 0])), (1, chain(1, [J.sizes[1] - 1, 12, 2, 0]))], 0, ev)


@pytest.mark.parametrize("seg", [None, "1", "2", "4"], ids=["default3", "1", "2", "4"])
def test_segments(gpu, monkeypatch, seg):
    """Bands cut into SLIDE_SEGMENTS segments: 65 consecutive poses across the cuts, so the trajectory holds window poses (their rows
    are border rows) and poses of two segments; m = 64 is the cap."""
    if seg is None:
        monkeypatch.delenv("SLIDE_SEGMENTS", raising=False)
    else:
        monkeypatch.setenv("SLIDE_SEGMENTS", seg)
    n = 3 if seg is None else int(seg)
    J = jg.segments_case()

    def ev(r):
        for sh in r.shards:
            segs, nwin = sh.graph.segments()
            assert (segs == []) if n == 1 else (len(segs) == n and nwin > 0), (segs, nwin)
    P = J.sizes[0]
    lo = P // 4
    run_gain(gpu, J, [(0, chain(0, range(lo, lo + 65))), (1, chain(1, [P - 1, P // 2, 0]))], 0, ev)


def test_separator_tiles(gpu):
    """Dissected separator: each leaf and the top block past one tile (the leaves' columns side by side)."""
    J = jg.separator_tiles_case()

    def ev(r):
        Ta, Tb, used_a, used_b = r.info["sep_prof"][1]
        top = r.info["sep_dim"] - NB * (Ta + Tb)
        assert used_a > NB and used_b > NB and top > NB, (Ta, Tb, used_a, used_b, top)
    run_gain(gpu, J, [(0, chain(0, [J.sizes[0] - 1, 0])), (1, chain(1, [J.sizes[1] - 1, J.sizes[1] // 2, 1, 0]))], 0, ev)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("R,n_rel", [(2, 3), (4, 11)], ids=["2x3", "4x11"])
def test_relative_pose_factors(gpu, R, n_rel, chart):
    """The lambda block (D = -I) of 18 / 66 coordinates, under both charts; an inter-robot candidate as well."""
    J = jg.relmeas_case(R, n_rel)

    def ev(r):
        assert r.drv.lam_dim == 6 * n_rel
    P0, P1 = J.sizes[0], J.sizes[1]
    run_gain(gpu, J, [(0, chain(0, [P0 - 1, 0])), (1, [(1, P1 - 1), (0, P0 // 2), (1, 2), (1, 0)])], chart, ev)


@pytest.mark.parametrize("shared", [False, True], ids=["private", "shared"])
def test_landmark_count_points(gpu, shared):
    """One point landmark seen from 25 poses: private (V through its robot's U) or shared (the separator's rows of U)."""
    J = jg.landmark_count_case(2, 25, shared=shared)

    def ev(r):
        g = int(r.gid[0][2][0])
        assert (g in {int(x) for x in r.gid[1][2]}) == shared
    run_gain(gpu, J, [(0, chain(0, [J.sizes[0] - 1, 0])), (0, chain(0, [20, 10, 3, 0]))], 0, ev)


def test_sizes_empty_border(gpu):
    """Robots of unequal sizes, one with an empty border (no rows of separator coordinates)."""
    J = jg.sizes_case([20, 45, 9], private_only=(2,))
    run_gain(gpu, J, [(2, chain(2, [8, 0])), (1, chain(1, [44, 30, 10, 0])), (0, [(0, 19), (2, 4)])])


# ---- properties ------------------------------------------------------------------------------------------------------------------

def test_inter_robot_and_properties(gpu):
    """A rendezvous between robots 0 and 1 (out4[3] covers both), far > near, the pose drop within marginal_traces' sum, the default
    sigma = the slot graph's odometry noise, repeated queries bit-identical."""
    J = jg.shared_mix_case(2)
    g = GainRun(gpu, J)
    try:
        P0, P1 = J.sizes[0], J.sizes[1]
        rv = g.check(0, [(1, P1 - 1), (0, P0 - 1)])
        assert rv[3] > rv[1] > 0
        b = g.r.batch
        assert np.array_equal(rv, b.closure_info_gain(0, [P1 - 1, P0 - 1], [4.0], SIGMA, [1, 0]))
        near = b.closure_info_gain(0, [1, 0], [4.0], SIGMA)
        far = b.closure_info_gain(0, [P0 - 1, 0], [4.0], SIGMA)
        assert far[0] > near[0] > 0
        assert far[1] <= g.r.batch.marginal_traces(0)[0]
        d1 = b.closure_info_gain(0, [P0 - 1, 0], [5.0])          # (the shards' graphs run on default_params)
        assert np.array_equal(d1, b.closure_info_gain(0, [P0 - 1, 0], [5.0], list(gpu.default_params().noise_model_odom_vec)))
        assert d1[0] > 0
        assert np.array_equal(g.r.drv.closure_info_gain(0, [P0 - 1, 0], [4.0], SIGMA), far)
    finally:
        g.close()


# ---- the pass and the cached Sigma are untouched; status paths -------------------------------------------------------------------

@pytest.mark.parametrize("case", ["relmeas", "segments"])
def test_queries_leave_the_pass_and_sigma(gpu, case):
    """Pose covariances read the same bits before and after gain queries; a pass after them gives the same bits as one without."""
    import torch
    J = jg.relmeas_case(2, 3) if case == "relmeas" else jg.segments_case()
    g = GainRun(gpu, J)
    try:
        r = g.r
        cov0 = r.batch.get_pose_covariances(0, np.arange(J.sizes[0]))
        g.check(0, chain(0, [J.sizes[0] - 1, 0]))
        n1 = min(J.sizes[1], 65)
        long1 = r.batch.closure_info_gain(1, list(range(n1)), [1.0] * (n1 - 1), SIGMA)
        assert np.array_equal(long1, r.batch.closure_info_gain(1, list(range(n1)), [1.0] * (n1 - 1), SIGMA))      # (bit for bit)
        assert np.array_equal(cov0, r.batch.get_pose_covariances(0, np.arange(J.sizes[0])))
        r.drv.one_pass()
        torch.cuda.synchronize()
        with_q = r.values()
    finally:
        g.close()
    r2 = Run(gpu, J, 0)
    try:
        r2.drv.one_pass()
        r2.drv.one_pass()
        torch.cuda.synchronize()
        assert np.array_equal(with_q, r2.values())
    finally:
        r2.close()


def test_status_paths(gpu):
    import torch
    from slide_slam_amd.api import SlideError
    J = jg.shared_mix_case(2, sizes=[70, 66])          # (room for m = 65 steps)
    P = J.sizes[0]
    r = Run(gpu, J, 0)
    try:
        with pytest.raises(SlideError, match="no whole exact joint pass"):
            r.batch.closure_info_gain(0, [1, 0], [1.0])
        r.drv.one_pass()
        torch.cuda.synchronize()
        assert r.batch.closure_info_gain(0, [1, 0], [1.0])[0] > 0
        with pytest.raises(KeyError):
            r.batch.closure_info_gain(0, [P + 5, 0], [1.0])
        with pytest.raises(KeyError):
            r.batch.closure_info_gain(0, [J.sizes[1] + 5, 0], [1.0], None, [1, 0])
        with pytest.raises(SlideError):
            r.batch.closure_info_gain(0, [1], [])
        with pytest.raises(SlideError):
            r.batch.closure_info_gain(0, [1, 0], [0.0])
        with pytest.raises(SlideError):
            r.batch.closure_info_gain(0, [1, 0], [-1.0])
        with pytest.raises(SlideError):
            r.batch.closure_info_gain(0, [1, 0], [float("nan")])
        with pytest.raises(SlideError):
            r.batch.closure_info_gain(0, [1, 0], [1.0], [0.1, 0.1, 0.0, 0.1, 0.1, 0.1])
        assert r.batch.closure_info_gain(0, list(range(65)), [1.0] * 64)[0] > 0            # (m = 64: the cap)
        with pytest.raises(SlideError, match="MAX_STEPS"):                                     # (SLIDE_ERR_CAPACITY)
            r.batch.closure_info_gain(0, list(range(66)), [1.0] * 65)
        g = r.shards[0].graph
        st, v = g.get_pose12(0, P - 1)
        rel = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
        est = np.concatenate([v[9:12] + np.array([1.0, 0.0, 0.0]), [0.0, 0.0, 0.0, 1.0]])
        g.add_keypose_between(0, P - 1, P, rel, est)
        with pytest.raises(SlideError, match="changed since the last exact joint pass"):
            r.batch.closure_info_gain(0, [1, 0], [1.0])
    finally:
        r.close()
    rp = Run(gpu, J, 0, pcg_iters=20, pcg_tol=1e-10)
    try:
        rp.drv.one_pass()
        torch.cuda.synchronize()
        with pytest.raises(SlideError, match="does not run exact joint passes"):
            rp.batch.closure_info_gain(0, [1, 0], [1.0])
        with pytest.raises(ValueError):
            rp.drv.closure_info_gain(0, [1, 0], [1.0])
    finally:
        rp.close()
    r1 = Run(gpu, J, 0)
    try:
        r1.drv.one_pass()
        torch.cuda.synchronize()
        r1.drv.world = 2
        with pytest.raises(ValueError):
            r1.drv.closure_info_gain(0, [1, 0], [1.0])
    finally:
        r1.drv.world = 1
        r1.close()
