"""Marginal covariances on the JOINT multi-robot graph (CholBatch.get_pose_covariances / get_landmark_covariances / marginal_traces,
joint_cov_kernels.hip, host side in host_marginals.hip) against the dense inverse of the joint Gauss-Newton H of gn_reference (the full whitened Jacobian of one graph
holding every robot, tests/joint_graphs.py), which shares no code with the kernels.

Per case: the shards of tests/test_gpu_joint_step.py's Run, one exact joint pass, then every pose of every robot and every landmark of
every shard, Jacobi-scaled against inv(H) at the point the pass linearised, with test_gpu_marginals.dense_inverse's tolerance
(8 n eps kappa, plus the central-difference floor for cubes and cylinders).  A shared landmark must read the same bits from every
replica's slot; marginal_traces must equal the sums of the dense blocks.  Every case asserts the edge it exists for."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_graphs as jg                                                      # noqa: E402
from gn_reference import EPS                                                   # noqa: E402
from oracle import pyoracle as po                                              # noqa: E402
from test_gpu_joint_step import NB, Run                                        # noqa: E402

pytestmark = pytest.mark.gpu


def dense_inverse(ref, vals):
    """inv(H) at vals, its Jacobi scaling w and the tolerance of a scaled entry relative to max |W inv(H) W| (as test_gpu_marginals)."""
    _, H = ref.step(vals)
    w = np.sqrt(np.diag(H))
    kappa = float(np.linalg.cond(H / np.outer(w, w)))
    Sig = np.linalg.inv(H)
    nd = 0.0
    if np.isin(ref.ftype, (po.F_CUBE, po.F_CYL)).any():
        _, H2 = ref.step(vals, delta=1.00001e-6)
        nd = float(np.abs((np.linalg.inv(H2) - Sig) * np.outer(w, w)).max() / np.abs(Sig * np.outer(w, w)).max())
    return Sig, w, 8 * H.shape[0] * EPS * kappa + 10 * nd, kappa


def query_all(r):
    """{reference variable: block} for every pose of every robot and every landmark of every shard (shared ones: every replica)."""
    J, ref = r.J, r.ref
    out = {}
    for rr in range(J.R):
        blocks = r.drv.get_pose_covariances(rr, np.arange(J.sizes[rr]))
        for k, b in enumerate(blocks):
            out[ref.pose_var(rr, k)] = b
    for rr in range(J.R):
        for cls in range(3):
            ids = r.gid[rr][cls]
            if len(ids) == 0:
                continue
            blocks = r.batch.get_landmark_covariances(rr, cls, np.arange(len(ids)))
            for loc, b in enumerate(blocks):
                v = ref.lm_var(cls, int(ids[loc]))
                if v in out:
                    assert np.array_equal(out[v], b), ("shared landmark differs between replicas", rr, cls, loc)
                out[v] = b
    return out


def check_case(gpu, J, chart=0, evidence=None):
    """One pass, every marginal against the dense inverse; returns (worst error / tolerance, the Run, still open)."""
    import torch
    r = Run(gpu, J, chart)
    if evidence is not None:
        evidence(r)
    vals = r.values()
    Sig, w, tol, kappa = dense_inverse(r.ref, vals)
    r.drv.one_pass()
    torch.cuda.synchronize()
    if evidence is not None:
        evidence(r)
    ref = r.ref
    got = query_all(r)
    assert len(got) == len(ref.vtype)
    scale = np.abs(Sig * np.outer(w, w)).max()
    worst = 0.0
    for k, b in got.items():
        o0, o1 = ref.off[k], ref.off[k + 1]
        worst = max(worst, float(np.abs((b - Sig[o0:o1, o0:o1]) * np.outer(w[o0:o1], w[o0:o1])).max() / scale))
    assert worst <= tol, (worst, tol, kappa)
    # logEntropy: the robot's pose traces, the job's point landmarks (each once)
    pts = [k for k in range(len(ref.vtype)) if int(ref.vtype[k]) == po.V_POINT]
    pt_tr = sum(np.trace(Sig[ref.off[k]:ref.off[k + 1], ref.off[k]:ref.off[k + 1]]) for k in pts)
    for rr in range(J.R):
        tr = r.drv.marginal_traces(rr)
        ps = [ref.pose_var(rr, k) for k in range(J.sizes[rr])]
        pose_tr = sum(np.trace(Sig[ref.off[k]:ref.off[k + 1], ref.off[k]:ref.off[k + 1]]) for k in ps)
        assert tr[2] == len(ps) and tr[3] == len(pts), (tr, len(ps), len(pts))
        assert abs(tr[0] - pose_tr) <= 10 * tol * scale * len(ps), (tr[0], pose_tr)
        assert abs(tr[1] - pt_tr) <= 10 * tol * scale * max(len(pts), 1), (tr[1], pt_tr)
        assert tr[0] == pytest.approx(sum(np.trace(got[k]) for k in ps), rel=1e-12)
    print(f"[joint-marginals] worst / tolerance {worst / tol:.3e} (tol {tol:.2e}, kappa {kappa:.2e})")
    return worst / tol, r


def run_check(gpu, J, chart=0, evidence=None):
    _, r = check_case(gpu, J, chart, evidence)
    r.close()


# ---- the structural cases of the pass ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [2, 4])
def test_shared_mix(gpu, R):
    J = jg.shared_mix_case(R)

    def ev(r):
        assert r.info["n_slots"] > 0 and r.drv.arrow
    run_check(gpu, J, 0, ev)


BORDERS = {63: (9, 0, 0), 64: (1, 5, 4), 129: (3, 10, 6)}


@pytest.mark.parametrize("coords", sorted(BORDERS))
def test_border_rows(gpu, coords):
    """Robot 0's border of 63 / 64 / 129 coordinates from cylinders, cubes and points (all three classes)."""
    mix = BORDERS[coords]
    J = jg.border_case(mix)

    def ev(r):
        assert r.info["sep_dim"] == coords
        assert len(r.shards[0].graph.border_profile()) == (coords + NB - 1) // NB
    run_check(gpu, J, 0, ev)


def test_sizes(gpu):
    """Robots of unequal sizes, one with an empty border."""
    J = jg.sizes_case([20, 45, 9], private_only=(2,))

    def ev(r):
        assert len(set(J.sizes)) == 3
    run_check(gpu, J, 0, ev)


@pytest.mark.parametrize("seg", [None, "1", "2", "4"], ids=["default3", "1", "2", "4"])
def test_segments(gpu, monkeypatch, seg):
    """Bands cut into SLIDE_SEGMENTS segments (3 unset): the windows' poses are read from the border rows."""
    if seg is None:
        monkeypatch.delenv("SLIDE_SEGMENTS", raising=False)
    else:
        monkeypatch.setenv("SLIDE_SEGMENTS", seg)
    n = 3 if seg is None else int(seg)
    J = jg.segments_case()

    def ev(r):
        for sh in r.shards:
            segs, _ = sh.graph.segments()
            assert (segs == []) if n == 1 else (len(segs) == n), segs
    run_check(gpu, J, 0, ev)


def test_separator_tiles(gpu):
    """Dissected separator: each leaf and the top block past one tile."""
    J = jg.separator_tiles_case()

    def ev(r):
        Ta, Tb, used_a, used_b = r.info["sep_prof"][1]
        top = r.info["sep_dim"] - NB * (Ta + Tb)
        assert used_a > NB and used_b > NB and top > NB, (Ta, Tb, used_a, used_b, top)
    run_check(gpu, J, 0, ev)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("R,n_rel", [(2, 3), (4, 11)], ids=["2x3", "4x11"])
def test_relative_pose_factors(gpu, R, n_rel, chart):
    """The lambda block (D = -I) of 18 / 66 coordinates (66: past one tile), under both charts."""
    J = jg.relmeas_case(R, n_rel)

    def ev(r):
        assert r.drv.lam_dim == 6 * n_rel
    run_check(gpu, J, chart, ev)


@pytest.mark.parametrize("shared", [False, True], ids=["private", "shared"])
@pytest.mark.parametrize("cls", [0, 1, 2], ids=["cyl", "cube", "point"])
def test_landmark_count(gpu, cls, shared):
    """One landmark seen from 25 poses: private (the Schur identity over its factors) or shared (the separator's Sigma)."""
    J = jg.landmark_count_case(cls, 25, shared=shared)

    def ev(r):
        g = int(r.gid[0][cls][0])
        assert (g in {int(x) for x in r.gid[1][cls]}) == shared
    run_check(gpu, J, 0, ev)


# ---- the pass is untouched; status paths ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["relmeas", "segments"])
def test_second_pass_bits_unchanged(gpu, case):
    """A pass after the queries gives the same bits as a pass without them."""
    import torch
    J = jg.relmeas_case(2, 3) if case == "relmeas" else jg.segments_case()
    _, r = check_case(gpu, J)
    try:
        r.drv.one_pass()
        torch.cuda.synchronize()
        with_q = r.values()
    finally:
        r.close()
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
    J = jg.shared_mix_case(2)
    r = Run(gpu, J, 0)
    try:
        with pytest.raises(SlideError, match="no whole exact joint pass"):
            r.batch.get_pose_covariances(0, [0])
        r.drv.one_pass()
        torch.cuda.synchronize()
        assert r.batch.get_pose_covariances(0, [0]).shape == (1, 6, 6)
        with pytest.raises(KeyError):
            r.batch.get_pose_covariances(0, [J.sizes[0] + 5])
        with pytest.raises(KeyError):
            r.batch.get_landmark_covariances(1, 2, [10 ** 6])
        with pytest.raises(SlideError):          # (the single-graph getters keep refusing on a joined shard)
            r.shards[0].graph.get_pose_covariances(0, [0])
        g = r.shards[0].graph
        P = J.sizes[0]
        st, v = g.get_pose12(0, P - 1)
        rel = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
        est = np.concatenate([v[9:12] + np.array([1.0, 0.0, 0.0]), [0.0, 0.0, 0.0, 1.0]])
        g.add_keypose_between(0, P - 1, P, rel, est)
        with pytest.raises(SlideError, match="changed since the last exact joint pass"):
            r.batch.marginal_traces(0)
    finally:
        r.close()
    rp = Run(gpu, J, 0, pcg_iters=20, pcg_tol=1e-10)
    try:
        rp.drv.one_pass()
        torch.cuda.synchronize()
        with pytest.raises(SlideError, match="does not run exact joint passes"):
            rp.batch.get_pose_covariances(0, [0])
        with pytest.raises(ValueError):
            rp.drv.get_pose_covariances(0, [0])
    finally:
        rp.close()
