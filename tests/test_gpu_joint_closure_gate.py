"""The Mahalanobis gate of loop closures and the joint marginal of pose pairs on the JOINT multi-robot graph, on the device
(slide_chol_batch_closure_mahalanobis / slide_chol_batch_get_pose_pair_covariances: the forward half of the many-right-hand-side
solve over the exact joint pass's tree and a signed gram, host_gates.hip's joint_sigma_forms; closure_kernels.hip's
k_joint_closure_gate_lin / k_joint_pair_identity / k_gram_sub) against the dense reference of tests/joint_closure_gate_cases.py.

Per case: one Run (tests/test_gpu_joint_step.py), the reference at the values read before the pass, one exact joint pass, then the
queries; r and A of the reference are taken at the poses read back through get_pose12 after the pass.  Tolerances are the existing
tests': a pair block's Jacobi-scaled entries within dense_inverse's tol (test_gpu_joint_marginals); two routes to one block 1e-9
relative; d2, C and r within closure_gate_cases.gate_bound (tol x cond(C_ref), floor 1e-12).  The independence and read-only checks
are bit for bit.  Every case asserts the structural edge it exists for.  SLIDE_ERR_NOT_SPD is not covered: C = I + (a positive
semi-definite matrix up to rounding) has no non-positive pivot on any graph these cases can build with finite input."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import closure_gate_cases as gc                                                 # noqa: E402
import joint_closure_gate_cases as jc                                           # noqa: E402
import joint_graphs as jg                                                       # noqa: E402
from test_gpu_closure_gate import check_gate, swap_blocks                       # noqa: E402
from test_gpu_joint_step import NB, Run                                         # noqa: E402

pytestmark = pytest.mark.gpu

MISSING, INVALID = 1, -1


class GateRun:
    """One Run, the reference at the values the pass linearises at, then one exact joint pass."""

    def __init__(self, gpu, J, chart=0, evidence=None):
        import torch
        self.r = Run(gpu, J, chart)
        try:
            if evidence is not None:
                evidence(self.r)
            self.c = jc.JointGateCase(J, chart, ref=self.r.ref, vals=self.r.values())
            self.r.drv.one_pass()
            torch.cuda.synchronize()
            if evidence is not None:
                evidence(self.r)
        except BaseException:
            self.r.close()
            raise
        self.J, self.batch, self.tag = J, self.r.batch, f"chart {chart}"

    def pose12(self, robot, idx):
        st, p = self.r.shards[robot].graph.get_pose12(0, idx)
        assert st == 0
        return p

    def check_pairs(self, pairs):
        c = self.c
        got, st = self.batch.get_pose_pair_covariances(pairs)
        assert got.shape == (len(pairs), 12, 12) and (st == 0).all(), st
        worst = worst_diag = worst_swap = 0.0
        for k, (ra, ia, rb, ib) in enumerate(pairs):
            want, w = c.pair_sigma(ra, ia, rb, ib)
            worst = max(worst, float(np.abs((got[k] - want) * np.outer(w, w)).max() / c.scale))
            assert np.array_equal(got[k], got[k].T)
            if ra != rb:
                assert np.abs(got[k][:6, 6:]).max() > 0
            da, db = self.batch.get_pose_covariances(ra, [ia])[0], self.batch.get_pose_covariances(rb, [ib])[0]
            worst_diag = max(worst_diag, float(np.abs(got[k][:6, :6] - da).max() / np.abs(da).max()),
                             float(np.abs(got[k][6:, 6:] - db).max() / np.abs(db).max()))
            if (rb, ib, ra, ia) in pairs:
                other = got[pairs.index((rb, ib, ra, ia))]
                worst_swap = max(worst_swap, float(np.abs(swap_blocks(other) - got[k]).max() / np.abs(got[k]).max()))
        print(f"[joint-pair-cov] {self.tag}: vs dense inverse {worst:.3e} (tol {c.tol:.2e}, kappa {c.kappa:.2e}), diagonal blocks vs "
              f"get_pose_covariances {worst_diag:.2e}, (b, a) vs (a, b) {worst_swap:.2e}")
        assert worst <= c.tol, (worst, c.tol, c.kappa)
        assert worst_diag <= 1e-9 and worst_swap <= 1e-9, (worst_diag, worst_swap)
        return got

    def check_gate(self, closures, tag=""):
        out = self.batch.closure_mahalanobis(closures)
        d2, worst = check_gate(self.c, closures, out, self.pose12, f"joint {self.tag} {tag}")
        assert np.array_equal(out["C"], np.transpose(out["C"], (0, 2, 1)))
        print(f"[joint-gate] {self.tag} {tag}: largest error / bound {worst:.3e}; d2_ref from {d2.min():.3g} to {d2.max():.3g}")
        return out

    def check_planted(self):
        closures, flags, _ = jc.planted_list(self.c)
        out = self.check_gate(closures, "planted")
        assert ((out["d2"] < jc.GATE2) == flags).all(), (out["d2"], flags)
        print(f"[joint-gate] {self.tag} planted: true max {out['d2'][flags].max():.3f}, false min {out['d2'][~flags].min():.1f}")

    def check_all(self, pairs=None, ends=None, planted=True):
        J = self.J
        pairs = jc.pair_list(J) + list(pairs or [])
        assert sum((p[2], p[3], p[0], p[1]) in pairs for p in pairs) >= 4 and len(jc.inter(pairs)) >= 4
        self.check_pairs(pairs)
        self.check_gate(jc.perturbed_list(J, self.pose12), "perturbed")
        if ends:
            self.check_gate([gc.measured(self.pose12, *e, 2.0 * jc.SIGMA6 * np.array([1, -1, 1, -1, 1, -1.0])) for e in ends], "edge ends")
        if planted:
            self.check_planted()

    def close(self):
        self.r.close()


def run_all(gpu, J, chart=0, evidence=None, pairs=None, ends=None, planted=True):
    g = GateRun(gpu, J, chart, evidence)
    try:
        g.check_all(pairs, ends, planted)
    finally:
        g.close()


# ---- the structural cases of the pass ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chart", [0, 1])
def test_relative_pose_factors(gpu, chart):
    """Lambda rows (18 coordinates): the gram's D = -I part."""
    J = jg.relmeas_case(R=2, n_rel=3, P=14)

    def ev(r):
        assert r.drv.lam_dim == 18
    run_all(gpu, J, chart, ev)


@pytest.mark.parametrize("R", [2, 4])
def test_shared_mix(gpu, R):
    """No relative-pose factor: the cross blocks exist through the shared landmarks (the separator's rows of W) alone."""
    J = jg.shared_mix_case(R)

    def ev(r):
        assert r.info["n_slots"] > 0 and r.drv.arrow and not J.relmeas and getattr(r.drv, "lam_dim", 0) == 0
    run_all(gpu, J, 0, ev)


@pytest.mark.parametrize("coords", [64, 129])
def test_border_rows(gpu, coords):
    """Robot 0's border of 64 / 129 coordinates: one tile, and past two tiles."""
    J = jg.border_case({64: (1, 5, 4), 129: (3, 10, 6)}[coords])

    def ev(r):
        assert r.info["sep_dim"] == coords
    run_all(gpu, J, 0, ev)


@pytest.mark.parametrize("seg", [None, "1", "2", "4"], ids=["default3", "1", "2", "4"])
def test_segments(gpu, monkeypatch, seg):
    """Bands cut into SLIDE_SEGMENTS segments: a window pose (its rows are border rows of its robot's system) paired with band poses
    of the first and the last segment and with poses of the other robot."""
    if seg is None:
        monkeypatch.delenv("SLIDE_SEGMENTS", raising=False)
    else:
        monkeypatch.setenv("SLIDE_SEGMENTS", seg)
    n = 3 if seg is None else int(seg)
    J = jg.segments_case()
    P = J.sizes[0]
    w = P // n + 1 if n > 1 else P // 2          # (the window behind the first cut starts at pose P // n)

    def ev(r):
        for sh in r.shards:
            segs, nwin = sh.graph.segments()
            assert (segs == []) if n == 1 else (len(segs) == n and nwin > 0), (segs, nwin)
            if n > 1:
                assert 6 * (w + 1) <= NB * segs[1][0], (w, segs)      # pose w lies before the second segment's first row: in the window
    edge = [(0, w, 0, P - 5), (0, 3, 0, w), (0, w, 1, 20), (1, w, 0, w), (1, 20, 0, w)]
    # (no planted list: over 150 poses of drift the reference itself puts a 20 m displacement at d2_ref = 19, inside 4 x 16.81)
    run_all(gpu, J, 0, ev, pairs=edge, ends=edge[:4], planted=False)


def test_separator_tiles(gpu):
    """Dissected separator: pose pairs coupled through leaf a (robots 0, 1), leaf b (2, 3), the top block (1, 2), and all three (0, 3)."""
    J = jg.separator_tiles_case()

    def ev(r):
        Ta, Tb, used_a, used_b = r.info["sep_prof"][1]
        top = r.info["sep_dim"] - NB * (Ta + Tb)
        assert used_a > NB and used_b > NB and top > NB, (Ta, Tb, used_a, used_b, top)
    edge = [(0, 5, 1, 6), (1, 6, 0, 5), (2, 4, 3, 5), (3, 5, 2, 4), (1, 3, 2, 5), (2, 5, 1, 3), (0, 9, 3, 9), (3, 9, 0, 9)]
    run_all(gpu, J, 0, ev, pairs=edge, ends=edge[::2])


# ---- properties ------------------------------------------------------------------------------------------------------------------

def test_candidates_do_not_depend_on_their_neighbours(gpu):
    """65 closures and 33 pairs (a second sweep of one each), with duplicates and shared poses, inside and across robots: candidate k is
    bit for bit what the call gives for it alone, in a permuted list, and in two halves."""
    J = jg.relmeas_case(R=2, n_rel=3, P=14)
    g = GateRun(gpu, J)
    try:
        b = g.batch
        closures = jc.long_closure_list(J, g.pose12)
        full = b.closure_mahalanobis(closures)
        assert (full["status"] == 0).all() and (full["d2"] > 0).all()
        for k in (0, 64, 63, 17):
            one = b.closure_mahalanobis([closures[k]])
            for f in ("d2", "C", "r"):
                assert np.array_equal(one[f][0], full[f][k]), (k, f)
        assert np.array_equal(full["d2"][61], full["d2"][0]) and np.array_equal(full["C"][62], full["C"][7])
        rng = np.random.default_rng(11)
        perm = rng.permutation(65)
        sh = b.closure_mahalanobis([closures[k] for k in perm])
        h0, h1 = b.closure_mahalanobis(closures[:30]), b.closure_mahalanobis(closures[30:])
        for f in ("d2", "C", "r"):
            assert np.array_equal(sh[f], full[f][perm]), f
            assert np.array_equal(np.concatenate([h0[f], h1[f]]), full[f]), f
        pairs = jc.long_pair_list(J)
        pf, st = b.get_pose_pair_covariances(pairs)
        assert (st == 0).all() and np.array_equal(pf[30], pf[0])
        for k in (0, 32, 31, 9):
            assert np.array_equal(b.get_pose_pair_covariances([pairs[k]])[0][0], pf[k]), k
        perm = rng.permutation(33)
        assert np.array_equal(b.get_pose_pair_covariances([pairs[k] for k in perm])[0], pf[perm])
        assert np.array_equal(np.concatenate([b.get_pose_pair_covariances(pairs[:17])[0], b.get_pose_pair_covariances(pairs[17:])[0]]), pf)
        dg, ds = g.r.drv.get_pose_pair_covariances(pairs[:3])          # (the driver's methods are the batch's)
        assert np.array_equal(dg, pf[:3]) and (ds == 0).all()
        assert np.array_equal(g.r.drv.closure_mahalanobis(closures[:2])["d2"], full["d2"][:2])
    finally:
        g.close()


def test_status_per_candidate(gpu):
    """A missing pose, a slot the batch does not have, from == to: zeros and the code for that candidate, its neighbours unchanged."""
    J = jg.shared_mix_case(2)
    g = GateRun(gpu, J)
    try:
        b, P0 = g.batch, J.sizes[0]
        good = [gc.measured(g.pose12, *e, 0.5 * jc.SIGMA6) for e in [(0, 3, 1, 4), (1, 5, 0, 9), (0, 2, 0, 7)]]
        z, sg = good[0][4], good[0][5]
        bad = [(0, P0 + 5, 1, 4, z, sg), (0, 3, 2, 4, z, sg), (1, 6, 1, 6, z, sg), (2, 0, 0, 0, z, sg)]
        mixed = [good[0], bad[0], good[1], bad[1], bad[2], good[2], bad[3]]
        out, alone = b.closure_mahalanobis(mixed), b.closure_mahalanobis(good)
        assert out["status"].tolist() == [0, MISSING, 0, MISSING, INVALID, 0, MISSING]
        for k in (1, 3, 4, 6):
            assert out["d2"][k] == 0 and not out["C"][k].any() and not out["r"][k].any()
        for f in ("d2", "C", "r"):
            assert np.array_equal(out[f][[0, 2, 5]], alone[f]), f
        pairs = [(0, 3, 1, 4), (0, P0 + 5, 1, 4), (1, 5, 0, 9), (0, 3, 2, 4), (1, 6, 1, 6)]
        pf, st = b.get_pose_pair_covariances(pairs)
        assert st.tolist() == [0, MISSING, 0, MISSING, INVALID]
        assert not pf[[1, 3, 4]].any()
        assert np.array_equal(pf[[0, 2]], b.get_pose_pair_covariances([pairs[0], pairs[2]])[0])
        only_bad = b.closure_mahalanobis(bad)                                   # (no candidate left: nothing is launched)
        assert only_bad["status"].tolist() == [MISSING, MISSING, INVALID, MISSING] and not only_bad["d2"].any()
        assert b.closure_mahalanobis([])["d2"].shape == (0,) and b.get_pose_pair_covariances([])[0].shape == (0, 12, 12)
    finally:
        g.close()


def _raw_calls(gpu, b, closure, pair):
    """Both calls through the C ABI with outputs filled with 77: (return codes, outputs untouched?)"""
    L = gpu.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    fs, fi, ts, ti = (np.array([closure[j]], t) for j, t in ((0, np.int32), (1, np.uint64), (2, np.int32), (3, np.uint64)))
    rel, sg = np.ascontiguousarray(closure[4], float).reshape(1, 7), np.ascontiguousarray(closure[5], float).reshape(1, 6)
    d2, Cm, r, st = np.full(1, 77.0), np.full(36, 77.0), np.full(6, 77.0), np.full(1, 77, np.int32)
    rc1 = L.slide_chol_batch_closure_mahalanobis(C.c_void_p(b.h), C.c_int(1), P(fs), P(fi), P(ts), P(ti), P(rel), P(sg), P(d2), P(Cm), P(r), P(st))
    sa, ia, sb, ib = (np.array([pair[j]], t) for j, t in ((0, np.int32), (1, np.uint64), (2, np.int32), (3, np.uint64)))
    out, st2 = np.full(144, 77.0), np.full(1, 77, np.int32)
    rc2 = L.slide_chol_batch_get_pose_pair_covariances(C.c_void_p(b.h), C.c_int(1), P(sa), P(ia), P(sb), P(ib), P(out), P(st2))
    untouched = all((a == 77).all() for a in (d2, Cm, r, st, out, st2))
    return (rc1, rc2), untouched


def test_whole_call_refusals(gpu):
    """joint_state's refusals: before a pass, after a graph changed, in PCG mode; nothing is written."""
    import torch
    from slide_slam_amd.api import SlideError
    J = jg.shared_mix_case(2)
    P0 = J.sizes[0]
    I7 = np.array([1.0, 0, 0, 0, 0, 0, 1])
    cl, pr = (0, 3, 1, 4, I7, jc.SIGMA6), (0, 3, 1, 4)
    r = Run(gpu, J, 0)
    try:
        with pytest.raises(SlideError, match="no whole exact joint pass"):
            r.batch.closure_mahalanobis([cl])
        with pytest.raises(SlideError, match="no whole exact joint pass"):
            r.batch.get_pose_pair_covariances([pr])
        assert _raw_calls(gpu, r.batch, cl, pr) == ((-1, -1), True)
        r.drv.one_pass()
        torch.cuda.synchronize()
        rcs, untouched = _raw_calls(gpu, r.batch, cl, pr)
        assert rcs == (0, 0) and not untouched
        G = r.shards[0].graph
        st, v = G.get_pose12(0, P0 - 1)
        est = np.concatenate([v[9:12] + np.array([1.0, 0.0, 0.0]), [0.0, 0.0, 0.0, 1.0]])
        G.add_keypose_between(0, P0 - 1, P0, I7, est)
        with pytest.raises(SlideError, match="changed since the last exact joint pass"):
            r.batch.closure_mahalanobis([cl])
        with pytest.raises(SlideError, match="changed since the last exact joint pass"):
            r.batch.get_pose_pair_covariances([pr])
        assert _raw_calls(gpu, r.batch, cl, pr) == ((-1, -1), True)
    finally:
        r.close()
    rp = Run(gpu, J, 0, pcg_iters=20, pcg_tol=1e-10)
    try:
        rp.drv.one_pass()
        torch.cuda.synchronize()
        with pytest.raises(SlideError, match="does not run exact joint passes"):
            rp.batch.closure_mahalanobis([cl])
        with pytest.raises(SlideError, match="does not run exact joint passes"):
            rp.batch.get_pose_pair_covariances([pr])
        assert _raw_calls(gpu, rp.batch, cl, pr) == ((-1, -1), True)
        with pytest.raises(ValueError):
            rp.drv.closure_mahalanobis([cl])
        with pytest.raises(ValueError):
            rp.drv.get_pose_pair_covariances([pr])
    finally:
        rp.close()


def test_queries_leave_the_pass_sigma_and_the_gain_plan(gpu):
    """The cached joint Sigma reads the same bits before and after the queries, closure_info_gain_batch (both halves of the plan the
    queries walk the first half of) too, and the next pass gives the bits of a run without queries."""
    import torch
    J = jg.relmeas_case(R=2, n_rel=3, P=14)
    g = GateRun(gpu, J)
    try:
        r, b = g.r, g.batch
        cov0 = [b.get_pose_covariances(s, np.arange(J.sizes[s])) for s in range(J.R)]
        trajs, slots = [[5, 4], [9, 2, 0], [7, 3]], [[0, 1], [1, 1, 1], [1, 0]]
        travels = [[1.0], [2.0, 3.0], [1.5]]
        sig = np.array([0.02, 0.02, 0.02, 0.05, 0.05, 0.05])
        gain0, gst0 = b.closure_info_gain_batch(0, trajs, travels, sig, slots)
        assert (gst0 == 0).all() and (gain0[:, 0] > 0).all()
        first = b.closure_mahalanobis(jc.long_closure_list(J, g.pose12))
        pf, _ = b.get_pose_pair_covariances(jc.long_pair_list(J))
        for s in range(J.R):
            assert np.array_equal(cov0[s], b.get_pose_covariances(s, np.arange(J.sizes[s])))
        gain1, _ = b.closure_info_gain_batch(0, trajs, travels, sig, slots)
        assert np.array_equal(gain0, gain1)
        again = b.closure_mahalanobis(jc.long_closure_list(J, g.pose12))
        assert all(np.array_equal(first[f], again[f]) for f in ("d2", "C", "r"))
        assert np.array_equal(pf, b.get_pose_pair_covariances(jc.long_pair_list(J))[0])
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
