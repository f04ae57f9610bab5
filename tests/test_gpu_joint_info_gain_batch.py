"""Many loop-closure candidates in one call on the JOINT multi-robot graph (slide_chol_batch_closure_info_gain_batch /
CholBatch.closure_info_gain_batch / PassDriver.closure_info_gain_batch: one walk of the k_jms_* schedule per sweep, then
cov_kernels.hip's k_gram_blocks and k_woodbury_blocks) on the structural cases of tests/test_gpu_joint_info_gain.py: every candidate
against the dense joint reference (that module's ref_gain and tolerance, all four outputs) and against the single-candidate call; a
candidate's bits do not depend on its neighbours; the pass and the cached joint Sigma are left as they were.  No candidate is filtered
out: every generated one must come back with status 0."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_graphs as jg                                                      # noqa: E402
from test_gpu_info_gain_batch import STEPS, walk                               # noqa: E402
from test_gpu_joint_info_gain import SIGMA, GainRun, chain, ref_gain           # noqa: E402
from test_gpu_joint_step import NB, Run                                        # noqa: E402

pytestmark = pytest.mark.gpu


def batch_of(J, slot, own, seed, other=None):
    """The candidates of one call for `slot`: the case's own ones, a trajectory that visits a pose twice, one long-stepped walk per
    entry of STEPS over the slot's robot and, with `other`, a rendezvous with that robot.  ends = [(robot, index)]."""
    rng = np.random.default_rng(seed)
    P = J.sizes[slot]
    out = [list(e) for e in own] + [chain(slot, [P - 1, 2, P - 1, 0])] + [chain(slot, walk(rng, P, m)) for m in STEPS]
    if other is not None:
        out.append([(other, J.sizes[other] - 1), (slot, P // 2), (other, 1)])
    return out


def check_batch(g, slot, cands, seed=0):
    rng = np.random.default_rng(1000 + seed)
    travels = [[float(rng.uniform(1.0, 9.0)) for _ in e[1:]] for e in cands]
    idx = [[p for _, p in e] for e in cands]
    slots = [[r for r, _ in e] for e in cands]
    assert len(cands) >= 12 and {len(e) - 1 for e in cands} >= {1, 64}
    got, st = g.r.batch.closure_info_gain_batch(slot, idx, travels, SIGMA, slots)
    assert got.shape == (len(cands), 4) and (st == 0).all(), st
    worst = worst1 = 0.0
    for k, e in enumerate(cands):
        want, traces = ref_gain(g.r.ref, g.H, g.vals, slot, e, travels[k], SIGMA)
        scale = np.maximum(np.abs(want), 1e-3 * traces)
        one = g.r.batch.closure_info_gain(slot, idx[k], travels[k], SIGMA, slots[k])
        err, err1 = np.abs(got[k] - want) / scale, np.abs(got[k] - one) / scale
        assert (err <= max(g.tol, 1e-12)).all(), (k, got[k], want, err, g.tol, g.kappa)
        assert (err1 <= max(g.tol, 1e-12)).all(), (k, got[k], one, err1, g.tol, g.kappa)
        worst, worst1 = max(worst, err.max()), max(worst1, err1.max())
    print(f"[joint-gain-batch] slot {slot}, {len(cands)} candidates: worst vs dense {worst:.3e}, vs single {worst1:.3e} (tol {g.tol:.2e})")
    check_bits(g, slot, cands, travels, got, rng)
    return got


def check_bits(g, slot, cands, travels, got, rng):
    """On this case's structure, bit for bit: the same call again; the batch permuted gives the permuted outputs; the first, the
    widest and the last candidate (the rendezvous where the case has one) alone, and first, in the middle and last in a batch of 100
    (several sweeps, other chunks of 16 columns), give the bits they had in `got`."""
    b = g.r.batch

    def call(ends, dist):
        out, st = b.closure_info_gain_batch(slot, [[p for _, p in e] for e in ends], dist, SIGMA, [[r for r, _ in e] for e in ends])
        assert (st == 0).all(), st
        return out

    assert np.array_equal(call(cands, travels), got)
    perm = rng.permutation(len(cands))
    assert np.array_equal(call([cands[i] for i in perm], [travels[i] for i in perm]), got[perm])
    P = max(p for e in cands for r, p in e if r == slot) + 1          # (the poses of the slot's robot the candidates reach)
    others = [chain(slot, walk(rng, P, int(rng.choice([1, 1, 2, 3, 6])))) for _ in range(99)]
    d_others = [[float(rng.uniform(1.0, 9.0)) for _ in e[1:]] for e in others]
    assert 6 * sum(len(e) - 1 for e in others) > 384
    widest = max(range(len(cands)), key=lambda k: len(cands[k]))
    for k in (0, widest, len(cands) - 1):
        assert np.array_equal(call([cands[k]], [travels[k]])[0], got[k]), k
        for at in (0, 50, 99):
            out = call(others[:at] + [cands[k]] + others[at:], d_others[:at] + [travels[k]] + d_others[at:])
            assert np.array_equal(out[at], got[k]), (k, at, out[at], got[k])


def run_batches(gpu, J, calls, chart=0, evidence=None):
    """calls: [(slot, own candidates, robot of a rendezvous or None)]."""
    g = GainRun(gpu, J, chart, evidence)
    try:
        for n, (slot, own, other) in enumerate(calls):
            check_batch(g, slot, batch_of(J, slot, own, 10 * chart + n, other), n)
    finally:
        g.close()


@pytest.mark.parametrize("R", [2, 4])
def test_shared_mix(gpu, R):
    J = jg.shared_mix_case(R)

    def ev(r):
        assert r.info["n_slots"] > 0 and r.drv.arrow
    run_batches(gpu, J, [(0, [chain(0, [J.sizes[0] - 1, 0])], 1),
                         (R - 1, [chain(R - 1, [J.sizes[R - 1] - 2, J.sizes[R - 1] // 2, 3, 1])], None)], 0, ev)


@pytest.mark.parametrize("coords", [64, 129])
def test_border_rows(gpu, coords):
    J = jg.border_case({64: (1, 5, 4), 129: (3, 10, 6)}[coords])

    def ev(r):
        assert r.info["sep_dim"] == coords
    run_batches(gpu, J, [(0, [chain(0, [J.sizes[0] - 1, 0])], None), (1, [chain(1, [J.sizes[1] - 1, 12, 2, 0])], 0)], 0, ev)


@pytest.mark.parametrize("seg", [None, "1", "2", "4"], ids=["default3", "1", "2", "4"])
def test_segments(gpu, monkeypatch, seg):
    """65 consecutive poses across the cuts (window poses and poses of two segments) among the walks."""
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
    run_batches(gpu, J, [(0, [chain(0, range(lo, lo + 65))], None), (1, [chain(1, [P - 1, P // 2, 0])], 0)], 0, ev)


def test_separator_tiles(gpu):
    J = jg.separator_tiles_case()

    def ev(r):
        Ta, Tb, used_a, used_b = r.info["sep_prof"][1]
        top = r.info["sep_dim"] - NB * (Ta + Tb)
        assert used_a > NB and used_b > NB and top > NB, (Ta, Tb, used_a, used_b, top)
    run_batches(gpu, J, [(0, [chain(0, [J.sizes[0] - 1, 0])], None),
                         (1, [chain(1, [J.sizes[1] - 1, J.sizes[1] // 2, 1, 0])], 0)], 0, ev)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("R,n_rel", [(2, 3), (4, 11)], ids=["2x3", "4x11"])
def test_relative_pose_factors(gpu, R, n_rel, chart):
    J = jg.relmeas_case(R, n_rel)

    def ev(r):
        assert r.drv.lam_dim == 6 * n_rel
    P0, P1 = J.sizes[0], J.sizes[1]
    run_batches(gpu, J, [(0, [chain(0, [P0 - 1, 0])], 1), (1, [[(1, P1 - 1), (0, P0 // 2), (1, 2), (1, 0)]], 0)], chart, ev)


@pytest.mark.parametrize("case", ["shared_mix", "relmeas"])
def test_a_candidate_does_not_see_its_neighbours(gpu, case):
    """The same candidate (one of them a rendezvous) first, in the middle and last of batches of 1, 17 and 100: the same bits;
    a permuted batch gives the permuted outputs; the same call twice gives the same bits; PassDriver's call is CholBatch's."""
    J = jg.shared_mix_case(2) if case == "shared_mix" else jg.relmeas_case(2, 3)
    g = GainRun(gpu, J)
    try:
        b = g.r.batch
        rng = np.random.default_rng(3)
        P0, P1 = J.sizes[0], J.sizes[1]

        def rnd(n):
            ends = [chain(0, walk(rng, P0, int(rng.choice([1, 1, 2, 3, 6, 20])))) for _ in range(n)]
            return ends, [[float(rng.uniform(1.0, 9.0)) for _ in e[1:]] for e in ends]

        def call(ends, travels):
            got, st = b.closure_info_gain_batch(0, [[p for _, p in e] for e in ends], travels, SIGMA, [[r for r, _ in e] for e in ends])
            assert (st == 0).all(), st
            return got

        for mine in (chain(0, [P0 - 1, 0]), [(1, P1 - 1), (0, P0 // 2), (1, 2), (1, 0)], chain(0, walk(rng, P0, 17))):
            d_mine = [2.5 + i for i in range(len(mine) - 1)]
            alone = call([mine], [d_mine])
            assert alone[0][1] > 0
            for n in (17, 100):
                others, d_others = rnd(n - 1)
                assert 6 * sum(len(e) - 1 for e in others) > (384 if n == 100 else 0)
                for at in (0, n // 2, n - 1):
                    got = call(others[:at] + [mine] + others[at:], d_others[:at] + [d_mine] + d_others[at:])
                    assert np.array_equal(got[at], alone[0]), (n, at, got[at], alone[0])
        ends = [chain(0, walk(rng, P0, m)) for m in STEPS + STEPS]
        travels = [[float(rng.uniform(1.0, 9.0)) for _ in e[1:]] for e in ends]
        a = call(ends, travels)
        assert np.array_equal(a, call(ends, travels))
        perm = rng.permutation(len(ends))
        assert np.array_equal(call([ends[i] for i in perm], [travels[i] for i in perm]), a[perm])
        idx = [[p for _, p in e] for e in ends]
        d, st = g.r.drv.closure_info_gain_batch(0, idx, travels, SIGMA)
        assert (st == 0).all() and np.array_equal(d, a)
    finally:
        g.close()


@pytest.mark.parametrize("case", ["relmeas", "segments"])
def test_batch_leaves_the_pass_and_sigma(gpu, case):
    """Pose covariances read the same bits before and after a batch; a pass after it gives the same bits as one without."""
    import torch
    J = jg.relmeas_case(2, 3) if case == "relmeas" else jg.segments_case()
    g = GainRun(gpu, J)
    try:
        r = g.r
        cov0 = r.batch.get_pose_covariances(0, np.arange(J.sizes[0]))
        check_batch(g, 0, batch_of(J, 0, [chain(0, [J.sizes[0] - 1, 0])], 7, 1))
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
    """Per-candidate codes and the whole-call refusals of test_gpu_joint_info_gain.test_status_paths."""
    import torch
    from slide_slam_amd.api import SlideError
    J = jg.shared_mix_case(2, sizes=[70, 66])
    P = J.sizes[0]
    one = ([[1, 0]], [[1.0]])
    r = Run(gpu, J, 0)
    try:
        with pytest.raises(SlideError, match="no whole exact joint pass"):
            r.batch.closure_info_gain_batch(0, *one)
        r.drv.one_pass()
        torch.cuda.synchronize()
        good, d_good = [[P - 1, 0], [40, 20, 1]], [[3.0], [2.0, 4.0]]
        trajs = [good[0], [P + 5, 0], [1], [1, 0], [1, 0], list(range(66)), good[1], [J.sizes[1] + 5, 0], [1, 0]]
        travels = [d_good[0], [1.0], [], [0.0], [float("nan")], [1.0] * 65, d_good[1], [1.0], [1.0]]
        slots = [[0, 0], [0, 0], [0], [0, 0], [0, 0], [0] * 66, [0, 0, 0], [1, 0], [5, 0]]
        got, st = r.batch.closure_info_gain_batch(0, trajs, travels, SIGMA, slots)
        assert list(st) == [0, 1, -1, -1, -1, -3, 0, 1, -1], st
        assert (got[[1, 2, 3, 4, 5, 7, 8]] == 0.0).all()
        ref, st_ref = r.batch.closure_info_gain_batch(0, good, d_good, SIGMA)
        assert (st_ref == 0).all() and np.array_equal(got[[0, 6]], ref) and (ref[:, 0] > 0).all()
        # the same list through the raw entry point with marked buffers: the library writes every status word and the zeros
        import ctypes as C
        vp = C.c_void_p
        off = np.cumsum([0] + [len(t) for t in trajs]).astype(np.int32)
        flat = np.concatenate(trajs).astype(np.uint64)
        fslots = np.concatenate(slots).astype(np.int32)
        dist = np.concatenate([list(d) + [0.0] for d in travels]).astype(np.float64)
        sg = np.ascontiguousarray(SIGMA, dtype=np.float64)
        out, stat = np.full(4 * len(trajs), 7.0), np.full(len(trajs), 7, dtype=np.int32)
        rc = r.batch.L.slide_chol_batch_closure_info_gain_batch(
            C.c_void_p(r.batch.h), C.c_int(0), C.c_int(len(trajs)), off.ctypes.data_as(vp), fslots.ctypes.data_as(vp), flat.ctypes.data_as(vp),
            dist.ctypes.data_as(vp), sg.ctypes.data_as(vp), out.ctypes.data_as(vp), stat.ctypes.data_as(vp))
        assert rc == 0 and np.array_equal(stat, st) and np.array_equal(out.reshape(-1, 4), got) and not (out == 7.0).any()
        cap, st = r.batch.closure_info_gain_batch(0, [list(range(65))], [[1.0] * 64])
        assert st[0] == 0 and cap[0][0] > 0                                              # (m = 64: the cap)
        with pytest.raises(SlideError):
            r.batch.closure_info_gain_batch(0, *one, [0.1, 0.1, 0.0, 0.1, 0.1, 0.1])
        with pytest.raises(SlideError, match="no such slot"):
            r.batch.closure_info_gain_batch(9, *one)
        with pytest.raises(SlideError):
            r.batch.closure_info_gain_batch(0, [], [])
        g = r.shards[0].graph
        _, v = g.get_pose12(0, P - 1)
        rel = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
        est = np.concatenate([v[9:12] + np.array([1.0, 0.0, 0.0]), [0.0, 0.0, 0.0, 1.0]])
        g.add_keypose_between(0, P - 1, P, rel, est)
        with pytest.raises(SlideError, match="changed since the last exact joint pass"):
            r.batch.closure_info_gain_batch(0, *one)
    finally:
        r.close()
    rp = Run(gpu, J, 0, pcg_iters=20, pcg_tol=1e-10)
    try:
        rp.drv.one_pass()
        torch.cuda.synchronize()
        with pytest.raises(SlideError, match="does not run exact joint passes"):
            rp.batch.closure_info_gain_batch(0, *one)
        with pytest.raises(ValueError):
            rp.drv.closure_info_gain_batch(0, *one)
    finally:
        rp.close()
    r1 = Run(gpu, J, 0)
    try:
        r1.drv.one_pass()
        torch.cuda.synchronize()
        r1.drv.world = 2
        with pytest.raises(ValueError):
            r1.drv.closure_info_gain_batch(0, *one)
    finally:
        r1.drv.world = 1
        r1.close()
