"""The duplicate-landmark queries on the JOINT multi-robot graph, on the device (slide_chol_batch_landmark_pair_mahalanobis /
_get_landmark_pair_covariances: obs_gate_kernels.hip's k_joint_lm_pair_fill / k_joint_lm_pair_cov_finish through host_gates.hip's
joint_sigma_forms; slide_chol_batch_landmark_pairs_within: pairs_kernels.hip's gather and group-inequality sibling) against the dense
reference of tests/joint_landmark_pair_cases.py.

Per case: one GateRun (test_gpu_joint_observation_gate.py: the reference at the values the pass linearises at, one exact joint pass),
then the queries; r of the reference is taken at the landmarks read back through get_landmark after the pass.  Tolerances are
test_gpu_landmark_pairs.py's, nothing new: d2 within tol x cond(C_ref), floor 1e-12 (gate_bound), relative to d2_ref, C and r entry-wise
by the same figure against the largest entry of C_ref; covariance blocks Jacobi-scaled (|got - ref| w_i w_j relative to the largest
scaled entry of inv(H)) within dense_inverse's tol.  The replica, independence and read-only checks are bit for bit."""
import ctypes as C

import numpy as np
import pytest

import joint_graphs as jg
import joint_landmark_pair_cases as jp
import joint_observation_gate_cases as jo
import landmark_pair_cases as lp
from test_gpu_joint_observation_gate import GateRun, sync
from test_gpu_joint_step import NB, Run

pytestmark = pytest.mark.gpu

MISSING, INVALID, CAPACITY = 1, -1, -3
FIELDS = ("d2", "C", "r", "dof", "status")


def check_pairs(g, kind, rows, out, tag):
    c = g.c
    rs, Cs, d2 = jp.ref_pairs(c, kind, rows, g.vals)
    D = jp.DIM[kind]
    assert (out["status"] == 0).all(), out["status"]
    worst = 0.0
    for k, row in enumerate(rows):
        assert out["dof"][k] == D
        bound = jo.gate_bound(c, Cs[k])
        top = float(np.abs(Cs[k]).max())
        e_d = abs(out["d2"][k] - d2[k]) / d2[k]
        e_C = float(np.abs(out["C"][k][:D, :D] - Cs[k]).max() / top)
        e_r = float(np.abs(out["r"][k][:D] - rs[k]).max() / top)
        print(f"[joint-lm-pairs] {tag} {kind} {tuple(int(x) for x in row)}: d2 {out['d2'][k]:.6g} ref {d2[k]:.6g} err {e_d:.2e}, C {e_C:.2e}, "
              f"r {e_r:.2e} (bound {bound:.2e})")
        assert max(e_d, e_C, e_r) <= bound, (k, e_d, e_C, e_r, bound)
        assert not out["C"][k][D:].any() and not out["C"][k][:, D:].any() and not out["r"][k][D:].any()
        worst = max(worst, max(e_d, e_C, e_r) / bound)
    assert np.array_equal(out["C"], np.transpose(out["C"], (0, 2, 1)))      # symmetric bit for bit
    print(f"[joint-lm-pairs] {tag} {kind}: largest error / bound {worst:.3e}")
    return d2, Cs


def check_covs(g, kind, rows, tag):
    """The joint marginals against the dense blocks (Jacobi-scaled); the diagonal blocks against the cached joint Sigma's
    get_landmark_covariances, another route on the device."""
    c, b = g.c, g.batch
    cls, D = jp.CLS[kind], jp.DIM[kind]
    cov, st = b.get_landmark_pair_covariances(cls, rows)
    assert cov.shape == (len(rows), 2 * D, 2 * D) and (st == 0).all(), st
    worst = 0.0
    for k, row in enumerate(rows):
        sel = jp.sel(c, kind, row)
        ws = np.outer(c.w[sel], c.w[sel])
        worst = max(worst, float(np.abs((cov[k] - c.Sig[np.ix_(sel, sel)]) * ws).max() / c.scale))
        assert np.abs(c.Sig[np.ix_(sel[:D], sel[D:])]).max() > 0
        for side in (0, 1):
            single = b.get_landmark_covariances(int(row[2 * side]), cls, [int(row[2 * side + 1])])[0]
            blk = slice(D * side, D * side + D)
            assert np.abs((cov[k][blk, blk] - single) * ws[blk, blk]).max() / c.scale <= c.tol
        assert np.array_equal(cov[k], cov[k].T)
    print(f"[joint-lm-pairs] {tag} {kind}: joint marginals, largest scaled error {worst:.3e} (tol {c.tol:.3e})")
    assert worst <= c.tol, (worst, c.tol)
    return cov


def check_case(gpu, J, chart=0, evidence=None, want=None):
    """Every side combination the case holds, per class: the test (points, cylinders) and the covariances (all three classes) against
    the reference; a shared side through its other replica, bit for bit; the swapped pair."""
    g = GateRun(gpu, J, chart, evidence)
    try:
        c, b = g.c, g.batch
        seen = set()
        for kind in ("point", "cylinder", "cube"):
            named = jp.side_pairs(c, kind)
            if not named:
                continue
            seen |= set(named)
            rows = np.array(list(named.values()), np.int64)
            tag = f"chart {chart}"
            cov = check_covs(g, kind, rows, tag)
            alt = rows.copy()
            for k, row in enumerate(rows):
                for side in (0, 1):
                    if jp.is_shared(c, int(row[2 * side]), kind, int(row[2 * side + 1])):
                        alt[k, 2 * side:2 * side + 2] = jp.other_replica(c, kind, int(row[2 * side]), int(row[2 * side + 1]))
            assert (alt != rows).any() or not any("shared" in n for n in named)
            cov_alt, st = b.get_landmark_pair_covariances(jp.CLS[kind], alt)
            assert (st == 0).all() and np.array_equal(cov_alt, cov)
            if kind == "cube":
                with pytest.raises(gpu.SlideError, match="SLIDE_ERR_INVALID"):
                    b.landmark_pair_mahalanobis(jp.CLS[kind], rows, np.full(3, 0.05))
                continue
            sg, D = jp.SIGMA[kind], jp.DIM[kind]
            out = b.landmark_pair_mahalanobis(jp.CLS[kind], rows, sg)
            d2, Cs = check_pairs(g, kind, rows, out, tag)
            other = b.landmark_pair_mahalanobis(jp.CLS[kind], alt, sg)
            for f in FIELDS:
                assert np.array_equal(other[f], out[f]), (kind, f)
            swapped = b.landmark_pair_mahalanobis(jp.CLS[kind], rows[:, [2, 3, 0, 1]], sg)
            assert np.array_equal(swapped["r"], -out["r"]) and (swapped["status"] == 0).all()
            for k in range(len(rows)):
                bound = jo.gate_bound(c, Cs[k])
                assert abs(swapped["d2"][k] - out["d2"][k]) / d2[k] <= bound
                assert np.abs(swapped["C"][k] - out["C"][k]).max() / np.abs(Cs[k]).max() <= bound
                Sd = cov[k][:D, :D] + cov[k][D:, D:] - cov[k][:D, D:] - cov[k][D:, :D]      # Sig_d rebuilt from the four blocks
                assert np.abs(np.eye(D) + Sd / np.outer(sg, sg) - out["C"][k][:D, :D]).max() / np.abs(Cs[k]).max() <= bound
        if want is not None:
            assert want <= seen, seen
    finally:
        g.close()


ALL_FOUR = {"private-private, one graph", "private-private, across", "private-shared", "shared-shared"}


# ---- the structural cases of the pass ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,chart", [(2, 0), (2, 1), (4, 0)])
def test_shared_mix(gpu, R, chart):
    J = jg.shared_mix_case(R)

    def ev(r):
        assert r.info["n_slots"] > 0 and r.drv.arrow and not J.relmeas and getattr(r.drv, "lam_dim", 0) == 0
    check_case(gpu, J, chart, ev, ALL_FOUR)


def test_relative_pose_factors(gpu):
    """Lambda rows (18 coordinates): the gram's D = -I part."""
    J = jg.relmeas_case(R=2, n_rel=3, P=14)

    def ev(r):
        assert r.drv.lam_dim == 18
    check_case(gpu, J, 0, ev, ALL_FOUR)


@pytest.mark.parametrize("coords", [64, 129])
def test_border_rows(gpu, coords):
    J = jg.border_case({64: (1, 5, 4), 129: (3, 10, 6)}[coords])

    def ev(r):
        assert r.info["sep_dim"] == coords
    check_case(gpu, J, 0, ev, {"private-private, one graph", "private-shared", "shared-shared"})


def test_segments(gpu, monkeypatch):
    """Bands cut into three segments: the landmarks' factors sit at band poses and at window poses (border rows of their robot)."""
    monkeypatch.delenv("SLIDE_SEGMENTS", raising=False)
    J = jg.segments_case()

    def ev(r):
        for sh in r.shards:
            segs, nwin = sh.graph.segments()
            assert len(segs) == 3 and nwin > 0, (segs, nwin)
    check_case(gpu, J, 0, ev, ALL_FOUR)


def test_separator_tiles(gpu):
    """Dissected separator: shared cubes of a leaf and of the top block paired across the halves (covariances; cubes have no test)."""
    J = jg.separator_tiles_case()

    def ev(r):
        Ta, Tb, used_a, used_b = r.info["sep_prof"][1]
        assert used_a > NB and used_b > NB and r.info["sep_dim"] - NB * (Ta + Tb) > NB
    check_case(gpu, J, 0, ev, {"private-private, across", "private-shared", "shared-shared"})


# ---- properties ------------------------------------------------------------------------------------------------------------------

def _all_pairs(c, kind, limit=24):
    ents = jp.job_landmarks(c, kind)
    rows = list(jp.side_pairs(c, kind).values())
    for i in range(len(ents)):
        for j in range(i + 1, len(ents)):
            row = (ents[i][0], ents[i][1], ents[j][0], ents[j][1])
            if row not in rows and len(rows) < limit:
                rows.append(row)
    return np.array(rows, np.int64)


def test_a_pair_does_not_depend_on_the_list(gpu):
    """129 point and 55 cylinder pairs (one more than a sweep holds), on a job with lambda rows: every pair's bits are those of the
    call that gives it alone, also in a permuted list; the driver's method is the batch's."""
    J = jg.relmeas_case(R=2, n_rel=3, P=14)
    g = GateRun(gpu, J)
    try:
        b = g.batch
        for kind, n in (("point", 129), ("cylinder", 55)):
            cls, sg = jp.CLS[kind], jp.SIGMA[kind]
            uniq = _all_pairs(g.c, kind)
            assert len(uniq) >= 10
            alone = [b.landmark_pair_mahalanobis(cls, uniq[k:k + 1], sg) for k in range(len(uniq))]
            assert all(a["status"][0] == 0 and a["d2"][0] > 0 for a in alone)
            pick = np.arange(n) % len(uniq)
            whole = b.landmark_pair_mahalanobis(cls, uniq[pick], sg)
            perm = np.random.default_rng(n).permutation(n)
            shuffled = b.landmark_pair_mahalanobis(cls, uniq[pick[perm]], sg)
            for i in range(n):
                for f in FIELDS:
                    assert np.array_equal(whole[f][i], alone[pick[i]][f][0]), (kind, i, f)
                    assert np.array_equal(shuffled[f][i], whole[f][perm[i]]), (kind, i, f)
            cov_alone = [b.get_landmark_pair_covariances(cls, uniq[k:k + 1])[0][0] for k in range(len(uniq))]
            m = 384 // (2 * jp.DIM[kind]) + 1                                  # one more than a sweep of the covariances holds
            pick = np.arange(m) % len(uniq)
            cov, st = b.get_landmark_pair_covariances(cls, uniq[pick])
            assert (st == 0).all() and all(np.array_equal(cov[i], cov_alone[pick[i]]) for i in range(m))
            drv = g.r.drv.landmark_pair_mahalanobis(cls, uniq[:3], sg)
            for f in FIELDS:
                assert np.array_equal(drv[f], whole[f][:3])
    finally:
        g.close()


def _search_want(g, kind, radius, cross_only):
    ents = jp.job_landmarks(g.c, kind)
    xyz = np.array([jp.anchor(kind, g.vals.lm(sl, kind, i)) for sl, i, _ in ents]).reshape(-1, 3)
    return ents, xyz, jp.brute_job_pairs(ents, xyz, lp.clear_radius(xyz, radius), cross_only)


def _check_search(got, want):
    for a, b in zip(got[:4], want[:4]):
        assert np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64))          # the set AND the order
    assert got[4].shape == want[4].shape and (np.abs(got[4] - want[4]) <= 1e-12 * want[4]).all()


@pytest.mark.parametrize("chart", [0, 1])
def test_planted_duplicates_across_robots(gpu, chart):
    """DupJoint: every planted pair against the reference; the decision at the 0.99 quantile equals the planted flag; the search
    against numpy on the union of the members' estimates (cross_only on and off, every shared slot once, a cap below the total); and
    duplicate_landmarks(cross_only=True) returns exactly the cross-robot true pairs and the private re-mapping of a shared point."""
    J = jp.DupJoint()
    g = GateRun(gpu, J, chart, okw=jp.DUP_OKW, kw=jp.DUP_KW)
    try:
        b, c = g.batch, g.c
        assert g.r.drv.lam_dim == 12
        for kind in ("point", "cylinder"):
            cls, D = jp.CLS[kind], jp.DIM[kind]
            rows, flags, cross, _ = jp.planted(c, kind)
            out = b.landmark_pair_mahalanobis(cls, rows, jp.SIGMA[kind])
            check_pairs(g, kind, rows, out, f"planted chart {chart}")
            q = gpu.chi2_quantile(0.99, D)
            print(f"[joint-lm-pairs] planted chart {chart} {kind}: true max {out['d2'][flags].max():.4f}, false min {out['d2'][~flags].min():.1f} "
                  f"(quantile {q:.3f})")
            assert np.array_equal(out["d2"] <= q, flags) and np.array_equal(out["d2"] <= jp.QUANTILE[D], flags)
            check_covs(g, kind, rows[:6], f"planted chart {chart}")
            for cross_only in (False, True):
                ents, xyz, want = _search_want(g, kind, 1.5, cross_only)
                got = b.landmark_pairs_within(cls, 1.5, cross_only)
                _check_search(got, want)
                assert len(got[0]) > 0
            assert len({(sl, i) for sl, i, _ in ents}) == len(ents) == sum(1 for k, *_ in J.lms if k == cls)      # shared slots once
            every = b.landmark_pairs_within(cls, 1.5)
            assert len(every[0]) > len(got[0])
            sa, ia, sb, ib, d2, dist = b.duplicate_landmarks(cls, 1.5, jp.SIGMA[kind], cross_only=True)
            kept = {frozenset([(int(w), int(x)), (int(y), int(z))]) for w, x, y, z in zip(sa, ia, sb, ib)}
            planted = {frozenset([(int(r[0]), int(r[1])), (int(r[2]), int(r[3]))]) for r, f, x in zip(rows, flags, cross) if f and x}
            assert kept == planted and len(kept) == len(sa), (kind, kept ^ planted)
            assert (d2 <= q).all() and (dist <= 1.5).all()
            both = g.r.drv.duplicate_landmarks(cls, 1.5, jp.SIGMA[kind])
            assert len(both[0]) == int(flags.sum())                                # (the same-robot duplicates too)
        # a cap below the total: SLIDE_ERR_CAPACITY, the total, nothing else written
        total = len(every[0])
        P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        for cap, rc_want in ((total - 1, CAPACITY), (total, 0)):
            sa, sb, ia, ib = np.full(total, 77, np.int32), np.full(total, 77, np.int32), np.full(total, 77, np.uint64), np.full(total, 77, np.uint64)
            dist, tot = np.full(total, 77.0), np.zeros(1, np.int64)
            rc = gpu.lib().slide_chol_batch_landmark_pairs_within(C.c_void_p(b.h), C.c_int(cls), C.c_double(1.5), C.c_int(0), C.c_int64(cap), P(sa),
                                                                  P(ia), P(sb), P(ib), P(dist), P(tot))
            assert rc == rc_want and tot[0] == total
            if rc:
                assert (sa == 77).all() and (ia == 77).all() and (sb == 77).all() and (ib == 77).all() and (dist == 77).all()
            else:
                _check_search((sa, ia, sb, ib, dist), every)
    finally:
        g.close()


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_search_straddles_the_chunk(gpu, n):
    """column_cap_case(n - 1): a union of n point landmarks (n - 1 of them around one pose of robot 0, two shared with robot 1) against
    numpy, cross_only on and off; a class the job does not hold gives no pair."""
    J = jg.column_cap_case(n_lm=n - 1)
    g = GateRun(gpu, J)
    try:
        for cross_only in (False, True):
            ents, xyz, want = _search_want(g, "point", 1.0, cross_only)
            assert len(ents) == n and sum(1 for e in ents if e[2] < 0) == 2
            _check_search(g.batch.landmark_pairs_within(2, 1.0, cross_only), want)
            assert len(want[0]) > (0 if cross_only else n // 2)
        ents, xyz, want = _search_want(g, "cube", 50.0, False)
        _check_search(g.batch.landmark_pairs_within(1, 50.0), want)
        assert len(ents) >= 1
        with pytest.raises(gpu.SlideError, match="SLIDE_ERR_INVALID"):
            g.batch.landmark_pairs_within(2, 0.0)
    finally:
        g.close()


def test_status_words(gpu):
    """SLIDE_MISSING: a slot the batch lacks, a landmark its graph does not hold, a landmark with neither a factor nor a shared slot;
    SLIDE_ERR_INVALID: one private landmark twice, two replicas of one shared slot (and one replica twice); each next to served
    neighbours with the bits they have alone."""
    J = jg.shared_mix_case(2)

    def prepare(r):
        r.shards[1].graph.add_point_landmark(999, [1.0, 2.0, 3.0])              # never observed, not shared
    g = GateRun(gpu, J, prepare=prepare)
    try:
        b, c = g.batch, g.c
        sg = jp.SIGMA["point"]
        named = jp.side_pairs(c, "point")
        good = np.array(list(named.values()), np.int64)
        alone = b.landmark_pair_mahalanobis(2, good, sg)
        assert (alone["status"] == 0).all() and (alone["d2"] > 0).all()
        assert len(good) == 3                                                     # (this job holds one private point per robot)
        pp, ps = named["private-private, across"], named["private-shared"]
        rep = jp.other_replica(c, "point", ps[2], ps[3])
        bad = [(2, 0, pp[2], pp[3]), (pp[0], pp[1], -1, 0),                        # a slot the batch lacks
               (pp[0], 777, pp[2], pp[3]),                                       # a landmark its graph does not hold
               (1, 999, pp[2], pp[3]), (pp[0], pp[1], 1, 999),                   # neither a factor nor a shared slot
               (pp[0], pp[1], pp[0], pp[1]),                                     # one private landmark twice
               (ps[2], ps[3], rep[0], rep[1]), (ps[2], ps[3], ps[2], ps[3])]      # two replicas of one shared slot; one replica twice
        want_bad = [MISSING] * 5 + [INVALID] * 3
        mixed = [good[0]] + bad[:3] + [good[1]] + bad[3:6] + [good[2]] + bad[6:]
        where = [0, 4, 8]
        want = [0] + want_bad[:3] + [0] + want_bad[3:6] + [0] + want_bad[6:]
        out = b.landmark_pair_mahalanobis(2, np.array(mixed, np.int64), sg)
        assert out["status"].tolist() == want, out["status"]
        assert out["dof"].tolist() == [3] * len(mixed)
        for k, w in enumerate(want):
            if w:
                assert out["d2"][k] == 0 and not out["C"][k].any() and not out["r"][k].any()
        for f in ("d2", "C", "r"):
            assert np.array_equal(out[f][where], alone[f]), f
        cov, st = b.get_landmark_pair_covariances(2, np.array(mixed, np.int64))
        assert st.tolist() == want and all(cov[k].any() == (w == 0) for k, w in enumerate(want))
        only_bad = b.landmark_pair_mahalanobis(2, np.array(bad, np.int64), sg)     # (no pair left: nothing is launched)
        assert only_bad["status"].tolist() == want_bad and not only_bad["d2"].any()
        empty = b.landmark_pair_mahalanobis(2, np.zeros((0, 4)), sg)
        assert len(empty["d2"]) == 0 and empty["C"].shape == (0, 9, 9)
        assert b.get_landmark_pair_covariances(1, np.zeros((0, 4)))[0].shape == (0, 18, 18)
        with pytest.raises(gpu.SlideError, match="SLIDE_ERR_INVALID"):              # an argument refusal on a live batch
            b.landmark_pair_mahalanobis(2, good, [0.05, 0.0, 0.05])
        sa, ia, sb, ib, _ = b.landmark_pairs_within(2, 100.0)                       # the factor-less landmark is a landmark of the job
        assert (1, 999) in set(zip(sb.tolist(), ib.tolist())) | set(zip(sa.tolist(), ia.tolist()))
    finally:
        g.close()


def test_whole_call_refusals(gpu):
    """joint_state's refusals — before a pass, after a cut pass, after a member changed, in PCG mode — and cubes in the test; nothing
    is written."""
    J = jg.shared_mix_case(2)
    P0 = J.sizes[0]
    I7 = np.array([1.0, 0, 0, 0, 0, 0, 1])
    rows = np.array([(0, 0, 1, 1)], np.int64)          # (two different shared landmarks, of either class used below)
    sg = jp.SIGMA["point"]

    def refused(b, drv, why):
        for call in (lambda: b.landmark_pair_mahalanobis(2, rows, sg), lambda: b.get_landmark_pair_covariances(2, rows),
                     lambda: b.landmark_pairs_within(2, 1.0), lambda: b.duplicate_landmarks(2, 1.0, sg)):
            with pytest.raises(gpu.SlideError, match=why):
                call()
        P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        cls, sa, ia = np.full(1, 2, np.int32), np.zeros(1, np.int32), np.zeros(1, np.uint64)
        sb, ib = np.ones(1, np.int32), np.ones(1, np.uint64)
        d2, dof, Cm, r9, st = np.full(1, 77.0), np.full(1, 77, np.int32), np.full(81, 77.0), np.full(9, 77.0), np.full(1, 77, np.int32)
        rc = gpu.lib().slide_chol_batch_landmark_pair_mahalanobis(C.c_void_p(b.h), C.c_int(1), P(cls), P(sa), P(ia), P(sb), P(ib), P(sg), P(sg), P(d2),
                                                                  P(dof), P(Cm), P(r9), P(st))
        assert rc == INVALID and all((a == 77).all() for a in (d2, dof, Cm, r9, st))

    r = Run(gpu, J, 0)
    try:
        refused(r.batch, r.drv, "no whole exact joint pass")
        r.drv.one_pass()
        sync()
        assert (r.batch.landmark_pair_mahalanobis(2, rows, sg)["status"] == 0).all()
        with pytest.raises(gpu.SlideError, match="neither SLIDE_CLS_ELLIPSOID nor SLIDE_CLS_CYLINDER"):
            r.batch.landmark_pair_mahalanobis(1, rows, np.full(3, 0.05))             # cubes: covariances only
        assert (r.batch.get_landmark_pair_covariances(1, rows)[1] == 0).all()
        r.drv.force_parts = True                                                     # a cut pass leaves no whole factor behind
        r.drv.one_pass()
        sync()
        refused(r.batch, r.drv, "no whole exact joint pass")
        r.drv.force_parts = False
        r.drv.one_pass()
        sync()
        assert (r.batch.landmark_pair_mahalanobis(2, rows, sg)["status"] == 0).all()
        G = r.shards[0].graph
        st, v = G.get_pose12(0, P0 - 1)
        est = np.concatenate([v[9:12] + np.array([1.0, 0.0, 0.0]), [0.0, 0.0, 0.0, 1.0]])
        G.add_keypose_between(0, P0 - 1, P0, I7, est)
        refused(r.batch, r.drv, "changed since the last exact joint pass")
    finally:
        r.close()
    rp = Run(gpu, J, 0, pcg_iters=20, pcg_tol=1e-10)
    try:
        rp.drv.one_pass()
        sync()
        refused(rp.batch, rp.drv, "does not run exact joint passes")
        with pytest.raises(ValueError):
            rp.drv.landmark_pair_mahalanobis(2, rows, sg)
        with pytest.raises(ValueError):
            rp.drv.landmark_pairs_within(2, 1.0)
    finally:
        rp.close()


def test_queries_leave_the_batch_as_it_was(gpu):
    """The cached joint Sigma, closure_info_gain_batch, observation_mahalanobis and the next pass of a batch that served the pair
    queries are bit for bit those of a batch that never did."""
    J = jg.relmeas_case(R=2, n_rel=3, P=14)

    def state(run, c):
        vals = jo.shard_values(run.shards)
        cov = [run.batch.get_pose_covariances(s, np.arange(J.sizes[s])) for s in range(J.R)]
        lmc = [run.batch.get_landmark_covariances(s, 2, np.arange(len(c.gid[s][2]))) for s in range(J.R)]
        gain = run.batch.closure_info_gain_batch(0, [[2, 9], [3, 11, 12]], [[4.0], [5.0, 1.0]])
        gate = run.batch.observation_mahalanobis(jo.perturbed_list(c, vals))
        return cov + lmc, gain, gate

    g = GateRun(gpu, J)
    try:
        c = g.c
        lists = {kind: _all_pairs(c, kind) for kind in ("point", "cylinder", "cube")}

        def queries():
            out = {kind: g.batch.landmark_pair_mahalanobis(jp.CLS[kind], lists[kind], jp.SIGMA[kind]) for kind in ("point", "cylinder")}
            return out, {kind: g.batch.get_landmark_pair_covariances(jp.CLS[kind], v)[0] for kind, v in lists.items()}, \
                [g.batch.landmark_pairs_within(cls, 2.0, True) for cls in (0, 1, 2)]
        first = queries()
        st1 = state(g.r, c)
        again = queries()                                                            # (with the joint Sigma cached now)
        for kind in first[0]:
            for f in FIELDS:
                assert np.array_equal(first[0][kind][f], again[0][kind][f]), (kind, f)
        for kind in lists:
            assert np.array_equal(first[1][kind], again[1][kind])
        for x, y in zip(first[2], again[2]):
            assert all(np.array_equal(p, q) for p, q in zip(x, y))
        g.r.drv.one_pass()
        sync()
        with_q = g.r.values()
    finally:
        g.close()
    r2 = Run(gpu, J, 0)
    try:
        r2.drv.one_pass()
        sync()
        st2 = state(r2, c)
        r2.drv.one_pass()
        sync()
        for a, b in zip(st1[0], st2[0]):
            assert np.array_equal(a, b)
        assert np.array_equal(st1[1][0], st2[1][0]) and np.array_equal(st1[1][1], st2[1][1])
        for f in ("d2", "C", "r", "status"):
            assert np.array_equal(st1[2][f], st2[2][f]), f
        assert np.array_equal(with_q, r2.values())
    finally:
        r2.close()
