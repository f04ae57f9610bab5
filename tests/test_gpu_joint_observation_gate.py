"""The Mahalanobis gate of landmark observations on the JOINT multi-robot graph, on the device
(slide_chol_batch_observation_mahalanobis: the forward half of the many-right-hand-side solve over the exact joint pass's tree and a
signed gram, host_gates.hip's joint_sigma_forms; obs_gate_kernels.hip's k_joint_obs_gate_lin / k_obs_gate_finish) against the dense
reference of tests/joint_observation_gate_cases.py.

Per case: one Run (tests/test_gpu_joint_step.py), the reference at the values read before the pass, one exact joint pass, then the
query; r, Ap and Al of the reference are taken at the poses and landmarks read back through get_pose12 / get_landmark after the pass,
z and the sigmas from observation_gate_cases.add_rules.  The bound is the single-graph gate's: tol x cond(C_ref), floor 1e-12
(observation_gate_cases.gate_bound), relative to d2_ref and entry-wise for C and r against max |C_ref|.  The independence and read-only
checks are bit for bit.  Every case asserts the structural edge it exists for.  SLIDE_ERR_NOT_SPD is not covered: C = I + (a positive
semi-definite matrix up to rounding) has no non-positive pivot on any graph these cases can build with finite input."""
import numpy as np
import pytest

import joint_closure_gate_cases as jc
import joint_graphs as jg
import joint_observation_gate_cases as jo
import observation_loss_cases as oc
import robust_cases as rc
from test_gpu_joint_marginals import dense_inverse
from test_gpu_joint_step import NB, Run

pytestmark = pytest.mark.gpu

MISSING = 1
FIELDS = ("d2", "C", "r", "dof")


def sync():
    import torch
    torch.cuda.synchronize()


class ParamRun(Run):
    """test_gpu_joint_step.Run with the reference and the shards under parameters of the caller's (okw: the oracle's keywords or its
    parameter object, kw: the product's default_params keywords)."""

    def __init__(self, s, J, chart=0, okw=None, kw=None):
        import torch
        from slide_slam_amd.distributed import PassDriver, setup_local_shards
        self.dev = torch.device("cuda", 0)
        self.J, self.chart = J, chart
        self.ref = jo.reference(J, chart, **(okw or {}))
        self.shards, assoc = jg.build(J, lambda: s.SlideGraph(s.default_params(pose_chart=chart, **(kw or {}))))
        self.gid = assoc[0]
        self.batch = s.CholBatch(J.R)
        for t, sh in enumerate(self.shards):
            sh.graph.join_chol_batch(self.batch, t)
        bufs, self.info = setup_local_shards(self.shards, None, device=self.dev, assoc=assoc)
        self.drv = PassDriver(self.shards, bufs, self.info["n_slots"], batch=self.batch, device=self.dev, arrow=True, sep_dim=self.info["sep_dim"],
                              sep_prof=self.info.get("sep_prof"))
        if J.relmeas:
            assert self.drv.setup_ghosts(J.relmeas) > 0


class GateRun:
    """One Run, the reference at the values the pass linearises at, then one exact joint pass."""

    def __init__(self, gpu, J, chart=0, evidence=None, okw=None, kw=None, prepare=None, case=None):
        self.r = ParamRun(gpu, J, chart, okw, kw)
        try:
            if prepare is not None:
                prepare(self.r)
            if evidence is not None:
                evidence(self.r)
            self.c = case(self.r) if case is not None else jo.JointObsCase(J, chart, ref=self.r.ref, vals=self.r.values(), **(okw or {}))
            self.r.drv.one_pass()
            sync()
            if evidence is not None:
                evidence(self.r)
        except BaseException:
            self.r.close()
            raise
        self.J, self.batch, self.tag = J, self.r.batch, f"chart {chart}"
        self.vals = jo.shard_values(self.r.shards)

    def check_gate(self, cands, tag=""):
        c = self.c
        out = self.batch.observation_mahalanobis(cands)
        rs, _, Cs, d2 = jo.ref_gate(c, cands, self.vals)
        assert (out["status"] == 0).all(), out["status"]
        worst = 0.0
        for k, cand in enumerate(cands):
            m = jo.KIND[cand[0]][3]
            assert out["dof"][k] == m
            bound = jo.gate_bound(c, Cs[k])
            top = float(np.abs(Cs[k]).max())
            e_d = abs(out["d2"][k] - d2[k]) / d2[k]
            e_C = float(np.abs(out["C"][k][:m, :m] - Cs[k]).max() / top)
            e_r = float(np.abs(out["r"][k][:m] - rs[k]).max() / top)
            print(f"[joint-obs-gate] {self.tag} {tag} {cand[0]} pose {cand[1:3]} landmark {jo.split(cand)[1], cand[3]}: d2 {out['d2'][k]:.6g} ref "
                  f"{d2[k]:.6g} err {e_d:.2e}, C {e_C:.2e}, r {e_r:.2e} (bound {bound:.2e})")
            assert max(e_d, e_C, e_r) <= bound, (k, e_d, e_C, e_r, bound)
            assert not out["C"][k][m:].any() and not out["C"][k][:, m:].any() and not out["r"][k][m:].any()
            worst = max(worst, max(e_d, e_C, e_r) / bound)
        assert np.array_equal(out["C"], np.transpose(out["C"], (0, 2, 1)))
        print(f"[joint-obs-gate] {self.tag} {tag}: largest error / bound {worst:.3e}; d2_ref from {d2.min():.3g} to {d2.max():.3g}")
        return out

    def check_existing_calls(self, cands, out):
        """C - I = Ap Spp Ap^T + Al Sll Al^T + (Ap Spl Al^T + its transpose).  Spp from get_pose_covariances and Sll from
        get_landmark_covariances (the cached joint Sigma: another route on the device), only the cross block Spl from the dense
        reference.  Two routes to one block agree to the existing 1e-9, here of the largest of the terms (they cancel where pose and
        landmark are strongly correlated); the reference's cross block carries its own error, tol x scale / (w_i w_j) per entry
        (test_gpu_joint_marginals' Jacobi-scaled tolerance), which enters through |Ap| . |Al|^T twice."""
        c, ref = self.c, self.c.ref
        worst = 0.0
        for k, cand in enumerate(cands):
            base, ls = jo.split(cand)
            kind, slot, p, l = base[:4]
            m = jo.KIND[kind][3]
            _, Ap, Al = jo.linearize(c, cand, self.vals)
            sel = c.sel(cand)
            Spp = self.batch.get_pose_covariances(slot, [p])[0]
            Sll = self.batch.get_landmark_covariances(ls, jo.KIND[kind][2], [l])[0]
            Spl, w = c.Sig[np.ix_(sel[:6], sel[6:])], c.w[sel]
            terms = [Ap @ Spp @ Ap.T, Al @ Sll @ Al.T, Ap @ Spl @ Al.T]
            want = np.eye(m) + terms[0] + terms[1] + terms[2] + terms[2].T
            cross = 2 * float((np.abs(Ap) @ (c.tol * c.scale / np.outer(w[:6], w[6:])) @ np.abs(Al).T).max())
            top = max(float(np.abs(t).max()) for t in terms + [want])
            err = float(np.abs(out["C"][k][:m, :m] - want).max())
            assert err <= 1e-9 * top + cross, (k, cand[:4], err, top, cross)
            worst = max(worst, err / (1e-9 * top + cross))
            if len(c.robots_of(ls, kind, l)) > 1 and kind == "point":
                assert np.abs(terms[1]).max() > 0
        print(f"[joint-obs-gate] {self.tag}: against get_pose_covariances / get_landmark_covariances, largest error / bound {worst:.3e}")

    def check_all(self, extra=()):
        c = self.c
        rows = list(jo.named_pairs(c)) + list(extra)
        notes = [x[5] for x in rows]
        kinds = {jo.CLS_KIND[k] for k, _, _, _ in c.J.lms}
        for kind in kinds:
            have = {n for x, n in zip(rows, notes) if x[0] == kind}
            assert {"observer", "not an observer", "first pose", "last pose", "cross-robot, private", "repeat"} <= have or \
                not any(x[0] == jo.KIND[kind][2] and len({r for r, _ in x[3]}) == 1 for x in c.J.lms), (kind, have)
            assert {"shared, own replica", "shared, other replica", "cross-robot, shared"} <= have or \
                not any(x[0] == jo.KIND[kind][2] and len({r for r, _ in x[3]}) > 1 for x in c.J.lms), (kind, have)
        cands = jo.perturbed_list(c, self.vals, extra)
        out = self.check_gate(cands, "perturbed")
        for k, (x, n) in enumerate(zip(rows, notes)):
            if n == "shared, other replica":                            # (the same landmark through the other robot's replica: one variable)
                assert notes[k - 1] == "shared, own replica"
                for f in FIELDS:
                    assert np.array_equal(out[f][k], out[f][k - 1]), (x, f)
            if n == "repeat":
                first = next(i for i, y in enumerate(rows) if y[:5] == x[:5])
                for f in FIELDS:
                    assert np.array_equal(out[f][k], out[f][first]), (x, f)
        self.check_existing_calls(cands, out)
        return out

    def close(self):
        self.r.close()


def run_all(gpu, J, chart=0, evidence=None, extra=None):
    g = GateRun(gpu, J, chart, evidence)
    try:
        g.check_all(extra(g) if extra is not None else ())
    finally:
        g.close()


# ---- the structural cases of the pass ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,chart", [(2, 0), (2, 1), (4, 0)])
def test_shared_mix(gpu, R, chart):
    """No relative-pose factor: the robots are coupled through the shared landmarks (the separator's rows of W) alone."""
    J = jg.shared_mix_case(R)

    def ev(r):
        assert r.info["n_slots"] > 0 and r.drv.arrow and not J.relmeas and getattr(r.drv, "lam_dim", 0) == 0
    run_all(gpu, J, chart, ev)


def test_relative_pose_factors(gpu):
    """Lambda rows (18 coordinates): the gram's D = -I part."""
    J = jg.relmeas_case(R=2, n_rel=3, P=14)

    def ev(r):
        assert r.drv.lam_dim == 18
    run_all(gpu, J, 0, ev)


@pytest.mark.parametrize("coords", [64, 129])
def test_border_rows(gpu, coords):
    """Robot 0's border of 64 / 129 coordinates: one tile, and past two tiles."""
    J = jg.border_case({64: (1, 5, 4), 129: (3, 10, 6)}[coords])

    def ev(r):
        assert r.info["sep_dim"] == coords
    run_all(gpu, J, 0, ev)


def test_segments(gpu, monkeypatch):
    """Bands cut into three segments: a window pose (its rows are border rows of its robot's system) as the candidate's pose, against
    a private landmark whose own factors sit at a band pose and a window pose, against a shared landmark, and from the other robot."""
    monkeypatch.delenv("SLIDE_SEGMENTS", raising=False)
    J = jg.segments_case()
    P = J.sizes[0]
    w = P // 3 + 1                                                        # (the window behind the first cut starts at pose P // 3)

    def ev(r):
        for sh in r.shards:
            segs, nwin = sh.graph.segments()
            assert len(segs) == 3 and nwin > 0, (segs, nwin)
            assert 6 * (w + 1) <= NB * segs[1][0], (w, segs)              # pose w lies before the second segment's first row: in the window

    def extra(g):
        c = g.c
        cut = next(gl for cls, gl, _, obs in J.lms if cls == 2 and obs == [(0, P // 3 - 2), (0, P // 3 + 12)])
        l = jo.local_id(c, 0, 2, cut)
        sh = next((cls, gl, obs) for cls, gl, _, obs in J.lms if len({r for r, _ in obs}) > 1)
        ls = jo.local_id(c, 0, sh[0], sh[1])
        return [("point", 0, w, 0, l, "window pose, private"), ("point", 0, P // 3 + 12, 0, l, "observer in the window"),
                ("point", 1, 20, 0, l, "cross-robot onto the cut's landmark"), ("point", 1, w, 0, l, "the other robot's window pose"),
                (jo.CLS_KIND[sh[0]], 0, w, 0, ls, "window pose, shared")]
    run_all(gpu, J, 0, ev, extra)


def test_separator_tiles(gpu):
    """Dissected separator (cubes in leaf a, leaf b and the top block): shared cubes of each, named across the halves."""
    J = jg.separator_tiles_case()

    def ev(r):
        Ta, Tb, used_a, used_b = r.info["sep_prof"][1]
        top = r.info["sep_dim"] - NB * (Ta + Tb)
        assert used_a > NB and used_b > NB and top > NB, (Ta, Tb, used_a, used_b, top)

    def extra(g):
        c = g.c
        out = []
        for pair, note in (((0, 1), "leaf a"), ((2, 3), "leaf b"), ((1, 2), "top block")):
            gl = next(gl for cls, gl, _, obs in J.lms if cls == 1 and tuple(sorted({r for r, _ in obs})) == pair)
            o = 3 - pair[0]                                               # (for the leaves: a robot of the other half)
            out += [("cube", pair[1], 7, pair[0], jo.local_id(c, pair[0], 1, gl), note),
                    ("cube", o, 5, pair[1], jo.local_id(c, pair[1], 1, gl), note + ", from robot %d" % o)]
        return out
    run_all(gpu, J, 0, ev, extra)


# ---- properties ------------------------------------------------------------------------------------------------------------------

def _same(a, b, ka, kb, what):
    for f in FIELDS:
        assert np.array_equal(a[f][ka], b[f][kb]), (what, f, ka, kb)


def test_candidates_do_not_depend_on_their_neighbours(gpu):
    """129 points, 43 cubes and 55 cylinders (one more than a sweep holds of each; private and shared landmarks, about half of the
    candidates cross-robot), on a job with lambda rows: d2, C and r of a candidate are bit for bit what the call gives for it alone,
    in its class's list, in a permuted list and in a mixed-class list; C is symmetric bit for bit."""
    J = jg.relmeas_case(R=2, n_rel=3, P=14)
    g = GateRun(gpu, J)
    try:
        b = g.batch
        lists = jo.long_lists(g.c, g.vals)
        rng = np.random.default_rng(11)
        fulls = {}
        for kind, cl in lists.items():
            full = fulls[kind] = b.observation_mahalanobis(cl)
            assert (full["status"] == 0).all() and (full["d2"] > 0).all()
            assert sum(jo.split(x)[1] != x[1] for x in cl[:24]) >= 4
            for k in list(range(24)) + [len(cl) - 1]:                            # every distinct candidate alone, and the second sweep's
                _same(b.observation_mahalanobis([cl[k]]), full, 0, k, kind)
            _same(full, full, 24, 0, kind)                                       # exact duplicates
            perm = rng.permutation(len(cl))
            sh = b.observation_mahalanobis([cl[k] for k in perm])
            for f in FIELDS:
                assert np.array_equal(sh[f], full[f][perm]), (kind, f)
            assert np.array_equal(full["C"], np.transpose(full["C"], (0, 2, 1)))
        mixed = [lists[kind][i] for i in range(20) for kind in ("cube", "point", "cylinder")]
        mx = b.observation_mahalanobis(mixed)
        for i in range(20):
            for n, kind in enumerate(("cube", "point", "cylinder")):
                _same(fulls[kind], mx, i, 3 * i + n, "mixed " + kind)
        _same(g.r.drv.observation_mahalanobis(mixed[:3]), mx, slice(0, 3), slice(0, 3), "driver")      # (the driver's method is the batch's)
    finally:
        g.close()


@pytest.mark.parametrize("chart", [0, 1])
def test_planted_true_and_false_matches(gpu, chart):
    """The generator has asserted under d2_ref alone that the true candidates lie below 0.75 of their class's quantile and the false
    ones above twice it (cross-robot ones on both sides); the device puts each on the same side of the quantile, at its own estimate."""
    J = jo.PlantedJoint()
    g = GateRun(gpu, J, chart, okw=jo.PLANTED_OKW, kw=jo.PLANTED_KW)
    try:
        cands, flags, _, dof = jo.planted_list(g.c)
        out = g.check_gate(cands, "planted")
        assert (out["dof"] == dof).all()
        q = np.array([gpu.OBSERVATION_GATE_CHI2_99[int(d)] for d in out["dof"]])
        for m in (3, 7, 9):
            s = dof == m
            print(f"[joint-obs-gate] planted chart {chart} dof {m}: true max {out['d2'][s & flags].max():.2f}, false min "
                  f"{out['d2'][s & ~flags].min():.1f} (quantile {gpu.OBSERVATION_GATE_CHI2_99[m]})")
        assert ((out["d2"] < q) == flags).all(), (out["d2"], q, flags)
    finally:
        g.close()


def test_gate_noise_is_the_base_noise_under_an_observation_loss(gpu):
    """Under a batch Huber observation loss the call is served; K is the reweighted joint system (the reference is built from the
    factors scaled by the loss's weights at the point the pass linearises, observation_loss_cases.obs_step), the candidate's own noise
    is the base noise and C's identity is unscaled."""
    import joint_observation_loss_cases as jl
    J = jl.kinds_case()
    okw, kw = oc.params(0)
    seen = {}

    def prepare(r):
        r.drv.set_observation_loss("huber")

    def case(r):
        ref, vals = r.ref, r.values()
        sel = oc.selected(ref)
        _, _, w, _, _ = oc.obs_step(ref, vals, rc.HUBER, 0.0, sel)
        assert (w[sel] < 0.9).sum() >= 3                                  # the loss does reweight this graph
        seen["plain"] = dense_inverse(ref, vals)[0]
        base = ref.fsig
        ref.fsig = base / np.sqrt(w)[:, None]
        try:
            return jo.JointObsCase(J, 0, ref=ref, vals=vals, params=okw)
        finally:
            ref.fsig = base
    kw = {k: v for k, v in kw.items() if k != "pose_chart"}
    g = GateRun(gpu, J, 0, okw=dict(bearing_sigma=oc.SIGMA, cyl_sigma=oc.SIGMA), kw=kw, prepare=prepare, case=case)
    try:
        cands = jo.perturbed_list(g.c, g.vals)
        out = g.check_gate(cands, "huber")
        # the same candidates against the unweighted H differ: the weights did enter Sigma
        g.c.Sig = seen["plain"]
        _, _, _, d2u = jo.ref_gate(g.c, cands, g.vals)
        assert np.abs(d2u / out["d2"] - 1).max() > 1e-3
    finally:
        g.close()


def test_status_per_candidate(gpu):
    """A slot the batch does not have (as the pose's and as the landmark's), a pose and a landmark its graph does not hold: zeros and
    SLIDE_MISSING for that candidate, its neighbours served with the bits they have alone.  A member's own
    SlideGraph.observation_mahalanobis keeps refusing, as it does for any graph joined to a batch."""
    J = jg.shared_mix_case(2)
    g = GateRun(gpu, J)
    try:
        b, c = g.batch, g.c
        rows = [x for x in jo.named_pairs(c) if x[5] in ("not an observer", "cross-robot, private", "shared, other replica")]
        good = [jo.at_estimate(c, g.vals, k, s, p, l, 0.5 * np.ones(jo.KIND[k][3]), ls) for k, s, p, ls, l, _ in rows]
        assert len(good) == 9
        pt = next(x for x in good if x[0] == "point")
        n = jo.NARGS["point"]
        bad = [("point", 0, J.sizes[0] + 5) + pt[3:n],                              # a pose its graph does not hold
               ("point", 0, 3, 999) + pt[4:n],                                      # a landmark its graph does not hold
               ("point", 2, 3) + pt[3:n],                                           # a slot the batch does not have
               ("point", 0, 3) + pt[3:n] + (2,),                                    # ... as the landmark's slot
               ("cube", 1, 3, 999) + next(x for x in good if x[0] == "cube")[4:jo.NARGS["cube"]] + (0,)]
        mixed = [good[0], bad[0], good[1], bad[1], bad[2]] + good[2:5] + [bad[3], bad[4]] + good[5:]
        where = [0, 2, 5, 6, 7, 10, 11, 12, 13]
        out, alone = b.observation_mahalanobis(mixed), b.observation_mahalanobis(good)
        assert (alone["status"] == 0).all()
        assert out["status"].tolist() == [0, MISSING, 0, MISSING, MISSING, 0, 0, 0, MISSING, MISSING, 0, 0, 0, 0]
        assert out["dof"].tolist() == [jo.KIND[x[0]][3] for x in mixed]
        for k in (1, 3, 4, 8, 9):
            assert out["d2"][k] == 0 and not out["C"][k].any() and not out["r"][k].any()
        for f in FIELDS:
            assert np.array_equal(out[f][where], alone[f]), f
        only_bad = b.observation_mahalanobis(bad)                                   # (no candidate left: nothing is launched)
        assert only_bad["status"].tolist() == [MISSING] * 5 and not only_bad["d2"].any()
        empty = b.observation_mahalanobis([])
        assert empty["d2"].shape == (0,) and empty["C"].shape == (0, 9, 9)
        with pytest.raises(gpu.SlideError, match="SLIDE_ERR_INVALID"):              # (an argument refusal on a live batch)
            b.observation_mahalanobis([("point", 0, 3, 0, [0.0, 0.0, 0.0], 5.0)])
        member = ("point", 0, 3, 0, [1.0, 0.0, 0.0], 5.0)
        with pytest.raises(gpu.SlideError, match="SLIDE_ERR_INVALID"):
            g.r.shards[0].graph.observation_mahalanobis([member])
    finally:
        g.close()


def test_whole_call_refusals(gpu):
    """joint_state's refusals: before a pass, after a graph changed, in PCG mode; nothing is written."""
    import ctypes as C
    J = jg.shared_mix_case(2)
    P0 = J.sizes[0]
    I7 = np.array([1.0, 0, 0, 0, 0, 0, 1])
    cand = ("point", 0, 3, 0, [1.0, 0.0, 0.0], 5.0, 1)

    def raw(b):
        L = gpu.lib()
        P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
        n, k, slot, pidx, cls, lidx, meas, lslot = gpu.api._observation_arrays([cand], True)
        d2, dof, Cm, r9, st = np.full(1, 77.0), np.full(1, 77, np.int32), np.full(81, 77.0), np.full(9, 77.0), np.full(1, 77, np.int32)
        rc_ = L.slide_chol_batch_observation_mahalanobis(C.c_void_p(b.h), C.c_int(1), P(slot), P(pidx), P(lslot), P(cls), P(lidx), P(meas), P(d2),
                                                         P(dof), P(Cm), P(r9), P(st))
        return rc_, all((a == 77).all() for a in (d2, dof, Cm, r9, st))

    r = Run(gpu, J, 0)
    try:
        with pytest.raises(gpu.SlideError, match="no whole exact joint pass"):
            r.batch.observation_mahalanobis([cand])
        assert raw(r.batch) == (-1, True)
        r.drv.one_pass()
        sync()
        assert raw(r.batch) == (0, False)
        G = r.shards[0].graph
        st, v = G.get_pose12(0, P0 - 1)
        est = np.concatenate([v[9:12] + np.array([1.0, 0.0, 0.0]), [0.0, 0.0, 0.0, 1.0]])
        G.add_keypose_between(0, P0 - 1, P0, I7, est)
        with pytest.raises(gpu.SlideError, match="changed since the last exact joint pass"):
            r.batch.observation_mahalanobis([cand])
        assert raw(r.batch) == (-1, True)
    finally:
        r.close()
    rp = Run(gpu, J, 0, pcg_iters=20, pcg_tol=1e-10)
    try:
        rp.drv.one_pass()
        sync()
        with pytest.raises(gpu.SlideError, match="does not run exact joint passes"):
            rp.batch.observation_mahalanobis([cand])
        assert raw(rp.batch) == (-1, True)
        with pytest.raises(ValueError):
            rp.drv.observation_mahalanobis([cand])
    finally:
        rp.close()


def test_queries_leave_the_batch_as_it_was(gpu):
    """The cached joint Sigma, closure_mahalanobis, observation_weights and the next pass of a batch that served observation queries
    are bit for bit those of a batch that never did."""
    J = jg.relmeas_case(R=2, n_rel=3, P=14)

    def state(run):
        vals = jo.shard_values(run.shards)
        cov = [run.batch.get_pose_covariances(s, np.arange(J.sizes[s])) for s in range(J.R)]
        gate = run.batch.closure_mahalanobis(jc.perturbed_list(J, vals.pose12))
        ow = run.batch.observation_weights()
        return cov, gate, ow

    g = GateRun(gpu, J)
    try:
        lists = jo.long_lists(g.c, g.vals)
        first = {k: g.batch.observation_mahalanobis(v) for k, v in lists.items()}
        st1 = state(g.r)
        again = {k: g.batch.observation_mahalanobis(v) for k, v in lists.items()}          # (with the joint Sigma cached now)
        for k in lists:
            _same(first[k], again[k], slice(None), slice(None), k)
        g.r.drv.one_pass()
        sync()
        with_q = g.r.values()
    finally:
        g.close()
    r2 = Run(gpu, J, 0)
    try:
        r2.drv.one_pass()
        sync()
        st2 = state(r2)
        r2.drv.one_pass()
        sync()
        for a, b in zip(st1[0], st2[0]):
            assert np.array_equal(a, b)
        for f in ("d2", "C", "r"):
            assert np.array_equal(st1[1][f], st2[1][f]), f
        for f in ("weight", "s2", "slot", "pose_idx", "cls", "lm_idx"):
            assert np.array_equal(st1[2][f], st2[2][f]), f
        assert np.array_equal(with_q, r2.values())
    finally:
        r2.close()
