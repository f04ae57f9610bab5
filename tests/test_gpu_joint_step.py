"""Each batched pass of the sharded solve (CholBatch.pass_all: all robots in one replayed hipGraph) against the JOINT Gauss-Newton
step: the step of one graph holding every robot, computed by gn_reference (the full whitened Jacobian by QR), which
shares no code with the kernels.  tests/joint_graphs.py describes each multi-robot graph once and emits it into the joint oracle
graph and into one SlideGraph shard per robot; test_joint_reference.py checks the builders and the reference on the CPU.

Per case: two passes, each against the reference rebuilt at the point the pass starts from; every pose (get_pose12(0, k) of each
shard) and every landmark (get_landmark; a shared landmark from EVERY replica, which must agree bit for bit); before the first pass
the values read back are the built ones (a shared landmark: its owner's).  Every case asserts that its edge was reached.  The exact
joint pass (arrow) covers k_landmark_b<3>, k_schur_lb / k_schur_b, the border fill and product, the separator solve (with the lambda
rows of relative-pose factors), the segments and the back-substitution; the PCG pass covers k_landmark_b<1> / <2>,
k_shared_unpack_b and k_schur_b through launch_phase3_batched."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_graphs as jg                                                      # noqa: E402
from gn_reference import scaled_error, tolerance                              # noqa: E402
from test_gn_reference import numdiff_floor                                    # noqa: E402
from test_joint_reference import joint_reference, read_values                  # noqa: E402

pytestmark = pytest.mark.gpu

LM_RED_MAX = 24           # solver_kernels.hip: k_landmark_b<3> reduces through LDS in rounds of this many lanes
SCHUR_PJ_CAP = 256        # solver_kernels.hip: entries of the column pose's list k_schur_b keeps in LDS
CHOL_BATCH_MAX = 8
NB = 64


class Run:
    """The shards of J in one CholBatch, set up by setup_local_shards and driven by PassDriver (exact joint pass, or PCG)."""

    def __init__(self, s, J, chart, pcg_iters=0, pcg_tol=0.0):
        import torch
        from slide_slam_amd.distributed import PassDriver, setup_local_shards
        self.dev = torch.device("cuda", 0)
        self.J, self.chart = J, chart
        self.ref, _ = joint_reference(J, chart)
        self.shards, assoc = jg.build(J, lambda: s.SlideGraph(s.default_params(pose_chart=chart)))
        self.gid = assoc[0]
        self.batch = s.CholBatch(J.R)
        for t, sh in enumerate(self.shards):
            sh.graph.join_chol_batch(self.batch, t)
        bufs, self.info = setup_local_shards(self.shards, None, device=self.dev, assoc=assoc)
        self.drv = PassDriver(self.shards, bufs, self.info["n_slots"], batch=self.batch, device=self.dev, pcg_iters=pcg_iters,
                              pcg_tol=pcg_tol, arrow=not pcg_iters, sep_dim=self.info["sep_dim"], sep_prof=self.info.get("sep_prof"))
        if J.relmeas:
            assert self.drv.setup_ghosts(J.relmeas) > 0

    def values(self):
        return read_values(self.shards, self.gid, self.ref, self.J.sizes)

    def check(self, steps=2, extra=None):
        """`steps` passes, each against the joint step at the point it starts from; returns the worst scaled_error / tolerance, the
        tolerance being gn_reference.tolerance alone.  extra(run, H, tol, kappa), called after each pass -> a term added to the
        tolerance (the PCG passes' bound)."""
        import torch
        vals = self.values()
        assert np.array_equal(vals, self.ref.values)          # (the pass starts where the reference starts: owners' values)
        worst = 0.0
        for s in range(steps):
            dx, H = self.ref.step(vals)
            self.drv.one_pass()
            torch.cuda.synchronize()
            new = self.values()
            got = self.ref.tangent(vals, new)
            tol, kappa = tolerance(H, dx, self.ref.magnitude(vals), numdiff_floor(self.ref, dx, H, vals))
            add = extra(self, H, tol, kappa) if extra is not None else 0.0
            err = scaled_error(got, dx, H)
            assert np.linalg.norm(dx) > 1e-6                   # (the step really moves the graph)
            assert err <= tol + add, (s, err, tol, add, kappa)
            worst = max(worst, err / tol)
            vals = new
        return worst

    def close(self):
        for sh in self.shards:
            sh.graph.join_chol_batch(None)


def run_case(s, J, chart=0, steps=2, evidence=None, pcg_iters=0, pcg_tol=0.0, extra=None):
    r = Run(s, J, chart, pcg_iters, pcg_tol)
    try:
        if evidence is not None:
            evidence(r)
        ratio = r.check(steps, extra)
        if evidence is not None:
            evidence(r)                 # (after the passes as well: the layout the passes used)
        return r, ratio
    finally:
        r.close()


def _report(family, ratio):
    print(f"[joint-step] {family}: worst scaled_error / tolerance {ratio:.3e}")


# ---- k_landmark_b<3>: one landmark with 1 .. 130 factors -------------------------------------------------------------------------

COUNTS = [1, 23, 24, 25, 48, 49, 64, 65, 130]


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("cls", [0, 1, 2], ids=["cyl", "cube", "point"])
@pytest.mark.parametrize("nf", COUNTS)
def test_private_landmark_factor_count(gpu, chart, cls, nf):
    """A private landmark (D = 7 / 9 / 3) with nf factors: one LDS round of LM_RED_MAX lanes, its edges, more than one factor per
    lane."""
    J = jg.landmark_count_case(cls, nf)

    def ev(r):
        _, per_lm = r.ref.list_lengths()
        assert per_lm[r.ref.lm_var(cls, 0)] == nf
        assert r.gid[0][cls][0] == 0 and 0 not in r.gid[1][cls]      # (robot 1 does not see it: private)
    _, ratio = run_case(gpu, J, chart, evidence=ev)
    _report("private landmark count", ratio)


@pytest.mark.parametrize("cls", [0, 1, 2], ids=["cyl", "cube", "point"])
@pytest.mark.parametrize("nf", COUNTS)
def test_separator_landmark_factor_count(gpu, cls, nf):
    """The same counts on a separator landmark (robot 1 sees it once more): its sums go to lm_Hacc for the border."""
    J = jg.landmark_count_case(cls, nf, shared=True)

    def ev(r):
        _, per_lm = r.ref.list_lengths()
        assert per_lm[r.ref.lm_var(cls, 0)] == nf + 1
        assert 0 in r.gid[1][cls] and r.info["n_slots"] >= 2
    _, ratio = run_case(gpu, J, 0, evidence=ev)
    _report("separator landmark count", ratio)


# ---- shared landmarks, batch shapes --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("R", [2, 3, 4, 8])
def test_shared_landmarks(gpu, R, chart):
    """Landmarks seen by two robots, by every robot, and many times by robot 0 and once by the last.  3 robots: no dissection;
    4 and 8 (CHOL_BATCH_MAX): the two-half dissection."""
    J = jg.shared_mix_case(R, sizes=[12] * R if R < 8 else [10] * R)

    def ev(r):
        blocks = r.info["sep_prof"][1] if isinstance(r.info["sep_prof"], tuple) else None
        assert (blocks is not None) == (R in (4, 8))
        obs = [len({a for a, _ in J.observers(cls, g)}) for cls in range(3) for g in range(J.n_global[cls])]
        assert max(obs) == R and obs.count(2) >= R
    _, ratio = run_case(gpu, J, chart, evidence=ev)
    _report("shared landmarks", ratio)


@pytest.mark.parametrize("sizes,private", [([10, 33, 65, 150], ()), ([150, 10, 65, 33], (1,)), ([33, 10], ()),
                                           ([65, 10, 33], (2,))], ids=["4-mixed", "4-mixed-empty-border", "2-mixed", "3-empty-border"])
def test_robot_sizes(gpu, sizes, private):
    """Robots of different sizes and landmark counts in one batch: every grid is sized for the largest (the early exits of the
    smaller ones, k_pad_rhs_b's padding); a robot that shares nothing has an empty border."""
    J = jg.sizes_case(sizes, private_only=private)

    def ev(r):
        assert r.info["n_slots"] > 0
        for t in range(J.R):
            if t in private:        # (robot t observes no landmark another robot observes, and its band is too short to cut)
                assert all({a for a, _ in J.observers(c, int(g))} == {t} for c in range(3) for g in r.gid[t][c])
                assert len(r.shards[t].graph.border_profile()) == 0
            else:
                assert len(r.shards[t].graph.border_profile()) > 0
    _, ratio = run_case(gpu, J, 0, evidence=ev)
    _report("robot sizes", ratio)


# ---- Schur assembly paths ------------------------------------------------------------------------------------------------------

def _strip_width(G, Pn):
    """build_schur_pairs' W: the widest Schur strip of the tile profile, in poses (Pn poses)."""
    prof = G.tile_profile()
    w = 1
    for pj in range(Pn):
        c = (6 * pj + 5) // NB
        if c >= len(prof):
            break
        w = max(w, min(Pn, ((int(prof[c]) + 1) * NB + 5) // 6) - pj)
    return w


@pytest.mark.parametrize("walk_env", [False, True], ids=["pairs", "walk-env"])
def test_schur_pair_lists_and_walk(gpu, monkeypatch, walk_env):
    """k_schur_lb (pair lists, the default) and k_schur_b (the walk) on the same graph: SLIDE_SCHUR_WALK=1 forces the walk."""
    if walk_env:
        monkeypatch.setenv("SLIDE_SCHUR_WALK", "1")
    J = jg.shared_mix_case(2, sizes=[40, 40])

    _, ratio = run_case(gpu, J, 0, evidence=_ev_pairs(J))
    _report("schur " + ("walk (env)" if walk_env else "pairs"), ratio)


def test_schur_walk_wide_strip(gpu):
    """A landmark re-observed 270 poses later: the strip is wider than 256 poses and build_schur_pairs falls back to the walk."""
    J = jg.walk_case()

    def ev(r):
        assert _strip_width(r.shards[0].graph, J.sizes[0]) > 256
    _, ratio = run_case(gpu, J, 0, evidence=ev)
    _report("schur walk (wide strip)", ratio)


@pytest.mark.parametrize("walk", [False, True], ids=["pairs", "walk"])
def test_schur_column_past_lds_cap(gpu, monkeypatch, walk):
    """A column pose with more than SCHUR_PJ_CAP landmark factors: k_schur_b reads the entries past the cap from global memory."""
    if walk:
        monkeypatch.setenv("SLIDE_SCHUR_WALK", "1")
    J = jg.column_cap_case()

    _, ratio = run_case(gpu, J, 0, evidence=_ev_cap(J))
    _report("schur column past the LDS cap", ratio)


def _child(case, env):
    """A case in a fresh process (the launchers read SLIDE_SCHUR_SPLIT / SLIDE_SCHUR_XCD into static locals)."""
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), case], cwd=ROOT, env=e, timeout=600,
                       capture_output=True, text=True)
    sys.stdout.write(r.stdout[-4000:])
    sys.stderr.write(r.stderr[-4000:])
    assert r.returncode == 0, r.returncode
    return json.loads(r.stdout.strip().splitlines()[-1])


# Which launcher reads which knob (solver_kernels.hip): SLIDE_SCHUR_XCD only launch_phase3_arrow_batched (k_schur_lb's workgroup order,
# exact joint passes on pair lists); SLIDE_SCHUR_SPLIT only launch_schur (un-batched) and launch_phase3_batched (k_schur_b of the PCG
# pass) — the exact joint pass takes its split from the graphs.  Each variant runs on the pass that reads it.

def test_schur_xcd_order(gpu):
    """SLIDE_SCHUR_XCD=1 on exact joint passes through k_schur_lb (pair lists)."""
    _report("schur launch SLIDE_SCHUR_XCD=1", max(_child("schur_xcd", {"SLIDE_SCHUR_XCD": "1"})))


@pytest.mark.parametrize("split", ["1", "3"])
def test_schur_split_on_pcg_pass(gpu, split):
    """SLIDE_SCHUR_SPLIT on the batched PCG pass (k_schur_b's grid: split workgroups per pose column; the default is 2)."""
    _report(f"pcg schur launch SLIDE_SCHUR_SPLIT={split}", max(_child("schur_split_pcg", {"SLIDE_SCHUR_SPLIT": split})))


def _ev_pairs(J):
    def ev(r):
        assert _strip_width(r.shards[0].graph, J.sizes[0]) <= 256
    return ev


def _ev_cap(J):
    def ev(r):
        per_pose, _ = r.ref.list_lengths()
        assert per_pose[r.ref.pose_var(0, 2)] > SCHUR_PJ_CAP
    return ev


def _child_main(case):
    import slide_slam_amd as s
    out = []
    if case == "schur_xcd":
        assert os.environ.get("SLIDE_SCHUR_XCD") == "1" and "SLIDE_SCHUR_WALK" not in os.environ
        J = jg.shared_mix_case(2, sizes=[40, 40])
        out.append(run_case(s, J, 0, evidence=_ev_pairs(J))[1])
    elif case == "schur_split_pcg":
        assert int(os.environ["SLIDE_SCHUR_SPLIT"]) != 2
        for J, ev in ((jg.shared_mix_case(2, sizes=[40, 40]), _ev_pairs), (jg.column_cap_case(), _ev_cap)):
            out.append(_pcg_case(s, J, ev(J)))
    return out


# ---- border rows, separator tiles, segments ------------------------------------------------------------------------------------

BORDERS = {63: (9, 0, 0), 64: (1, 5, 4), 65: (2, 5, 2), 128: (5, 10, 1), 129: (3, 10, 6)}


@pytest.mark.parametrize("coords", sorted(BORDERS))
def test_border_rows(gpu, coords):
    """Robot 0's border holds 63 / 64 / 65 / 128 / 129 coordinates, from mixes of 7 / 9 / 3-dimensional slots."""
    mix = BORDERS[coords]
    assert sum(n * d for n, d in zip(mix, (7, 9, 3))) == coords
    J = jg.border_case(mix)

    def ev(r):
        assert r.info["sep_dim"] == coords
        assert len(r.shards[0].graph.border_profile()) == (coords + NB - 1) // NB
    _, ratio = run_case(gpu, J, 0, evidence=ev)
    _report("border rows", ratio)


def test_separator_blocks_cross_tiles(gpu):
    """Four robots, dissected: each leaf block and the top block hold more than one tile of coordinates."""
    J = jg.separator_tiles_case()

    def ev(r):
        Ta, Tb, used_a, used_b = r.info["sep_prof"][1]
        top = r.info["sep_dim"] - NB * (Ta + Tb)
        assert used_a > NB and used_b > NB and top > NB, (Ta, Tb, used_a, used_b, top)
    _, ratio = run_case(gpu, J, 0, evidence=ev)
    _report("separator blocks", ratio)


@pytest.mark.parametrize("seg", [None, "1", "2", "4"], ids=["default3", "1", "2", "4"])
def test_segments(gpu, monkeypatch, seg):
    """Robots of 150 poses: PassDriver cuts every band into SLIDE_SEGMENTS segments (3 unset)."""
    if seg is None:
        monkeypatch.delenv("SLIDE_SEGMENTS", raising=False)
    else:
        monkeypatch.setenv("SLIDE_SEGMENTS", seg)
    n = 3 if seg is None else int(seg)
    J = jg.segments_case()

    def ev(r):
        for sh in r.shards:
            segs, _ = sh.graph.segments()
            if n == 1:
                assert segs == []
            else:
                assert len(segs) == n, segs
    _, ratio = run_case(gpu, J, 0, evidence=ev)
    _report("segments", ratio)


# ---- relative-pose factors -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("R,n_rel", [(2, 3), (4, 11)], ids=["2x3", "4x11"])
def test_relative_pose_factors(gpu, R, n_rel, chart):
    """Inter-robot relative-pose factors between equal and different key-frame indices; 11 of them = 66 lambda coordinates (past
    one tile).  The second pass linearises them at the refreshed ghosts."""
    J = jg.relmeas_case(R, n_rel)

    def ev(r):
        assert r.drv.lam_dim == 6 * n_rel
        assert any(e[0] == e[4] for e in J.relmeas) and any(e[0] != e[4] for e in J.relmeas)
    _, ratio = run_case(gpu, J, chart, evidence=ev)
    _report("relative-pose factors", ratio)


# ---- the batched PCG pass ------------------------------------------------------------------------------------------------------

PCG_ITERS, PCG_TOL = 300, 1e-14


def _pcg_kappa(ref, H):
    """kappa(M^-1 S): S = the joint graph's Schur complement onto the poses (the system the PCG pass solves), M = its diagonal robot
    blocks (every robot's own factor, the preconditioner)."""
    import scipy.linalg
    pose = np.zeros(ref.n, bool)
    robot = np.full(ref.n, -1)
    for k in range(len(ref.vtype)):
        if int(ref.vtype[k]) == 0:
            pose[ref.off[k]:ref.off[k + 1]] = True
            robot[ref.off[k]:ref.off[k + 1]] = int(ref.vkey[k]) >> 56
    p, l = np.nonzero(pose)[0], np.nonzero(~pose)[0]
    S = H[np.ix_(p, p)] - H[np.ix_(p, l)] @ np.linalg.solve(H[np.ix_(l, l)], H[np.ix_(l, p)])
    rp = robot[p]
    M = np.where(rp[:, None] == rp[None, :], S, 0.0)
    lam = scipy.linalg.eigh(S, M, eigvals_only=True)
    return float(lam[-1] / lam[0])


def _pcg_extra(run, H, tol, kappa):
    """What the PCG pass's inexact solve may add to scaled_error.  CG starts at x = 0, so gamma_first = b^T M^-1 b and rho =
    sqrt(gamma_last / gamma_first) is the relative residual in the M^-1 norm:  ||e||_S / ||x||_S <= sqrt(kappa(M^-1 S)) rho.  The
    landmarks' back-substitution extends the pose error e_p to the full e = [e_p; -H_ll^-1 H_lp e_p], whose H-norm is ||e_p||_S (and
    likewise for the step), so the same bound holds for ||e||_H / ||dx||_H; the W-norm of scaled_error (W = diag(H)^1/2) is within
    sqrt(kappa_s) of the H-norm.  Added term: sqrt(kappa_s kappa(M^-1 S)) rho — from the rho every robot's stats report after the pass
    (all of them: the scalars are all-reduced), which must have reached PCG_TOL.  The term must stay below the reference tolerance
    itself: a bound that swamps it would make the comparison vacuous."""
    stats = [sh.graph.pcg_stats() for sh in run.shards]
    for st in stats:
        assert st["gamma_first"] > 0 and st["gamma_last"] <= PCG_TOL ** 2 * st["gamma_first"], st       # (the tolerance was reached)
        assert st["gamma_first"] == stats[0]["gamma_first"] and st["gamma_last"] == stats[0]["gamma_last"], stats
    rho = np.sqrt(max(stats[0]["gamma_last"], 0.0) / stats[0]["gamma_first"])
    add = float(np.sqrt(kappa * _pcg_kappa(run.ref, H)) * rho)
    assert add <= tol, (add, tol)
    return add


def _pcg_case(s, J, evidence=None):
    def ev(r):
        assert r.info["n_slots"] > 0 and r.drv.pcg_iters == PCG_ITERS and not r.drv.arrow
        if evidence is not None:
            evidence(r)
    _, ratio = run_case(s, J, 0, evidence=ev, pcg_iters=PCG_ITERS, pcg_tol=PCG_TOL, extra=_pcg_extra)
    return ratio


@pytest.mark.parametrize("R", [2, 4])
def test_pcg_pass(gpu, R):
    _report("pcg pass", _pcg_case(gpu, jg.shared_mix_case(R)))


@pytest.mark.parametrize("cls", [0, 1, 2], ids=["cyl", "cube", "point"])
@pytest.mark.parametrize("nf", COUNTS)
def test_pcg_separator_landmark_factor_count(gpu, cls, nf):
    """k_landmark_b<1> / <2> over the landmark-count sweep on a shared landmark."""
    _report("pcg landmark count", _pcg_case(gpu, jg.landmark_count_case(cls, nf, shared=True)))


if __name__ == "__main__":
    import torch  # noqa: F401   (torch before the product library: tests/conftest.py)
    torch.zeros(1, device="cuda:0")
    print(json.dumps(_child_main(sys.argv[1])))
