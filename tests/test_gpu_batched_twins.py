"""The batched kernels against their by-value twins.  Every kernel of a batched pass that takes the graphs as a table in memory
(const GraphDev* Gs, Gs[blockIdx.z]: k_relin_b, k_lin_lf_b / k_lin_lf_robust_b, k_robust_reweight_b, k_landmark_b<1> / <2>, k_pose_b,
k_schur_b, k_pad_rhs_b, k_backsub_b, k_estimate_b) shares its body with a kernel that takes ONE graph by value (k_relin, k_lin_lf, ...).
The table's pointer members are global pointers on the device (graph_dev.hpp); a wrong pointer type or a lost predicate in a _b kernel
would show where the two paths part.

A batch of ONE robot with no shared slot takes the block-Jacobi batched pass (CholBatch.pass_all through PassDriver, no separator, no
PCG) through the _b kernels; the same graph on its own takes SlideGraph.gauss_newton through the by-value kernels.  Both are the
same Gauss-Newton passes of the same graph: every pose (get_pose12) and every landmark (get_landmark) is compared after one pass and
after three, under both Pose3 charts, on
  small     the golden `small` replay (tests/golden/replay_small.npz: 40 key frames through SlideBackend), and
  handmade  one robot of 72 poses built with joint_graphs / assembly_cases' builders: a point with ONE factor, a point with 66 factors
            (more than the 64 lanes of k_landmark's wave), a cylinder, a cube and points in turn (any four consecutive landmarks, one
            workgroup of k_landmark_b, are of three classes), poses 67 and 71 with NO landmark factor, and one loop closure whose
            measurement is off by decimetres;
and once more on `handmade` with the relative-pose robust loss (Huber on the closure: k_robust_reweight / k_robust_reweight_b) and once
with the observation loss (Huber on every class: k_lin_lf_robust / k_lin_lf_robust_b).

Tolerance.  The two paths' factorisation kernels differ (k_chol_step against k_chol_step_batched), so whether they agree bit for
bit had to be measured: on the PARENT of the commit that made the table's pointers global, max |batched - by value| over every value
of both read-outs (values up to 60) was
  small-chart0 0.0  small-expmap 0.0  handmade-chart0 0.0  handmade-expmap 0.0  handmade-closure-loss 0.0  handmade-observation-loss 0.0
and the weights of both losses were the same bits as well.  PARENT_DIFF holds these figures; a case whose figure is 0 asserts bitwise
equality (all six do), any other would assert ten times its figure."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import assembly_cases as ac                                                    # noqa: E402,F401  (its builders are joint_graphs')
import gn_graphs as gg                                                         # noqa: E402
import joint_graphs as jg                                                      # noqa: E402

pytestmark = pytest.mark.gpu

PASSES = (1, 3)
P_HAND, N_MANY = 72, 66
HUBER_K = 0.5

# case -> max |batched - by value| measured on the parent library (see the docstring)
PARENT_DIFF = {"small-chart0": 0.0, "small-expmap": 0.0, "handmade-chart0": 0.0, "handmade-expmap": 0.0,
               "handmade-closure-loss": 0.0, "handmade-observation-loss": 0.0}

CASES = [("small-chart0", "small", 0, None), ("small-expmap", "small", 1, None), ("handmade-chart0", "handmade", 0, None),
         ("handmade-expmap", "handmade", 1, None), ("handmade-closure-loss", "handmade", 0, "closure"),
         ("handmade-observation-loss", "handmade", 0, "observation")]


def handmade():
    """(J, closure) — the graph of the docstring; closure = (rel7, i, j) of the loop closure."""
    J = jg.Joint([P_HAND], seed=51, step=0.3)
    rng = np.random.default_rng(51)
    J.point(jg._near(J, 0, 30, rng), [(0, k) for k in range(N_MANY)])
    J.point(jg._near(J, 0, 3, rng), [(0, 3)])
    n = 0
    for k in range(0, P_HAND, 4):               # (poses k, k + 1, k + 2: 67 and 71 stay without a landmark factor)
        jg._add(J, n % 3, jg._near(J, 0, k, rng), [(0, j) for j in range(k, min(P_HAND - 1, k + 3))], rng)
        n += 1
    (Ra, ta), (Rb, tb) = J.T(0, 5), J.T(0, 40)
    rel = gg.p7(Ra.T @ Rb, Ra.T @ (tb - ta) + np.array([0.3, -0.2, 0.1]))
    return J, (rel, 5, 40)


def handmade_claims(J):
    per_lm = [len(obs) for _, _, _, obs in J.lms]
    seen = {k for _, _, _, obs in J.lms for _, k in obs}
    assert per_lm[0] == N_MANY > 64 and per_lm[1] == 1
    assert {cls for cls, _, _, _ in J.lms} == {0, 1, 2}
    assert 67 not in seen and P_HAND - 1 not in seen and len(seen) == P_HAND - 2
    order = [cls for cls, _, _, _ in J.lms][2:]
    assert all(len(set(order[i:i + 3])) == 3 for i in range(len(order) - 3))


class _Graph:
    """A graph, the ids of its poses and landmarks, and what keeps it alive."""

    def __init__(self, graph, n_poses, n_lm, keep=None):
        self.graph, self.n_poses, self.n_lm, self.keep = graph, n_poses, n_lm, keep

    def landmark_table(self, cls):
        n = self.n_lm[cls]
        return np.zeros((n, 3)), np.zeros(n, np.int32)

    def values(self):
        poses = np.array([self.graph.get_pose12(0, k)[1] for k in range(self.n_poses)])
        lms = [np.array([self.graph.get_landmark(cls, i)[1] for i in range(self.n_lm[cls])]).reshape(-1) for cls in range(3)]
        return np.concatenate([poses.reshape(-1)] + lms)


def make_graph(s, which, chart):
    kw = dict(pose_chart=chart)
    if which == "small":
        from slide_slam_amd.replay import replay_single
        z = np.load(os.path.join(ROOT, "tests", "golden", "replay_small.npz"))
        log = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
        be = s.SlideBackend(s.default_params(**kw), 1)
        replay_single(be, log, collect=False)
        c = be.counts()
        assert [c["cyl"], c["cube"], c["point"], c["factors"]] == list(z["counts"])
        return _Graph(be.graph, len(log["rel7"]), [c["cyl"], c["cube"], c["point"]], keep=be)
    J, (rel, i, j) = handmade()
    handmade_claims(J)
    G = J.emit_shard(s.SlideGraph(s.default_params(**kw)), 0)
    G.add_loop_closure(rel, i, 0, j, 0)
    return _Graph(G, P_HAND, [len(x) for x in J.local_ids()[0]])


def set_loss(obj, loss):
    if loss == "closure":
        obj.set_robust_loss("huber", HUBER_K, closures=True, relative_meas=True)
    elif loss == "observation":
        obj.set_observation_loss("huber", HUBER_K)


def read_weights(obj, loss):
    """The weights of the last pass's linearisation (graph or batch: the same columns)."""
    if loss == "closure":
        return obj.closure_weights()["weight"]
    if loss == "observation":
        return obj.observation_weights()["weight"]
    return np.zeros(0)


def run_by_value(s, which, chart, loss):
    g = make_graph(s, which, chart)
    set_loss(g.graph, loss)
    out, weights, done = [], [], 0
    for n in PASSES:
        assert g.graph.gauss_newton(n - done) == 0
        done = n
        out.append(g.values())
        weights.append(read_weights(g.graph, loss))
    return out, weights


def run_batched(s, which, chart, loss):
    import torch
    from slide_slam_amd.distributed import PassDriver, setup_local_shards
    dev = torch.device("cuda", 0)
    g = make_graph(s, which, chart)
    batch = s.CholBatch(1)
    g.graph.join_chol_batch(batch, 0)
    try:
        gid = [[np.arange(n, dtype=np.int64) for n in g.n_lm]]
        bufs, info = setup_local_shards([g], None, device=dev, assoc=(gid, list(g.n_lm)))
        assert info["n_slots"] == 0
        drv = PassDriver([g], bufs, 0, batch=batch, device=dev)
        assert not drv.arrow and drv.pcg_iters == 0          # (block-Jacobi: the robot's own factorisation, nothing exchanged)
        set_loss(batch, loss)
        out, weights, done = [], [], 0
        for n in PASSES:
            for _ in range(n - done):
                drv.one_pass()
            torch.cuda.synchronize()
            done = n
            out.append(g.values())
            weights.append(read_weights(batch, loss))
        return out, weights
    finally:
        g.graph.join_chol_batch(None)


@pytest.mark.parametrize("name,which,chart,loss", CASES, ids=[c[0] for c in CASES])
def test_batched_pass_matches_by_value_pass(gpu, name, which, chart, loss):
    start = make_graph(gpu, which, chart).values()
    a, wa = run_by_value(gpu, which, chart, loss)
    b, wb = run_batched(gpu, which, chart, loss)
    diffs = [float(np.abs(x - y).max()) for x, y in zip(a, b)]
    moved = [float(np.abs(x - start).max()) for x in a]
    print(f"[batched-twins] {name}: max |batched - by value| after {PASSES} passes {diffs}, moved from the start by {moved}, "
          f"{len(start)} values, max |value| {np.abs(a[-1]).max():.3g}")
    assert all(np.isfinite(x).all() for x in a + b)
    assert moved[0] > 1e-6 and np.abs(a[1] - a[0]).max() > 1e-9          # (the passes really move the graph, the later ones too)
    if loss is not None:
        # the first pass linearises at the built values, where the closure is decimetres off and the perturbed poses leave large
        # residuals: the loss really reweights; by the third pass the graph has settled and most weights are back at 1
        print(f"[batched-twins] {name}: {len(wa[0])} weights, below 1 after pass {PASSES}: {[int((w < 1.0).sum()) for w in wa]}, "
              f"max |difference| {[float(np.abs(x - y).max()) for x, y in zip(wa, wb)]}")
        assert len(wa[0]) == len(wb[0]) > 0 and (wa[0] < 1.0).any()
        for x, y in zip(wa, wb):
            assert np.array_equal(x, y)
    bound = 10.0 * PARENT_DIFF[name]
    for n, x, y, d in zip(PASSES, a, b, diffs):
        if bound == 0.0:
            assert np.array_equal(x, y), (n, d)
        else:
            assert d <= bound, (n, d, bound)
