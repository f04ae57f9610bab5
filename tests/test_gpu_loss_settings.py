"""The settings of the two robust losses at their four entry points (SlideGraph / CholBatch x closure loss / observation loss): what
the setters refuse and in which words, what param = 0 means, what clearing does, and that a changed setting - or joining and leaving
a batch - leaves nothing of the last streaming solve behind for the next one.  The weighted steps themselves are compared with
their references in test_gpu_robust_loss.py, test_gpu_observation_loss.py and their joint counterparts; here only bits are compared
with bits, and the streaming poses under the wildfire bound with those without it (test_gpu_gn_step.test_wildfire_after_chi2's
scheme and bound)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gn_graphs as gg                                                          # noqa: E402
import joint_graphs as jg                                                       # noqa: E402
import joint_observation_loss_cases as jo                                       # noqa: E402
import joint_robust_cases as jr                                                 # noqa: E402
import observation_loss_cases as oc                                             # noqa: E402
import robust_cases as rc                                                       # noqa: E402

pytestmark = pytest.mark.gpu

KIND_TEXT = "kind must be 0 (off), 1 Huber, 2 Cauchy, 3 Geman-McClure or 4 DCS"
NAN_TEXT = "param is not a number"
CLOSURE_MASK = "class_mask has bit 0 (loop closures) and bit 1 (relative measurements) only"
OBSERVATION_MASK = "class_mask has bit 0 (bearing-range), bit 1 (cube) and bit 2 (cylinder) only"
PCG_TEXT = "the batch runs PCG passes (pcg_iters > 0), whose step leaves the inter-robot factors' cross block out; they do not carry "
# entry point -> (on a batch, the observation loss, C ABI setter, prefix of its messages, first mask bit it does not know, its mask
# sentence, its own refusal: a graph that has joined a batch / a batch that runs PCG passes)
ENTRIES = {
    "graph-closure": (False, False, "slide_graph_set_robust_loss", "set_robust_loss", 4, CLOSURE_MASK,
                      "the graph has joined a batch; the sharded and joint paths do not carry a robust loss"),
    "graph-observation": (False, True, "slide_graph_set_observation_loss", "set_observation_loss", 8, OBSERVATION_MASK,
                          "the graph has joined a batch; a batch carries its own observation loss (slide_chol_batch_set_observation_loss), "
                          "the un-batched sharded passes carry none"),
    "batch-closure": (True, False, "slide_chol_batch_set_robust_loss", "chol_batch_set_robust_loss", 4, CLOSURE_MASK,
                      PCG_TEXT + "a robust loss"),
    "batch-observation": (True, True, "slide_chol_batch_set_observation_loss", "chol_batch_set_observation_loss", 8, OBSERVATION_MASK,
                          PCG_TEXT + "an observation loss"),
}


def sync():
    import torch
    torch.cuda.synchronize()


def raw_set(s, fn, obj, kind, param, mask):
    """The C ABI's setter as it is: SlideGraph / CholBatch assemble the mask themselves and cannot pass a bit out of range."""
    h = obj.h if isinstance(obj.h, C.c_void_p) else C.c_void_p(obj.h)
    s.api._check(getattr(s.lib(), fn)(h, C.c_int(kind), C.c_double(param), C.c_int(mask)))


def refused(s, fn, obj, kind, param, mask, text):
    with pytest.raises(s.SlideError) as e:
        raw_set(s, fn, obj, kind, param, mask)
    assert str(e.value) == "SLIDE_ERR_INVALID: " + text


# ---- 1: the refusals, word for word -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusal_texts(gpu, entry):
    on_batch, _, fn, who, bad_bit, mask_text, own = ENTRIES[entry]
    full = bad_bit - 1
    batch = gpu.CholBatch(1)
    G = gpu.SlideGraph(gpu.default_params())
    obj = batch if on_batch else G
    refused(gpu, fn, obj, -1, 0.0, full, f"{who}: {KIND_TEXT}")
    refused(gpu, fn, obj, 5, 0.0, full, f"{who}: {KIND_TEXT}")
    refused(gpu, fn, obj, 1, 0.0, full | bad_bit, f"{who}: {mask_text}")
    refused(gpu, fn, obj, 1, float("nan"), full, f"{who}: {NAN_TEXT}")
    refused(gpu, fn, obj, -1, float("nan"), full | bad_bit, f"{who}: {KIND_TEXT}")      # (the checks' order: kind, mask, number)
    refused(gpu, fn, obj, 1, float("nan"), full | bad_bit, f"{who}: {mask_text}")
    raw_set(gpu, fn, obj, 1, 0.0, full)                                                 # (and a call that is right is taken)
    raw_set(gpu, fn, obj, 0, 0.0, 0)
    if on_batch:
        batch.set_pcg(1)
        refused(gpu, fn, batch, 1, 0.0, full, f"{who}: {own}")
        refused(gpu, fn, batch, 1, float("nan"), full, f"{who}: {NAN_TEXT}")            # (the number is looked at first here)
        raw_set(gpu, fn, batch, 0, 0.0, 0)                                              # (clearing is no loss: not refused)
    else:
        G.join_chol_batch(batch, 0)
        try:
            refused(gpu, fn, G, 1, 0.0, full, f"{who}: {own}")
            refused(gpu, fn, G, 1, float("nan"), full, f"{who}: {own}")                 # (wrong twice: the batch is named, not the number)
            refused(gpu, fn, G, 1, float("nan"), full | bad_bit, f"{who}: {mask_text}")
        finally:
            G.join_chol_batch(None)
        raw_set(gpu, fn, G, 1, 0.0, full)


# ---- 2: param = 0 is the loss's default, bit for bit; kind 0 clears ------------------------------------------------------------------

_CASES = {}


def joint_case(observation):
    """The builders are deterministic and nothing here changes a J: built once."""
    if observation not in _CASES:
        _CASES[observation] = jo.kinds_case() if observation else jr.kinds_case()
    return _CASES[observation]


class Single:
    """robust_cases.chain_graph / observation_loss_cases.mixed_graph on one SlideGraph; a step is gauss_newton(1)."""

    def __init__(self, s, observation):
        self.observation = observation
        if observation:
            if "sig" not in _CASES:
                _CASES["sig"] = oc.mixed_cube_sigmas(0)
            self.G = s.SlideGraph(s.default_params(**oc.params(0)[1]))
            oc.mixed_graph(self.G, _CASES["sig"])
        else:
            self.G = s.SlideGraph(s.default_params())
            rc.chain_graph(self.G)
        self.target = self.G

    def step(self):
        assert self.G.gauss_newton(1) == 0

    def close(self):
        pass


class Batched:
    """joint_robust_cases.kinds_case / joint_observation_loss_cases.kinds_case as two shards in one CholBatch; a step is one exact
    joint pass (test_gpu_joint_step.Run's setup, without its reference)."""

    def __init__(self, s, observation):
        import torch
        from slide_slam_amd.distributed import PassDriver, setup_local_shards
        self.observation = observation
        J = joint_case(observation)
        kw = oc.params(0)[1] if observation else {}
        dev = torch.device("cuda", 0)
        self.shards, assoc = jg.build(J, lambda: s.SlideGraph(s.default_params(**kw)))
        self.target = s.CholBatch(J.R)
        for t, sh in enumerate(self.shards):
            sh.graph.join_chol_batch(self.target, t)
        bufs, info = setup_local_shards(self.shards, None, device=dev, assoc=assoc)
        self.drv = PassDriver(self.shards, bufs, info["n_slots"], batch=self.target, device=dev, arrow=True, sep_dim=info["sep_dim"],
                              sep_prof=info.get("sep_prof"))
        if J.relmeas:
            assert self.drv.setup_ghosts(J.relmeas) > 0

    def step(self):
        self.drv.one_pass()
        sync()

    def close(self):
        for sh in self.shards:
            sh.graph.join_chol_batch(None)


def weighted_step(s, entry, kind, param):
    """A fresh graph or batch, the loss set, one step -> (the harness, its read-back)."""
    on_batch, observation = ENTRIES[entry][:2]
    run = (Batched if on_batch else Single)(s, observation)
    try:
        (run.target.set_observation_loss if observation else run.target.set_robust_loss)(kind, param)
        run.step()
        return run, (run.target.observation_weights() if observation else run.target.closure_weights())
    except BaseException:
        run.close()
        raise


@pytest.mark.parametrize("kind", sorted(rc.KINDS))
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_default_param(gpu, entry, kind):
    observation = ENTRIES[entry][1]
    a, wa = weighted_step(gpu, entry, kind, 0.0)
    try:
        b, wb = weighted_step(gpu, entry, rc.KINDS[kind], rc.DEFAULT[rc.KINDS[kind]])      # (and the kind by its number)
        b.close()
        assert wa["n"] == wb["n"] == len(wa["weight"]) > 0
        assert (wa["weight"] < 1.0).any()                      # (the loss is at work: the cases carry gross factors of every kind)
        classes = set(wa["cls"].tolist()) if observation else set(wa["kind"].tolist())
        assert classes == ({0, 1, 2} if observation else {1, 2})
        assert wa["weight"].tobytes() == wb["weight"].tobytes()
        assert wa["s2"].tobytes() == wb["s2"].tobytes()
        # cleared: the next step linearises unweighted
        (a.target.set_observation_loss if observation else a.target.set_robust_loss)(None)
        a.step()
        wc = a.target.observation_weights() if observation else a.target.closure_weights()
        assert wc["n"] == wa["n"] and (wc["weight"] == 1.0).all()
    finally:
        a.close()


# ---- 3: a changed setting, or a batch joined and left, resets what the streaming update keeps ---------------------------------------
# The graph of test_wildfire_after_chi2 holds odometry alone, so no loss selects a factor of it and joining a batch that runs no pass
# moves nothing: with the bound off every event leaves the oracle's trajectory (solve, key frame, solve) as it is.  What the events
# must do is drop the kept solution, the factor and the streaming update's predictions, as chi2() does there.

def _join_leave(s, G):
    batch = s.CholBatch(1)
    G.join_chol_batch(batch, 0)
    G.join_chol_batch(None)


EVENTS = {      # name -> (before the first solve, between the first solve and the key frame)
    "closure-loss-on": (None, lambda s, G: G.set_robust_loss("huber")),
    "closure-loss-off": (lambda s, G: G.set_robust_loss("huber"), lambda s, G: G.set_robust_loss(None)),
    "observation-loss-on": (None, lambda s, G: G.set_observation_loss("huber")),
    "observation-loss-off": (lambda s, G: G.set_observation_loss("huber"), lambda s, G: G.set_observation_loss(None)),
    "join-leave": (None, _join_leave),
}


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("event", sorted(EVENTS))
def test_wildfire_after_event(gpu, event, chart):
    before, between = EVENTS[event]
    thr = 1e-3
    P = 30
    runs = []
    for wf in (0.0, thr):
        G = gpu.SlideGraph(gpu.default_params(pose_chart=chart))
        G.set_wildfire(wf)
        if before is not None:
            before(gpu, G)
        W = gg.World(G, P, seed=6, noise=0.0, perturb={3: [0.05, -0.03, 0.02]})
        assert G.solve() == 0
        between(gpu, G)
        (Ra, ta) = W.T[-1]
        rel = gg.p7(gg.rot([0, 0, 0.1]), np.array([1.0, 0.0, 0.0]))
        Rb, tb = Ra @ gg.rot([0, 0, 0.1]), ta + Ra @ np.array([1.0, 0.0, 0.0])
        G.add_keypose_between(0, P - 1, P, rel, gg.p7(Rb, tb))
        assert G.solve() == 0
        runs.append(np.array([G.get_pose12(0, k)[1] for k in range(P + 1)]))
    print(f"[loss-settings] {event} chart {chart}: max pose difference {np.abs(runs[1] - runs[0]).max():.3e} (bound {thr})")
    assert np.abs(runs[1] - runs[0]).max() <= thr, np.abs(runs[1] - runs[0]).max()
