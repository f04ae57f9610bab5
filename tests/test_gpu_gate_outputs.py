"""The output contract of the covariance-weighted queries at the C ABI (host_gates.hip): slide_graph_closure_mahalanobis,
_observation_mahalanobis, _landmark_pair_mahalanobis, _get_landmark_pair_covariances, _get_pose_pair_covariances and their
slide_chol_batch_* counterparts, called through ctypes as a C caller would — the Python wrappers always pass every array, zeroed.

Per call, a list of five candidates with a SLIDE_MISSING one and, where the call has that refusal, a SLIDE_ERR_INVALID one between
served neighbours.  The wrapper runs the list once with its library handle replaced by a recorder, which gives the call's name and
its exact input arrays; the call is then repeated on gpu.lib()
  (a) with every output pre-filled with a sentinel (NaN, -7): a refused candidate's d2 / C / r / covariance block is exactly zero and
      its status word set, a served one's outputs are bit for bit the wrapper's, dof and route are written for served and refused alike;
  (b) with every optional output NULL: SLIDE_OK, and d2 (or the covariance array) is bit for bit that of (a).
No tolerance anywhere.  Graphs: observation_gate_cases' chain40, landmark_pair_cases' dup40, and the two-robot 14-pose DupJoint after
one exact pass, built as test_gpu_joint_landmark_pairs.py builds it."""
import ctypes as C

import numpy as np
import pytest

import joint_landmark_pair_cases as jp
import joint_observation_gate_cases as jo
import landmark_pair_cases as lp
import observation_gate_cases as og
from test_gpu_joint_observation_gate import GateRun

pytestmark = pytest.mark.gpu

MISSING, INVALID = 1, -1
I7 = [0.0, 0, 0, 0, 0, 0, 1]
SIGMA6 = [0.01] * 3 + [0.05] * 3
# how many trailing arguments of each call are outputs: the first is needed, the others may be NULL, the last is status
N_OUT = {"get_pose_pair_covariances": 2, "closure_mahalanobis": 4, "observation_mahalanobis": 5,
         "graph_landmark_pair_mahalanobis": 6, "chol_batch_landmark_pair_mahalanobis": 5,
         "graph_get_landmark_pair_covariances": 3, "chol_batch_get_landmark_pair_covariances": 2}


class Recorder:
    """Stands in for a wrapper object's library handle: forwards every call and keeps its name and arguments."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def recorded(obj, method, *args):
    """obj.method(*args) -> (the C call's name, its arguments; the pointers hold their arrays, the outputs filled by the wrapper)."""
    rec = Recorder(obj.L)
    obj.L = rec
    try:
        getattr(obj, method)(*args)
    finally:
        obj.L = rec.lib
    assert len(rec.calls) == 1, [name for name, _ in rec.calls]
    return rec.calls[0]


def check_contract(gpu, obj, method, args, want_status):
    name, cargs = recorded(obj, method, *args)
    n = len(want_status)
    n_out = next(v for k, v in N_OUT.items() if name.endswith(k))
    fn = getattr(gpu.lib(), name)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    ins, ref = cargs[:-n_out], [p.keep for p in cargs[-n_out:]]
    assert ref[-1][:n].tolist() == want_status, (name, ref[-1][:n])
    refused = np.array(want_status) != 0
    assert refused.any() and not refused.all()

    def sentinel(a):
        return np.full_like(a, np.nan if a.dtype == np.float64 else -7)
    # (a) every output pre-filled with a sentinel
    got = [sentinel(a) for a in ref]
    assert fn(*ins, *[ptr(a) for a in got]) == 0, name
    for g, r in zip(got, ref):
        assert np.array_equal(g[:n], r[:n]), (name, g[:n], r[:n])
        if g.dtype == np.float64:
            assert not g[:n][refused].any() and all(x.any() for x in g[:n][~refused]), name      # exactly zero / served
        else:
            assert (g[:n] != -7).all(), name                                                     # status, dof, route: every word written
    assert got[-1][:n].tolist() == want_status
    print(f"[gate-outputs] {name}: status {want_status}, {n_out} outputs bit for bit the wrapper's, zeros where refused")
    # (b) every optional output NULL
    alone = sentinel(ref[0])
    assert fn(*ins, ptr(alone), *[None] * (n_out - 1)) == 0, name
    assert np.array_equal(alone[:n], got[0][:n]), name


def test_single_graph_calls(gpu):
    G, _ = og.device_graph(gpu, "chain40", 0)
    ends = [(0, 35, 0, 1), (0, 99, 0, 1), (0, 20, 0, 3), (0, 7, 0, 7), (0, 30, 0, 12)]
    want = [0, MISSING, 0, INVALID, 0]
    check_contract(gpu, G, "closure_mahalanobis", ([e + (I7, SIGMA6) for e in ends],), want)
    check_contract(gpu, G, "get_pose_pair_covariances", (ends,), want)
    c, vals = og.case("chain40", 0), og.device_values(G)
    rng = np.random.default_rng(4)
    pt, cube, cyl = (og.at_estimate(c, vals, kind, 0, p, l, rng.normal(0, 1, og.KIND[kind][3]))
                     for kind, p, l in (("point", 7, 0), ("cube", 12, 3), ("cylinder", 13, 6)))
    cands = [pt, ("point", 0, 99, 0) + pt[4:], cube, ("cube", 0, 12, 4) + cube[4:], cyl]      # an unknown pose, an unknown cube
    check_contract(gpu, G, "observation_mahalanobis", (cands,), [0, MISSING, 0, MISSING, 0])
    D, _ = lp.device_graph(gpu, "dup40", 0)
    pairs = [(0, 100), (0, 777), lp.REVISIT, (3, 3), (3, 103)]                                 # both routes among the served
    name, cargs = recorded(D, "landmark_pair_mahalanobis", 2, pairs, lp.SIGMA["point"])
    assert sorted(set(cargs[-2].keep[[0, 2, 4]].tolist())) == [0, 1], cargs[-2].keep
    check_contract(gpu, D, "landmark_pair_mahalanobis", (2, pairs, lp.SIGMA["point"]), want)
    check_contract(gpu, D, "get_landmark_pair_covariances", (2, pairs), want)


def test_joint_graph_calls(gpu):
    g = GateRun(gpu, jp.DupJoint(), 0, okw=jp.DUP_OKW, kw=jp.DUP_KW)
    try:
        b, c = g.batch, g.c
        ends = [(0, 2, 1, 3), (0, 99, 1, 3), (1, 9, 0, 8), (0, 5, 0, 5), (2, 1, 0, 12)]       # a pose, then a slot, the batch lacks
        want = [0, MISSING, 0, INVALID, MISSING]
        check_contract(gpu, b, "closure_mahalanobis", ([e + (I7, SIGMA6) for e in ends],), want)
        check_contract(gpu, b, "get_pose_pair_covariances", (ends,), want)
        named = jo.perturbed_list(c, g.vals)
        first = {kind: next(x for x in named if x[0] == kind) for kind in ("point", "cylinder", "cube")}
        pt, cyl, cube = first["point"], first["cylinder"], first["cube"]
        cands = [pt, pt[:2] + (99,) + pt[3:], cyl, cube[:3] + (777,) + cube[4:], named[-1]]     # (and the list's last candidate)
        check_contract(gpu, b, "observation_mahalanobis", (cands,), [0, MISSING, 0, MISSING, 0])
        rows = [(ra, jo.local_id(c, ra, 2, ga), rb, jo.local_id(c, rb, 2, gb)) for ra, ga, rb, gb, _, _ in c.J.dups["point"]]
        pairs = [rows[0], (0, 777, 1, 0), rows[1], rows[0][:2] + rows[0][:2], rows[-1]]         # (the last: private-shared)
        check_contract(gpu, b, "landmark_pair_mahalanobis", (2, pairs, jp.SIGMA["point"]), want[:4] + [0])
        check_contract(gpu, b, "get_landmark_pair_covariances", (2, pairs), want[:4] + [0])
    finally:
        g.close()
