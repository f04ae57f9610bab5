"""The Mahalanobis gate and the pose-pair marginal on the JOINT graph (slide_chol_batch_closure_mahalanobis /
slide_chol_batch_get_pose_pair_covariances): what can be checked without a device.

- The symbols, the header's words and the Python methods.
- The argument refusals, decided in capi.hip before the batch or the device is looked at, provoked with a NULL batch as
  test_closure_gate_host.py provokes the single-graph calls': good arguments are refused FOR the handle, a bad argument for itself,
  and nothing is written.
- The identity B^T K^-1 B = W^T D W, L W = B, in numpy on test_joint_multi_solve.py's systems, lists and levels: the FORWARD half of
  that schedule alone, then the signed sum over every coordinate once.  D = +I on the lambda rows, or counting a robot's rows of
  separator coordinates (partial sums the separator already holds), gives a different matrix.
- The list generators' own conditions (tests/joint_closure_gate_cases.py), on the reference alone."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import slide_slam_amd as s                                                      # noqa: E402

import closure_gate_cases as gc                                                 # noqa: E402
import joint_closure_gate_cases as jc                                           # noqa: E402
import joint_graphs as jg                                                       # noqa: E402
from test_joint_multi_solve import LEVEL, T_, lists, node_of, rhs, split_systems      # noqa: E402
from test_joint_selected_inverse import B, joint_layout, ldl_blocks             # noqa: E402

NEW = ["slide_chol_batch_get_pose_pair_covariances", "slide_chol_batch_closure_mahalanobis"]
I7 = [0.0, 0, 0, 0, 0, 0, 1]
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731


def test_new_symbols_declared_exported_and_documented():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = s.lib()
    for f in NEW:
        assert re.search(r"\bint\s+" + f + r"\s*\(", code), f
        assert hasattr(L, f), f
        assert f in s.api.EXPORTS
    comments = " ".join(re.findall(r"/\*.*?\*/", txt, flags=re.S))
    assert "JOINT graph: block k" in comments and "W^T D W" in comments and "No counterpart in the reference" in comments
    assert callable(s.CholBatch.get_pose_pair_covariances) and callable(s.CholBatch.closure_mahalanobis)
    from slide_slam_amd.distributed import PassDriver
    assert callable(PassDriver.get_pose_pair_covariances) and callable(PassDriver.closure_mahalanobis)


def _change(good, change):
    a = {k: v.copy() for k, v in good.items()}
    for k, v in change.items():
        if v is None:
            a[k] = None
        else:
            v(a[k])
    return a


def put(i, j, v):
    def f(a):
        a[i, j] = v
    return f


def slot13(a):
    a[1] = 13


def test_gate_argument_refusals_come_before_the_batch_and_write_nothing():
    good = dict(fs=np.array([0, 1, 0], np.int32), fi=np.array([30, 31, 32], np.uint64), ts=np.array([1, 0, 0], np.int32),
                ti=np.array([1, 2, 3], np.uint64), rel=np.tile(I7, (3, 1)), sg=np.full((3, 6), 0.1))

    def refused(why, L=3, d2_null=False, **change):
        a = _change(good, change)
        d2, Cm, r, st = np.full(3, 77.0), np.full((3, 36), 77.0), np.full((3, 6), 77.0), np.full(3, 77, np.int32)
        rc = s.lib().slide_chol_batch_closure_mahalanobis(None, C.c_int(L), P(a["fs"]), P(a["fi"]), P(a["ts"]), P(a["ti"]), P(a["rel"]),
                                                          P(a["sg"]), None if d2_null else P(d2), P(Cm), P(r), P(st))
        assert rc == -1, (change, rc)                                  # SLIDE_ERR_INVALID
        err = s.api.last_error()
        assert "closure_mahalanobis" in err and why in err, (change, err)
        assert (d2 == 77).all() and (Cm == 77).all() and (r == 77).all() and (st == 77).all()

    def zero_quat(a):
        a[0, 3:] = 0.0
    refused("the batch is NULL")                                        # good arguments: only the handle is wrong
    for name in good:
        refused("pointer is NULL", **{name: None})
    refused("pointer is NULL", d2_null=True)
    refused("L < 0", L=-1)
    refused("outside", fs=slot13)
    refused("outside", ts=slot13)
    refused("non-finite", rel=put(1, 0, np.nan))
    refused("non-finite", rel=put(2, 6, np.inf))
    refused("zero quaternion", rel=zero_quat)
    refused("non-finite", sg=put(1, 3, np.nan))
    refused("sigma <= 0", sg=put(1, 3, 0.0))
    refused("sigma <= 0", sg=put(2, 0, -0.1))


def test_pair_argument_refusals_come_before_the_batch_and_write_nothing():
    good = dict(sa=np.array([0, 1], np.int32), ia=np.array([0, 5], np.uint64), sb=np.array([1, 1], np.int32), ib=np.array([9, 6], np.uint64))

    def refused(why, n=2, out_null=False, **change):
        a = _change(good, change)
        out, st = np.full((2, 144), 77.0), np.full(2, 77, np.int32)
        rc = s.lib().slide_chol_batch_get_pose_pair_covariances(None, C.c_int(n), P(a["sa"]), P(a["ia"]), P(a["sb"]), P(a["ib"]),
                                                                None if out_null else P(out), P(st))
        assert rc == -1, (change, rc)
        err = s.api.last_error()
        assert "get_pose_pair_covariances" in err and why in err, (change, err)
        assert (out == 77).all() and (st == 77).all()

    refused("the batch is NULL")
    for name in good:
        refused("pointer is NULL", **{name: None})
    refused("pointer is NULL", out_null=True)
    refused("n < 0", n=-1)
    refused("outside", sa=slot13)
    refused("outside", sb=slot13)


# ---- the identity, in numpy ---------------------------------------------------------------------------------------------------------

def forward_half(L, names, Bfull):
    """W = L^-1 Bfull by the forward half of test_joint_multi_solve.multi_solve's schedule (the same systems, lists and levels): per
    system the tiles after the walk — a robot's column tiles hold W, its rows of separator coordinates the partial sums that went
    into the separator, the separator's tiles W."""
    systems, maps = split_systems(L, names)
    nrhs = Bfull.shape[1]
    Xs, info = [], []
    for si, (tiles, nodes, ncols, Lr) in enumerate(systems):
        X = np.zeros((len(tiles) * B, nrhs))
        for a, t in enumerate(tiles[:ncols] if si < 2 else []):
            X[a * B:(a + 1) * B] = Bfull[t * B:(t + 1) * B]
        Xs.append(X)
        info.append(lists(Lr, nodes, ncols))
    Lt = lambda si, i, k: systems[si][3][i * B:(i + 1) * B, k * B:(k + 1) * B]       # noqa: E731

    def push(si, lev):
        tiles, nodes, ncols, _ = systems[si]
        groups = {}
        for k in range(ncols):
            if LEVEL[nodes[k]] == lev:
                groups.setdefault(node_of(nodes[k]), []).append(k)
        for g in groups.values():
            for k in g:
                x = np.linalg.solve(Lt(si, k, k), T_(Xs[si], k))
                for i in info[si][0][k]:
                    T_(Xs[si], i)[:] -= Lt(si, i, k) @ x
                T_(Xs[si], k)[:] = x

    def pull(si, lev):
        tiles, nodes, ncols, _ = systems[si]
        for k in range(len(tiles)):
            if LEVEL[nodes[k]] == lev:
                for j in info[si][2][k]:
                    T_(Xs[si], k)[:] -= Lt(si, k, j) @ T_(Xs[si], j)

    for r in (0, 1):
        push(r, 0)
        pull(r, 1); push(r, 1)
        pull(r, 2)
    for r in (0, 1):
        for o, st in enumerate(maps[r]):
            if st >= 0:
                T_(Xs[2], st)[:] += T_(Xs[r], systems[r][2] + o)
    push(2, 3)
    pull(2, 4); push(2, 4)
    return Xs, systems


def signed_gram(Xs, systems, sign, lam_sign=True, robots_sep_rows=False):
    """sum over the coordinates of W^T D W: a robot's column tiles (+), the separator's tiles with the factor's sign"""
    M = 0.0
    for si, (tiles, nodes, ncols, _) in enumerate(systems):
        for a, t in enumerate(tiles):
            if a >= ncols and not robots_sep_rows:
                continue
            W = T_(Xs[si], a)
            d = sign[t * B] if (t >= 0 and a < ncols and lam_sign) else 1.0
            M = M + d * (W.T @ W)
    return M


@pytest.mark.parametrize("lam_tiles", [1, 2])
def test_forward_half_and_signed_gram_give_the_block_of_the_inverse(lam_tiles):
    rng = np.random.default_rng(8 + lam_tiles)
    A, sign, names, npose = joint_layout(rng, lam_tiles)
    L = ldl_blocks(A, sign)
    Bf = rhs(rng, names, 12)
    assert np.abs(A[npose:, :npose]).max() > 0                          # (a case with relative-pose factors)
    want = Bf.T @ np.linalg.solve(A, Bf)
    Xs, systems = forward_half(L, names, Bf)
    got = signed_gram(Xs, systems, sign)
    scale = np.abs(want).max()
    tol = 1e-11
    assert np.abs(got - want).max() / scale < tol
    assert np.array_equal(got, got.T)
    plus = signed_gram(Xs, systems, sign, lam_sign=False)               # D = +I on the lambda rows
    twice = signed_gram(Xs, systems, sign, robots_sep_rows=True)        # a robot's rows of separator coordinates counted as well
    assert np.abs(plus - want).max() / scale > 1e6 * tol, np.abs(plus - want).max() / scale
    assert np.abs(twice - want).max() / scale > 1e6 * tol, np.abs(twice - want).max() / scale


# ---- the generators' own conditions, on the reference alone ---------------------------------------------------------------------------

CASES = {"relmeas": lambda: jg.relmeas_case(2, 3, 14), "shared_mix2": lambda: jg.shared_mix_case(2), "shared_mix4": lambda: jg.shared_mix_case(4),
         "border64": lambda: jg.border_case((1, 5, 4)), "border129": lambda: jg.border_case((3, 10, 6)),
         "separator_tiles": jg.separator_tiles_case}


# (the device tests run relmeas under both charts, the others under chart 0)
@pytest.mark.parametrize("name,chart", [("relmeas", 0), ("relmeas", 1)] + [(n, 0) for n in sorted(CASES) if n != "relmeas"])
def test_generators_meet_their_conditions_on_the_reference(name, chart):
    J = CASES[name]()
    c = jc.JointGateCase(J, chart)
    closures, flags, d2 = jc.planted_list(c)                            # (asserts true < 16.81 / 2 and false > 4 x 16.81)
    assert flags.sum() == 6 and (~flags).sum() == 4 and all(x[0] != x[2] for x in closures)
    assert d2[flags].max() < jc.GATE2 / 2 and d2[~flags].min() > 4 * jc.GATE2
    used = jc.inter(jc.pair_list(J)) + jc.inter(jc.end_list(J)) + [x[:4] for x in closures]
    assert len(jc.inter(jc.pair_list(J))) >= 4 and len(jc.inter(jc.end_list(J))) >= 3
    for e in used:
        assert c.cross_ratio(*e) >= 1e-3, (e, c.cross_ratio(*e))
    pl = jc.perturbed_list(J, c.cpu_pose12)
    assert len(pl) == 18 and len({tuple(x[5]) for x in pl}) == 18
    _, _, Cm, d2p = gc.ref_gate(c, pl, c.cpu_pose12)
    assert d2p.min() < jc.GATE2 < d2p.max()                             # (both sides of the gate)
    long_c = jc.long_closure_list(J, c.cpu_pose12)
    assert long_c[61] is long_c[0] and sum(x[0] != x[2] for x in long_c) >= 20
    long_p = jc.long_pair_list(J)
    assert len(long_p) == 33 and long_p[30] == long_p[0] and sum(x[0] != x[2] for x in long_p) >= 10
